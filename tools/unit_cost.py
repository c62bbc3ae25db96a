"""Kernel time of qpgpu_solve_batched_unit against qpgpu_solve_batched_eq (QPGPU_FLAG_EXACT) on the
materialised problem with G = I, same build, same QPs, both with the eq triple (the control cycle's
call).

For each shape and g0 mode the two entries are launched alternately on one stream, each launch
between its own HIP-event pair, over resident input sets (set r = set 0 rolled by r*B/R QPs; R
chosen per entry so that its sets together exceed twice the Infinity Cache), so every launch reads
cold inputs; untimed launches of both entries run first until the clocks are steady.  The QPs are
qpgpu.make_unit_problems(n, p, m, ...) with g0 = 0 (the controller's) and with g0 ~ 10 N(0, 1).
Prints one JSON line per shape and mode: median / min / max kernel ms per launch for both entries,
the ratio of the medians and the mean l1 passes; the seven outputs of the two entries are compared
bit for bit once per line.

    python tools/unit_cost.py [--reps 40] [--shapes mgqp,C1,C2,C3] [--out profiles/unit/unit_cost.log]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "motion-generation-using-quadratic-programs_amd"))

MALL_BYTES = 256 << 20
# name -> (n, p, m, QPs per launch)
SHAPES = {"mgqp": (14, 10, 28, 65536), "C1": (7, 6, 14, 65536), "C2": (7, 0, 14, 65536), "C3": (30, 6, 60, 65536)}
OUTS = ("x", "f", "status", "iters", "x_eq", "f_eq", "status_eq")


def rolled_sets(torch, make, base, keys, R, B):
    sets = [base]
    for r in range(1, R):
        db = make()  # a shell: its tensors are replaced below
        db.batch = B
        for k in keys:
            setattr(db, k, torch.roll(getattr(base, k), shifts=r * (B // R), dims=0).contiguous())
        sets.append(db)
    for db in sets:
        for k, like in zip(OUTS, ("x", "f", "status", "status", "x", "f", "status")):
            setattr(db, k, torch.zeros_like(getattr(base, like)))
    return sets


def main():
    import torch

    import qpgpu

    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=40, help="timed launches per entry, shape and mode")
    ap.add_argument("--warm-ms", type=float, default=300.0)
    ap.add_argument("--shapes", default="mgqp,C1,C2,C3")
    ap.add_argument("--g0-scales", default="0,10")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda", 0)
    lines = []
    for name in args.shapes.split(","):
        n, p, m, B = SHAPES[name]
        for g0_scale in [float(v) for v in args.g0_scales.split(",")]:
            up = qpgpu.make_unit_problems(n, p, m, 0, B, seed=2026, g0_scale=g0_scale)
            one = up.slice(0, 1)
            sets_of = lambda per_qp: max(2, -(-2 * MALL_BYTES // (per_qp * B)) + 1)
            Rd = sets_of(qpgpu.algorithmic_bytes_per_qp(n, p, m))
            Ru = sets_of(qpgpu.algorithmic_bytes_per_qp_unit(n, p, m))
            dense = rolled_sets(torch, lambda: qpgpu.DeviceBatch(one.to_dense(), dev),
                                qpgpu.DeviceBatch(up.to_dense(), dev), ("G", "g0", "CE", "ce0", "CI", "ci0"), Rd, B)
            unit = rolled_sets(torch, lambda: qpgpu.DeviceUnitBatch(one, dev), qpgpu.DeviceUnitBatch(up, dev),
                               ("g0", "CE", "ce0", "CI", "ci0"), Ru, B)
            s = torch.cuda.current_stream(dev)

            def launch(is_unit, q):
                if is_unit:
                    unit[q % Ru].solve(stream=s, eq=True)
                else:
                    d = dense[q % Rd]
                    d.solve(stream=s, exact=True, eq_out=(d.x_eq, d.f_eq, d.status_eq))

            t0, q = time.perf_counter(), 0
            while q < 8 or (time.perf_counter() - t0) * 1e3 < args.warm_ms:
                launch(q & 1, q)
                q += 1
                if q % 4 == 0:
                    torch.cuda.synchronize()
            torch.cuda.synchronize()
            ms = {0: [], 1: []}
            for k in range(2 * args.reps):
                is_unit = k & 1
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(s)
                launch(is_unit, q)
                e1.record(s)
                q += 1
                e1.synchronize()
                ms[is_unit].append(e0.elapsed_time(e1))
            # the same bits from both entries (set 0 of each holds the QPs in the same order)
            launch(0, 0)
            launch(1, 0)
            torch.cuda.synchronize()
            bits = lambda t: t.view(torch.int64) if t.dtype == torch.float64 else t
            same = all(bool(torch.equal(bits(getattr(dense[0], k)), bits(getattr(unit[0], k)))) for k in OUTS)
            st = lambda v: {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}
            rec = {"shape": name, "n": n, "p": p, "m": m, "batch": B, "g0_scale": g0_scale,
                   "dense_input_sets": Rd, "unit_input_sets": Ru, "reps": args.reps,
                   "dense_kernel": qpgpu.LIB.qpgpu_kernel_name_flags(n, p, m, qpgpu.FLAG_EXACT).decode(),
                   "unit_kernel": qpgpu.kernel_name_unit(n, p, m),
                   "dense_bytes_per_qp": qpgpu.algorithmic_bytes_per_qp(n, p, m),
                   "unit_bytes_per_qp": qpgpu.algorithmic_bytes_per_qp_unit(n, p, m),
                   "dense_ms": st(ms[0]), "unit_ms": st(ms[1]),
                   "unit_over_dense": float(np.median(ms[1]) / np.median(ms[0])),
                   "bitwise_equal": same, "ok_qps": int((unit[0].status == 0).sum().item()),
                   "mean_l1_passes": float(unit[0].iters.float().mean().item()),
                   "dense_raw_ms": [round(v, 4) for v in ms[0]], "unit_raw_ms": [round(v, 4) for v in ms[1]]}
            lines.append(json.dumps(rec))
            print(lines[-1], flush=True)
            del dense, unit
            torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
