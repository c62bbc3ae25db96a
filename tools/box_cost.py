"""Kernel time of qpgpu_solve_batched_box against qpgpu_solve_batched (QPGPU_FLAG_EXACT) on the
materialised problem, same build, same QPs.

For each shape the two entries are launched alternately on one stream, each launch between its own
HIP-event pair, over resident input sets (set r = set 0 rolled by r*B/R QPs; R chosen per entry so
that its sets together exceed twice the Infinity Cache), so every launch reads cold inputs;
untimed launches of both entries run first until the clocks are steady.  The QPs are
qpgpu.make_box_problems(n, p, ...) — to_dense() of which is make_problems("box", n, p, 2n, ...),
the C2 benchmark's data — with g0 multiplied by --g0-scale (default 1).  Prints one JSON line per
shape: median / min / max kernel ms per launch for both entries and the ratio of the medians; the
results of the two entries are compared bit for bit once per shape.

    python tools/box_cost.py [--reps 40] [--shapes C2,mgqp,C3,C5] [--out profiles/box/box_cost.log]
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
# name -> (n, p, QPs per launch)
SHAPES = {"C2": (7, 0, 65536), "mgqp": (14, 10, 65536), "C3": (30, 6, 65536), "C5": (256, 0, 512)}


def rolled_sets(qpgpu, torch, make, base, keys, R, B):
    sets = [base]
    for r in range(1, R):
        db = make()  # a shell: its tensors are replaced below
        db.batch = B
        for k in keys:
            setattr(db, k, torch.roll(getattr(base, k), shifts=r * (B // R), dims=0).contiguous())
        for k in ("x", "f", "status", "iters"):
            setattr(db, k, torch.zeros_like(getattr(base, k)))
        sets.append(db)
    return sets


def main():
    import torch

    import qpgpu

    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=40, help="timed launches per entry and shape")
    ap.add_argument("--warm-ms", type=float, default=300.0)
    ap.add_argument("--shapes", default="C2,mgqp,C3,C5")
    ap.add_argument("--g0-scale", type=float, default=1.0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda", 0)
    lines = []
    for name in args.shapes.split(","):
        n, p, B = SHAPES[name]
        m = 2 * n
        bp = qpgpu.make_box_problems(n, p, 0, B, seed=2026)
        bp.g0 *= args.g0_scale
        one = bp.slice(0, 1)
        sets_of = lambda per_qp: max(2, -(-2 * MALL_BYTES // (per_qp * B)) + 1)
        Rd, Rb = sets_of(qpgpu.algorithmic_bytes_per_qp(n, p, m)), sets_of(qpgpu.algorithmic_bytes_per_qp_box(n, p))
        dense = rolled_sets(qpgpu, torch, lambda: qpgpu.DeviceBatch(one.to_dense(), dev),
                            qpgpu.DeviceBatch(bp.to_dense(), dev), ("G", "g0", "CE", "ce0", "CI", "ci0"), Rd, B)
        box = rolled_sets(qpgpu, torch, lambda: qpgpu.DeviceBoxBatch(one, dev), qpgpu.DeviceBoxBatch(bp, dev),
                          ("G", "g0", "CE", "ce0", "hi", "lo"), Rb, B)
        s = torch.cuda.current_stream(dev)

        def launch(is_box, q):
            if is_box:
                box[q % Rb].solve(stream=s)
            else:
                dense[q % Rd].solve(stream=s, exact=True)

        t0, q = time.perf_counter(), 0
        while q < 8 or (time.perf_counter() - t0) * 1e3 < args.warm_ms:
            launch(q & 1, q)
            q += 1
            if q % 4 == 0:
                torch.cuda.synchronize()
        torch.cuda.synchronize()
        ms = {0: [], 1: []}
        for k in range(2 * args.reps):
            is_box = k & 1
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            launch(is_box, q)
            e1.record(s)
            q += 1
            e1.synchronize()
            ms[is_box].append(e0.elapsed_time(e1))
        # the same bits from both entries (set 0 of each holds the QPs in the same order)
        launch(0, 0)
        launch(1, 0)
        torch.cuda.synchronize()
        same = all(bool(torch.equal(getattr(dense[0], k).view(torch.int64) if k in ("x", "f") else getattr(dense[0], k),
                                    getattr(box[0], k).view(torch.int64) if k in ("x", "f") else getattr(box[0], k)))
                   for k in ("x", "f", "status", "iters"))
        st = lambda v: {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}
        rec = {"shape": name, "n": n, "p": p, "m": m, "batch": B, "g0_scale": args.g0_scale,
               "dense_input_sets": Rd, "box_input_sets": Rb, "reps": args.reps,
               "dense_kernel": qpgpu.LIB.qpgpu_kernel_name_flags(n, p, m, qpgpu.FLAG_EXACT).decode(),
               "box_kernel": qpgpu.kernel_name_box(n, p),
               "dense_bytes_per_qp": qpgpu.algorithmic_bytes_per_qp(n, p, m),
               "box_bytes_per_qp": qpgpu.algorithmic_bytes_per_qp_box(n, p),
               "dense_ms": st(ms[0]), "box_ms": st(ms[1]),
               "box_over_dense": float(np.median(ms[1]) / np.median(ms[0])),
               "bitwise_equal": same, "ok_qps": int((box[0].status == 0).sum().item()),
               "mean_l1_passes": float(box[0].iters.float().mean().item()),
               "dense_raw_ms": [round(v, 4) for v in ms[0]], "box_raw_ms": [round(v, 4) for v in ms[1]]}
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
        del dense, box
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
