"""Kernel time of one qpgpu_jvp_many launch beside K qpgpu_jvp launches on the same directions.

For each shape (default: tools/jvp_cost.py's: C1 = 65 536 x (7, 6, 14), 65 536 x (8, 0, 16), mgqp =
65 536 x (14, 10, 28), C3 = 16 384 x (30, 6, 60) and 2 048 x (64, 0, 128)), each layout and each
K in {1, 4, n}, two things are launched in turn on one stream, each between its own HIP-event pair:
  (a) one qpgpu_jvp_many with K directions, all six tangents (standard normal) and all three outputs
      given, status given, on the (x, u, status) that qpgpu_solve_batched_dual left on the device;
  (b) K launches of qpgpu_jvp, launch k on direction k of the same tangents (a contiguous copy of
      slice k, made once), all three outputs given: one event pair round the K launches.
With --parent-lib PATH (b) is launched from that build of libqpgpu.so (the parent commit's) on the
same device arrays; without it, from the library under test, whose qpgpu_jvp kernels are the
parent's.  Inputs rotate over R resident sets (set r = set 0 rolled by r*B/R QPs, whole tiles, with
its own tangents) that together exceed twice the Infinity Cache, so every launch reads cold inputs,
and the order of the two alternates from one repetition to the next; untimed launches of both run
first.  After the timing, (a) and (b) on set 0 are compared bit for bit.  Prints one JSON line per
shape, layout and K: median / min / max ms of each and the ratio of the medians.

    python tools/jvp_many_cost.py [--reps 20] [--parent-lib PATH] [--out profiles/jvp_many/jvp_many_cost.log]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "motion-generation-using-quadratic-programs_amd"))

MALL_BYTES = 256 << 20
SHAPES = {"C1": (7, 6, 14, 65536), "C2": (8, 0, 16, 65536), "mgqp": (14, 10, 28, 65536),
          "C3": (30, 6, 60, 16384), "n64": (64, 0, 128, 2048)}
INPUTS = ("G", "g0", "CE", "ce0", "CI", "ci0")


def main():
    import torch

    import qpgpu

    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20, help="timed launches of each kind per shape, layout and K")
    ap.add_argument("--warm-ms", type=float, default=200.0)
    ap.add_argument("--shapes", default="C1,C2,mgqp,C3,n64")
    ap.add_argument("--layouts", default="qp_major,tiled64")
    ap.add_argument("--ks", default="1,4,n", help="direction counts; n stands for the shape's n")
    ap.add_argument("--parent-lib", default=None, help="a libqpgpu.so of the parent commit for (b)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda", 0)
    s = torch.cuda.current_stream(dev)
    old = qpgpu.LIB
    if args.parent_lib:  # its own copies of the library's internal symbols, not the loaded library's
        old = ctypes.CDLL(os.path.abspath(args.parent_lib), mode=os.RTLD_LOCAL | os.RTLD_NOW | os.RTLD_DEEPBIND)
        old.qpgpu_jvp.argtypes = [ctypes.POINTER(qpgpu.ProblemDesc)] + [ctypes.c_void_p] * 16
        old.qpgpu_jvp.restype = ctypes.c_int
    vp = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    stream = ctypes.c_void_p(s.cuda_stream)
    lines = []
    for name in args.shapes.split(","):
        n, p, m, B = SHAPES[name]
        E = {"G": n * n, "g0": n, "CE": n * p, "ce0": p, "CI": n * m, "ci0": m}
        pr = qpgpu.make_problems("general", n, p, m, 0, B, seed=2026)
        for layout in args.layouts.split(","):
            for ks in args.ks.split(","):
                K = n if ks == "n" else int(ks)
                in_bytes = 8 * (sum(E.values()) + K * (n * n + n * p)) * B
                R = max(2, -(-2 * MALL_BYTES // in_bytes) + 1)
                base = qpgpu.DeviceBatch(pr, dev, with_iters=False, layout=layout)
                tiled = base.layout == qpgpu.LAYOUT_TILED64
                sets = []
                for r in range(R):
                    if r == 0:
                        db = base
                    else:
                        db = qpgpu.DeviceBatch(pr.slice(0, 1), dev, with_iters=False, layout=layout)  # a shell
                        db.batch = B
                        q0 = r * (B // R) // 64 * 64
                        for k in INPUTS:
                            t = getattr(base, k)
                            setattr(db, k, torch.roll(t.reshape(-1), shifts=q0 * E[k], dims=0).reshape(t.shape).contiguous())
                        for k in ("x", "f", "status"):
                            setattr(db, k, torch.zeros_like(getattr(base, k)))
                    rows = db.x.shape[0]
                    db.u = torch.zeros((rows, p + m), dtype=torch.float64, device=dev)
                    db.tan = {k: torch.randn((rows, K * E[k]), dtype=torch.float64, device=dev) for k in INPUTS if E[k]}
                    if tiled:  # direction d of a tile: elements [d E, (d + 1) E) of its K E
                        cut = lambda t, e, d: t.reshape(rows // 64, K * e, 64)[:, d * e:(d + 1) * e].contiguous().reshape(rows, e)
                    else:
                        cut = lambda t, e, d: t.reshape(rows, K, e)[:, d].contiguous()
                    db.tan1 = [{k: cut(t, E[k], d) for k, t in db.tan.items()} for d in range(K)]
                    db.sens = {"tx": torch.empty((rows, K * n), dtype=torch.float64, device=dev),
                               "tu": torch.empty((rows, K * (p + m)), dtype=torch.float64, device=dev),
                               "tf": torch.empty((rows, K), dtype=torch.float64, device=dev)}
                    db.sens1 = [{"tx": torch.empty((rows, n), dtype=torch.float64, device=dev),
                                 "tu": torch.empty((rows, p + m), dtype=torch.float64, device=dev),
                                 "tf": torch.empty(B, dtype=torch.float64, device=dev)} for d in range(K)]
                    db.d = qpgpu.ProblemDesc(n, p, m, 0, B, 0, db.layout)
                    db.solve_args = ([ctypes.byref(db.d)] + [vp(getattr(db, k)) for k in INPUTS]
                                     + [vp(db.x), vp(db.f), vp(db.status), None, vp(db.u), None, stream])
                    db.jvp_args = [[ctypes.byref(db.d)] + [vp(t) for t in (db.G, db.CE, db.CI, db.x, db.u, db.status)]
                                   + [vp(db.tan1[d].get(k)) for k in INPUTS]
                                   + [vp(db.sens1[d][k]) for k in ("tx", "tu", "tf")] + [stream] for d in range(K)]
                    sets.append(db)

                def many(q):
                    db = sets[q % R]
                    db.jvp_many(db.u, db.tan, K, outs=db.sens, stream=s)

                def singles(q):
                    for a in sets[q % R].jvp_args:
                        rc = old.qpgpu_jvp(*a)
                        assert rc == 0, rc

                def timed(fn, q):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(s)
                    fn(q)
                    e1.record(s)
                    e1.synchronize()
                    return e0.elapsed_time(e1)

                for db in sets:  # every set's (x, u, status)
                    rc = qpgpu.LIB.qpgpu_solve_batched_dual(*db.solve_args)
                    assert rc == 0, rc
                torch.cuda.synchronize()
                kinds = {"many": many, "singles": singles}
                t0, q = time.perf_counter(), 0
                while q < 4 or (time.perf_counter() - t0) * 1e3 < args.warm_ms:
                    for fn in kinds.values():
                        fn(q)
                    q += 1
                    torch.cuda.synchronize()
                ms = {k: [] for k in kinds}
                order = list(kinds.items())
                for k in range(args.reps):
                    for name_, fn in order:  # every launch on the next input set: cold inputs for each kind
                        q += 1
                        ms[name_].append(timed(fn, q))
                    order = order[1:] + order[:1]  # and neither kind always behind the other
                st = lambda v: {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}
                many(0)
                singles(0)
                torch.cuda.synchronize()
                db = sets[0]
                got = db.jvp_many_rows(db.sens, K)
                same = True
                for d in range(K):
                    one = db.jvp_rows(db.sens1[d])
                    same = same and all(np.array_equal(got[k][:, d].view(np.uint64), one[k].view(np.uint64)) for k in one)
                ok = (db.status == 0).cpu().numpy()
                med = {k: float(np.median(v)) for k, v in ms.items()}
                rec = {"shape": name, "n": n, "p": p, "m": m, "batch": B, "layout": layout, "K": K, "input_sets": R,
                       "reps": args.reps, "many_kernel": qpgpu.kernel_name_jvp_many(n, p, m),
                       "jvp_kernel": qpgpu.kernel_name_jvp(n, p, m), "parent_lib": args.parent_lib,
                       **{k + "_ms": st(v) for k, v in ms.items()},
                       "many_over_singles": med["many"] / med["singles"],
                       "many_ms_per_direction": med["many"] / K, "ok_qps": int(ok.sum()),
                       "bit_equal_to_singles": bool(same),
                       **{k + "_raw_ms": [round(v, 4) for v in vs] for k, vs in ms.items()}}
                lines.append(json.dumps(rec))
                print(lines[-1], flush=True)
                del sets, base, db
                torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
