"""Kernel time of qpgpu_jvp beside the backward step and the dual solve of the same QPs.

For each shape (default: C1 = 65 536 x (7, 6, 14), 65 536 x (8, 0, 16), mgqp = 65 536 x (14, 10, 28),
C3 = 16 384 x (30, 6, 60) and 2 048 x (64, 0, 128)) and each layout, three things are launched in
turn on one stream, each between its own HIP-event pair:
  (a) qpgpu_jvp with all six tangents (standard normal) and all three outputs given, status given,
      on the (x, u, status) that qpgpu_solve_batched_dual left on the device;
  (b) qpgpu_vjp_full with gu and gf given and all six gradients requested;
  (c) qpgpu_solve_batched_dual of the same QPs.
With --parent-lib PATH (b) and (c) are launched from that build of libqpgpu.so (the parent commit's)
on the same device arrays; without it, from the library under test, whose kernels for them are the
parent's.  Inputs rotate over R resident sets (set r = set 0 rolled by r*B/R QPs, whole tiles) that
together exceed twice the Infinity Cache, so every launch reads cold inputs, and the order of the
three rotates from one repetition to the next; untimed launches of all three run first.  Prints one
JSON line per shape and layout: median / min / max ms of each, the ratios of the medians, and the
bytes the forward-mode entry moves (read: G, tG, CE, tCE, x, u, tg0, tce0, status, the working
columns of CI and tCI and their tci0 entries; written: tx, tu, tf).

    python tools/jvp_cost.py [--reps 20] [--parent-lib PATH] [--out profiles/jvp_cost/jvp_cost.log]
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
    ap.add_argument("--reps", type=int, default=20, help="timed launches of each kind per shape and layout")
    ap.add_argument("--warm-ms", type=float, default=200.0)
    ap.add_argument("--shapes", default="C1,C2,mgqp,C3,n64")
    ap.add_argument("--layouts", default="qp_major,tiled64")
    ap.add_argument("--parent-lib", default=None, help="a libqpgpu.so of the parent commit for (b) and (c)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda", 0)
    s = torch.cuda.current_stream(dev)
    old = qpgpu.LIB
    if args.parent_lib:  # its own copies of the library's internal symbols, not the loaded library's
        old = ctypes.CDLL(os.path.abspath(args.parent_lib), mode=os.RTLD_LOCAL | os.RTLD_NOW | os.RTLD_DEEPBIND)
        old.qpgpu_solve_batched_dual.argtypes = [ctypes.POINTER(qpgpu.ProblemDesc)] + [ctypes.c_void_p] * 13
        old.qpgpu_vjp_full.argtypes = ([ctypes.POINTER(qpgpu.ProblemDesc)] + [ctypes.c_void_p] * 15
                                       + [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p])
        old.qpgpu_solve_batched_dual.restype = old.qpgpu_vjp_full.restype = ctypes.c_int
    vp = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    lines = []
    for name in args.shapes.split(","):
        n, p, m, B = SHAPES[name]
        E = {"G": n * n, "g0": n, "CE": n * p, "ce0": p, "CI": n * m, "ci0": m}
        pr = qpgpu.make_problems("general", n, p, m, 0, B, seed=2026)
        in_bytes = 8 * (sum(E.values()) + n * n + n * p) * B
        R = max(2, -(-2 * MALL_BYTES // in_bytes) + 1)
        for layout in args.layouts.split(","):
            base = qpgpu.DeviceBatch(pr, dev, with_iters=False, layout=layout)
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
                db.tan = {k: torch.randn((rows, E[k]), dtype=torch.float64, device=dev) for k in INPUTS if E[k]}
                db.sens = {"tx": torch.empty((rows, n), dtype=torch.float64, device=dev),
                           "tu": torch.empty((rows, p + m), dtype=torch.float64, device=dev),
                           "tf": torch.empty(B, dtype=torch.float64, device=dev)}
                db.gx = torch.randn((rows, n), dtype=torch.float64, device=dev)
                db.gu = torch.randn((rows, p + m), dtype=torch.float64, device=dev)
                db.gf = torch.randn(B, dtype=torch.float64, device=dev)
                db.grads = {k: torch.empty((rows, db._vjp_elems(k)), dtype=torch.float64, device=dev)
                            for k in db._VJP_OUTPUTS}
                db.d = qpgpu.ProblemDesc(n, p, m, 0, B, 0, db.layout)
                stream = ctypes.c_void_p(s.cuda_stream)
                db.solve_args = ([ctypes.byref(db.d)] + [vp(getattr(db, k)) for k in INPUTS]
                                 + [vp(db.x), vp(db.f), vp(db.status), None, vp(db.u), None, stream])
                db.vjp_args = ([ctypes.byref(db.d)] + [vp(t) for t in (db.G, db.CE, db.CI, db.x, db.u, db.status, db.gx,
                                                                      db.gu, db.gf)]
                               + [vp(db.grads[k]) for k in db._VJP_OUTPUTS] + [None, 0, stream])
                sets.append(db)

            def solve(q):
                rc = old.qpgpu_solve_batched_dual(*sets[q % R].solve_args)
                assert rc == 0, rc

            def vjp_full(q):
                rc = old.qpgpu_vjp_full(*sets[q % R].vjp_args)
                assert rc == 0, rc

            def jvp(q):
                db = sets[q % R]
                db.jvp(db.u, db.tan, outs=db.sens, stream=s)

            def timed(fn, q):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(s)
                fn(q)
                e1.record(s)
                e1.synchronize()
                return e0.elapsed_time(e1)

            for q in range(R):  # every set's (x, u, status)
                solve(q)
            torch.cuda.synchronize()
            kinds = {"jvp": jvp, "vjp_full": vjp_full, "dual_solve": solve}
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
                order = order[1:] + order[:1]  # and no kind always behind the same other
            st = lambda v: {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}
            db = sets[0]
            jvp(0)
            torch.cuda.synchronize()
            uh = db.u.cpu().numpy().reshape(-1)
            uh = qpgpu.from_tiled64(uh, B, (p + m,)) if layout == "tiled64" else uh.reshape(-1, p + m)[:B]
            ok = (db.status == 0).cpu().numpy()
            nact = int((uh[:, p:] != 0).sum(axis=1)[ok].sum())
            read = 8 * B * (2 * n * n + 2 * n * p + n + (p + m) + n + p) + 4 * B + 8 * (2 * n + 1) * nact
            written = 8 * B * (n + p + m + 1)
            out = db.jvp_rows(db.sens)
            med = {k: float(np.median(v)) for k, v in ms.items()}
            rec = {"shape": name, "n": n, "p": p, "m": m, "batch": B, "layout": layout, "input_sets": R,
                   "reps": args.reps, "jvp_kernel": qpgpu.kernel_name_jvp(n, p, m),
                   "vjp_full_kernel": qpgpu.kernel_name_vjp_full(n, p, m), "solve_kernel": qpgpu.kernel_name(n, p, m),
                   "parent_lib": args.parent_lib, **{k + "_ms": st(v) for k, v in ms.items()},
                   "jvp_over_vjp_full": med["jvp"] / med["vjp_full"],
                   "jvp_over_dual_solve": med["jvp"] / med["dual_solve"],
                   "jvp_bytes_read": read, "jvp_bytes_written": written,
                   "jvp_GBps": (read + written) / (med["jvp"] * 1e-3) * 1e-9,
                   "ok_qps": int(ok.sum()), "mean_active_inequalities": nact / max(1, int(ok.sum())),
                   "all_finite": bool(all(np.all(np.isfinite(v[ok])) for v in out.values())),
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
