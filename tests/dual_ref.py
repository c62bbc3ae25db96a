"""CPU reference for the multipliers of qpgpu_solve_batched_dual (TEST INFRASTRUCTURE ONLY).

At import this builds, into a temporary directory, a variant of oracle/qp_oracle.c with an export
hook inserted at the `done:` label of qpo_solve(): the function's own u[0..iq), A[0..iq), iq, p and
status, scattered dense exactly as include/qpgpu.h defines the output —
    u_out[j]      j < p   entry k with A[k] == -j-1 (equality j)
    u_out[p + i]  i < m   entry k >= p with A[k] == i (inequality i)
every other slot +0.0, nact = iq - p; for any status but QPGPU_QP_OK the whole block +0.0 and
nact = 0.  oracle/ itself is not modified; the flags are those of oracle/Makefile.  Nothing else
of the restatement changes (tests/test_dual_cpu.py checks x, f, status and iters bit for bit
against the unmodified oracle on every case used).

Also the case lists the CPU and GPU dual tests share, and the KKT measures of DESIGN §3.5.
"""
from __future__ import annotations

import atexit
import ctypes
import functools
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np

import qp_cases
import qpgpu

HERE = os.path.dirname(os.path.abspath(__file__))
ORACLE_DIR = os.path.join(os.path.dirname(HERE), "oracle")

ANCHOR = "done:\n  *iters = iter;\n"
HOOK = """done:
  if (qpo_dual_u || qpo_dual_nact) {
    int na_ = 0;
    if (qpo_dual_u)
      for (int k_ = 0; k_ < mp; k_++) qpo_dual_u[k_] = 0.0;
    if (status == QPGPU_QP_OK) {
      if (qpo_dual_u)
        for (int k_ = 0; k_ < iq; k_++) qpo_dual_u[A[k_] < 0 ? -A[k_] - 1 : p + A[k_]] = u[k_];
      na_ = iq - p;
    }
    if (qpo_dual_nact) *qpo_dual_nact = na_;
  }
  *iters = iter;
"""
PROLOGUE = "static double *qpo_dual_u;\nstatic int *qpo_dual_nact;\n"
EPILOGUE = "\nvoid qpo_dual_target(double *u, int *nact) {\n  qpo_dual_u = u;\n  qpo_dual_nact = nact;\n}\n"


def _makefile_var(name: str) -> list:
    txt = open(os.path.join(ORACLE_DIR, "Makefile")).read()
    mt = re.search(rf"^{name}\s*\??=\s*(.*)$", txt, re.M)
    assert mt, f"oracle/Makefile has no {name}"
    return mt.group(1).split()


def _build() -> ctypes.CDLL:
    src = open(os.path.join(ORACLE_DIR, "qp_oracle.c")).read()
    assert src.count(ANCHOR) == 1, "the `done:` anchor of qpo_solve() must occur exactly once"
    out = tempfile.mkdtemp(prefix="dual_ref_")
    atexit.register(shutil.rmtree, out, ignore_errors=True)
    c = os.path.join(out, "qp_oracle_dual.c")
    with open(c, "w") as fh:
        fh.write(PROLOGUE + src.replace(ANCHOR, HOOK) + EPILOGUE)
    so = os.path.join(out, "liboracle_qp_dual.so")
    cc = os.environ.get("CC") or _makefile_var("CC")[0]
    # (-iquote: the source's "../include/qpgpu.h" resolves against oracle/ as in place)
    subprocess.check_call([cc, *_makefile_var("CFLAGS"), "-Wno-maybe-uninitialized", "-iquote", ORACLE_DIR,
                           "-shared", "-o", so, c, "-lm", "-lpthread"])
    L = ctypes.CDLL(so)
    vp = ctypes.c_void_p
    L.qpo_solve.argtypes = [ctypes.c_int] * 3 + [vp] * 9 + [ctypes.c_int]
    L.qpo_solve.restype = ctypes.c_int
    L.qpo_dual_target.argtypes = [vp, vp]
    L.qpo_dual_target.restype = None
    return L


LIB = _build()


def default_cap(n: int, p: int, m: int) -> int:
    """The C-ABI's default step cap (qpgpu_api.cpp default_max_steps)."""
    return 1000 + 100 * (n + p + m)


def solve(pr, max_steps: int = 0):
    """The variant on a qpgpu.Problems batch, one QP at a time: (x, f, status, iters, u, nact),
    u of shape (B, p + m).  max_steps as oracle.solve_batch (0 = no cap)."""
    B, n, p, m = pr.batch, pr.n, pr.p, pr.m
    a = [np.ascontiguousarray(v, dtype=np.float64) for v in (pr.g0, pr.CE, pr.ce0, pr.CI, pr.ci0)]
    G = np.array(pr.G, dtype=np.float64, order="C", copy=True)  # overwritten with the factor
    x = np.zeros((B, n))
    f = np.zeros(B)
    st = np.zeros(B, dtype=np.int32)
    it = np.zeros(B, dtype=np.int32)
    u = np.full((B, p + m), np.nan)
    nact = np.full(B, -7, dtype=np.int32)
    P = lambda v, off: ctypes.c_void_p(v.ctypes.data + off)
    try:
        for b in range(B):
            LIB.qpo_dual_target(P(u, b * (p + m) * 8), P(nact, b * 4))
            st[b] = LIB.qpo_solve(n, p, m, P(G, b * n * n * 8), P(a[0], b * n * 8), P(a[1], b * n * p * 8),
                                  P(a[2], b * p * 8), P(a[3], b * n * m * 8), P(a[4], b * m * 8),
                                  P(x, b * n * 8), P(f, b * 8), P(it, b * 4), max_steps)
    finally:
        LIB.qpo_dual_target(None, None)
    return x, f, st, it, u, nact


# ---- cases -------------------------------------------------------------------------------------
# the GPU bitwise list: (id, kind, n, p, m, B)
GPU_SHAPES = [
    ("lane_7_6_14", "general", 7, 6, 14, 200),  # partial last wave
    ("lane_box_7_0_14", "box", 7, 0, 14, 64),
    ("lane_8_0_16", "general", 8, 0, 16, 64),
    ("subgroup_14_10_28", "general", 14, 10, 28, 64),
    ("subgroup_16_3_64", "general", 16, 3, 64, 64),
    ("subgroup_5_2_30", "general", 5, 2, 30, 64),
    ("wave_17_3_40", "general", 17, 3, 40, 16),
    ("wave_30_6_60", "general", 30, 6, 60, 16),
    ("wave_64_0_128", "general", 64, 0, 128, 4),
    ("ws_65_2_130", "general", 65, 2, 130, 3),
    ("ws_100_20_200", "general", 100, 20, 200, 2),
    ("ws_8_2_257", "general", 8, 2, 257, 4),
    ("generic_4_0_1025", "general", 4, 0, 1025, 4),
    ("degenerate_1_0_2", "general", 1, 0, 2, 5),
    ("degenerate_3_0_0", "general", 3, 0, 0, 5),
    ("degenerate_4_4_0", "general", 4, 4, 0, 5),
]
FUZZ_SEEDS = [(s, False) for s in range(12)] + [(s, True) for s in range(4)]


def _truncate(pr, B):
    return pr if pr.batch <= B else pr.slice(0, B)


@functools.lru_cache(maxsize=None)
def gpu_cases() -> dict:
    """id -> Problems: the shapes above and every qp_cases.edge_cases() batch."""
    out = {cid: qp_cases.make(kind, n, p, m, B, seed=77) for cid, kind, n, p, m, B in GPU_SHAPES}
    for name, pr in qp_cases.edge_cases():
        out["edge_" + name] = pr
    return out


@functools.lru_cache(maxsize=None)
def fuzz_cases() -> dict:
    out = {}
    for seed, large in FUZZ_SEEDS:
        pr, _ = qp_cases.fuzz_case(seed, large=large)
        out[f"fuzz_{'large_' if large else ''}{seed}"] = _truncate(pr, 4 if large else 32)
    return out


@functools.lru_cache(maxsize=None)
def kkt_cases() -> dict:
    """The well-posed list the KKT conditions are asserted on."""
    out = {}
    for name, kind, n, p, m in qp_cases.CONFIGS:
        out[name] = qp_cases.make(kind, n, p, m, 8 if n == 30 else 64)
    for name, pr in qp_cases.edge_cases():
        out["edge_" + name] = pr
    for name, kind, n, p, m, _ in qp_cases.LARGE_CONFIGS:
        if n <= 100:
            out[name] = qp_cases.make(kind, n, p, m, 2, seed=11)
    for n, p, m in ((65, 2, 130), (4, 0, 1025), (9, 2, 20)):
        out[f"general_{n}_{p}_{m}"] = qp_cases.make("general", n, p, m, 2, seed=11)
    return out


def case(cid: str):
    for d in (gpu_cases(), fuzz_cases(), kkt_cases()):
        if cid in d:
            return d[cid]
    raise KeyError(cid)


@functools.lru_cache(maxsize=None)
def reference(cid: str, max_steps: int = 0):
    """solve() of a named case under the C-ABI's default cap (or max_steps), computed once; the
    arrays are shared between tests and must be left unchanged."""
    pr = case(cid)
    res = solve(pr, max_steps or default_cap(pr.n, pr.p, pr.m))
    for a in res:
        a.setflags(write=False)
    return res


# ---- KKT measures ------------------------------------------------------------------------------
def kkt_measures(pr, x, st, u):
    """Over the status-OK QPs with finite x: (max scaled stationarity residual
    ||G x + g0 - CE ue - CI ui||_inf / || |G||x| + |g0| + |CE||ue| + |CI||ui| ||_inf,
    max complementarity |s_i| / (|CI[:,i]|^T |x| + |ci0[i]|) over the constraints with u != 0,
    min u[p:], QPs counted)."""
    p = pr.p
    stat = comp = 0.0
    umin = 0.0
    cnt = 0
    for b in range(pr.batch):
        if st[b] != qpgpu.QP_OK or not np.all(np.isfinite(x[b])):
            continue
        cnt += 1
        ue, ui = u[b, :p], u[b, p:]
        G, g0, CE, CI, ci0 = pr.G[b], pr.g0[b], pr.CE[b], pr.CI[b], pr.ci0[b]
        with np.errstate(invalid="ignore", over="ignore"):
            r = G @ x[b] + g0 - CE @ ue - CI @ ui
            sc = np.abs(G) @ np.abs(x[b]) + np.abs(g0) + np.abs(CE) @ np.abs(ue) + np.abs(CI) @ np.abs(ui)
            den = float(np.max(sc))
            q = float(np.max(np.abs(r))) / den if den > 0 else float(np.max(np.abs(r)))
            stat = max(stat, q) if q == q else float("inf")
            on = ui != 0
            if on.any():
                s = CI.T @ x[b] + ci0
                d = np.abs(CI).T @ np.abs(x[b]) + np.abs(ci0)
                c = float(np.max(np.abs(s[on]) / d[on]))
                comp = max(comp, c) if c == c else float("inf")
        if ui.size:
            umin = min(umin, float(ui.min()))
    return stat, comp, umin, cnt
