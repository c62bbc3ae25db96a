"""Cases and CPU reference for qpgpu_solve_batched_box (TEST INFRASTRUCTURE ONLY).

The reference of every case is the unmodified oracle (oracle/oracle.py) on BoxProblems.to_dense(),
the dense problem the entry is defined as, under the C-ABI's default step cap.  rollbacks() counts,
per QP, how often that solve takes the degenerate rollback (a full step whose add_constraint finds
the new column dependent): for that alone a variant of oracle/qp_oracle.c with a counter at that
site is built into a temporary directory at first use, as tests/dual_ref.py does for its hook;
oracle/ itself is not modified and the variant's results are not used as a reference.

No case uses hi = -inf, lo = +inf or NaN bounds, and none overflows: those leave the finite-data
condition of include/qpgpu.h under which the box entry equals the dense one bit for bit.
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

import oracle
import qpgpu

HERE = os.path.dirname(os.path.abspath(__file__))
ORACLE_DIR = os.path.join(os.path.dirname(HERE), "oracle")

# (n, p, B) per family: the smallest shapes at which each kernel can still go wrong.  B = 130, 70
# and 65 cross a 64-QP tile.
SHAPES = {
    "lane": [(7, 0, 130), (7, 3, 130), (8, 0, 65), (8, 8, 3), (1, 0, 5), (5, 2, 70)],
    "subgroup": [(14, 10, 100), (16, 0, 70), (9, 1, 65)],
    "wave_lds": [(30, 6, 64), (33, 0, 20), (64, 0, 8)],
    "wave_ws": [(65, 0, 3), (100, 5, 3), (256, 0, 2)],
    "generic": [(260, 0, 2)],
}
# data modes, each on these shapes
MODE_SHAPES = [(7, 3, 70), (14, 10, 66), (30, 6, 16)]
MODES = ("long", "rand", "crossed", "equal", "inf", "ints", "dupce", "indef", "scaled_ce")


def default_cap(n: int, p: int) -> int:
    """The C-ABI's default step cap for the dense problem (qpgpu_api.cpp default_max_steps)."""
    return 1000 + 100 * (n + p + 2 * n)


def g0_scale(n: int) -> float:
    """The generator's unconstrained minimiser shrinks like 1/n (G = M^T M + n I against
    g0 ~ 10 N(0, 1)), so unit bounds would bind nowhere at large n: g0 grows with n so that they
    do on every shape (test_box_cpu.py asserts it)."""
    return max(1.0, n / 4.0)


def _base(n, p, B, seed):
    bp = qpgpu.make_box_problems(n, p, 0, B, seed=seed)
    bp.g0 *= g0_scale(n)
    return bp


def _mode(mode, n, p, B):
    bp = _base(n, p, B, seed=1000 + n)
    rng = np.random.default_rng([n, p, MODES.index(mode)])
    if mode == "long":  # unit bounds, many strongly violated: long active-set paths
        bp.g0 *= 30.0
    elif mode == "rand":
        bp.hi = rng.uniform(0.05, 1.5, (B, n))
        bp.lo = -rng.uniform(0.05, 1.5, (B, n))
    elif mode == "crossed":  # lo > hi on one variable of every other QP: infeasible
        v = rng.integers(n, size=B)
        for b in range(0, B, 2):
            bp.hi[b, v[b]], bp.lo[b, v[b]] = -0.5, 0.5
    elif mode == "equal":  # lo = hi on two variables
        for b in range(B):
            for v in rng.choice(n, size=2, replace=False):
                bp.hi[b, v] = bp.lo[b, v] = rng.uniform(-0.5, 0.5)
    elif mode == "inf":  # absent bounds
        bp.hi[rng.random((B, n)) < 0.4] = np.inf
        bp.lo[rng.random((B, n)) < 0.4] = -np.inf
    elif mode == "ints":  # small integers everywhere: exact ties in every selection
        M = rng.integers(-2, 3, (B, n, n)).astype(float)
        bp.G = np.einsum("bki,bkj->bij", M, M) + n * np.eye(n)[None]
        bp.g0 = rng.integers(-40, 41, (B, n)).astype(float)
        bp.CE = rng.integers(-1, 2, (B, n, p)).astype(float)
        bp.ce0 = rng.integers(-1, 2, (B, p)).astype(float)
        bp.hi = rng.integers(0, 3, (B, n)).astype(float)
        bp.lo = -rng.integers(0, 3, (B, n)).astype(float)
    elif mode == "dupce":  # a duplicated CE column on every third QP: dependent
        bp.CE[::3, :, p - 1] = bp.CE[::3, :, 0]
        bp.ce0[::3, p - 1] = bp.ce0[::3, 0]
    elif mode == "indef":  # an indefinite G on every third QP
        bp.G[::3, n // 2, n // 2] = -1.0
    elif mode == "scaled_ce":
        # the last equality scaled so that eps * R_norm reaches the size of a bound's column: some
        # full steps' add_constraint report it dependent and roll back.  (The reference then never
        # leaves its loop — ss is not reset — so those QPs end at the step cap.)
        bp.CE[:, :, p - 1] *= 1e15
        bp.ce0[:, p - 1] *= 1e15
    else:
        raise ValueError(mode)
    return bp


@functools.lru_cache(maxsize=None)
def cases() -> dict:
    """id -> BoxProblems."""
    out = {}
    for fam, shapes in SHAPES.items():
        for n, p, B in shapes:
            out[f"{fam}_{n}_{p}"] = _base(n, p, B, seed=500 + n + p)
    for n, p, B in MODE_SHAPES:
        for mode in MODES:
            out[f"{mode}_{n}_{p}"] = _mode(mode, n, p, B)
    return out


def generator_cases() -> list:
    """ids of the multi-QP cases whose bounds are the generator's (unit) ones and whose bounds can
    bind: with p >= n the equalities alone determine x (the generator's feasible point,
    |x_f| ~ 0.1, inside the unit box), so on an OK QP no bound is ever active."""
    return [f"{fam}_{n}_{p}" for fam, shapes in SHAPES.items() for n, p, B in shapes if B > 1 and p < n] + \
           [f"long_{n}_{p}" for n, p, _ in MODE_SHAPES]


def case(cid: str):
    return cases()[cid]


@functools.lru_cache(maxsize=None)
def dense(cid: str):
    return case(cid).to_dense()


@functools.lru_cache(maxsize=None)
def reference(cid: str, max_steps: int = 0):
    """(x, f, status, iters) of the oracle on the materialised problem under the default cap (or
    max_steps), computed once; the arrays are shared between tests and must be left unchanged."""
    bp = case(cid)
    res = oracle.solve_batch(dense(cid), max_steps=max_steps or default_cap(bp.n, bp.p))
    for a in res:
        a.setflags(write=False)
    return res


# ---- the rollback counter ------------------------------------------------------------------------
ANCHOR = "      iaexcl[ip] = 0;\n"
_variant = None


def _makefile_var(name: str) -> list:
    txt = open(os.path.join(ORACLE_DIR, "Makefile")).read()
    mt = re.search(rf"^{name}\s*\??=\s*(.*)$", txt, re.M)
    assert mt, f"oracle/Makefile has no {name}"
    return mt.group(1).split()


def _build():
    global _variant
    if _variant is not None:
        return _variant
    src = open(os.path.join(ORACLE_DIR, "qp_oracle.c")).read()
    assert src.count(ANCHOR) == 1, "the rollback site of qpo_solve() must occur exactly once"
    out = tempfile.mkdtemp(prefix="box_ref_")
    atexit.register(shutil.rmtree, out, ignore_errors=True)
    c = os.path.join(out, "qp_oracle_rollback.c")
    with open(c, "w") as fh:
        fh.write("static int qpo_rollbacks;\n" + src.replace(ANCHOR, ANCHOR + "      qpo_rollbacks++;\n") +
                 "\nint qpo_take_rollbacks(void) {\n  int r = qpo_rollbacks;\n  qpo_rollbacks = 0;\n  return r;\n}\n")
    so = os.path.join(out, "liboracle_qp_rollback.so")
    cc = os.environ.get("CC") or _makefile_var("CC")[0]
    subprocess.check_call([cc, *_makefile_var("CFLAGS"), "-Wno-maybe-uninitialized", "-iquote", ORACLE_DIR,
                           "-shared", "-o", so, c, "-lm", "-lpthread"])
    L = ctypes.CDLL(so)
    L.qpo_solve.argtypes = [ctypes.c_int] * 3 + [ctypes.c_void_p] * 9 + [ctypes.c_int]
    L.qpo_solve.restype = ctypes.c_int
    L.qpo_take_rollbacks.restype = ctypes.c_int
    _variant = L
    return L


def rollbacks(cid: str) -> np.ndarray:
    """Per QP of the case, the number of degenerate rollbacks the reference's solve takes."""
    L = _build()
    pr = dense(cid)
    B, n, p, m = pr.batch, pr.n, pr.p, pr.m
    a = [np.ascontiguousarray(v, dtype=np.float64) for v in (pr.g0, pr.CE, pr.ce0, pr.CI, pr.ci0)]
    G = np.array(pr.G, dtype=np.float64, order="C", copy=True)
    x, f, it = np.zeros((B, n)), np.zeros(B), np.zeros(B, dtype=np.int32)
    P = lambda v, off: ctypes.c_void_p(v.ctypes.data + off)
    out = np.zeros(B, dtype=np.int64)
    L.qpo_take_rollbacks()
    for b in range(B):
        L.qpo_solve(n, p, m, P(G, b * n * n * 8), P(a[0], b * n * 8), P(a[1], b * n * p * 8), P(a[2], b * p * 8),
                    P(a[3], b * n * m * 8), P(a[4], b * m * 8), P(x, b * n * 8), P(f, b * 8), P(it, b * 4),
                    default_cap(n, p))
        out[b] = L.qpo_take_rollbacks()
    return out
