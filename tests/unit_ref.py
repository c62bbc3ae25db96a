"""Cases and CPU reference for qpgpu_solve_batched_unit (TEST INFRASTRUCTURE ONLY).

The reference of every case is the unmodified oracle (oracle/oracle.py) on UnitProblems.to_dense(),
the dense problem with a materialised G = I that the entry is defined as, under the C-ABI's
default step cap; the reference of the eq triple is the oracle on the same problem with m = 0.

No case has a non-finite or a -0.0 entry in g0: those leave the condition of include/qpgpu.h under
which the unit entry equals the dense one bit for bit (test_unit_cpu.py asserts it).
"""
from __future__ import annotations

import functools

import numpy as np

import oracle
import qpgpu

# (n, p, m, B) per family: the smallest shapes that still exercise each kernel's lane mapping,
# with B crossing a 64-QP tile where it can.  "subgroup_forced" shapes reach the subgroup kernel
# only when it is forced (the default order sends them to the wave kernel).
SHAPES = {
    "lane": [(7, 3, 14, 130), (8, 8, 16, 3), (1, 0, 2, 5), (5, 2, 9, 70), (7, 0, 0, 65), (4, 3, 8, 65)],
    "subgroup": [(8, 2, 32, 65), (6, 0, 20, 70)],
    "subgroup_forced": [(14, 10, 28, 100), (16, 0, 64, 70)],
    "wave": [(14, 10, 28, 66), (14, 1, 28, 66), (30, 6, 60, 16), (33, 0, 70, 20), (32, 20, 64, 8), (64, 0, 128, 4)],
}
# data modes, each on these shapes
MODE_SHAPES = [(7, 3, 14, 70), (14, 10, 28, 66), (30, 6, 60, 16)]
MODES = ("zero", "rand", "ints", "inf", "dupce", "scaled", "crossed", "dupexact")
FAMILIES = (None, "lane", "subgroup", "wave")


def covers(family, n: int, m: int) -> bool:
    """The shapes each family's unit kernels cover (include/qpgpu.h); the default order takes all."""
    if family == "lane":
        return n <= 8 and m <= 16
    if family == "subgroup":
        return n <= 16 and m <= 64
    return n <= 64 and m <= 256


def default_cap(n: int, p: int, m: int) -> int:
    """The C-ABI's default step cap (qpgpu_api.cpp default_max_steps)."""
    return 1000 + 100 * (n + p + m)


def _mode(mode, n, p, m, B):
    up = qpgpu.make_unit_problems(n, p, m, 0, B, seed=1000 + n, g0_scale=0.0 if mode == "zero" else 10.0)
    rng = np.random.default_rng([n, p, MODES.index(mode)])
    if mode in ("zero", "rand"):  # g0 = +0.0 (the reference's controller) / g0 ~ 10 N(0, 1)
        pass
    elif mode == "ints":  # small integers everywhere: exact ties in every selection
        up.g0 = rng.integers(-40, 41, (B, n)).astype(float)
        up.CE = rng.integers(-1, 2, (B, n, p)).astype(float)
        up.ce0 = rng.integers(-1, 2, (B, p)).astype(float)
        up.CI = rng.integers(-2, 3, (B, n, m)).astype(float)
        up.ci0 = rng.integers(0, 4, (B, m)).astype(float)
    elif mode == "inf":  # absent inequalities
        up.ci0[rng.random((B, m)) < 0.4] = np.inf
    elif mode == "dupce":
        # a duplicated CE column on every third QP.  The reference reports QPGPU_QP_DEPENDENT only
        # when the rounding noise of d = J^T np stays below eps * R_norm; duplicating the column
        # just before the last one gives the most such QPs of the choices tried (0 -> p-1,
        # 0 -> 1, p-2 -> p-1), the others end infeasible (test_unit_cpu.py holds the counts)
        up.CE[::3, :, p - 1] = up.CE[::3, :, p - 2]
        up.ce0[::3, p - 1] = up.ce0[::3, p - 2]
    elif mode == "dupexact":
        # equalities 0 and 1 of every third QP both 2 e_k: dependent in exact arithmetic.  With
        # J = I, d = J^T np is 2 e_k exactly, every Givens step on it has (cc, ss) = (0, 1) or is
        # skipped (h = 0), so J stays a signed permutation and the second copy's d[1:] is exactly
        # zero: the reference reports QPGPU_QP_DEPENDENT on every such QP whatever the shape
        k = rng.integers(n, size=B)
        for b in range(0, B, 3):
            up.CE[b, :, 0] = up.CE[b, :, 1] = 2.0 * np.eye(n)[k[b]]
            up.ce0[b, 1] = up.ce0[b, 0]
    elif mode == "scaled":  # the last equality scaled by 1e15
        up.CE[:, :, p - 1] *= 1e15
        up.ce0[:, p - 1] *= 1e15
    elif mode == "crossed":
        # on every other QP inequality 1 is the negation of inequality 0 with a gap of 1: no x
        # satisfies both, while the equalities alone have an answer (the controller's retry)
        up.CI[::2, :, 1] = -up.CI[::2, :, 0]
        up.ci0[::2, 1] = -up.ci0[::2, 0] - 1.0
    else:
        raise ValueError(mode)
    return up


@functools.lru_cache(maxsize=None)
def cases() -> dict:
    """id -> UnitProblems."""
    out = {}
    for fam, shapes in SHAPES.items():
        for n, p, m, B in shapes:
            out[f"{fam}_{n}_{p}_{m}"] = qpgpu.make_unit_problems(n, p, m, 0, B, seed=500 + n + p)
    for n, p, m, B in MODE_SHAPES:
        for mode in MODES:
            out[f"{mode}_{n}_{p}_{m}"] = _mode(mode, n, p, m, B)
    return out


def generator_cases() -> list:
    """ids of the cases whose data is the generator's own: every shape case and the zero and rand
    modes."""
    return [f"{fam}_{n}_{p}_{m}" for fam, shapes in SHAPES.items() for n, p, m, B in shapes] + \
           [f"{mode}_{n}_{p}_{m}" for n, p, m, _ in MODE_SHAPES for mode in ("zero", "rand")]


def case(cid: str):
    return cases()[cid]


@functools.lru_cache(maxsize=None)
def dense(cid: str):
    return case(cid).to_dense()


def _frozen(res):
    for a in res:
        a.setflags(write=False)
    return res


@functools.lru_cache(maxsize=None)
def reference(cid: str, max_steps: int = 0):
    """(x, f, status, iters) of the oracle on the materialised problem under the default cap (or
    max_steps), computed once; the arrays are shared between tests and must be left unchanged."""
    up = case(cid)
    return _frozen(oracle.solve_batch(dense(cid), max_steps=max_steps or default_cap(up.n, up.p, up.m)))


@functools.lru_cache(maxsize=None)
def reference_eq(cid: str):
    """(x_eq, f_eq, status_eq): the oracle on the same materialised problem with m = 0."""
    pr = dense(cid)
    B, n = pr.batch, pr.n
    eq = qpgpu.Problems(n, pr.p, 0, pr.G.copy(), pr.g0.copy(), pr.CE.copy(), pr.ce0.copy(),
                        np.zeros((B, n, 0)), np.zeros((B, 0)))
    return _frozen(oracle.solve_batch(eq, max_steps=default_cap(n, pr.p, pr.m))[:3])
