"""The cases of the backward step with a workspace, n > 64 (TEST INFRASTRUCTURE ONLY): what
tests/test_vjp_ws_cpu.py and tests/test_gpu_vjp_ws.py share.  Every pair (x, u) and status comes from
the CPU reference (tests/dual_ref.py, tests/box_dual_ref.py), every expected gradient from the
definition's restatement (tests/vjp_ref.py); each is computed once and left unchanged.

  ws_65_2_130, ws_100_20_200   dual_ref's own cases: the first shape past the on-chip kernels, and one
                                with n no multiple of the panels (q = 26..29 and 59..61)
  g_129_70_40                   q >= p = 70 > 64: S spans more than one wave of rows; n is two waves
                                plus one row
  c5_256_0_512                  BASELINE config C5's shape, the largest n (q = 149)
  nan_66_0_70                   three QPs, QP 1 with an indefinite G (status NOT_POSITIVE_DEFINITE);
                                the tests also set QP 0's u to ones: q = 70 > n
  free_66_0_0                   no constraint at all: q = 0, M is the column gx alone
  eq_256_256_0                  q = p = n = 256: M has n + 1 = 257 columns, one more than the workgroup
                                has lanes, and S is 256 x 256
  box: wave_ws_65_0, wave_ws_100_5, wave_ws_256_0 (box_ref's), upper and lower bounds active in every QP
"""
from __future__ import annotations

import functools

import numpy as np

import box_dual_ref
import box_ref
import dual_ref
import qp_cases
import qpgpu
import vjp_ref

DENSE_CASES = ("ws_65_2_130", "ws_100_20_200", "g_129_70_40", "c5_256_0_512")
NAN_CASE = "nan_66_0_70"
EDGE_CASES = ("free_66_0_0", "eq_256_256_0")  # beyond the issue's list: the ends of q
BOX_CASES = ("wave_ws_65_0", "wave_ws_100_5", "wave_ws_256_0")
_MADE = {"g_129_70_40": (129, 70, 40, 2, 565), "c5_256_0_512": (256, 0, 512, 1, 568), NAN_CASE: (66, 0, 70, 3, 9),
         "free_66_0_0": (66, 0, 0, 2, 571), "eq_256_256_0": (256, 256, 0, 1, 572)}


@functools.lru_cache(maxsize=None)
def pair(cid):
    """(problems, x, u, status, gx) of a dense case."""
    if cid in _MADE:
        n, p, m, B, seed = _MADE[cid]
        pr = qp_cases.make("general", n, p, m, B, seed=seed)
        if cid == NAN_CASE:
            pr.G[1, 33, 33] = -1.0
        x, f, st, it, u, nact = dual_ref.solve(pr, dual_ref.default_cap(n, p, m))
        if cid == NAN_CASE:
            assert list(st) == [qpgpu.QP_OK, qpgpu.QP_NOT_POSITIVE_DEFINITE, qpgpu.QP_OK]
            u = u.copy()
            u[0] = 1.0  # q = 70 > n = 66
    else:
        pr = dual_ref.case(cid)
        x, f, st, it, u, nact = dual_ref.reference(cid)
    for a in (x, u, st):
        a.setflags(write=False)
    return pr, x, u, st, vjp_ref.make_gx(pr)


@functools.lru_cache(maxsize=None)
def want(cid, masked):
    pr, x, u, st, gx = pair(cid)
    return vjp_ref.vjp(pr, x, u, gx, st if masked else None)


@functools.lru_cache(maxsize=None)
def box_pair(cid):
    bp = box_ref.case(cid)
    x, f, st, it, u, nact = box_dual_ref.reference(cid)
    return bp, x, u, st, vjp_ref.make_gx(bp)


@functools.lru_cache(maxsize=None)
def box_want(cid, masked):
    bp, x, u, st, gx = box_pair(cid)
    return vjp_ref.vjp_box(bp, x, u, gx, st if masked else None)


@functools.lru_cache(maxsize=None)
def box_dense_want(cid, masked):
    bp, x, u, st, gx = box_pair(cid)
    return vjp_ref.vjp(box_ref.dense(cid), x, u, gx, st if masked else None)


def box_as_dense(r, n):
    """A dense-form result on to_dense() mapped to the box entry's outputs."""
    on = r["dci0"][:, n:].view(np.uint64) != 0
    return {"dG": r["dG"], "dg0": r["dg0"], "dCE": r["dCE"], "dce0": r["dce0"],
            "dhi": r["dci0"][:, :n], "dlo": np.where(on, -r["dci0"][:, n:], 0.0)}


def assert_bits(got, ref, label):
    bad = vjp_ref.mismatches(got, ref)
    assert not bad, f"{label}: (output, index, got, definition) {bad}"
