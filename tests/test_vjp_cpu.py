"""qpgpu_vjp without a device: the export surface, the argument rules, and the definition
(tests/vjp_ref.py) on the CPU reference's own primal-dual pairs — against one dense solve of the KKT
system, against central differences of the reference solver's x, the box form against the dense one,
and the special values.

Bars (each 100 x the worst value measured with the reference alone, under its cap; the rounding of
the restatement grows with cond(G) * cond(M^T M), which the case lists do not pin):
  vs the dense KKT solve   worst 4.4e-12 of the largest gradient entry  -> KKT_MAX = 4.4e-10 (cap 1e-8)
  vs central differences   worst 3.2e-9 of the directional derivative   -> FD_MAX  = 3.2e-7 (cap 1e-4)
"""
import ctypes
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import box_dual_ref
import box_ref
import dual_ref
import qp_cases
import qpgpu
import vjp_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("qpgpu_vjp", "qpgpu_vjp_box", "qpgpu_kernel_name_vjp")
KKT_MAX = 4.4e-10
FD_MAX = 3.2e-7
FD_CASES = ("lane_7_6_14", "lane_box_7_0_14", "lane_8_0_16", "subgroup_14_10_28", "wave_30_6_60",
            "wave_64_0_128", "degenerate_3_0_0", "degenerate_4_4_0", "subgroup_5_2_30")
FD_QPS = 6
FD_H = 1e-6


def test_symbols_declared_listed_and_exported():
    hdr = open(os.path.join(ROOT, "include", "qpgpu.h")).read()
    out = subprocess.check_output(["nm", "-D", "--defined-only", qpgpu.LIB_PATH]).decode()
    for name in NEW_SYMBOLS:
        assert re.search(rf"\b{name}\s*\(", hdr), f"{name} is not declared in include/qpgpu.h"
        assert name in qpgpu.EXPORTED_SYMBOLS
        assert re.search(rf"\bT {name}$", out, flags=re.M), f"{name} is not exported by libqpgpu.so"
    assert qpgpu.LIB.qpgpu_abi_version() == 1


def test_kernel_names():
    for n in range(1, 9):
        assert "lane" in qpgpu.kernel_name_vjp(n, 0, 2 * n) and "group" not in qpgpu.kernel_name_vjp(n, 0, 2 * n)
    for n in (9, 16, 17, 32, 33, 64):
        assert "group" in qpgpu.kernel_name_vjp(n, 2, 20) and "lane" not in qpgpu.kernel_name_vjp(n, 2, 20)
    assert len({qpgpu.kernel_name_vjp(n) for n in (16, 32, 64)}) == 3
    for n in (65, 256, 0, -1):
        assert qpgpu.kernel_name_vjp(n, 0, 0) == ""


def test_argument_rules_without_a_device():
    """The C entries with NULL arrays: every rule checked here is decided before any array is read
    (and before anything is launched: no call below reaches the device)."""
    buf = (ctypes.c_double * 64)()
    some = ctypes.cast(buf, ctypes.c_void_p)

    def call(box, n, p, m, batch, flags=0, u=None, rest=None, **named):
        d = qpgpu.ProblemDesc(n, p, m, 0, batch, flags, 0)
        names = ["G", "CE"] + ([] if box else ["CI"]) + ["x", "u", "status", "gx"]
        args = {k: rest for k in names}
        args.update(u=u, status=None)
        args.update(named)
        fn = qpgpu.LIB.qpgpu_vjp_box if box else qpgpu.LIB.qpgpu_vjp
        return fn(ctypes.byref(d), *[args[k] for k in names], *([rest] * 6), None)

    inv, uns = qpgpu.ERR_INVALID_ARGUMENT, qpgpu.ERR_UNSUPPORTED_SHAPE
    for box in (False, True):
        assert call(box, 7, 0, 14, 0, u=some) == qpgpu.SUCCESS  # batch = 0
        assert call(box, 7, 0, 14, 0, flags=qpgpu.FLAG_EXACT, u=some) == inv  # non-zero flags
        assert call(box, 7, 0, 14, 0, flags=qpgpu.FLAG_FORCE_GENERIC, u=some) == inv
        assert call(box, 7, 0, 14, 0) == inv  # NULL u with p + m > 0
        assert call(box, 7, 0, 14, 4, u=some) == inv  # NULL G, x, gx
        for missing in ("G", "x", "gx"):
            assert call(box, 7, 2, 14, 4, u=some, rest=some, **{missing: None}) == inv
        assert call(box, 7, 2, 14, 4, u=some, rest=some, CE=None) == inv  # NULL CE with p > 0
        assert call(box, 64, 0, 128, 0, u=some) == qpgpu.SUCCESS
        assert call(box, 65, 0, 130, 0, u=some) == uns  # n > 64
        assert call(box, 65, 0, 130, 4, u=some, rest=some) == uns
        assert call(box, 65, 0, 130, 0) == inv  # ... and the argument rules come first
    assert call(False, 7, 0, 14, 4, u=some, rest=some, CI=None) == inv  # NULL CI with m > 0
    assert call(True, 7, 0, 13, 0, u=some) == inv  # box with m != 2n
    assert call(False, 7, 0, 13, 0, u=some) == qpgpu.SUCCESS
    assert call(False, 3, 0, 0, 0) == qpgpu.SUCCESS  # p + m == 0: u may be NULL
    assert call(False, 300, 0, 0, 0) == uns


# ---- the definition on the reference's own pairs ---------------------------------------------------
def _rel_per_qp(got: dict, want: dict) -> np.ndarray:
    """Per QP: the largest difference over all six gradients, relative to the largest entry of `want`."""
    B = next(iter(want.values())).shape[0]
    num, den = np.zeros(B), np.zeros(B)
    for k, w in want.items():
        if w.size:
            num = np.maximum(num, np.max(np.abs(got[k] - w).reshape(B, -1), axis=1))
            den = np.maximum(den, np.max(np.abs(w).reshape(B, -1), axis=1))
    return num / den


KKT_CASES = sorted(c for c, pr in dual_ref.kkt_cases().items() if pr.n <= 64)


@pytest.mark.parametrize("cid", KKT_CASES)
def test_restatement_vs_dense_kkt_solve(cid):
    """Measured worst over the list: 4.380e-12 (edge_scaled_dup_ineq; C1_general_7_6_14 2.0e-12,
    general_4_4_0 2.5e-12)."""
    pr = dual_ref.case(cid)
    x, f, st, it, u, nact = dual_ref.reference(cid)
    ok = (st == qpgpu.QP_OK) & np.all(np.isfinite(x), axis=1)
    if not ok.any():
        return
    sub = qpgpu.Problems(pr.n, pr.p, pr.m, *[np.asarray(a)[ok] for a in pr.arrays()])
    gx = vjp_ref.make_gx(pr)[ok]
    got = vjp_ref.vjp(sub, x[ok], u[ok], gx)
    want = vjp_ref.dense_kkt(sub, x[ok], u[ok], gx)
    rel = _rel_per_qp(got, want)
    print(f"{cid}: {int(ok.sum())} QPs, worst relative difference to the dense KKT solve {rel.max():.3e}")
    assert np.all(rel <= KKT_MAX), f"{cid}: {rel.max():.3e}"


def _direction(pr, rng):
    D = [rng.standard_normal(np.asarray(a).shape) for a in pr.arrays()]
    D[0] = 0.5 * (D[0] + np.swapaxes(D[0], 1, 2))  # G stays symmetric
    return D


@pytest.mark.parametrize("cid", FD_CASES)
def test_restatement_vs_central_differences(cid):
    """Measured worst over the nine cases: 3.116e-9 (subgroup_5_2_30); no QP's active set changed under
    the perturbation."""
    full = dual_ref.case(cid)
    B = min(FD_QPS, full.batch)
    pr = full.slice(0, B)
    cap = dual_ref.default_cap(pr.n, pr.p, pr.m)
    x, f, st, it, u, nact = [a[:B] for a in dual_ref.reference(cid)]
    assert np.all(st == qpgpu.QP_OK)
    assert np.array_equal((u[:, pr.p:] != 0).sum(axis=1), nact)  # "active" as u != 0 is the solver's set
    rng = np.random.default_rng([pr.n, pr.p, pr.m, 31])
    gx = rng.standard_normal((B, pr.n))
    D = _direction(pr, rng)
    grads = vjp_ref.vjp(pr, x, u, gx, st)
    an = sum(np.sum((grads[k] * d).reshape(B, -1), axis=1) for k, d in zip(vjp_ref.DENSE_OUTPUTS, D))
    side = []
    for sgn in (+1.0, -1.0):
        q = qpgpu.Problems(pr.n, pr.p, pr.m, *[np.asarray(a) + sgn * FD_H * d for a, d in zip(pr.arrays(), D)])
        xs, _, ss, _, us, _ = dual_ref.solve(q, cap)
        side.append((xs, (ss == qpgpu.QP_OK) & np.all((us != 0) == (u != 0), axis=1)))
    keep = side[0][1] & side[1][1]
    assert (~keep).sum() <= B // 8, f"{cid}: the active set changed on {int((~keep).sum())} of {B} QPs"
    fd = np.sum(gx * (side[0][0] - side[1][0]), axis=1) / (2 * FD_H)
    rel = np.abs(fd - an)[keep] / np.maximum(np.abs(fd), np.abs(an))[keep]
    print(f"{cid}: {int(keep.sum())} QPs, worst relative error of the directional derivative {rel.max():.3e}")
    assert np.all(rel <= FD_MAX), f"{cid}: {rel.max():.3e}"


@pytest.mark.parametrize("cid", sorted(box_ref.cases()))
def test_box_form_equals_dense_form(cid):
    bp = box_ref.case(cid)
    n = bp.n
    x, f, st, it, u, nact = box_dual_ref.reference(cid)
    gx = vjp_ref.make_gx(bp)
    for status in (st, None):
        gb = vjp_ref.vjp_box(bp, x, u, gx, status)
        gd = vjp_ref.vjp(box_ref.dense(cid), x, u, gx, status)
        want = {k: gd[k] for k in ("dG", "dg0", "dCE", "dce0")}
        want["dhi"] = gd["dci0"][:, :n]
        # ci0[n + k] = -lo[k]: dlo = -dci0 on a lower bound of W, and +0.0 (not -0.0) off it
        on = gd["dci0"][:, n:].view(np.uint64) != 0
        want["dlo"] = np.where(on, -gd["dci0"][:, n:], 0.0)
        assert not vjp_ref.mismatches(gb, want), f"{cid}: {vjp_ref.mismatches(gb, want)}"
        # dCI of the dense form is what the definition gives for those columns: nothing else to hold
        off = u[:, bp.p + n:] == 0
        assert not np.any(gb["dlo"][off & ~np.isnan(gb["dlo"])].view(np.uint64)), f"{cid}: dlo of an inactive bound"


# ---- structure ------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _grads(cid, masked=True):
    pr = dual_ref.case(cid)
    x, f, st, it, u, nact = dual_ref.reference(cid)
    return vjp_ref.vjp(pr, x, u, vjp_ref.make_gx(pr), st if masked else None)


@pytest.mark.parametrize("cid", ["lane_7_6_14", "subgroup_5_2_30", "wave_30_6_60"])
def test_structure_symmetry_and_zeros(cid):
    pr = dual_ref.case(cid)
    x, f, st, it, u, nact = dual_ref.reference(cid)
    g = _grads(cid)
    assert np.array_equal(g["dG"].view(np.uint64), np.swapaxes(g["dG"], 1, 2).copy().view(np.uint64))
    off = u[:, pr.p:] == 0
    assert off.any() and (~off).any()
    assert not np.any(g["dci0"][off].view(np.uint64))  # +0.0 exactly
    assert not np.any(np.swapaxes(g["dCI"], 1, 2)[off].view(np.uint64))
    assert np.all(g["dci0"][~off] != 0)


@pytest.mark.parametrize("cid", ["edge_infeasible", "edge_not_pd", "edge_dependent"])
def test_masked_qps_are_zero(cid):
    st = dual_ref.reference(cid)[2]
    assert np.all(st != qpgpu.QP_OK)
    for k, v in _grads(cid).items():
        assert not np.any(v.view(np.uint64)), f"{cid} {k}"


def test_more_working_columns_than_variables_is_nan():
    pr = qp_cases.make("general", 3, 0, 8, 2, seed=5)
    x = np.ones((2, 3))
    u = np.ones((2, 8))
    u[1, 3:] = 0.0  # QP 1: q = 3 = n, still defined
    g = vjp_ref.vjp(pr, x, u, vjp_ref.make_gx(pr))
    for k, v in g.items():
        assert np.all(np.isnan(v[0])), k
        assert not np.any(np.isnan(v[1])), k


def test_status_null_on_not_pd_gives_nan_from_the_arithmetic():
    g = _grads("edge_not_pd", masked=False)
    assert np.any(np.isnan(g["dg0"]))


def test_no_constraints_reduces_to_a_linear_solve():
    cid = "degenerate_3_0_0"
    pr = dual_ref.case(cid)
    x, f, st, it, u, nact = dual_ref.reference(cid)
    gx = vjp_ref.make_gx(pr)
    g = vjp_ref.vjp(pr, x, None, gx, st)
    a = np.stack([np.linalg.solve(pr.G[b], gx[b]) for b in range(pr.batch)])
    assert np.allclose(g["dg0"], -a, rtol=1e-12, atol=0)
    assert g["dCE"].size == g["dce0"].size == g["dCI"].size == g["dci0"].size == 0
