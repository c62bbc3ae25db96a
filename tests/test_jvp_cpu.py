"""qpgpu_jvp without a device: the export surface, the argument rules, and the definition
(tests/jvp_ref.py) on the CPU reference's own primal-dual pairs — against one dense solve of the KKT
system, against the backward step's definition through the adjoint identity, against central
differences of the reference solver, the box form against the dense one, and the special values.

Bars (each 100 x the worst value measured with the restatement alone, under its cap; the rounding of
the restatement grows with cond(G) * cond(M^T M), which the case lists do not pin):
  vs the dense KKT solve   worst 3.5e-12 of the largest output entry      -> KKT_MAX = 3.5e-10 (cap 1e-8)
  adjoint identity         worst 3.2e-16 of the sum of the terms' sizes   -> ADJ_MAX = 3.2e-14 (cap 1e-10)
  vs central differences   tx 5.3e-9, tu 6.0e-9, tf 1.3e-8                -> FD_MAX  = 5.3e-7, 6.0e-7, 1.3e-6 (cap 1e-4)
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
import jvp_ref
import qp_cases
import qpgpu
import vjp_full_ref
from test_vjp_cpu import FD_CASES, FD_H, FD_QPS
from vjp_ref import same_bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("qpgpu_jvp", "qpgpu_jvp_box", "qpgpu_kernel_name_jvp")
KKT_MAX = 3.5e-10
ADJ_MAX = 3.2e-14
FD_MAX = {"tx": 5.3e-7, "tu": 6.0e-7, "tf": 1.3e-6}


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
        name = qpgpu.kernel_name_jvp(n, 0, 2 * n)
        assert "jvp" in name and "lane" in name and "group" not in name, (n, name)
    for n in (9, 16, 17, 32, 33, 64):
        name = qpgpu.kernel_name_jvp(n, 2, 20)
        assert "jvp" in name and "group" in name and "lane" not in name, (n, name)
    assert len({qpgpu.kernel_name_jvp(n) for n in range(1, 9)}) == 8
    assert len({qpgpu.kernel_name_jvp(n) for n in (16, 32, 64)}) == 3
    assert qpgpu.kernel_name_jvp(9) == qpgpu.kernel_name_jvp(16)
    assert qpgpu.kernel_name_jvp(17) == qpgpu.kernel_name_jvp(32)
    assert qpgpu.kernel_name_jvp(33) == qpgpu.kernel_name_jvp(64)
    for n in (65, 0, -1):
        assert qpgpu.kernel_name_jvp(n, 0, 0) == ""


def test_argument_rules_without_a_device():
    """The C entries with NULL arrays: every rule checked here is decided before any array is read
    (and before anything is launched: no call below reaches the device)."""
    buf = (ctypes.c_double * 64)()
    some = ctypes.cast(buf, ctypes.c_void_p)

    def call(box, n, p, m, batch, flags=0, u=None, rest=None, outs=None, layout=0, **named):
        d = qpgpu.ProblemDesc(n, p, m, 0, batch, flags, layout)
        names = ["G", "CE"] + ([] if box else ["CI"]) + ["x", "u", "status"]
        args = {k: rest for k in names}
        args.update(u=u, status=None)
        args.update(named)
        fn = qpgpu.LIB.qpgpu_jvp_box if box else qpgpu.LIB.qpgpu_jvp
        return fn(ctypes.byref(d), *[args[k] for k in names], *([rest] * 6), *([outs] * 3), None)

    inv, uns = qpgpu.ERR_INVALID_ARGUMENT, qpgpu.ERR_UNSUPPORTED_SHAPE
    for box in (False, True):
        assert call(box, 7, 0, 14, 0, u=some) == qpgpu.SUCCESS  # batch = 0
        assert call(box, 7, 0, 14, 0, flags=qpgpu.FLAG_EXACT, u=some) == inv  # non-zero flags
        assert call(box, 7, 0, 14, 0, flags=qpgpu.FLAG_FORCE_GENERIC, u=some) == inv
        assert call(box, 7, 0, 14, 0, layout=7, u=some) == inv  # unknown layout
        assert call(box, 7, 0, 14, 0) == inv  # NULL u with p + m > 0
        assert call(box, 7, 0, 14, 4, u=some) == inv  # NULL G, x
        for missing in ("G", "x"):
            assert call(box, 7, 2, 14, 4, u=some, rest=some, **{missing: None}) == inv
        assert call(box, 7, 2, 14, 4, u=some, rest=some, CE=None) == inv  # NULL CE with p > 0
        # every array given, every output NULL: success, and nothing is launched
        assert call(box, 7, 2, 14, 4, u=some, rest=some) == qpgpu.SUCCESS
        assert call(box, 64, 0, 128, 0, u=some) == qpgpu.SUCCESS
        assert call(box, 65, 0, 130, 0, u=some) == uns  # n > 64
        assert call(box, 65, 0, 130, 4, u=some, rest=some) == uns
        assert call(box, 65, 0, 130, 4, u=some, rest=some, outs=some) == uns
        # ... and the argument rules come first
        assert call(box, 65, 0, 130, 0) == inv
        assert call(box, 65, 0, 130, 0, flags=qpgpu.FLAG_EXACT, u=some) == inv
        assert call(box, 65, 0, 130, 4, u=some, rest=some, G=None) == inv
    assert call(False, 7, 0, 14, 4, u=some, rest=some, CI=None) == inv  # NULL CI with m > 0
    assert call(True, 7, 0, 13, 0, u=some) == inv  # box with m != 2n
    assert call(True, 65, 0, 13, 0, u=some) == inv  # ... before the shape rule
    assert call(False, 7, 0, 13, 0, u=some) == qpgpu.SUCCESS
    assert call(False, 3, 0, 0, 0) == qpgpu.SUCCESS  # p + m == 0: u may be NULL
    assert call(False, 300, 0, 0, 0) == uns
    assert qpgpu.LIB.qpgpu_jvp(None, *([some] * 15), None) == inv


# ---- the definition on the reference's own pairs ---------------------------------------------------
def _rel_per_qp(got: dict, want: dict) -> np.ndarray:
    """Per QP: the largest difference over tx, tu and tf, relative to the largest entry of `want`."""
    B = want["tf"].shape[0]
    num, den = np.zeros(B), np.zeros(B)
    for k, w in want.items():
        if w.size:
            num = np.maximum(num, np.max(np.abs(got[k] - w).reshape(B, -1), axis=1))
            den = np.maximum(den, np.max(np.abs(w).reshape(B, -1), axis=1))
    return num / den


KKT_CASES = sorted(c for c, pr in dual_ref.kkt_cases().items() if pr.n <= 64)


def _ok_subset(cid):
    pr = dual_ref.case(cid)
    x, f, st, it, u, nact = dual_ref.reference(cid)
    ok = (st == qpgpu.QP_OK) & np.all(np.isfinite(x), axis=1)
    sub = qpgpu.Problems(pr.n, pr.p, pr.m, *[np.asarray(a)[ok] for a in pr.arrays()])
    tan = {k: v[ok] for k, v in jvp_ref.make_tangents(pr).items()}
    return ok, sub, x[ok], u[ok], tan


@pytest.mark.parametrize("cid", KKT_CASES)
def test_restatement_vs_dense_kkt_solve(cid):
    """Measured worst over the list: 3.421e-12 (general_4_4_0; edge_scaled_dup_ineq 2.2e-12,
    C1_general_7_6_14 2.0e-12)."""
    ok, sub, x, u, tan = _ok_subset(cid)
    if not ok.any():
        return
    got = jvp_ref.jvp(sub, x, u, tan)
    want = jvp_ref.dense_kkt(sub, x, u, tan)
    rel = _rel_per_qp(got, want)
    print(f"{cid}: {int(ok.sum())} QPs, worst relative difference to the dense KKT solve {rel.max():.3e}")
    assert np.all(rel <= KKT_MAX), f"{cid}: {rel.max():.3e}"


@pytest.mark.parametrize("cid", ["C1_general_7_6_14", "general_9_2_20", "edge_scaled_dup_ineq"])
def test_each_tangent_alone_adds_up(cid):
    """The entry is linear in the tangent: the six single-tangent calls add up to the call with all
    six, to the KKT bar.  The measure's denominator is the largest entry among the parts and the
    whole, since the parts may cancel in the sum (each part carries its own rounding)."""
    ok, sub, x, u, tan = _ok_subset(cid)
    whole = jvp_ref.jvp(sub, x, u, tan)
    parts = [jvp_ref.jvp(sub, x, u, {k: v}) for k, v in tan.items()]
    B = sub.batch
    worst = 0.0
    den = np.zeros(B)
    for k in whole:
        for part in parts + [whole]:
            den = np.maximum(den, np.max(np.abs(part[k]).reshape(B, -1), axis=1))
    for k in whole:
        diff = np.max(np.abs(sum(part[k] for part in parts) - whole[k]).reshape(B, -1), axis=1)
        worst = max(worst, float(np.max(diff / den)))
    print(f"{cid}: single tangents vs all six, worst {worst:.3e}")
    assert worst <= KKT_MAX, f"{cid}: {worst:.3e}"


def _fd_pair(cid):
    full = dual_ref.case(cid)
    B = min(FD_QPS, full.batch)
    pr = full.slice(0, B)
    x, f, st, it, u, nact = [a[:B] for a in dual_ref.reference(cid)]
    assert np.all(st == qpgpu.QP_OK)
    return pr, x, f, st, u


@pytest.mark.parametrize("cid", FD_CASES)
def test_adjoint_identity_with_the_backward_step(cid):
    """<gx, tx> + <gu, tu> + gf tf against <grad theta, t theta> over the six arrays, the gradients from
    tests/vjp_full_ref.py.  Measured worst over the nine cases: 3.166e-16 (degenerate_4_4_0) of the
    sum of the magnitudes of all terms."""
    pr, x, f, st, u = _fd_pair(cid)
    B = pr.batch
    rng = np.random.default_rng([pr.n, pr.p, pr.m, 41])
    gx, gu, gf = rng.standard_normal((B, pr.n)), rng.standard_normal((B, pr.p + pr.m)), rng.standard_normal(B)
    tan = jvp_ref.make_tangents(pr)
    t = jvp_ref.jvp(pr, x, u if pr.p + pr.m else None, tan, st)
    grads = vjp_full_ref.vjp_full(pr, x, u if pr.p + pr.m else None, gx, gu, gf, st)
    inW = np.ones((B, pr.p + pr.m), dtype=bool)
    inW[:, pr.p:] = u[:, pr.p:] != 0
    terms = [gx * t["tx"], np.where(inW, gu * t["tu"], 0.0), (gf * t["tf"])[:, None]]
    lhs = sum(a.sum(axis=1) for a in terms)
    size = sum(np.abs(a).sum(axis=1) for a in terms)
    rhs = np.zeros(B)
    for k, name in zip(vjp_full_ref.DENSE_OUTPUTS, jvp_ref.DENSE_TANGENTS):
        prod = (grads[k] * tan[name]).reshape(B, -1)
        rhs = rhs + prod.sum(axis=1)
        size = size + np.abs(prod).sum(axis=1)
    rel = np.abs(lhs - rhs) / size
    print(f"{cid}: {B} QPs, adjoint identity worst {rel.max():.3e}")
    assert np.all(rel <= ADJ_MAX), f"{cid}: {rel.max():.3e}"


@pytest.mark.parametrize("cid", FD_CASES)
def test_restatement_vs_central_differences(cid):
    """Measured worst over the nine cases: tx 5.202e-9 (lane_box_7_0_14), tu 5.940e-9 (lane_7_6_14),
    tf 1.266e-8 (wave_64_0_128); no QP was dropped: no active set changed under the perturbation."""
    pr, x, f, st, u = _fd_pair(cid)
    B = pr.batch
    cap = dual_ref.default_cap(pr.n, pr.p, pr.m)
    tan = jvp_ref.make_tangents(pr)
    t = jvp_ref.jvp(pr, x, u if pr.p + pr.m else None, tan, st)
    side = []
    for sgn in (+1.0, -1.0):
        q = qpgpu.Problems(pr.n, pr.p, pr.m, *[np.asarray(a) + sgn * FD_H * tan[k]
                                                for a, k in zip(pr.arrays(), jvp_ref.DENSE_TANGENTS)])
        xs, fs, ss, _, us, _ = dual_ref.solve(q, cap)
        side.append((xs, us, fs, (ss == qpgpu.QP_OK) & np.all((us != 0) == (u != 0), axis=1)))
    keep = side[0][3] & side[1][3]
    assert (~keep).sum() <= B // 8, f"{cid}: the active set changed on {int((~keep).sum())} of {B} QPs"
    fd = {k: (side[0][i] - side[1][i]) / (2 * FD_H) for i, k in enumerate(("tx", "tu", "tf"))}
    msg = []
    for k in ("tx", "tu", "tf"):
        if not t[k].size:
            continue
        if k == "tf":
            rel = np.abs(fd[k] - t[k]) / np.abs(t[k])
        else:  # (a QP with an empty W has tu = 0 on both sides: its difference must be 0 itself)
            diff, den = np.max(np.abs(fd[k] - t[k]), axis=1), np.max(np.abs(t[k]), axis=1)
            rel = np.where(den > 0, diff / np.where(den > 0, den, 1.0), np.where(diff == 0, 0.0, np.inf))
        rel = rel[keep]
        msg.append(f"{k} {rel.max():.3e}")
        assert np.all(rel <= FD_MAX[k]), f"{cid} {k}: {rel.max():.3e}"
    print(f"{cid}: {int(keep.sum())} QPs kept, worst relative error " + ", ".join(msg))


# ---- the box form ---------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", sorted(c for c, bp in box_ref.cases().items() if bp.n <= 64))
def test_box_form_equals_dense_form(cid):
    """Bit for bit, masked and not; on two cases also with thi, tlo or both NULL."""
    bp = box_ref.case(cid)
    x, f, st, it, u, nact = box_dual_ref.reference(cid)
    tan = jvp_ref.make_tangents(bp)
    for drop in ((), ("hi",), ("lo",), ("hi", "lo")) if cid in ("lane_7_3", "subgroup_9_1") else ((),):
        tn = {k: v for k, v in tan.items() if k not in drop}
        for status in (st, None):
            tb = jvp_ref.jvp_box(bp, x, u, tn, status)
            td = jvp_ref.jvp(box_ref.dense(cid), x, u, jvp_ref.box_tangents_as_dense(bp, tn), status)
            for k in jvp_ref.OUTPUTS:
                assert same_bits(tb[k], td[k]), f"{cid} without {drop} {k}"


# ---- structure ------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _sens(cid, masked=True):
    pr = dual_ref.case(cid)
    x, f, st, it, u, nact = dual_ref.reference(cid)
    return jvp_ref.jvp(pr, x, u, jvp_ref.make_tangents(pr), st if masked else None)


@pytest.mark.parametrize("cid", ["lane_7_6_14", "subgroup_5_2_30", "wave_30_6_60"])
def test_tu_is_zero_outside_w_and_tangents_there_never_enter(cid):
    pr = dual_ref.case(cid)
    x, f, st, it, u, nact = dual_ref.reference(cid)
    t = _sens(cid)
    off = u[:, pr.p:] == 0
    assert off.any() and (~off).any()
    assert not np.any(t["tu"][:, pr.p:][off].view(np.uint64))  # +0.0 exactly
    assert np.all(t["tu"][:, pr.p:][~off] != 0)
    tan = dict(jvp_ref.make_tangents(pr))
    tan["CI"] = tan["CI"].copy()
    tan["ci0"] = tan["ci0"].copy()
    np.swapaxes(tan["CI"], 1, 2)[off] = np.nan
    tan["ci0"][off] = np.nan
    assert np.isnan(tan["CI"]).any()
    poisoned = jvp_ref.jvp(pr, x, u, tan, st)
    for k in jvp_ref.OUTPUTS:
        assert same_bits(poisoned[k], t[k]), f"{cid} {k}: a tangent outside W entered the arithmetic"


@pytest.mark.parametrize("cid", ["edge_infeasible", "edge_not_pd", "edge_dependent"])
def test_masked_qps_are_zero(cid):
    st = dual_ref.reference(cid)[2]
    assert np.all(st != qpgpu.QP_OK)
    for k, v in _sens(cid).items():
        assert not np.any(v.view(np.uint64)), f"{cid} {k}"


def test_more_working_columns_than_variables_is_nan():
    pr = qp_cases.make("general", 3, 0, 8, 2, seed=5)
    x = np.ones((2, 3))
    u = np.ones((2, 8))
    u[1, 3:] = 0.0  # QP 1: q = 3 = n, still defined
    t = jvp_ref.jvp(pr, x, u, jvp_ref.make_tangents(pr))
    for k, v in t.items():
        assert np.all(np.isnan(v[0])), k
        assert not np.any(np.isnan(v[1])), k


def test_null_tangents_are_zero_tangents():
    """No tangent at all: tx = 0, tu = 0 on W, tf = 0 (k[t] = -(+0.0), so signed zeros are allowed)."""
    cid = "lane_7_6_14"
    pr = dual_ref.case(cid)
    x, f, st, it, u, nact = dual_ref.reference(cid)
    t = jvp_ref.jvp(pr, x, u, {}, st)
    for k, v in t.items():
        assert np.all(v == 0), k


def test_no_constraints_reduces_to_a_linear_solve():
    cid = "degenerate_3_0_0"
    pr = dual_ref.case(cid)
    x, f, st, it, u, nact = dual_ref.reference(cid)
    tan = jvp_ref.make_tangents(pr)
    t = jvp_ref.jvp(pr, x, None, tan, st)
    want = np.stack([-np.linalg.solve(pr.G[b], tan["G"][b] @ x[b] + tan["g0"][b]) for b in range(pr.batch)])
    assert np.allclose(t["tx"], want, rtol=1e-12, atol=0)
    assert t["tu"].size == 0
    tf = np.array([0.5 * x[b] @ tan["G"][b] @ x[b] + tan["g0"][b] @ x[b] for b in range(pr.batch)])
    assert np.allclose(t["tf"], tf, rtol=1e-12, atol=0)
