"""qpgpu_vjp_full / qpgpu_vjp_box_full without a device: the export surface, the kernel names, the
argument rules (those of tests/test_vjp_ws_cpu.py through the new entries, with NULL gu and gf), and
the definition's restatement (tests/vjp_full_ref.py) on the CPU reference's own primal-dual pairs —
bit for bit against tests/vjp_ref.py where no cotangent but gx is given, against one dense solve of
the KKT system with the envelope terms added, against central differences of the reference solver's
l = gx.x + gu.u + gf f, and the special values.

Bars, by the convention of tests/test_vjp_cpu.py (each 100 x the worst value measured with the
restatement alone, under that file's cap; the x-only figures on record there are 4.4e-12 and 3.2e-9):
  vs the dense KKT solve, gx, gu and gf given
      worst 3.413e-12 of the largest gradient entry (general_4_4_0)   -> KKT_MAX = 3.5e-10 (cap 1e-8)
  vs central differences, worst relative error of the directional derivative over the nine cases
      gu only 8.611e-9 (subgroup_14_10_28)   gf only 2.270e-8 (subgroup_5_2_30)
      gx only 3.166e-9 (subgroup_5_2_30)     all three 1.473e-8 (degenerate_4_4_0)
      worst of the four 2.270e-8                                      -> FD_MAX = 2.3e-6 (cap 1e-4)
  No QP's active set changed under the perturbation, in any case (asserted: B // 8 = 0 may be dropped).
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
import vjp_full_ref as F
import vjp_ref
from test_vjp_cpu import FD_CASES, FD_H, FD_QPS, KKT_CASES, _direction, _rel_per_qp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("qpgpu_vjp_full", "qpgpu_vjp_box_full", "qpgpu_kernel_name_vjp_full")
KKT_MAX = 3.5e-10
FD_MAX = 2.3e-6


def test_symbols_declared_listed_and_exported():
    hdr = open(os.path.join(ROOT, "include", "qpgpu.h")).read()
    out = subprocess.check_output(["nm", "-D", "--defined-only", qpgpu.LIB_PATH]).decode()
    for name in NEW_SYMBOLS:
        assert re.search(rf"\b{name}\s*\(", hdr), f"{name} is not declared in include/qpgpu.h"
        assert name in qpgpu.EXPORTED_SYMBOLS
        assert re.search(rf"\bT {name}$", out, flags=re.M), f"{name} is not exported by libqpgpu.so"
    assert qpgpu.LIB.qpgpu_abi_version() == 1


def test_kernel_names():
    for n in range(1, 257):
        name = qpgpu.kernel_name_vjp_full(n, 2, 2 * n)
        kind = "lane" if n <= 8 else "group" if n <= 64 else "ws"
        assert "full" in name and kind in name, (n, name)
        assert sum(k in name for k in ("lane", "group", "ws")) == 1, (n, name)
        assert name != qpgpu.kernel_name_vjp_ws(n, 2, 2 * n)  # its own build, not the x-only kernel
    assert len({qpgpu.kernel_name_vjp_full(n) for n in range(1, 9)}) == 8
    assert len({qpgpu.kernel_name_vjp_full(n) for n in (16, 32, 64)}) == 3
    for n in (257, 0, -1):
        assert qpgpu.kernel_name_vjp_full(n, 0, 0) == ""


def test_argument_rules_without_a_device():
    """The C entries with NULL or dummy arrays: every rule checked here is decided before any array is
    read and before anything is launched (no call below reaches the device).  Each rule holds with gu
    and gf given and with either NULL."""
    buf = (ctypes.c_double * 64)()
    some = ctypes.cast(buf, ctypes.c_void_p)
    per65 = 8 * (3 * 65 * 65 + 65)
    cot = [(some, some)]

    def call(box, n, p, m, batch, flags=0, u=None, rest=None, ws=some, ws_bytes=1 << 40, **named):
        d = qpgpu.ProblemDesc(n, p, m, 0, batch, flags, 0)
        names = ["G", "CE"] + ([] if box else ["CI"]) + ["x", "u", "status", "gx", "gu", "gf"]
        args = {k: rest for k in names}
        args.update(u=u, status=None, gu=cot[0][0], gf=cot[0][1])
        args.update(named)
        fn = qpgpu.LIB.qpgpu_vjp_box_full if box else qpgpu.LIB.qpgpu_vjp_full
        return fn(ctypes.byref(d), *[args[k] for k in names], *([rest] * 6), ws, ws_bytes, None)

    inv, uns = qpgpu.ERR_INVALID_ARGUMENT, qpgpu.ERR_UNSUPPORTED_SHAPE
    for cot[0] in ((some, some), (None, some), (some, None), (None, None)):
        for box in (False, True):
            for n in (7, 65):  # on both sides of the kernel boundary
                m = 2 * n
                assert call(box, n, 0, m, 0, u=some) == qpgpu.SUCCESS  # batch = 0
                assert call(box, n, 0, m, 0, u=some, ws=None, ws_bytes=0) == qpgpu.SUCCESS
                assert call(box, n, 0, m, 0, flags=qpgpu.FLAG_EXACT, u=some) == inv  # non-zero flags
                assert call(box, n, 0, m, 0, flags=qpgpu.FLAG_FORCE_GENERIC, u=some) == inv
                assert call(box, n, 0, m, 0) == inv  # NULL u with p + m > 0
                assert call(box, n, 0, m, 4, u=some) == inv  # NULL G, x, gx
                for missing in ("G", "x", "gx"):  # gx stays required
                    assert call(box, n, 2, m, 4, u=some, rest=some, **{missing: None}) == inv
                assert call(box, n, 2, m, 4, u=some, rest=some, CE=None) == inv  # NULL CE with p > 0
            assert call(box, 64, 0, 128, 0, u=some, ws=None, ws_bytes=0) == qpgpu.SUCCESS
            # n = 65, batch > 0: the workspace rules, after the rules above and before the device
            assert call(box, 65, 0, 130, 4, u=some, rest=some, ws=None, ws_bytes=0) == inv
            assert call(box, 65, 0, 130, 4, u=some, rest=some, ws=None) == inv
            assert call(box, 65, 0, 130, 4, u=some, rest=some, ws_bytes=per65 - 1) == inv  # one byte short of a slot
            assert call(box, 65, 0, 130, 4, u=some, rest=some, ws_bytes=0) == inv
            odd = ctypes.c_void_p(some.value + 4)
            assert call(box, 65, 0, 130, 4, u=some, rest=some, ws=odd) == inv  # not 8-byte aligned
            assert call(box, 65, 0, 130, 4, rest=some, ws=None) == inv  # (NULL u comes first: still invalid)
            # n > 256: unsupported, and the argument rules come first
            assert call(box, 257, 0, 514, 0, u=some) == uns
            assert call(box, 257, 0, 514, 4, u=some, rest=some) == uns
            assert call(box, 257, 0, 514, 4, u=some, rest=some, ws=None, ws_bytes=0) == uns
            assert call(box, 257, 0, 514, 0) == inv
            assert call(box, 257, 0, 514, 0, flags=qpgpu.FLAG_EXACT, u=some) == inv
        assert call(False, 7, 0, 14, 4, u=some, rest=some, CI=None) == inv  # NULL CI with m > 0
        assert call(False, 65, 0, 130, 4, u=some, rest=some, CI=None) == inv
        assert call(True, 7, 0, 13, 0, u=some) == inv  # box with m != 2n
        assert call(True, 65, 0, 129, 0, u=some) == inv
        assert call(False, 65, 0, 129, 0, u=some) == qpgpu.SUCCESS
        assert call(False, 66, 0, 0, 0) == qpgpu.SUCCESS  # p + m == 0: u may be NULL
        assert call(False, 300, 0, 0, 0) == uns
        assert call(False, 65, 0, (1 << 31) // 65 + 1, 0, u=some) == uns  # n * m reaches 2^31


def test_n_64_with_a_null_workspace_passes_the_rules():
    """n <= 64 is the launch without a workspace: NULL and 0 bytes are accepted.  The call is made with
    batch = 0 here (nothing may reach the device in this file); with batch > 0 it is every n <= 64
    case of tests/test_gpu_vjp_full.py."""
    d = qpgpu.ProblemDesc(64, 0, 128, 0, 0, 0, 0)
    buf = (ctypes.c_double * 8)()
    some = ctypes.cast(buf, ctypes.c_void_p)
    for gu, gf in ((some, some), (None, None)):
        rc = qpgpu.LIB.qpgpu_vjp_full(ctypes.byref(d), *([some] * 5), None, some, gu, gf, *([None] * 6), None, 0, None)
        assert rc == qpgpu.SUCCESS


# ---- the definition on the reference's own pairs ---------------------------------------------------
@pytest.mark.parametrize("cid", KKT_CASES)
def test_no_cotangent_but_gx_is_vjp_ref_bit_for_bit(cid):
    pr = dual_ref.case(cid)
    x, f, st, it, u, nact = dual_ref.reference(cid)
    gx = vjp_ref.make_gx(pr)
    for status in (st, None):
        got = F.vjp_full(pr, x, u if pr.p + pr.m else None, gx, None, None, status)
        want = vjp_ref.vjp(pr, x, u if pr.p + pr.m else None, gx, status)
        assert not vjp_ref.mismatches(got, want), f"{cid}: {vjp_ref.mismatches(got, want)}"


@pytest.mark.parametrize("cid", sorted(box_ref.cases()))
def test_no_cotangent_but_gx_is_vjp_ref_bit_for_bit_box(cid):
    bp = box_ref.case(cid)
    x, f, st, it, u, nact = box_dual_ref.reference(cid)
    gx = vjp_ref.make_gx(bp)
    for status in (st, None):
        got = F.vjp_box_full(bp, x, u, gx, None, None, status)
        want = vjp_ref.vjp_box(bp, x, u, gx, status)
        assert not vjp_ref.mismatches(got, want), f"{cid}: {vjp_ref.mismatches(got, want)}"


@pytest.mark.parametrize("cid", KKT_CASES)
def test_restatement_vs_dense_kkt_solve(cid):
    """Measured worst over the list: 3.413e-12 (general_4_4_0; C1_general_7_6_14 2.1e-12,
    edge_scaled_dup_ineq 1.8e-12)."""
    pr = dual_ref.case(cid)
    x, f, st, it, u, nact = dual_ref.reference(cid)
    ok = (st == qpgpu.QP_OK) & np.all(np.isfinite(x), axis=1)
    if not ok.any():
        return
    sub = qpgpu.Problems(pr.n, pr.p, pr.m, *[np.asarray(a)[ok] for a in pr.arrays()])
    gx = vjp_ref.make_gx(pr)[ok]
    gu, gf = F.make_cotangents(pr)
    gu, gf = gu[ok], gf[ok]
    got = F.vjp_full(sub, x[ok], u[ok], gx, gu, gf)
    want = F.dense_kkt(sub, x[ok], u[ok], gx, gu, gf)
    rel = _rel_per_qp(got, want)
    print(f"{cid}: {int(ok.sum())} QPs, worst relative difference to the dense KKT solve {rel.max():.3e}")
    assert np.all(rel <= KKT_MAX), f"{cid}: {rel.max():.3e}"


FD_VARIANTS = {"gu": (False, True, False), "gf": (False, False, True), "gx": (True, False, False),
               "all": (True, True, True)}


@functools.lru_cache(maxsize=None)
def _fd_sides(cid):
    """The nine cases' pairs, cotangents and the reference solver's answers at +-h D, computed once.
    gx and D are drawn first, from the sequence of tests/test_vjp_cpu.py: the perturbed problems are
    the ones that test solves.  gu and gf follow."""
    full = dual_ref.case(cid)
    B = min(FD_QPS, full.batch)
    pr = full.slice(0, B)
    cap = dual_ref.default_cap(pr.n, pr.p, pr.m)
    x, f, st, it, u, nact = [a[:B] for a in dual_ref.reference(cid)]
    assert np.all(st == qpgpu.QP_OK)
    assert np.array_equal((u[:, pr.p:] != 0).sum(axis=1), nact)
    rng = np.random.default_rng([pr.n, pr.p, pr.m, 31])
    gx = rng.standard_normal((B, pr.n))
    D = _direction(pr, rng)
    gu = rng.standard_normal((B, pr.p + pr.m))
    gf = rng.standard_normal(B)
    side = []
    for sgn in (+1.0, -1.0):
        q = qpgpu.Problems(pr.n, pr.p, pr.m, *[np.asarray(a) + sgn * FD_H * d for a, d in zip(pr.arrays(), D)])
        xs, fs, ss, _, us, _ = dual_ref.solve(q, cap)
        side.append((xs, us, fs, (ss == qpgpu.QP_OK) & np.all((us != 0) == (u != 0), axis=1)))
    return pr, x, u, st, gx, gu, gf, D, side


@pytest.mark.parametrize("variant", sorted(FD_VARIANTS))
@pytest.mark.parametrize("cid", FD_CASES)
def test_restatement_vs_central_differences(cid, variant):
    """l = gx.x + gu.u + gf f along a random direction of all six inputs, h = 1e-6.  Measured worst
    over the nine cases: gu 8.611e-9, gf 2.270e-8, gx 3.166e-9, all 1.473e-8; no QP's active set
    changed under the perturbation."""
    pr, x, u, st, gx, gu, gf, D, side = _fd_sides(cid)
    B = pr.batch
    use_x, use_u, use_f = FD_VARIANTS[variant]
    gxv = gx if use_x else np.zeros_like(gx)
    grads = F.vjp_full(pr, x, u, gxv, gu if use_u else None, gf if use_f else None, st)
    an = sum(np.sum((grads[k] * d).reshape(B, -1), axis=1) for k, d in zip(F.DENSE_OUTPUTS, D))
    keep = side[0][3] & side[1][3]
    assert (~keep).sum() <= B // 8, f"{cid}: the active set changed on {int((~keep).sum())} of {B} QPs"
    loss = lambda s: (np.sum(gxv * s[0], axis=1) + (np.sum(gu * s[1], axis=1) if use_u else 0.0)
                      + (gf * s[2] if use_f else 0.0))
    fd = (loss(side[0]) - loss(side[1])) / (2 * FD_H)
    # (a QP with no working constraint has u = 0 on both sides and no gradient through gu: 0 against 0)
    den = np.maximum(np.abs(fd), np.abs(an))
    rel = (np.abs(fd - an) / np.where(den == 0, 1.0, den))[keep]
    print(f"{cid} {variant}: {int(keep.sum())} QPs, worst relative error of the directional derivative {rel.max():.3e}")
    assert np.all(rel <= FD_MAX), f"{cid} {variant}: {rel.max():.3e}"


# ---- structure ------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", ["lane_7_6_14", "subgroup_5_2_30", "wave_30_6_60", "edge_infeasible"])
def test_gu_of_an_inequality_outside_w_never_enters(cid):
    """NaN at every gu position of an inequality whose multiplier is 0: the same bits everywhere."""
    pr = dual_ref.case(cid)
    x, f, st, it, u, nact = dual_ref.reference(cid)
    gx = vjp_ref.make_gx(pr)
    gu, gf = F.make_cotangents(pr)
    poisoned = gu.copy()
    off = np.zeros(u.shape, dtype=bool)
    off[:, pr.p:] = u[:, pr.p:] == 0
    poisoned[off] = np.nan
    if cid != "edge_infeasible":
        assert off.any() and (~off[:, pr.p:]).any()
    for status in (st, None):
        a = F.vjp_full(pr, x, u, gx, gu, gf, status)
        b = F.vjp_full(pr, x, u, gx, poisoned, gf, status)
        assert not vjp_ref.mismatches(b, a), f"{cid}: {vjp_ref.mismatches(b, a)}"


@pytest.mark.parametrize("cid", ["edge_infeasible", "edge_not_pd", "edge_dependent"])
def test_masked_qps_are_zero(cid):
    pr = dual_ref.case(cid)
    x, f, st, it, u, nact = dual_ref.reference(cid)
    assert np.all(st != qpgpu.QP_OK)
    gu, gf = F.make_cotangents(pr)
    for k, v in F.vjp_full(pr, x, u, vjp_ref.make_gx(pr), gu, gf, st).items():
        assert not np.any(v.view(np.uint64)), f"{cid} {k}"


def test_more_working_columns_than_variables_is_nan():
    pr = qp_cases.make("general", 3, 0, 8, 2, seed=5)
    x = np.ones((2, 3))
    u = np.ones((2, 8))
    u[1, 3:] = 0.0  # QP 1: q = 3 = n, still defined
    gu, gf = F.make_cotangents(pr)
    g = F.vjp_full(pr, x, u, vjp_ref.make_gx(pr), gu, gf)
    for k, v in g.items():
        assert np.all(np.isnan(v[0])), k
        assert not np.any(np.isnan(v[1])), k


@pytest.mark.parametrize("cid", ["lane_7_6_14", "subgroup_5_2_30", "wave_30_6_60"])
def test_dG_is_bit_symmetric_with_gf(cid):
    pr = dual_ref.case(cid)
    x, f, st, it, u, nact = dual_ref.reference(cid)
    gu, gf = F.make_cotangents(pr)
    g = F.vjp_full(pr, x, u, vjp_ref.make_gx(pr), gu, gf, st)
    assert np.array_equal(g["dG"].view(np.uint64), np.swapaxes(g["dG"], 1, 2).copy().view(np.uint64))
    plain = vjp_ref.vjp(pr, x, u, vjp_ref.make_gx(pr), st)
    assert not np.array_equal(g["dG"], plain["dG"])  # gf entered
    off = u[:, pr.p:] == 0
    assert not np.any(g["dci0"][off].view(np.uint64))  # +0.0 exactly, whatever gu holds there


@pytest.mark.parametrize("cid", sorted(box_ref.cases()))
def test_box_form_equals_dense_form(cid):
    """u and gu of the box form are u and gu of the dense form on to_dense(): [equalities, upper, lower]."""
    bp = box_ref.case(cid)
    n = bp.n
    x, f, st, it, u, nact = box_dual_ref.reference(cid)
    gx = vjp_ref.make_gx(bp)
    gu, gf = F.make_cotangents(bp)
    for status in (st, None):
        gb = F.vjp_box_full(bp, x, u, gx, gu, gf, status)
        gd = F.vjp_full(box_ref.dense(cid), x, u, gx, gu, gf, status)
        want = {k: gd[k] for k in ("dG", "dg0", "dCE", "dce0")}
        want["dhi"] = gd["dci0"][:, :n]
        on = gd["dci0"][:, n:].view(np.uint64) != 0
        want["dlo"] = np.where(on, -gd["dci0"][:, n:], 0.0)
        assert not vjp_ref.mismatches(gb, want), f"{cid}: {vjp_ref.mismatches(gb, want)}"
