"""qpgpu_kkt_residuals without a device: the export surface, the argument rules, and the definition
(tests/kkt_ref.py) on the CPU reference's own primal-dual pairs — that it certifies the well-posed
list, that it discriminates, its special values, and that the box form equals the dense one.

Bars: scaled stationarity 1e-12 and complementarity 1e-10 are tests/test_dual_cpu.py's; the
equality and inequality residuals are the same kind of measure (a residual over the magnitude of
its own terms) and take complementarity's bar.  Measured on the well-posed list with the reference
alone: 7.94e-16, 3.84e-14, 1.53e-14, 1.78e-14."""
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
import kkt_ref
import qpgpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("qpgpu_kkt_residuals", "qpgpu_kkt_residuals_box")
STATIONARITY_MAX = 1e-12
COMPLEMENTARITY_MAX = 1e-10
EQUALITY_MAX = 1e-10
INEQUALITY_MAX = 1e-10


def test_symbols_declared_listed_and_exported():
    hdr = open(os.path.join(ROOT, "include", "qpgpu.h")).read()
    out = subprocess.check_output(["nm", "-D", "--defined-only", qpgpu.LIB_PATH]).decode()
    for name in NEW_SYMBOLS:
        assert re.search(rf"\b{name}\s*\(", hdr), f"{name} is not declared in include/qpgpu.h"
        assert name in qpgpu.EXPORTED_SYMBOLS
        assert re.search(rf"\bT {name}$", out, flags=re.M), f"{name} is not exported by libqpgpu.so"
    assert re.search(r"#define\s+QPGPU_KKT_NRES\s+8\b", hdr)
    assert qpgpu.KKT_NRES == kkt_ref.NRES == 8
    names = ("STAT", "STAT_SCALE", "EQ", "INEQ", "COMP", "UMIN", "OBJ", "NNZ")
    enum = re.search(r"enum\s*\{\s*QPGPU_KKT_STAT\b([^}]*)\}", hdr)
    assert enum and re.findall(r"QPGPU_KKT_(\w+)", "QPGPU_KKT_STAT" + enum.group(1)) == list(names)
    for k, nm in enumerate(names):
        assert getattr(qpgpu, "KKT_" + nm) == getattr(kkt_ref, nm) == k
    assert qpgpu.LIB.qpgpu_abi_version() == 1


def test_argument_rules_without_a_device():
    """The C entries with NULL arrays: every rule checked here is decided before any array is read
    (and before anything is launched: no call below reaches the device)."""
    buf = (ctypes.c_double * 64)()
    some = ctypes.cast(buf, ctypes.c_void_p)

    def call(box, n, p, m, batch, flags=0, u=None, r=None, rest=None):
        d = qpgpu.ProblemDesc(n, p, m, 0, batch, flags, 0)
        args = [rest] * 11  # G g0 CE ce0 CI|hi ci0|lo x u status r stream
        args[7], args[8], args[9], args[10] = u, None, r, None
        fn = qpgpu.LIB.qpgpu_kkt_residuals_box if box else qpgpu.LIB.qpgpu_kkt_residuals
        return fn(ctypes.byref(d), *args)

    inv = qpgpu.ERR_INVALID_ARGUMENT
    for box in (False, True):
        assert call(box, 7, 0, 14, 0, u=some, r=some) == qpgpu.SUCCESS  # batch = 0
        assert call(box, 7, 0, 14, 0, flags=qpgpu.FLAG_EXACT, u=some, r=some) == inv  # non-zero flags
        assert call(box, 7, 0, 14, 0, flags=qpgpu.FLAG_FORCE_GENERIC, u=some, r=some) == inv
        assert call(box, 7, 0, 14, 0, r=some) == inv  # NULL u with p + m > 0
        assert call(box, 7, 0, 14, 4, u=some, r=None, rest=some) == inv  # NULL r with batch > 0
        assert call(box, 7, 0, 14, 4, u=some, r=some) == inv  # NULL G, g0, x, ...
    assert call(True, 7, 0, 13, 0, u=some, r=some) == inv  # box with m != 2n
    assert call(False, 7, 0, 13, 0, u=some, r=some) == qpgpu.SUCCESS
    assert call(False, 3, 0, 0, 0) == qpgpu.SUCCESS  # p + m == 0: u may be NULL


# ---- the definition on the reference's own pairs ---------------------------------------------------
@functools.lru_cache(maxsize=None)
def ref_residuals(cid, masked=True):
    x, f, st, it, u, nact = dual_ref.reference(cid)
    r = kkt_ref.residuals(dual_ref.case(cid), x, u, st if masked else None)
    r.setflags(write=False)
    return r


@pytest.mark.parametrize("cid", sorted(dual_ref.kkt_cases()))
def test_well_posed_list_is_certified(cid):
    pr = dual_ref.case(cid)
    x, f, st, it, u, nact = dual_ref.reference(cid)
    r = ref_residuals(cid)
    ok = (st == qpgpu.QP_OK) & np.all(np.isfinite(x), axis=1)
    assert np.all(np.isnan(r[st != qpgpu.QP_OK]))
    if not ok.any():
        return
    g = r[ok]
    print(f"{cid}: {int(ok.sum())} QPs, stat {np.max(g[:, kkt_ref.STAT]):.3e} comp {np.max(g[:, kkt_ref.COMP]):.3e} "
          f"eq {np.max(g[:, kkt_ref.EQ]):.3e} ineq {np.max(g[:, kkt_ref.INEQ]):.3e}")
    assert np.all(g[:, kkt_ref.STAT] <= STATIONARITY_MAX), f"{cid}: stationarity {np.max(g[:, kkt_ref.STAT]):.3e}"
    assert np.all(g[:, kkt_ref.COMP] <= COMPLEMENTARITY_MAX), f"{cid}: complementarity {np.max(g[:, kkt_ref.COMP]):.3e}"
    assert np.all(g[:, kkt_ref.EQ] <= EQUALITY_MAX), f"{cid}: equality residual {np.max(g[:, kkt_ref.EQ]):.3e}"
    # a NaN limit in the data (edge_nan_limit) is reported as such, by definition: INEQ is NaN
    # there and held to the bar on every QP whose ci0 is free of NaN
    nan_limit = np.isnan(pr.ci0).any(axis=1)[ok]
    assert np.all(np.isnan(g[nan_limit, kkt_ref.INEQ]))
    assert np.all(g[~nan_limit, kkt_ref.INEQ] <= INEQUALITY_MAX), f"{cid}: inequality violation {g[:, kkt_ref.INEQ]}"
    assert not np.any(g[:, kkt_ref.UMIN].view(np.uint64)), f"{cid}: a negative multiplier"  # +0.0 exactly
    assert np.array_equal(g[:, kkt_ref.NNZ], nact[ok].astype(np.float64))


def test_rollback_quirk_is_detected():
    """The header's warning made visible: on fuzz_3 the reference's own (x, u) violates an
    inequality at the scale of its terms."""
    _, _, st, _, _, _ = dual_ref.reference("fuzz_3")
    r = ref_residuals("fuzz_3")
    worst = np.nanmax(np.where(st == qpgpu.QP_OK, r[:, kkt_ref.INEQ], 0.0))
    print(f"fuzz_3: worst scaled inequality violation on a status-OK QP {worst:.3e}")
    assert worst >= 0.1


def test_perturbations_are_detected():
    cid = "C1_general_7_6_14"
    pr = dual_ref.case(cid)
    x, f, st, it, u, nact = dual_ref.reference(cid)
    base = ref_residuals(cid)
    ok = np.where((st == qpgpu.QP_OK) & np.any(u != 0, axis=1))[0]
    assert ok.size >= 8
    u2, x2 = np.array(u), np.array(x)
    for b in ok:
        j = int(np.argmax(u[b] != 0))
        u2[b, j] = -u2[b, j]
        i = int(b % pr.n)
        x2[b, i] += 1e-3 * np.max(np.abs(x[b]))
    ru, rx = kkt_ref.residuals(pr, x, u2, st), kkt_ref.residuals(pr, x2, u, st)
    for r in (ru, rx):
        up = np.maximum(r[ok, kkt_ref.STAT], r[ok, kkt_ref.EQ])
        assert np.all(up > 1e-6), f"undetected: {up.min():.3e}"
    assert np.all(np.maximum(base[ok, kkt_ref.STAT], base[ok, kkt_ref.EQ]) <= EQUALITY_MAX)


def test_special_values():
    # a NaN limit: the inequality slot says so, the others stay finite
    cid = "edge_nan_limit"
    st = dual_ref.reference(cid)[2]
    r = ref_residuals(cid, masked=False)
    assert np.all(np.isnan(r[:, kkt_ref.INEQ]))
    rest = [k for k in range(kkt_ref.NRES) if k != kkt_ref.INEQ]
    assert np.all(np.isfinite(r[:, rest])), r
    # a non-OK status: the whole block NaN with the mask, evaluated without it
    for cid in ("edge_infeasible", "edge_dependent", "edge_not_pd"):
        st = dual_ref.reference(cid)[2]
        assert np.all(st != qpgpu.QP_OK)
        assert np.all(np.isnan(ref_residuals(cid)))
        assert not np.all(np.isnan(ref_residuals(cid, masked=False)))
    # an absent bound, ci0 = +inf, with its multiplier 0: no NaN anywhere
    cid = "inf_7_3"
    bp = box_ref.case(cid)
    x, f, st, it, u, nact = box_dual_ref.reference(cid)
    assert np.isinf(bp.hi).any() and np.isinf(bp.lo).any()
    ok = st == qpgpu.QP_OK
    assert ok.sum() >= 8
    r = kkt_ref.residuals(box_ref.dense(cid), x, u, st)
    assert not np.any(np.isnan(r[ok]))
    assert np.all(r[ok, kkt_ref.INEQ] <= INEQUALITY_MAX) and np.all(r[ok, kkt_ref.COMP] <= COMPLEMENTARITY_MAX)


@pytest.mark.parametrize("cid", sorted(box_ref.cases()))
def test_box_form_equals_dense_form(cid):
    bp = box_ref.case(cid)
    x, f, st, it, u, nact = box_dual_ref.reference(cid)
    for status in (st, None):
        rb = kkt_ref.residuals_box(bp, x, u, status)
        rd = kkt_ref.residuals(box_ref.dense(cid), x, u, status)
        assert kkt_ref.same_bits(rb, rd), f"{cid}: (QP, slot, box, dense) {kkt_ref.mismatches(rb, rd)}"
    ok = st == qpgpu.QP_OK
    if cid in box_dual_ref.well_posed_cases() and ok.any():
        g = kkt_ref.residuals_box(bp, x, u, st)[ok]
        assert np.all(g[:, kkt_ref.STAT] <= STATIONARITY_MAX) and np.all(g[:, kkt_ref.COMP] <= COMPLEMENTARITY_MAX)
        assert np.all(g[:, kkt_ref.INEQ] <= INEQUALITY_MAX) and np.all(g[:, kkt_ref.EQ] <= EQUALITY_MAX)
        assert np.array_equal(g[:, kkt_ref.NNZ], nact[ok].astype(np.float64))
