"""qpgpu_solve_batched_box_dual without a device: the export surface, the kernel names, and the
conditions on the case list that keep tests/test_gpu_box_dual.py from passing vacuously — all
recomputed from the reference alone (tests/box_dual_ref.py: dual_ref's restatement on
BoxProblems.to_dense()), never from the code under test.

The KKT bars are those of tests/test_dual_cpu.py (1e-12 scaled stationarity, 1e-10 complementarity:
properties of the definition, three to four orders above binary64 rounding on these problems —
measured here 9.29e-16 and 4.17e-14 — and twelve below what a sign or slot error produces)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import box_dual_ref
import box_ref
import dual_ref
import qpgpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("qpgpu_solve_batched_box_dual", "qpgpu_kernel_name_box_dual")
STATIONARITY_MAX = 1e-12
COMPLEMENTARITY_MAX = 1e-10


def _same_bits(a, b):
    a = np.ascontiguousarray(a, dtype=np.float64).ravel()
    b = np.ascontiguousarray(b, dtype=np.float64).ravel()
    return bool(np.all((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))))


def test_symbols_declared_listed_and_exported():
    hdr = open(os.path.join(ROOT, "include", "qpgpu.h")).read()
    out = subprocess.check_output(["nm", "-D", "--defined-only", qpgpu.LIB_PATH]).decode()
    for name in NEW_SYMBOLS:
        assert re.search(rf"\b{name}\s*\(", hdr), f"{name} is not declared in include/qpgpu.h"
        assert name in qpgpu.EXPORTED_SYMBOLS
        assert re.search(rf"\bT {name}$", out, flags=re.M), f"{name} is not exported by libqpgpu.so"
    assert qpgpu.LIB.qpgpu_abi_version() == 1


def test_kernel_names():
    for flag, word in ((qpgpu.FLAG_FORCE_LANE, "lane"), (qpgpu.FLAG_FORCE_SUBGROUP, "small"),
                       (qpgpu.FLAG_FORCE_WAVE, "wave"), (qpgpu.FLAG_FORCE_GENERIC, "generic")):
        name = qpgpu.kernel_name_box_dual(7, 3, flag)
        assert word in name and "box" in name and "dual" in name, name
    assert qpgpu.kernel_name_box_dual(9, 0, qpgpu.FLAG_FORCE_LANE) == ""
    assert qpgpu.kernel_name_box_dual(17, 0, qpgpu.FLAG_FORCE_SUBGROUP) == ""
    assert qpgpu.kernel_name_box_dual(257, 0, qpgpu.FLAG_FORCE_WAVE) == ""
    assert qpgpu.kernel_name_box_dual(7, 3, qpgpu.FLAG_FAST) == ""
    # "" exactly where qpgpu_kernel_name_box is, and the default order covers every shape
    for n, p in ((0, 0), (7, 0), (7, 6), (14, 10), (30, 6), (65, 0), (256, 0), (300, 2)):
        for flag in (0, qpgpu.FLAG_FORCE_LANE, qpgpu.FLAG_FORCE_SUBGROUP, qpgpu.FLAG_FORCE_WAVE,
                     qpgpu.FLAG_FORCE_GENERIC, qpgpu.FLAG_FORCE_LANE | qpgpu.FLAG_FORCE_WAVE):
            a, b = qpgpu.kernel_name_box(n, p, flag), qpgpu.kernel_name_box_dual(n, p, flag)
            assert (a == "") == (b == ""), (n, p, flag, a, b)
            assert b == "" or ("box" in b and "dual" in b)


def test_argument_rules_without_a_device():
    """The C entry with NULL arrays: every rule checked here is decided before any is read."""
    def call(n, p, m, batch, flags=0, u=None):
        d = qpgpu.ProblemDesc(n, p, m, 0, batch, flags, 0)
        args = [None] * 13
        args[10] = u
        return qpgpu.LIB.qpgpu_solve_batched_box_dual(ctypes.byref(d), *args)

    inv = qpgpu.ERR_INVALID_ARGUMENT
    buf = (ctypes.c_double * 64)()
    up = ctypes.cast(buf, ctypes.c_void_p)
    assert call(7, 0, 13, 0, u=up) == inv  # m != 2n
    assert call(7, 0, 14, 0, flags=qpgpu.FLAG_FAST, u=up) == inv
    assert call(7, 0, 14, 4, u=up) == inv  # NULL hi / lo with batch > 0
    assert call(7, 0, 14, 0) == inv  # NULL u
    assert call(7, 0, 14, 0, u=up) == qpgpu.SUCCESS  # batch = 0


# ---- conditions on the case list -------------------------------------------------------------------
@pytest.mark.parametrize("cid", sorted(box_ref.cases()))
def test_reference_is_the_box_reference_with_multipliers(cid):
    bp = box_ref.case(cid)
    x, f, st, it, u, nact = box_dual_ref.reference(cid)
    xr, fr, sr, ir = box_ref.reference(cid)
    assert np.array_equal(st, sr) and np.array_equal(it, ir) and _same_bits(f, fr)
    has_x = sr != qpgpu.QP_NOT_POSITIVE_DEFINITE
    assert _same_bits(x[has_x], xr[has_x])
    assert u.shape == (bp.batch, bp.p + 2 * bp.n) and not np.any(np.isnan(u)) and not np.any(nact == -7)
    ui = u[:, bp.p:]
    assert np.array_equal(np.count_nonzero(ui, axis=1), nact)
    assert float(ui.min()) == 0.0
    bad = st != qpgpu.QP_OK
    assert not np.any(u[bad].view(np.uint64)) and not np.any(nact[bad])
    ok = ~bad
    if bp.p > 0 and ok.any():  # a kernel that skips the equality rows of u cannot pass
        assert np.all(np.any(u[ok, :bp.p] != 0, axis=1)), "an OK QP with all-zero equality multipliers"


@pytest.mark.parametrize("cid", box_ref.generator_cases())
def test_bounds_carry_multipliers_on_generator_cases(cid):
    _, _, st, _, _, nact = box_dual_ref.reference(cid)
    ok = st == qpgpu.QP_OK
    assert ok.sum() >= 2
    frac = float((nact[ok] > 0).mean())
    print(f"{cid}: {int(ok.sum())} OK QPs, nact > 0 on {frac:.2f}")
    assert frac >= 0.5


@pytest.mark.parametrize("fam", sorted(box_ref.SHAPES))
def test_upper_and_lower_active_at_once(fam):
    """Per family shape list, a QP with an upper-bound and a lower-bound slot non-zero."""
    hit = 0
    for n, p, _ in box_ref.SHAPES[fam]:
        u = box_dual_ref.reference(f"{fam}_{n}_{p}")[4]
        hit += int((np.any(u[:, p:p + n] != 0, axis=1) & np.any(u[:, p + n:] != 0, axis=1)).sum())
    assert hit > 0


@pytest.mark.parametrize("cid", box_dual_ref.well_posed_cases())
def test_kkt_on_well_posed(cid):
    pr = box_ref.dense(cid)
    x, f, st, it, u, nact = box_dual_ref.reference(cid)
    stat, comp, umin, cnt = dual_ref.kkt_measures(pr, x, st, u)
    print(f"{cid}: {cnt} QPs, stationarity {stat:.3e}, complementarity {comp:.3e}, min u[p:] {umin!r}")
    assert stat <= STATIONARITY_MAX, f"{cid}: scaled stationarity residual {stat:.3e}"
    assert comp <= COMPLEMENTARITY_MAX, f"{cid}: complementarity residual {comp:.3e}"
    # the header's form of stationarity: G x + g0 = CE u[:p] - u[p:p+n] + u[p+n:]
    bp = box_ref.case(cid)
    n, p = bp.n, bp.p
    ok = (st == qpgpu.QP_OK) & np.all(np.isfinite(x), axis=1)
    lhs = np.einsum("bij,bj->bi", bp.G[ok], x[ok]) + bp.g0[ok]
    rhs = np.einsum("bip,bp->bi", bp.CE[ok], u[ok, :p]) - u[ok, p:p + n] + u[ok, p + n:]
    sc = np.einsum("bij,bj->bi", np.abs(bp.G[ok]), np.abs(x[ok])) + np.abs(bp.g0[ok]) + \
        np.einsum("bip,bp->bi", np.abs(bp.CE[ok]), np.abs(u[ok, :p])) + u[ok, p:p + n] + u[ok, p + n:]
    if ok.any():
        assert float((np.abs(lhs - rhs).max(axis=1) / sc.max(axis=1)).max()) <= STATIONARITY_MAX


def test_well_posed_list():
    ids = box_dual_ref.well_posed_cases()
    assert len(box_ref.cases()) == 43 and len(ids) == 28
    assert sum(int((box_dual_ref.reference(c)[2] == qpgpu.QP_OK).sum()) for c in ids) > 1000
