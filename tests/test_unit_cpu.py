"""qpgpu_solve_batched_unit without a device: the export surface, the kernel names, the argument
rules that are decided before the device is touched, the Python helpers, and the conditions on
tests/unit_ref.py's case list that keep tests/test_gpu_unit.py from passing vacuously — all taken
from the oracle on the materialised problems, never from the code under test."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import oracle
import qpgpu
import unit_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("qpgpu_solve_batched_unit", "qpgpu_kernel_name_unit")


def test_symbols_declared_listed_and_exported():
    hdr = open(os.path.join(ROOT, "include", "qpgpu.h")).read()
    out = subprocess.check_output(["nm", "-D", "--defined-only", qpgpu.LIB_PATH]).decode()
    for name in NEW_SYMBOLS:
        assert re.search(rf"\b{name}\s*\(", hdr), f"{name} is not declared in include/qpgpu.h"
        assert name in qpgpu.EXPORTED_SYMBOLS
        assert re.search(rf"\bT {name}$", out, flags=re.M), f"{name} is not exported by libqpgpu.so"
    assert qpgpu.LIB.qpgpu_abi_version() == 1
    mh = open(os.path.join(ROOT, "include", "mgqp_amd.h")).read()
    bit = int(re.search(r"#define MGQP_SOLVER_UNIT_HESSIAN (0x[0-9a-fA-F]+)u", mh).group(1), 16)
    known = (qpgpu.FLAG_WRITE_FACTOR | qpgpu.FLAG_EXACT | qpgpu.FLAG_FAST | qpgpu.FLAG_FORCE_LANE |
             qpgpu.FLAG_FORCE_SUBGROUP | qpgpu.FLAG_FORCE_WAVE | qpgpu.FLAG_FORCE_GENERIC)
    assert bit and not (bit & known) and bit & (bit - 1) == 0


GRID = [(n, p, m) for n in (1, 4, 7, 8, 9, 14, 16, 17, 30, 32, 33, 64) for p in (0, 3) for m in (0, 14, 16, 17, 64, 65, 256)]


def test_kernel_name_unit_grid():
    for n, p, m in GRID:
        name = qpgpu.kernel_name_unit(n, p, m)
        assert "unit" in name, (n, p, m, name)
        # the default order is the dense entry's: the same family word in both names
        dense = qpgpu.LIB.qpgpu_kernel_name_flags(n, p, m, qpgpu.FLAG_EXACT).decode()
        for word in ("qp_lane", "qp_small", "qp_wave"):
            assert (word in name) == (word in dense), (n, p, m, name, dense)
        for fam, word in (("lane", "qp_lane_unit"), ("subgroup", "qp_small_unit"), ("wave", "qp_wave_unit")):
            forced = qpgpu.kernel_name_unit(n, p, m, qpgpu.FAMILY_FLAGS[fam])
            if unit_ref.covers(fam, n, m):
                assert word in forced, (n, p, m, fam, forced)
            else:
                assert forced == "", (n, p, m, fam, forced)


def test_kernel_name_unit_refusals():
    assert qpgpu.kernel_name_unit(65, 0, 14) == ""
    assert qpgpu.kernel_name_unit(14, 0, 257) == ""
    assert qpgpu.kernel_name_unit(65, 0, 14, qpgpu.FLAG_FORCE_WAVE) == ""
    for n, p, m in ((7, 3, 14), (14, 10, 28), (30, 6, 60)):
        for flag in (qpgpu.FLAG_FORCE_GENERIC, qpgpu.FLAG_FAST, qpgpu.FLAG_WRITE_FACTOR,
                     qpgpu.FLAG_FORCE_LANE | qpgpu.FLAG_FORCE_WAVE, 0x40):
            assert qpgpu.kernel_name_unit(n, p, m, flag) == "", (n, p, m, flag)
        assert "unit" in qpgpu.kernel_name_unit(n, p, m, qpgpu.FLAG_EXACT)
    assert qpgpu.kernel_name_unit(0, 0, 0) == "" and qpgpu.kernel_name_unit(7, -1, 0) == ""


def _call(n, p, m, batch, flags=0, layout=0, ptrs=()):
    """The C entry with the named arguments a dummy non-NULL address and the others NULL: every
    rule checked here is decided from the pointers' values, before any is read and before the
    device is touched.  Order: g0 CE ce0 CI ci0 x f status iters x_eq f_eq status_eq."""
    names = ("g0", "CE", "ce0", "CI", "ci0", "x", "f", "status", "iters", "x_eq", "f_eq", "status_eq")
    assert set(ptrs) <= set(names)
    d = qpgpu.ProblemDesc(n, p, m, 0, batch, flags, layout)
    args = [ctypes.c_void_p(0x1000) if k in ptrs else None for k in names]
    return qpgpu.LIB.qpgpu_solve_batched_unit(ctypes.byref(d), *args, None)


def test_argument_rules_without_a_device():
    inv, ok = qpgpu.ERR_INVALID_ARGUMENT, qpgpu.SUCCESS
    assert qpgpu.LIB.qpgpu_solve_batched_unit(None, *([None] * 13)) == inv
    assert _call(0, 0, 0, 0) == inv and _call(7, -1, 0, 0) == inv and _call(7, 0, -1, 0) == inv
    assert _call(7, 0, 14, -1) == inv and _call(7, 0, 14, 0, layout=2) == inv
    assert _call(7, 0, 14, 0, flags=qpgpu.FLAG_FAST) == inv
    assert _call(7, 0, 14, 0, flags=qpgpu.FLAG_WRITE_FACTOR) == inv
    assert _call(7, 0, 14, 0, flags=qpgpu.FLAG_FORCE_LANE | qpgpu.FLAG_FORCE_WAVE) == inv
    # batch = 0 is a success in both layouts, with EXACT accepted
    assert _call(7, 0, 14, 0) == ok and _call(7, 0, 14, 0, layout=1) == ok
    assert _call(7, 0, 14, 0, flags=qpgpu.FLAG_EXACT) == ok
    # a mixed eq triple, whatever the batch
    for mixed in (("x_eq",), ("f_eq", "status_eq"), ("x_eq", "status_eq")):
        assert _call(7, 0, 14, 0, ptrs=mixed) == inv, mixed
    assert _call(7, 0, 14, 0, ptrs=("x_eq", "f_eq", "status_eq")) == ok
    # batch > 0: each required array NULL in turn
    full = ("g0", "CE", "ce0", "CI", "ci0", "x", "f", "status")
    for missing in full:
        assert _call(7, 3, 14, 4, ptrs=tuple(k for k in full if k != missing)) == inv, missing
    # ... refused before the shape is looked at, too
    assert _call(65, 3, 14, 4, ptrs=("g0",)) == inv
    # a shape without a unit kernel: decided before any launch (every array given)
    uns = qpgpu.ERR_UNSUPPORTED_SHAPE
    assert _call(65, 3, 14, 4, ptrs=full) == uns
    assert _call(14, 3, 257, 4, ptrs=full) == uns
    assert _call(7, 3, 14, 4, flags=qpgpu.FLAG_FORCE_GENERIC, ptrs=full) == uns
    assert _call(9, 3, 14, 4, flags=qpgpu.FLAG_FORCE_LANE, ptrs=full) == uns
    assert _call(17, 3, 14, 4, flags=qpgpu.FLAG_FORCE_SUBGROUP, ptrs=full) == uns


def test_unit_problems_container():
    up = qpgpu.make_unit_problems(7, 3, 14, 3, 40, seed=9)
    pr = qpgpu.make_problems("general", 7, 3, 14, 3, 40, seed=9)
    assert up.batch == 37 and (up.n, up.p, up.m) == (7, 3, 14)
    for a, b in zip(up.arrays(), pr.arrays()[1:]):  # g0 scaled by 10 / 10: the generator's bits
        assert a.shape == b.shape and a.tobytes() == b.tobytes()
    de = up.to_dense()
    assert de.G.tobytes() == np.ascontiguousarray(np.broadcast_to(np.eye(7), (37, 7, 7))).tobytes()
    for a, b in zip(de.arrays()[1:], up.arrays()):
        assert a.tobytes() == b.tobytes()
    s = up.slice(1, 3)
    assert s.batch == 2 and np.array_equal(s.g0, up.g0[1:3]) and np.array_equal(s.CI, up.CI[1:3])
    z = qpgpu.make_unit_problems(7, 3, 14, 0, 5, g0_scale=0.0)
    assert not z.g0.any() and not np.signbit(z.g0).any()
    h = qpgpu.make_unit_problems(7, 3, 14, 3, 40, seed=9, g0_scale=5.0)
    assert np.array_equal(h.g0, 0.5 * pr.g0)


def test_byte_counts():
    assert qpgpu.algorithmic_bytes_per_qp_unit(7, 6, 14) == 8 * (7 + 42 + 6 + 98 + 14) + 64
    for n, p, m in ((7, 6, 14), (14, 10, 28), (30, 6, 60)):
        assert qpgpu.algorithmic_bytes_per_qp(n, p, m) - qpgpu.algorithmic_bytes_per_qp_unit(n, p, m) == 8 * n * n


# ---- conditions on the case list -------------------------------------------------------------------
def test_case_list_is_the_issue_s():
    ids = set(unit_ref.cases())
    assert len(ids) == 16 + 8 * 3
    for fam, shapes in unit_ref.SHAPES.items():
        for n, p, m, B in shapes:
            assert unit_ref.case(f"{fam}_{n}_{p}_{m}").batch == B
    # the default order reaches all three families
    seen = {qpgpu.kernel_name_unit(u.n, u.p, u.m).split("<")[0] for u in unit_ref.cases().values()}
    assert seen == {"qp_lane_unit", "qp_small_unit", "qp_wave_unit"}


@pytest.mark.parametrize("cid", unit_ref.generator_cases())
def test_generator_cases_are_ok_and_not_trivial(cid):
    """All QPs OK; mean l1 passes > 1.5 wherever p < n and m > 0 (m = 0 is one pass by construction:
    lane_7_0_0 measures 1.00; measured elsewhere: 1.60 on (1, 0, 2), 1.73 / 2.35 / 8.25 with
    g0 = 0, 4.2 - 80 with g0 ~ 10 N(0, 1))."""
    up = unit_ref.case(cid)
    x, f, st, it = unit_ref.reference(cid)
    print(f"{cid}: mean l1 passes {it.mean():.2f}")
    assert (st == qpgpu.QP_OK).all()
    assert (unit_ref.reference_eq(cid)[2] == qpgpu.QP_OK).all()
    if up.p < up.n and up.m > 0:
        assert it.mean() > 1.5


def test_crossed_cases_take_the_retry():
    for n, p, m, B in unit_ref.MODE_SHAPES:
        cid = f"crossed_{n}_{p}_{m}"
        st, se = unit_ref.reference(cid)[2], unit_ref.reference_eq(cid)[2]
        retry = (st == qpgpu.QP_INFEASIBLE) & (se == qpgpu.QP_OK)
        print(cid, int(retry.sum()), "of", B)
        assert retry.sum() * 4 >= B  # measured: 35 of 70, 33 of 66, 8 of 16
        assert (st[1::2] == qpgpu.QP_OK).all()


def test_duplicated_ce_is_reported_dependent():
    """A quarter where the reference reaches it.  A duplicated random column is dependent only up to
    rounding, and the reference reports it only when |d| <= eps * R_norm survives that rounding:
    measured 17 of 66 on (14, 10, 28) (a quarter), 11 of 70 on (7, 3, 14) and 0 of 16 on
    (30, 6, 60), where the six duplicates end INFEASIBLE instead.  The bars are those counts.  The
    dupexact mode, dependent in exact arithmetic, covers every shape: all of its every-third QPs."""
    bars = {(7, 3, 14): 11, (14, 10, 28): 17, (30, 6, 60): 0}
    for n, p, m, B in unit_ref.MODE_SHAPES:
        st = unit_ref.reference(f"dupce_{n}_{p}_{m}")[2]
        dep = int((st == qpgpu.QP_DEPENDENT).sum())
        print(n, p, m, dep, "of", B)
        assert dep >= bars[(n, p, m)]
        assert (st[1::3] != qpgpu.QP_DEPENDENT).all() and (st[2::3] != qpgpu.QP_DEPENDENT).all()
        st, se = unit_ref.reference(f"dupexact_{n}_{p}_{m}")[2], unit_ref.reference_eq(f"dupexact_{n}_{p}_{m}")[2]
        assert (st[::3] == qpgpu.QP_DEPENDENT).all() and (se[::3] == qpgpu.QP_DEPENDENT).all()
        assert (st[1::3] == qpgpu.QP_OK).all() and (st[2::3] == qpgpu.QP_OK).all()


def test_other_statuses_occur():
    seen = set()
    for cid in unit_ref.cases():
        seen |= set(int(s) for s in unit_ref.reference(cid)[2])
    assert {qpgpu.QP_OK, qpgpu.QP_INFEASIBLE, qpgpu.QP_DEPENDENT, qpgpu.QP_MAX_ITER} <= seen


@pytest.mark.parametrize("cid", list(unit_ref.cases()))
def test_factor_of_identity_is_identity_and_g0_inside_the_contract(cid):
    """oracle.solve_batch(to_dense(), write_factor=True) leaves G the identity bit for bit, and no
    g0 entry is non-finite or -0.0: the two facts the stated setup rests on."""
    up = unit_ref.case(cid)
    pr = up.to_dense()
    eye = pr.G.copy()
    oracle.solve_batch(pr, write_factor=True, max_steps=unit_ref.default_cap(up.n, up.p, up.m))
    assert pr.G.tobytes() == eye.tobytes()
    assert np.isfinite(up.g0).all() and not (np.signbit(up.g0) & (up.g0 == 0)).any()


def test_stated_setup_is_the_reference_s():
    """x0 = -g0 and f0 = 0.5 sum g0[i] x0[i] (ascending, each product rounded) are what the oracle
    returns for the materialised problem without constraints."""
    for n in (1, 7, 14, 30, 64):
        up = qpgpu.make_unit_problems(n, 0, 0, 0, 9, seed=n)
        up.g0[1] = 0.0
        x, f, st, it = oracle.solve_batch(up.to_dense())
        assert (st == qpgpu.QP_OK).all()
        assert x.tobytes() == (-up.g0).tobytes()
        f0 = np.zeros(9)
        for i in range(n):
            f0 = f0 + up.g0[:, i] * x[:, i]
        assert f.tobytes() == (0.5 * f0).tobytes()
