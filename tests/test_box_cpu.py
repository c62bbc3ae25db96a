"""qpgpu_solve_batched_box without a device: the export surface, the argument rules that need no
GPU, the Python helpers, and the conditions on tests/box_ref.py's case list that keep
tests/test_gpu_box.py from passing vacuously — all taken from the oracle on the materialised
problems, never from the code under test."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import box_ref
import qpgpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("qpgpu_solve_batched_box", "qpgpu_kernel_name_box")


def test_symbols_declared_listed_and_exported():
    hdr = open(os.path.join(ROOT, "include", "qpgpu.h")).read()
    out = subprocess.check_output(["nm", "-D", "--defined-only", qpgpu.LIB_PATH]).decode()
    for name in NEW_SYMBOLS:
        assert re.search(rf"\b{name}\s*\(", hdr), f"{name} is not declared in include/qpgpu.h"
        assert name in qpgpu.EXPORTED_SYMBOLS
        assert re.search(rf"\bT {name}$", out, flags=re.M), f"{name} is not exported by libqpgpu.so"
    assert qpgpu.LIB.qpgpu_abi_version() == 1


def _call(n, p, m, batch, flags=0, layout=0):
    """The C entry with NULL arrays: every rule checked here is decided before any is read."""
    d = qpgpu.ProblemDesc(n, p, m, 0, batch, flags, layout)
    return qpgpu.LIB.qpgpu_solve_batched_box(ctypes.byref(d), *([None] * 11))


def test_argument_rules_without_a_device():
    inv = qpgpu.ERR_INVALID_ARGUMENT
    assert _call(7, 0, 13, 0) == inv  # m != 2n
    assert _call(7, 0, 0, 0) == inv
    assert _call(7, 0, 15, 4) == inv
    assert _call(7, 0, 14, 0, flags=qpgpu.FLAG_FAST) == inv
    assert _call(7, 0, 14, 0, flags=qpgpu.FLAG_FORCE_LANE | qpgpu.FLAG_FORCE_WAVE) == inv
    assert _call(0, 0, 0, 0) == inv  # n = 0
    assert _call(7, 0, 14, 4) == inv  # NULL hi / lo with batch > 0
    assert _call(7, 0, 14, 0) == qpgpu.SUCCESS  # batch = 0
    assert _call(7, 0, 14, 0, layout=1) == qpgpu.SUCCESS


@pytest.mark.parametrize("n,p", [(7, 0), (7, 6), (14, 10), (30, 6), (64, 0), (65, 0), (256, 0), (300, 2)])
def test_kernel_name_box(n, p):
    name = qpgpu.kernel_name_box(n, p)
    assert name and "box" in name


def test_kernel_name_box_rejections_and_forced_families():
    assert qpgpu.kernel_name_box(0, 0) == ""
    assert qpgpu.kernel_name_box(7, 0, qpgpu.FLAG_FAST) == ""
    assert qpgpu.kernel_name_box(7, 0, qpgpu.FLAG_FORCE_LANE | qpgpu.FLAG_FORCE_WAVE) == ""
    for flag, word in ((qpgpu.FLAG_FORCE_LANE, "lane"), (qpgpu.FLAG_FORCE_SUBGROUP, "small"),
                       (qpgpu.FLAG_FORCE_WAVE, "wave"), (qpgpu.FLAG_FORCE_GENERIC, "generic")):
        name = qpgpu.kernel_name_box(7, 3, flag)
        assert word in name and "box" in name, name
    assert qpgpu.kernel_name_box(9, 0, qpgpu.FLAG_FORCE_LANE) == ""
    assert qpgpu.kernel_name_box(17, 0, qpgpu.FLAG_FORCE_SUBGROUP) == ""
    assert qpgpu.kernel_name_box(257, 0, qpgpu.FLAG_FORCE_WAVE) == ""


def test_make_box_problems_materialises_to_the_box_generator():
    bp = qpgpu.make_box_problems(7, 0, 3, 40, seed=9)
    assert bp.batch == 37 and bp.m == 14
    de, pr = bp.to_dense(), qpgpu.make_problems("box", 7, 0, 14, 3, 40, seed=9)
    assert (de.n, de.p, de.m) == (pr.n, pr.p, pr.m)
    for a, b in zip(de.arrays(), pr.arrays()):
        assert a.shape == b.shape and a.tobytes() == b.tobytes()
    bp = qpgpu.make_box_problems(14, 10, 0, 5)
    for a, b in zip(bp.to_dense().arrays(), qpgpu.make_problems("box", 14, 10, 28, 0, 5).arrays()):
        assert a.tobytes() == b.tobytes()
    s = bp.slice(1, 3)
    assert s.batch == 2 and np.array_equal(s.hi, bp.hi[1:3]) and np.array_equal(s.G, bp.G[1:3])


def test_to_dense_ordering():
    """Inequality k < n is the upper bound of variable k, n + k its lower bound."""
    bp = qpgpu.make_box_problems(3, 0, 0, 1)
    bp.hi[0] = [1.0, 2.0, np.inf]
    bp.lo[0] = [-4.0, -np.inf, -6.0]
    de = bp.to_dense()
    assert np.array_equal(de.CI[0], np.hstack([-np.eye(3), np.eye(3)]))
    assert np.array_equal(de.ci0[0], [1.0, 2.0, np.inf, 4.0, np.inf, 6.0])


def test_byte_counts():
    assert qpgpu.algorithmic_bytes_per_qp_box(7, 0) == 624
    assert qpgpu.algorithmic_bytes_per_qp_box(7, 6) == 1008
    assert qpgpu.algorithmic_bytes_per_qp_box(14, 10) == 3224
    # against the dense entry's count: the n x 2n CI becomes 2n bounds (C2: 1 408 -> 624)
    for n, p in ((7, 0), (14, 10), (30, 6)):
        assert qpgpu.algorithmic_bytes_per_qp(n, p, 2 * n) - qpgpu.algorithmic_bytes_per_qp_box(n, p) == 8 * 2 * n * n


# ---- conditions on the case list -------------------------------------------------------------------
def test_every_status_occurs():
    seen = set()
    for cid in box_ref.cases():
        seen |= set(int(s) for s in box_ref.reference(cid)[2])
    for st in (qpgpu.QP_OK, qpgpu.QP_INFEASIBLE, qpgpu.QP_DEPENDENT, qpgpu.QP_NOT_POSITIVE_DEFINITE):
        assert st in seen, qpgpu.STATUS_NAMES[st]


@pytest.mark.parametrize("cid", box_ref.generator_cases())
def test_bounds_bind_on_generator_cases(cid):
    """At least half of the OK QPs end with a bound active: |x_v - bound| = 0 exactly when the
    bound's row is in the final active set, <= 1e-12 accepted.  (box_ref.generator_cases() leaves
    out p >= n, where the equalities alone determine x.)"""
    bp = box_ref.case(cid)
    x, f, st, it = box_ref.reference(cid)
    ok = st == qpgpu.QP_OK
    assert ok.sum() >= 2
    gap = np.minimum(np.abs(x - bp.hi), np.abs(x - bp.lo)).min(axis=1)
    frac = float((gap[ok] <= 1e-12).mean())
    print(f"{cid}: {int(ok.sum())} OK QPs, bound active on {frac:.2f}, exact on {float((gap[ok] == 0).mean()):.2f}")
    assert frac >= 0.5


def test_long_paths_exist():
    assert any((box_ref.reference(cid)[3] >= 4).any() for cid in box_ref.cases())
    for n, p, _ in box_ref.MODE_SHAPES:
        assert (box_ref.reference(f"long_{n}_{p}")[3] >= 4).all()


def test_degenerate_rollback_is_taken():
    """add_constraint returning false in a full step, counted at that site of the restatement."""
    hit = {cid: int((box_ref.rollbacks(cid) > 0).sum()) for cid in box_ref.cases() if cid.startswith("scaled_ce")}
    print(hit)
    assert all(v > 0 for v in hit.values()), hit


def test_cases_stay_inside_the_finite_data_condition():
    for cid, bp in box_ref.cases().items():
        assert not np.any(np.isnan(bp.hi)) and not np.any(np.isnan(bp.lo)), cid
        assert not np.any(bp.hi == -np.inf) and not np.any(bp.lo == np.inf), cid
        x, f, st, it = box_ref.reference(cid)
        has_x = st != qpgpu.QP_NOT_POSITIVE_DEFINITE
        assert np.all(np.isfinite(x[has_x])), cid
