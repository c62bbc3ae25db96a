"""qpgpu_jvp_many without a device: the export surface, the kernel names, the argument rules and their
order, and the restatement (tests/jvp_many_ref.py), which factors once per QP and runs K right-hand
sides: direction k must have exactly the bits of tests/jvp_ref.py on slice k."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import box_dual_ref
import box_ref
import dual_ref
import jvp_many_ref
import jvp_ref
import qp_cases
import qpgpu
from vjp_ref import same_bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("qpgpu_jvp_many", "qpgpu_jvp_box_many", "qpgpu_kernel_name_jvp_many")
K = 3


def test_symbols_declared_listed_and_exported():
    hdr = open(os.path.join(ROOT, "include", "qpgpu.h")).read()
    out = subprocess.check_output(["nm", "-D", "--defined-only", qpgpu.LIB_PATH]).decode()
    for name in NEW_SYMBOLS:
        assert re.search(rf"\b{name}\s*\(", hdr), f"{name} is not declared in include/qpgpu.h"
        assert name in qpgpu.EXPORTED_SYMBOLS
        assert re.search(rf"\bT {name}$", out, flags=re.M), f"{name} is not exported by libqpgpu.so"
    assert qpgpu.LIB.qpgpu_abi_version() == 1


def test_kernel_names():
    """The header's boundary: lane for n <= 8 (the n = 8 instantiation has no scratch and stays a lane
    kernel), group beyond."""
    for n in range(1, 9):
        name = qpgpu.kernel_name_jvp_many(n, 0, 2 * n)
        assert "jvp" in name and "many" in name and "lane" in name and "group" not in name, (n, name)
    for n in (9, 16, 17, 32, 33, 64):
        name = qpgpu.kernel_name_jvp_many(n, 2, 20)
        assert "jvp" in name and "many" in name and "group" in name and "lane" not in name, (n, name)
    assert len({qpgpu.kernel_name_jvp_many(n) for n in range(1, 9)}) == 8
    assert len({qpgpu.kernel_name_jvp_many(n) for n in (16, 32, 64)}) == 3
    assert qpgpu.kernel_name_jvp_many(9) == qpgpu.kernel_name_jvp_many(16)
    assert qpgpu.kernel_name_jvp_many(17) == qpgpu.kernel_name_jvp_many(32)
    assert qpgpu.kernel_name_jvp_many(33) == qpgpu.kernel_name_jvp_many(64)
    for n in (65, 0, -1):
        assert qpgpu.kernel_name_jvp_many(n, 0, 0) == ""
    for n in (1, 8, 9, 64):  # another kernel than the single-direction entry's
        assert qpgpu.kernel_name_jvp_many(n) != qpgpu.kernel_name_jvp(n)


def test_argument_rules_without_a_device():
    """The C entries with NULL arrays: every rule checked here is decided before any array is read
    (and before anything is launched: no call below reaches the device)."""
    buf = (ctypes.c_double * 64)()
    some = ctypes.cast(buf, ctypes.c_void_p)

    def call(box, n, p, m, batch, ntan=2, flags=0, u=None, rest=None, outs=None, layout=0, **named):
        d = qpgpu.ProblemDesc(n, p, m, 0, batch, flags, layout)
        names = ["G", "CE"] + ([] if box else ["CI"]) + ["x", "u", "status"]
        args = {k: rest for k in names}
        args.update(u=u, status=None)
        args.update(named)
        fn = qpgpu.LIB.qpgpu_jvp_box_many if box else qpgpu.LIB.qpgpu_jvp_many
        return fn(ctypes.byref(d), ntan, *[args[k] for k in names], *([rest] * 6), *([outs] * 3), None)

    inv, uns = qpgpu.ERR_INVALID_ARGUMENT, qpgpu.ERR_UNSUPPORTED_SHAPE
    for box in (False, True):
        # qpgpu_jvp's rules as they are
        assert call(box, 7, 0, 14, 0, u=some) == qpgpu.SUCCESS  # batch = 0
        assert call(box, 7, 0, 14, 0, ntan=1, u=some) == qpgpu.SUCCESS
        assert call(box, 7, 0, 14, 0, flags=qpgpu.FLAG_EXACT, u=some) == inv  # non-zero flags
        assert call(box, 7, 0, 14, 0, layout=7, u=some) == inv  # unknown layout
        assert call(box, 7, 0, 14, 0) == inv  # NULL u with p + m > 0
        assert call(box, 7, 0, 14, 4, u=some) == inv  # NULL G, x
        for missing in ("G", "x"):
            assert call(box, 7, 2, 14, 4, u=some, rest=some, **{missing: None}) == inv
        assert call(box, 7, 2, 14, 4, u=some, rest=some, CE=None) == inv  # NULL CE with p > 0
        # every array given, every output NULL: success, and nothing is launched
        assert call(box, 7, 2, 14, 4, u=some, rest=some) == qpgpu.SUCCESS
        assert call(box, 64, 0, 128, 0, u=some) == qpgpu.SUCCESS
        # ntan < 1, also with batch = 0 ...
        for ntan in (0, -1, -(2 ** 31)):
            assert call(box, 7, 0, 14, 0, ntan=ntan, u=some) == inv
            assert call(box, 7, 2, 14, 4, ntan=ntan, u=some, rest=some) == inv
            assert call(box, 65, 0, 130, 0, ntan=ntan, u=some) == inv  # ... and before the shape rule
        # ... but after qpgpu_jvp's rules (each of these is INVALID_ARGUMENT either way; the order shows
        # where both the ntan rule and the shape rule would otherwise speak)
        assert call(box, 65, 0, 130, 0, ntan=0) == inv
        assert call(box, 65, 0, 130, 0, ntan=0, flags=qpgpu.FLAG_EXACT, u=some) == inv
        # the shape rule: n > 64
        assert call(box, 65, 0, 130, 0, u=some) == uns
        assert call(box, 65, 0, 130, 4, u=some, rest=some) == uns
        assert call(box, 65, 0, 130, 4, u=some, rest=some, outs=some) == uns
        assert call(box, 65, 0, 130, 0) == inv  # the argument rules come first
        assert call(box, 65, 0, 130, 4, u=some, rest=some, G=None) == inv
        # the shape rule: a K-fold block reaches 2^31, with batch = 0 too (the rule precedes it)
        assert call(box, 64, 0, 128, 0, ntan=2 ** 18 - 1, u=some) == qpgpu.SUCCESS  # K n m = 2^31 - 8192
        assert call(box, 64, 0, 128, 0, ntan=2 ** 18, u=some) == uns  # K n m = 2^31
        assert call(box, 64, 0, 128, 4, ntan=2 ** 18, u=some, rest=some, outs=some) == uns
        assert call(box, 64, 0, 128, 0, ntan=2 ** 31 - 1, u=some) == uns
        assert call(box, 1, 0, 2, 0, ntan=2 ** 30 - 1, u=some) == qpgpu.SUCCESS  # K (p + m) = 2^31 - 2
        assert call(box, 1, 0, 2, 0, ntan=2 ** 30, u=some) == uns  # K (p + m) = 2^31
        assert call(box, 2, 2 ** 20, 4, 0, ntan=2 ** 10 - 1, u=some) == qpgpu.SUCCESS
        assert call(box, 2, 2 ** 20, 4, 0, ntan=2 ** 10, u=some) == uns  # K n p = 2^31
        assert call(box, 64, 0, 128, 0, ntan=2 ** 19, flags=qpgpu.FLAG_EXACT, u=some) == inv
    assert call(False, 64, 0, 0, 0, ntan=2 ** 19 - 1) == qpgpu.SUCCESS  # K n n = 2^31 - 4096
    assert call(False, 64, 0, 0, 0, ntan=2 ** 19) == uns  # K n n = 2^31
    assert call(False, 2, 0, 2 ** 20, 0, ntan=2 ** 10 - 1, u=some) == qpgpu.SUCCESS
    assert call(False, 2, 0, 2 ** 20, 0, ntan=2 ** 10, u=some) == uns  # K n m = 2^31
    assert call(False, 1, 0, 2 ** 30, 0, ntan=1, u=some) == qpgpu.SUCCESS
    assert call(False, 1, 0, 2 ** 30, 0, ntan=2, u=some) == uns
    assert call(False, 7, 0, 14, 4, u=some, rest=some, CI=None) == inv  # NULL CI with m > 0
    assert call(True, 7, 0, 13, 0, u=some) == inv  # box with m != 2n
    assert call(True, 65, 0, 13, 0, u=some) == inv  # ... before the shape rule
    assert call(True, 7, 0, 13, 0, ntan=2 ** 30, u=some) == inv
    assert call(False, 7, 0, 13, 0, u=some) == qpgpu.SUCCESS
    assert call(False, 3, 0, 0, 0) == qpgpu.SUCCESS  # p + m == 0: u may be NULL
    assert call(False, 300, 0, 0, 0) == uns
    assert qpgpu.LIB.qpgpu_jvp_many(None, 2, *([some] * 15), None) == inv
    assert qpgpu.LIB.qpgpu_jvp_box_many(None, 2, *([some] * 14), None) == inv


# ---- the restatement: sharing the factorisation changes no bit ----------------------------------------
KKT_CASES = sorted(c for c, pr in dual_ref.kkt_cases().items() if pr.n <= 64)
BOX_CASES = sorted(c for c, bp in box_ref.cases().items() if bp.n <= 64)
MAX_PAIRS = 200  # (QP, direction) pairs per case through the per-slice restatement


def _head(pr, arrays, K):
    """The first QPs of a case: at most MAX_PAIRS (QP, direction) pairs."""
    B = max(1, min(pr.batch, MAX_PAIRS // K))
    return pr.slice(0, B), [a[:B] for a in arrays]


@pytest.mark.parametrize("cid", KKT_CASES)
def test_direction_k_has_the_bits_of_the_single_direction_definition(cid):
    pr, (x, st, u) = _head(dual_ref.case(cid), [dual_ref.reference(cid)[i] for i in (0, 2, 4)], K)
    uu = u if pr.p + pr.m else None
    tan = jvp_many_ref.make_many_tangents(pr, K)
    for status in (st, None):
        many = jvp_many_ref.jvp_many(pr, x, uu, tan, K, status)
        assert many["tx"].shape == (pr.batch, K, pr.n) and many["tf"].shape == (pr.batch, K)
        assert many["tu"].shape == (pr.batch, K, pr.p + pr.m)
        for k in range(K):
            one = jvp_ref.jvp(pr, x, uu, jvp_many_ref.slice_tangents(tan, k), status)
            for name in jvp_ref.OUTPUTS:
                assert same_bits(many[name][:, k], one[name]), f"{cid} direction {k} {name}"


@pytest.mark.parametrize("cid", BOX_CASES)
def test_box_direction_k_has_the_bits_of_the_single_direction_definition(cid):
    bp, (x, st, u) = _head(box_ref.case(cid), [box_dual_ref.reference(cid)[i] for i in (0, 2, 4)], K)
    tan = jvp_many_ref.make_many_tangents(bp, K)
    for status in (st, None):
        many = jvp_many_ref.jvp_box_many(bp, x, u, tan, K, status)
        for k in range(K):
            one = jvp_ref.jvp_box(bp, x, u, jvp_many_ref.slice_tangents(tan, k), status)
            for name in jvp_ref.OUTPUTS:
                assert same_bits(many[name][:, k], one[name]), f"{cid} direction {k} {name}"


def test_make_many_tangents_stacks_the_seeds():
    pr = dual_ref.case("lane_7_6_14")
    tan = jvp_many_ref.make_many_tangents(pr, K)
    for k in range(K):
        for name, t in jvp_ref.make_tangents(pr, seed=k).items():
            assert tan[name].shape == (pr.batch, K) + t.shape[1:]
            assert same_bits(tan[name][:, k], t)


@pytest.mark.parametrize("cid", ["lane_7_6_14", "wave_30_6_60"])
def test_each_tangent_alone_null_is_the_single_direction_definition(cid):
    pr, (x, st, u) = _head(dual_ref.case(cid), [dual_ref.reference(cid)[i] for i in (0, 2, 4)], 2 * len(jvp_ref.DENSE_TANGENTS))
    tan = jvp_many_ref.make_many_tangents(pr, 2)
    for drop in jvp_ref.DENSE_TANGENTS:
        tn = {k: v for k, v in tan.items() if k != drop}
        many = jvp_many_ref.jvp_many(pr, x, u, tn, 2, st)
        for k in range(2):
            one = jvp_ref.jvp(pr, x, u, jvp_many_ref.slice_tangents(tn, k), st)
            for name in jvp_ref.OUTPUTS:
                assert same_bits(many[name][:, k], one[name]), f"{cid} without {drop}, direction {k} {name}"


def test_null_tangents_are_zero_tangents():
    cid = "lane_7_6_14"
    pr = dual_ref.case(cid)
    x, f, st, it, u, nact = dual_ref.reference(cid)
    t = jvp_many_ref.jvp_many(pr, x, u, {}, K, st)
    for k, v in t.items():
        assert v.shape[:2] == (pr.batch, K) and np.all(v == 0), k


@pytest.mark.parametrize("cid", ["edge_infeasible", "edge_not_pd", "edge_dependent"])
def test_masked_qps_are_zero(cid):
    pr = dual_ref.case(cid)
    x, f, st, it, u, nact = dual_ref.reference(cid)
    assert np.all(st != qpgpu.QP_OK)
    t = jvp_many_ref.jvp_many(pr, x, u if pr.p + pr.m else None, jvp_many_ref.make_many_tangents(pr, K), K, st)
    for k, v in t.items():
        assert not np.any(v.view(np.uint64)), f"{cid} {k}"  # +0.0 exactly in all K blocks


def test_more_working_columns_than_variables_is_nan():
    pr = qp_cases.make("general", 3, 0, 8, 2, seed=5)
    x = np.ones((2, 3))
    u = np.ones((2, 8))
    u[1, 3:] = 0.0  # QP 1: q = 3 = n, still defined
    t = jvp_many_ref.jvp_many(pr, x, u, jvp_many_ref.make_many_tangents(pr, K), K)
    for k, v in t.items():
        assert np.all(np.isnan(v[0])), k  # all K blocks
        assert not np.any(np.isnan(v[1])), k
