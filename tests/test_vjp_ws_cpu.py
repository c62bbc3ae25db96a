"""qpgpu_vjp_ws / qpgpu_vjp_box_ws without a device: the export surface, the kernel names, the
workspace size, the argument rules (those of tests/test_vjp_cpu.py through the new entries, then the
workspace's own), and the definition's restatement (tests/vjp_ref.py) on the n > 64 cases the GPU
tests use — against one dense solve of the KKT system, and the box form against the dense one.

Bar, by the convention of tests/test_vjp_cpu.py (100 x the worst value measured with the restatement
alone, under its cap of 1e-8):
  vs the dense KKT solve   worst 4.226e-15 of the largest gradient entry (g_129_70_40; c5_256_0_512
                           4.107e-15, ws_100_20_200 4.069e-15)   -> KKT_MAX = 4.3e-13
"""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import box_ref
import dual_ref
import qpgpu
import vjp_ref
import vjp_ws_cases as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("qpgpu_vjp_workspace_bytes", "qpgpu_vjp_ws", "qpgpu_vjp_box_ws", "qpgpu_kernel_name_vjp_ws")
KKT_MAX = 4.3e-13


def test_symbols_declared_listed_and_exported():
    hdr = open(os.path.join(ROOT, "include", "qpgpu.h")).read()
    out = subprocess.check_output(["nm", "-D", "--defined-only", qpgpu.LIB_PATH]).decode()
    for name in NEW_SYMBOLS:
        assert re.search(rf"\b{name}\s*\(", hdr), f"{name} is not declared in include/qpgpu.h"
        assert name in qpgpu.EXPORTED_SYMBOLS
        assert re.search(rf"\bT {name}$", out, flags=re.M), f"{name} is not exported by libqpgpu.so"
    assert qpgpu.LIB.qpgpu_abi_version() == 1


def test_kernel_names():
    for n in (1, 7, 8, 9, 16, 17, 32, 33, 64):
        assert qpgpu.kernel_name_vjp_ws(n, 2, 20) == qpgpu.kernel_name_vjp(n, 2, 20) != ""
    for n in (65, 66, 100, 129, 255, 256):
        assert "ws" in qpgpu.kernel_name_vjp_ws(n, 0, 2 * n)
        assert qpgpu.kernel_name_vjp(n, 0, 2 * n) == ""  # the entries without a workspace stay as they were
    for n in (257, 0, -1):
        assert qpgpu.kernel_name_vjp_ws(n, 0, 0) == ""


def _bytes(n, p, m, slots, out=True):
    d = qpgpu.ProblemDesc(n, p, m, 0, 0, 0, 0)
    b = ctypes.c_int64(-1)
    rc = qpgpu.LIB.qpgpu_vjp_workspace_bytes(ctypes.byref(d), slots, ctypes.byref(b) if out else None)
    return rc, b.value


def test_workspace_bytes():
    for n in (1, 8, 33, 64):
        assert _bytes(n, 2, 2 * n, 5) == (qpgpu.SUCCESS, 0)
    for n in (65, 100, 256):
        rc, one = _bytes(n, 0, 2 * n, 1)
        assert rc == qpgpu.SUCCESS and one > 0 and one % 8 == 0
        assert one == 8 * (3 * n * n + n)  # the header's formula
        assert one >= 8 * (2 * n * n + n * (n + 1))  # L, M with gx as an extra column, S
        for slots in (2, 3, 512):
            assert _bytes(n, 0, 2 * n, slots) == (qpgpu.SUCCESS, slots * one)
        assert _bytes(n, 5, 7, 3) == (qpgpu.SUCCESS, 3 * one)  # p and m do not enter
        assert qpgpu.vjp_workspace_bytes(n, 0, 2 * n, 4) == 4 * one
    inv = qpgpu.ERR_INVALID_ARGUMENT
    assert _bytes(65, 0, 130, 0)[0] == inv and _bytes(65, 0, 130, -1)[0] == inv
    assert _bytes(7, 0, 14, 0)[0] == inv
    assert _bytes(65, 0, 130, 1, out=False)[0] == inv
    assert _bytes(257, 0, 0, 1)[0] == qpgpu.ERR_UNSUPPORTED_SHAPE


def test_argument_rules_without_a_device():
    """The C entries with NULL or dummy arrays: every rule checked here is decided before any array is
    read and before anything is launched (no call below reaches the device)."""
    buf = (ctypes.c_double * 64)()
    some = ctypes.cast(buf, ctypes.c_void_p)
    per65 = 8 * (3 * 65 * 65 + 65)

    def call(box, n, p, m, batch, flags=0, u=None, rest=None, ws=some, ws_bytes=1 << 40, **named):
        d = qpgpu.ProblemDesc(n, p, m, 0, batch, flags, 0)
        names = ["G", "CE"] + ([] if box else ["CI"]) + ["x", "u", "status", "gx"]
        args = {k: rest for k in names}
        args.update(u=u, status=None)
        args.update(named)
        fn = qpgpu.LIB.qpgpu_vjp_box_ws if box else qpgpu.LIB.qpgpu_vjp_ws
        return fn(ctypes.byref(d), *[args[k] for k in names], *([rest] * 6), ws, ws_bytes, None)

    inv, uns = qpgpu.ERR_INVALID_ARGUMENT, qpgpu.ERR_UNSUPPORTED_SHAPE
    for box in (False, True):
        for n in (7, 65):  # the rules of test_vjp_cpu.py, on both sides of the kernel boundary
            m = 2 * n
            assert call(box, n, 0, m, 0, u=some) == qpgpu.SUCCESS  # batch = 0
            assert call(box, n, 0, m, 0, u=some, ws=None, ws_bytes=0) == qpgpu.SUCCESS
            assert call(box, n, 0, m, 0, flags=qpgpu.FLAG_EXACT, u=some) == inv  # non-zero flags
            assert call(box, n, 0, m, 0, flags=qpgpu.FLAG_FORCE_GENERIC, u=some) == inv
            assert call(box, n, 0, m, 0) == inv  # NULL u with p + m > 0
            assert call(box, n, 0, m, 4, u=some) == inv  # NULL G, x, gx
            for missing in ("G", "x", "gx"):
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
    """n <= 64 is the launch without a workspace: NULL and 0 bytes are accepted with batch > 0.  The
    call is made with batch = 0 here (nothing may reach the device in this file); with batch > 0 it is
    tests/test_gpu_vjp_ws.py::test_on_chip_shapes_through_the_new_entry."""
    d = qpgpu.ProblemDesc(64, 0, 128, 0, 0, 0, 0)
    buf = (ctypes.c_double * 8)()
    some = ctypes.cast(buf, ctypes.c_void_p)
    rc = qpgpu.LIB.qpgpu_vjp_ws(ctypes.byref(d), *([some] * 5), None, some, *([None] * 6), None, 0, None)
    assert rc == qpgpu.SUCCESS


# ---- the definition on the reference's own pairs ---------------------------------------------------
def _rel_per_qp(got: dict, want: dict) -> np.ndarray:
    B = next(iter(want.values())).shape[0]
    num, den = np.zeros(B), np.zeros(B)
    for k, w in want.items():
        if w.size:
            num = np.maximum(num, np.max(np.abs(got[k] - w).reshape(B, -1), axis=1))
            den = np.maximum(den, np.max(np.abs(w).reshape(B, -1), axis=1))
    return num / den


KKT_CASES = list(W.DENSE_CASES) + sorted(c for c, pr in dual_ref.kkt_cases().items() if pr.n > 64)


@pytest.mark.parametrize("cid", KKT_CASES)
def test_restatement_vs_dense_kkt_solve(cid):
    """Measured worst over the list: 4.226e-15 (g_129_70_40; c5_256_0_512 4.107e-15, ws_100_20_200
    4.069e-15, n100_general 2.6e-15, ws_65_2_130 2.1e-15, general_65_2_130 9.1e-16)."""
    if cid in W.DENSE_CASES:
        pr, x, u, st, gx = W.pair(cid)
    else:
        pr = dual_ref.case(cid)
        x, f, st, it, u, nact = dual_ref.reference(cid)
        gx = vjp_ref.make_gx(pr)
    assert pr.n > 64
    ok = (st == qpgpu.QP_OK) & np.all(np.isfinite(x), axis=1)
    assert ok.all()
    got = W.want(cid, False) if cid in W.DENSE_CASES else vjp_ref.vjp(pr, x, u, gx)
    want = vjp_ref.dense_kkt(pr, x, u, gx)
    rel = _rel_per_qp(got, want)
    print(f"{cid}: {pr.batch} QPs, worst relative difference to the dense KKT solve {rel.max():.3e}")
    assert np.all(rel <= KKT_MAX), f"{cid}: {rel.max():.3e}"


def test_cases_have_the_working_sets_the_kernel_is_tested_on():
    q = lambda cid: [int(W.pair(cid)[0].p + (W.pair(cid)[2][b, W.pair(cid)[0].p:] != 0).sum())
                     for b in range(W.pair(cid)[0].batch)]
    assert all(26 <= v <= 29 for v in q("ws_65_2_130"))
    assert all(59 <= v <= 61 for v in q("ws_100_20_200"))
    assert all(v > 64 for v in q("g_129_70_40"))  # S spans more than one wave of rows
    assert q("c5_256_0_512") == [149]
    assert q("free_66_0_0") == [0, 0] and q("eq_256_256_0") == [256]  # the ends of q
    for cid in W.EDGE_CASES:
        assert np.all(W.pair(cid)[3] == qpgpu.QP_OK)
        assert all(np.all(np.isfinite(v)) for v in W.want(cid, True).values())
    pr, x, u, st, gx = W.pair(W.NAN_CASE)
    assert q(W.NAN_CASE)[0] == 70 > pr.n
    for masked in (True, False):
        g = W.want(W.NAN_CASE, masked)
        for k, v in g.items():
            assert np.all(np.isnan(v[0])), k  # q > n
            assert not np.any(np.isnan(v[2])), k
            if masked:
                assert not np.any(v[1].view(np.uint64)), k  # +0.0 exactly
        if not masked:
            assert np.any(np.isnan(g["dg0"][1]))  # NaN from the arithmetic


@pytest.mark.parametrize("cid", W.BOX_CASES)
def test_box_form_equals_dense_form(cid):
    bp, x, u, st, gx = W.box_pair(cid)
    n, p = bp.n, bp.p
    assert n > 64 and np.all(st == qpgpu.QP_OK)
    # both an upper and a lower bound active in every QP
    assert np.all(np.any(u[:, p:p + n] != 0, axis=1) & np.any(u[:, p + n:] != 0, axis=1))
    for masked in (True, False):
        gb = W.box_want(cid, masked)
        want = W.box_as_dense(W.box_dense_want(cid, masked), n)
        assert not vjp_ref.mismatches(gb, want), f"{cid}: {vjp_ref.mismatches(gb, want)}"
        off = u[:, p + n:] == 0
        assert not np.any(gb["dlo"][off & ~np.isnan(gb["dlo"])].view(np.uint64)), f"{cid}: dlo of an inactive bound"
    assert box_ref.dense(cid).m == 2 * n
