"""qpgpu_solve_batched_box_dual on the GPU: x, f, status, iters, the multipliers u and the
active-set size nact of every kernel family and both layouts, bit for bit against the reference on
the materialised problem (tests/box_dual_ref.py; its case list is vetted on the CPU by
tests/test_box_dual_cpu.py).  NaNs compare equal to NaNs; -0.0 and +0.0 in u are different values
(an inactive slot must be +0.0).  Before every solve x, f and u are filled with NaN and status,
iters and nact with -7, so a slot the kernel did not write shows; in the TILED64 layout the padding
entries of x and u must still hold that NaN afterwards.  All batches are small."""
import ctypes

import numpy as np
import pytest

import box_dual_ref
import box_ref
import dual_ref
import qpgpu
from test_gpu_box import _bit_mismatch, covers, run_box
from test_gpu_dual import run_dual

pytestmark = pytest.mark.gpu

FAMILIES = (None, "lane", "subgroup", "wave", "generic")
FORCED = ("lane", "subgroup", "wave", "generic")
LAYOUTS = ("qp_major", "tiled64")
FIVE = [("lane_7_3", "lane"), ("subgroup_14_10", "subgroup"), ("wave_lds_30_6", "wave"),
        ("wave_ws_65_0", "wave"), ("long_7_3", "generic")]


def _prefill(db, u, nact):
    db.x.fill_(float("nan"))
    db.f.fill_(float("nan"))
    db.status.fill_(-7)
    if db.iters is not None:
        db.iters.fill_(-7)
    if u is not None:
        u.fill_(float("nan"))
    if nact is not None:
        nact.fill_(-7)


def _dual_tensors(db, u_null=False, nact_null=False):
    import torch

    E = db.p + 2 * db.n
    rows = (db.batch + 63) // 64 * 64 if db.layout == qpgpu.LAYOUT_TILED64 else db.batch
    u = None if u_null else torch.empty((rows, E), dtype=torch.float64, device=db.x.device)
    nact = None if nact_null else torch.empty((db.batch,), dtype=torch.int32, device=db.x.device)
    return u, nact


def _collect(db, u, nact):
    """(x, f, status, iters, u, nact) as numpy, QP-major, after checking the TILED64 padding."""
    B, n, E = db.batch, db.n, db.p + 2 * db.n
    uh = None
    if db.layout == qpgpu.LAYOUT_TILED64 and B % 64:
        # padding QPs of the last tile: slots b >= B of every element row stay as prefilled
        xt = db.x.cpu().numpy().reshape(-1, n, 64)
        assert np.all(np.isnan(xt[-1][:, B % 64:])), "a padding entry of x was written"
        if u is not None:
            ut = u.cpu().numpy().reshape(-1, E, 64)
            assert np.all(np.isnan(ut[-1][:, B % 64:])), "a padding entry of u was written"
    if u is not None:
        uh = u.cpu().numpy()
        uh = qpgpu.from_tiled64(uh.reshape(-1), B, (E,)) if db.layout == qpgpu.LAYOUT_TILED64 else uh
        uh = uh.reshape(B, E)
    x, f, st, it = db.results()
    return x, f, st, it, uh, None if nact is None else nact.cpu().numpy()


def run_box_dual(bp, family=None, layout=None, max_iter=0, write_factor=False, nact_null=False, null_ce=False):
    """One box-dual solve through DeviceBoxBatch: (x, f, status, iters, u, nact) and the batch."""
    import torch

    db = qpgpu.DeviceBoxBatch(bp, "cuda:0", layout=layout)
    if null_ce:
        db.CE = db.ce0 = None
    u, nact = _dual_tensors(db, nact_null=nact_null)
    _prefill(db, u, nact)
    db.solve(max_iter=max_iter, family=family, write_factor=write_factor, dual_out=(u, nact))
    torch.cuda.synchronize()
    return _collect(db, u, nact), db


def assert_matches(got, ref, label, x_rows=None):
    x, f, st, it, u, nact = got
    xr, fr, sr, ir, ur, nr = ref
    assert np.array_equal(st, sr), f"{label}: status differs at {np.where(st != sr)[0][:8]}: {st[st != sr][:8]} vs {sr[st != sr][:8]}"
    assert np.array_equal(it, ir), f"{label}: l1 passes differ at {np.where(it != ir)[0][:8]}"
    assert not _bit_mismatch(f, fr), f"{label}: f (index, gpu, ref) {_bit_mismatch(f, fr)}"
    # the reference leaves x of a QP whose G is not positive definite unwritten: so does the GPU
    rows = sr != qpgpu.QP_NOT_POSITIVE_DEFINITE if x_rows is None else x_rows
    assert not _bit_mismatch(x[rows], xr[rows]), f"{label}: x (index, gpu, ref) {_bit_mismatch(x[rows], xr[rows])}"
    assert np.all(np.isnan(x[~rows])), f"{label}: x of a not-positive-definite QP was written"
    assert not _bit_mismatch(u, ur), f"{label}: u (index, gpu, ref) {_bit_mismatch(u, ur)}"
    if nact is not None:
        assert np.array_equal(nact, nr), f"{label}: nact differs at {np.where(nact != nr)[0][:8]}"


def _family_params():
    out = []
    for cid, bp in box_ref.cases().items():
        for fam in FAMILIES:
            if covers(fam, bp.n):
                for lay in LAYOUTS:
                    out.append(pytest.param(cid, fam, lay, id=f"{cid}-{fam or 'default'}-{lay}"))
    return out


@pytest.mark.parametrize("cid,family,layout", _family_params())
def test_bitwise_against_reference(gpu, cid, family, layout):
    bp = box_ref.case(cid)
    name = qpgpu.kernel_name_box_dual(bp.n, bp.p, qpgpu.FAMILY_FLAGS[family])
    assert "box" in name and "dual" in name
    got, _ = run_box_dual(bp, family=family, layout=layout)
    assert_matches(got, box_dual_ref.reference(cid), f"{cid} {family} {layout}")


@pytest.mark.parametrize("cid,family", FIVE)
def test_equals_dense_dual_entry(gpu, cid, family):
    """The same bits as qpgpu_solve_batched_dual on to_dense()."""
    got, _ = run_box_dual(box_ref.case(cid), family=family)
    dense = run_dual(box_ref.dense(cid), family=family)
    st = dense[2]
    # (run_dual starts from x = 0, this file from NaN: rows the kernels leave unwritten differ)
    assert_matches(got, dense, f"{cid} {family} vs dense dual", x_rows=st != qpgpu.QP_NOT_POSITIVE_DEFINITE)


@pytest.mark.parametrize("cid,family", FIVE)
def test_primal_side_equals_box_entry(gpu, cid, family):
    got, _ = run_box_dual(box_ref.case(cid), family=family)
    (x, f, st, it), _ = run_box(box_ref.case(cid), family=family)
    assert np.array_equal(got[2], st) and np.array_equal(got[3], it)
    assert not _bit_mismatch(got[1], f) and not _bit_mismatch(got[0], x)


@pytest.mark.parametrize("family", FORCED)
def test_step_cap(gpu, family):
    """max_iter = 1 on the long-paths case: capped QPs have an all-+0.0 u block and nact = 0, the
    rest match the reference under the same cap."""
    cid = "long_7_3"
    ref = box_dual_ref.reference(cid, 1)
    assert (ref[2] == qpgpu.QP_MAX_ITER).any()
    got, _ = run_box_dual(box_ref.case(cid), family=family, max_iter=1)
    assert_matches(got, ref, f"max_iter = 1 {family}")
    capped = got[2] == qpgpu.QP_MAX_ITER
    assert capped.any()
    assert not np.any(np.ascontiguousarray(got[4][capped]).view(np.uint64)) and not np.any(got[5][capped])


def _raw_call(bp, flags=0, m=None, hi_null=False, lo_null=False, u_null=False, nact_null=False):
    import torch

    db = qpgpu.DeviceBoxBatch(bp, "cuda:0")
    u, nact = _dual_tensors(db)
    d = qpgpu.ProblemDesc(bp.n, bp.p, 2 * bp.n if m is None else m, 0, bp.batch, flags, 0)
    vp = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    rc = qpgpu.LIB.qpgpu_solve_batched_box_dual(
        ctypes.byref(d), vp(db.G), vp(db.g0), vp(db.CE), vp(db.ce0), None if hi_null else vp(db.hi),
        None if lo_null else vp(db.lo), vp(db.x), vp(db.f), vp(db.status), vp(db.iters),
        None if u_null else vp(u), None if nact_null else vp(nact),
        ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc


def test_argument_rules(gpu):
    bp = box_ref.case("lane_7_3")
    inv = qpgpu.ERR_INVALID_ARGUMENT
    assert _raw_call(bp) == qpgpu.SUCCESS
    assert _raw_call(bp, flags=qpgpu.FLAG_FAST) == inv
    assert _raw_call(bp, u_null=True) == inv
    assert _raw_call(bp, hi_null=True) == inv
    assert _raw_call(bp, lo_null=True) == inv
    assert _raw_call(bp, m=2 * bp.n - 1) == inv
    assert _raw_call(bp, nact_null=True) == qpgpu.SUCCESS
    big = box_ref.case("wave_lds_30_6")
    assert _raw_call(big, flags=qpgpu.FLAG_FORCE_LANE) == qpgpu.ERR_UNSUPPORTED_SHAPE
    assert _raw_call(big, flags=qpgpu.FLAG_FORCE_SUBGROUP) == qpgpu.ERR_UNSUPPORTED_SHAPE
    assert _raw_call(box_ref.case("generic_260_0"), flags=qpgpu.FLAG_FORCE_WAVE) == qpgpu.ERR_UNSUPPORTED_SHAPE
    # nact == NULL changes nothing else
    got, _ = run_box_dual(bp, nact_null=True)
    assert got[5] is None
    assert_matches(got, box_dual_ref.reference("lane_7_3"), "nact NULL")


@pytest.mark.parametrize("family", FORCED)
def test_null_ce_with_p0(gpu, family):
    """CE and ce0 may be NULL when p = 0 (a torch tensor of no elements has a NULL data_ptr)."""
    got, _ = run_box_dual(box_ref.case("lane_7_0"), family=family, null_ce=True)
    assert_matches(got, box_dual_ref.reference("lane_7_0"), f"NULL CE {family}")


@pytest.mark.parametrize("layout,B", [("qp_major", 10), ("tiled64", 150)])
def test_generic_sub_batches(gpu, layout, B):
    """u, nact, hi and lo are offset per sub-batch like x: a workspace cap of three QPs against one
    launch and against the reference."""
    n, p = 12, 3
    qpgpu.LIB.qpk_generic_workspace_bytes.restype = ctypes.c_int64
    qpgpu.LIB.qpk_generic_workspace_bytes.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int64]
    per = qpgpu.LIB.qpk_generic_workspace_bytes(n, 2 * n, 1)
    setcap = qpgpu.LIB.qpgpu_debug_set_generic_ws_cap
    setcap.argtypes = [ctypes.c_int64]
    bp = qpgpu.make_box_problems(n, p, 0, B, seed=B + 1)
    rng = np.random.default_rng(B)
    bp.g0 *= 3.0
    bp.hi = rng.uniform(0.05, 1.5, (B, n))  # per-QP bounds: a wrong offset changes the answer
    bp.lo = -rng.uniform(0.05, 1.5, (B, n))
    ref = dual_ref.solve(bp.to_dense(), box_ref.default_cap(n, p))
    assert (ref[5] > 0).mean() >= 0.5 and len(set(ref[5].tolist())) > 1
    one, _ = run_box_dual(bp, family="generic", layout=layout)
    setcap(3 * per)
    try:
        sub, _ = run_box_dual(bp, family="generic", layout=layout)
    finally:
        setcap(0)
    assert_matches(one, ref, f"one launch {layout} B={B}")
    assert_matches(sub, ref, f"sub-batches {layout} B={B}")


def test_write_factor(gpu):
    """QPGPU_FLAG_WRITE_FACTOR on (14, 10): u is unchanged and G is the dense entry's factor."""
    import torch

    cid = "subgroup_14_10"
    bp = box_ref.case(cid)
    for family in (None, "subgroup", "generic"):
        got, db = run_box_dual(bp, family=family, write_factor=True)
        assert_matches(got, box_dual_ref.reference(cid), f"write_factor {family}")
        dd = qpgpu.DeviceBatch(box_ref.dense(cid), "cuda:0")
        dd.solve(exact=True, write_factor=True, family=family)
        torch.cuda.synchronize()
        assert not _bit_mismatch(db.G.cpu().numpy(), dd.G.cpu().numpy())
        assert _bit_mismatch(db.G.cpu().numpy(), bp.G), "G was not overwritten"


@pytest.mark.parametrize("cid,B", [("lane_7_0", 128), ("wave_ws_65_0", 3)])
def test_graph_capture(gpu, cid, B):
    """One capture and replay (as tests/test_gpu_graph.py) after a warm-up call on the capturing
    stream: replay = eager = reference."""
    import torch

    bp = box_ref.case(cid).slice(0, B)
    eager, _ = run_box_dual(bp)
    dev = torch.device("cuda", 0)
    db = qpgpu.DeviceBoxBatch(bp, dev)
    u, nact = _dual_tensors(db)
    s = torch.cuda.Stream(dev)
    with torch.cuda.stream(s):
        db.solve(stream=s, dual_out=(u, nact))  # warm-up: the workspace and the LDS grant exist before the capture
    s.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        db.solve(stream=s, dual_out=(u, nact))
    _prefill(db, u, nact)
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    got = _collect(db, u, nact)
    assert_matches(got, eager, f"graph replay {cid}")
    assert_matches(got, tuple(a[:B] for a in box_dual_ref.reference(cid)), f"graph replay {cid} vs reference")


def test_convenience_wrapper(gpu):
    cid = "subgroup_9_1"
    bp = box_ref.case(cid)
    for layout in LAYOUTS:
        got = qpgpu.solve_batched_box_dual(bp, layout=layout)
        assert got[0].shape == (bp.batch, bp.n) and got[4].shape == (bp.batch, bp.p + 2 * bp.n)
        xr, fr, sr, ir, ur, nr = box_dual_ref.reference(cid)
        assert np.array_equal(got[2], sr) and np.array_equal(got[3], ir) and np.array_equal(got[5], nr)
        assert not _bit_mismatch(got[1], fr) and not _bit_mismatch(got[0], xr) and not _bit_mismatch(got[4], ur)
