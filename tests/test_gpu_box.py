"""qpgpu_solve_batched_box on the GPU: x, f, status and iters of every kernel family and both
layouts, bit for bit against the oracle on the materialised problem (tests/box_ref.py; its case
list is vetted on the CPU by tests/test_box_cpu.py).  NaNs compare equal to NaNs.  x and f are
filled with NaN and status and iters with -7 before every solve, so a slot the kernel did not
write shows; in the TILED64 layout the padding entries of x must still hold that NaN afterwards.
All batches are small."""
import ctypes

import numpy as np
import pytest

import box_ref
import qpgpu

pytestmark = pytest.mark.gpu

FAMILIES = (None, "lane", "subgroup", "wave", "generic")
LAYOUTS = ("qp_major", "tiled64")


def covers(family, n):
    """The shapes (n, p, 2n) each family's box kernels cover (include/qpgpu.h)."""
    if family == "lane":
        return n <= 8
    if family == "subgroup":
        return n <= 16
    if family == "wave":
        return n <= 256
    return True  # generic, and the default order, take any shape


def _bit_mismatch(a, b, show=6):
    a = np.ascontiguousarray(a, dtype=np.float64).ravel()
    b = np.ascontiguousarray(b, dtype=np.float64).ravel()
    assert a.shape == b.shape
    diff = (a.view(np.uint64) != b.view(np.uint64)) & ~(np.isnan(a) & np.isnan(b))
    return [(int(i), float(a[i]).hex(), float(b[i]).hex()) for i in np.where(diff)[0][:show]]


def _prefill(db):
    db.x.fill_(float("nan"))
    db.f.fill_(float("nan"))
    db.status.fill_(-7)
    db.iters.fill_(-7)


def run_box(bp, family=None, layout=None, max_iter=0, write_factor=False, stream=None):
    """One box solve through DeviceBoxBatch: (x, f, status, iters) and the batch object."""
    import torch

    db = qpgpu.DeviceBoxBatch(bp, "cuda:0", layout=layout)
    _prefill(db)
    db.solve(max_iter=max_iter, family=family, write_factor=write_factor, stream=stream)
    torch.cuda.synchronize()
    if db.layout == qpgpu.LAYOUT_TILED64 and bp.batch % 64:
        # padding QPs of the last tile: slots b >= B of every element row stay as prefilled
        xt = db.x.cpu().numpy().reshape(-1, bp.n, 64)
        assert np.all(np.isnan(xt[-1][:, bp.batch % 64:])), "a padding entry of x was written"
    return db.results(), db


def assert_matches(got, ref, label, x_rows=None):
    x, f, st, it = got
    xr, fr, sr, ir = ref
    assert np.array_equal(st, sr), f"{label}: status differs at {np.where(st != sr)[0][:8]}: {st[st != sr][:8]} vs {sr[st != sr][:8]}"
    assert np.array_equal(it, ir), f"{label}: l1 passes differ at {np.where(it != ir)[0][:8]}"
    assert not _bit_mismatch(f, fr), f"{label}: f (index, gpu, ref) {_bit_mismatch(f, fr)}"
    # the reference leaves x of a QP whose G is not positive definite unwritten: so does the GPU
    rows = sr != qpgpu.QP_NOT_POSITIVE_DEFINITE if x_rows is None else x_rows
    assert not _bit_mismatch(x[rows], xr[rows]), f"{label}: x (index, gpu, ref) {_bit_mismatch(x[rows], xr[rows])}"
    assert np.all(np.isnan(x[~rows])), f"{label}: x of a not-positive-definite QP was written"


def _family_params():
    out = []
    for cid, bp in box_ref.cases().items():
        for fam in FAMILIES:
            if covers(fam, bp.n):
                for lay in LAYOUTS:
                    out.append(pytest.param(cid, fam, lay, id=f"{cid}-{fam or 'default'}-{lay}"))
    return out


@pytest.mark.parametrize("cid,family,layout", _family_params())
def test_bitwise_against_oracle(gpu, cid, family, layout):
    bp = box_ref.case(cid)
    flag = qpgpu.FAMILY_FLAGS[family]
    assert "box" in qpgpu.kernel_name_box(bp.n, bp.p, flag)
    got, _ = run_box(bp, family=family, layout=layout)
    assert_matches(got, box_ref.reference(cid), f"{cid} {family} {layout}")


@pytest.mark.parametrize("cid,family", [("lane_7_3", "lane"), ("subgroup_14_10", "subgroup"),
                                        ("wave_lds_30_6", "wave"), ("wave_ws_65_0", "wave"),
                                        ("long_7_3", "generic")])
def test_equals_dense_exact_entry(gpu, cid, family):
    """The same bits as qpgpu_solve_batched with QPGPU_FLAG_EXACT on to_dense()."""
    import torch

    got, _ = run_box(box_ref.case(cid), family=family)
    db = qpgpu.DeviceBatch(box_ref.dense(cid), "cuda:0")
    db.solve(exact=True, family=family)
    torch.cuda.synchronize()
    x, f, st, it = db.results()
    assert_matches(got, (x, f, st, it), f"{cid} {family} vs dense", x_rows=np.ones(len(f), dtype=bool))


@pytest.mark.parametrize("family", ["lane", "subgroup", "wave", "generic"])
def test_step_cap(gpu, family):
    """max_iter = 1 on the long-paths case: the capped QPs match the oracle under the same cap."""
    cid = "long_7_3"
    ref = box_ref.reference(cid, 1)
    assert (ref[2] == qpgpu.QP_MAX_ITER).any()
    got, _ = run_box(box_ref.case(cid), family=family, max_iter=1)
    assert_matches(got, ref, f"max_iter = 1 {family}")


def test_write_factor(gpu):
    """QPGPU_FLAG_WRITE_FACTOR on (14, 10): G receives the factor the dense entry writes."""
    import torch

    cid = "subgroup_14_10"
    bp = box_ref.case(cid)
    for family in (None, "subgroup", "generic"):
        got, db = run_box(bp, family=family, write_factor=True)
        assert_matches(got, box_ref.reference(cid), f"write_factor {family}")
        dd = qpgpu.DeviceBatch(box_ref.dense(cid), "cuda:0")
        dd.solve(exact=True, write_factor=True, family=family)
        torch.cuda.synchronize()
        assert not _bit_mismatch(db.G.cpu().numpy(), dd.G.cpu().numpy())
        assert _bit_mismatch(db.G.cpu().numpy(), bp.G), "G was not overwritten"


def _raw_call(bp, flags=0, hi_null=False, lo_null=False):
    import torch

    db = qpgpu.DeviceBoxBatch(bp, "cuda:0")
    d = qpgpu.ProblemDesc(bp.n, bp.p, 2 * bp.n, 0, bp.batch, flags, 0)
    vp = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    rc = qpgpu.LIB.qpgpu_solve_batched_box(
        ctypes.byref(d), vp(db.G), vp(db.g0), vp(db.CE), vp(db.ce0), None if hi_null else vp(db.hi),
        None if lo_null else vp(db.lo), vp(db.x), vp(db.f), vp(db.status), vp(db.iters),
        ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc


def test_argument_rules(gpu):
    bp = box_ref.case("lane_7_3")
    assert _raw_call(bp) == qpgpu.SUCCESS
    assert _raw_call(bp, flags=qpgpu.FLAG_FAST) == qpgpu.ERR_INVALID_ARGUMENT
    assert _raw_call(bp, hi_null=True) == qpgpu.ERR_INVALID_ARGUMENT
    assert _raw_call(bp, lo_null=True) == qpgpu.ERR_INVALID_ARGUMENT
    assert _raw_call(bp, flags=qpgpu.FLAG_EXACT) == qpgpu.SUCCESS  # implied anyway
    big = box_ref.case("wave_lds_30_6")
    assert _raw_call(big, flags=qpgpu.FLAG_FORCE_LANE) == qpgpu.ERR_UNSUPPORTED_SHAPE
    assert _raw_call(big, flags=qpgpu.FLAG_FORCE_SUBGROUP) == qpgpu.ERR_UNSUPPORTED_SHAPE
    assert _raw_call(box_ref.case("subgroup_9_1"), flags=qpgpu.FLAG_FORCE_LANE) == qpgpu.ERR_UNSUPPORTED_SHAPE
    assert _raw_call(box_ref.case("generic_260_0"), flags=qpgpu.FLAG_FORCE_WAVE) == qpgpu.ERR_UNSUPPORTED_SHAPE


def test_null_ce_with_p0(gpu):
    """CE and ce0 may be NULL when p = 0 (a torch tensor of no elements has a NULL data_ptr)."""
    import torch

    bp = box_ref.case("lane_7_0")
    for family in ("lane", "subgroup", "wave", "generic"):
        db = qpgpu.DeviceBoxBatch(bp, "cuda:0")
        db.CE = db.ce0 = None
        _prefill(db)
        db.solve(family=family)
        torch.cuda.synchronize()
        assert_matches(db.results(), box_ref.reference("lane_7_0"), f"NULL CE {family}")


@pytest.mark.parametrize("layout,B", [("qp_major", 10), ("tiled64", 150)])
def test_generic_sub_batches(gpu, layout, B):
    """hi and lo are offset per sub-batch like x: a workspace cap of three QPs against one launch
    and against the oracle."""
    import oracle

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
    ref = oracle.solve_batch(bp.to_dense(), max_steps=box_ref.default_cap(n, p))
    one, _ = run_box(bp, family="generic", layout=layout)
    setcap(3 * per)
    try:
        sub, _ = run_box(bp, family="generic", layout=layout)
    finally:
        setcap(0)
    assert_matches(one, ref, f"one launch {layout} B={B}")
    assert_matches(sub, ref, f"sub-batches {layout} B={B}")


@pytest.mark.parametrize("cid,B", [("lane_7_0", 128), ("wave_ws_65_0", 3)])
def test_graph_capture(gpu, cid, B):
    """One capture and replay (as tests/test_gpu_graph.py) after a warm-up call on the capturing
    stream: replay = eager."""
    import torch

    bp = box_ref.case(cid).slice(0, B)
    eager, _ = run_box(bp)
    dev = torch.device("cuda", 0)
    db = qpgpu.DeviceBoxBatch(bp, dev)
    s = torch.cuda.Stream(dev)
    with torch.cuda.stream(s):
        db.solve(stream=s)  # warm-up: the workspace and the LDS grant exist before the capture
    s.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        db.solve(stream=s)
    _prefill(db)
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    assert_matches(db.results(), eager, f"graph replay {cid}")
    xr, fr, sr, ir = box_ref.reference(cid)
    assert_matches(db.results(), (xr[:B], fr[:B], sr[:B], ir[:B]), f"graph replay {cid} vs oracle")


def test_launcher(gpu):
    import torch

    cid = "lane_5_2"
    db = qpgpu.DeviceBoxBatch(box_ref.case(cid), "cuda:0", layout="tiled64")
    _prefill(db)
    db.launcher(torch.cuda.current_stream())()
    torch.cuda.synchronize()
    assert_matches(db.results(), box_ref.reference(cid), "launcher")


def test_convenience_wrapper(gpu):
    cid = "subgroup_9_1"
    bp = box_ref.case(cid)
    for layout in LAYOUTS:
        got = qpgpu.solve_batched_box(bp, layout=layout)
        assert got[0].shape == (bp.batch, bp.n)
        xr, fr, sr, ir = box_ref.reference(cid)
        assert np.array_equal(got[2], sr) and np.array_equal(got[3], ir)
        assert not _bit_mismatch(got[1], fr) and not _bit_mismatch(got[0], xr)
