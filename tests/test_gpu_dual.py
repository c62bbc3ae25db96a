"""qpgpu_solve_batched_dual on the GPU: the multipliers u and the active-set size nact of every
kernel family, bit for bit against tests/dual_ref.py (the CPU restatement with an export hook),
with x, f, status and iters.  NaNs compare as in test_gpu_parity._bit_mismatch; -0.0 and +0.0 in
u are different values (an inactive slot must be +0.0).  u and nact are filled with NaN and -7
before every solve, so a slot the kernel did not write shows.  All batches are small."""
import ctypes

import numpy as np
import pytest

import dual_ref
import qp_cases
import qpgpu

pytestmark = pytest.mark.gpu

FAMILIES = (None, "lane", "subgroup", "wave", "generic")
LAYOUTS = ("qp_major", "tiled64")


def covers(family, n, m):
    """The shapes each family's kernels cover (include/qpgpu.h)."""
    if family == "lane":
        return n <= 8 and m <= 16
    if family == "subgroup":
        return n <= 16 and m <= 64
    if family == "wave":
        return n <= 256 and m <= 1024
    return True  # generic, and the default order, take any shape


def _bit_mismatch(a, b, show=6):
    a = np.ascontiguousarray(a, dtype=np.float64).ravel()
    b = np.ascontiguousarray(b, dtype=np.float64).ravel()
    assert a.shape == b.shape
    diff = (a.view(np.uint64) != b.view(np.uint64)) & ~(np.isnan(a) & np.isnan(b))
    return [(int(i), float(a[i]).hex(), float(b[i]).hex()) for i in np.where(diff)[0][:show]]


def run_dual(pr, family=None, layout=None, max_iter=0, u_null=False, nact_null=False, write_factor=False):
    """One dual solve through DeviceBatch: (x, f, status, iters, u, nact), u as (B, p + m)."""
    import torch

    db = qpgpu.DeviceBatch(pr, "cuda:0", layout=layout)
    B, E = pr.batch, pr.p + pr.m
    rows = (B + 63) // 64 * 64 if db.layout == qpgpu.LAYOUT_TILED64 else B
    u = None if u_null else torch.full((rows, E), float("nan"), dtype=torch.float64, device="cuda:0")
    nact = None if nact_null else torch.full((B,), -7, dtype=torch.int32, device="cuda:0")
    db.solve(max_iter=max_iter, family=family, write_factor=write_factor, dual_out=(u, nact))
    torch.cuda.synchronize()
    x, f, st, it = db.results()
    uh = None
    if u is not None:
        uh = u.cpu().numpy()
        uh = qpgpu.from_tiled64(uh.reshape(-1), B, (E,)) if db.layout == qpgpu.LAYOUT_TILED64 else uh
    return x, f, st, it, uh, None if nact is None else nact.cpu().numpy()


def assert_matches_ref(got, ref, label):
    x, f, st, it, u, nact = got
    xr, fr, sr, ir, ur, nr = ref
    assert np.array_equal(st, sr), f"{label}: status differs at {np.where(st != sr)[0][:8]}"
    assert np.array_equal(it, ir), f"{label}: l1 passes differ at {np.where(it != ir)[0][:8]}"
    assert not _bit_mismatch(f, fr), f"{label}: f (index, gpu, ref) {_bit_mismatch(f, fr)}"
    assert not _bit_mismatch(x, xr), f"{label}: x (index, gpu, ref) {_bit_mismatch(x, xr)}"
    if u is not None:
        assert not _bit_mismatch(u, ur), f"{label}: u (index, gpu, ref) {_bit_mismatch(u, ur)}"
    if nact is not None:
        assert np.array_equal(nact, nr), f"{label}: nact differs at {np.where(nact != nr)[0][:8]}"


def _family_params():
    out = []
    for cid, pr in dual_ref.gpu_cases().items():
        for fam in FAMILIES:
            if covers(fam, pr.n, pr.m):
                for lay in LAYOUTS:
                    out.append(pytest.param(cid, fam, lay, id=f"{cid}-{fam or 'default'}-{lay}"))
    return out


@pytest.mark.parametrize("cid,family,layout", _family_params())
def test_bitwise_against_reference(gpu, cid, family, layout):
    pr = dual_ref.case(cid)
    got = run_dual(pr, family=family, layout=layout, u_null=(pr.p + pr.m == 0))
    assert_matches_ref(got, dual_ref.reference(cid), f"{cid} {family} {layout}")


@pytest.mark.parametrize("cid", sorted(dual_ref.fuzz_cases()))
def test_fuzz_bitwise(gpu, cid):
    """Rollback, dual-step and rank-deficient paths (qp_cases.fuzz_case), default family."""
    pr = dual_ref.case(cid)
    got = run_dual(pr, u_null=(pr.p + pr.m == 0))
    assert_matches_ref(got, dual_ref.reference(cid), cid)


@pytest.mark.parametrize("cid", ["lane_7_6_14", "wave_30_6_60"])
def test_primal_side_equals_plain_exact(gpu, cid):
    """x, f, status, iters of the dual entry = qpgpu_solve_batched with QPGPU_FLAG_EXACT."""
    import torch

    pr = dual_ref.case(cid)
    x, f, st, it, _, _ = run_dual(pr)
    db = qpgpu.DeviceBatch(pr, "cuda:0")
    db.solve(exact=True)
    torch.cuda.synchronize()
    xp, fp, sp, ip = db.results()
    assert np.array_equal(st, sp) and np.array_equal(it, ip)
    assert not _bit_mismatch(f, fp) and not _bit_mismatch(x, xp)


@pytest.mark.parametrize("layout,B", [("qp_major", 10), ("tiled64", 150)])
def test_generic_sub_batches(gpu, layout, B):
    """u and nact are offset per sub-batch like x and status: a workspace cap of three QPs against
    one launch."""
    n, p, m = 40, 5, 90
    qpgpu.LIB.qpk_generic_workspace_bytes.restype = ctypes.c_int64
    qpgpu.LIB.qpk_generic_workspace_bytes.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int64]
    per = qpgpu.LIB.qpk_generic_workspace_bytes(n, m, 1)
    setcap = qpgpu.LIB.qpgpu_debug_set_generic_ws_cap
    setcap.argtypes = [ctypes.c_int64]
    pr = qp_cases.make("general", n, p, m, B, seed=B + 1)
    one = run_dual(pr, family="generic", layout=layout)
    setcap(3 * per)
    try:
        sub = run_dual(pr, family="generic", layout=layout)
    finally:
        setcap(0)
    assert_matches_ref(sub, one, f"sub-batches {layout} B={B}")
    assert np.count_nonzero(one[4]) > 0 and not np.any(np.isnan(one[4]))


def _raw_call(pr, flags=0, u_null=False, nact_null=False, max_iter=0):
    import torch

    db = qpgpu.DeviceBatch(pr, "cuda:0")
    u = torch.zeros((pr.batch, max(1, pr.p + pr.m)), dtype=torch.float64, device="cuda:0")
    nact = torch.zeros(pr.batch, dtype=torch.int32, device="cuda:0")
    d = qpgpu.ProblemDesc(pr.n, pr.p, pr.m, max_iter, pr.batch, flags, 0)
    vp = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    rc = qpgpu.LIB.qpgpu_solve_batched_dual(
        ctypes.byref(d), vp(db.G), vp(db.g0), vp(db.CE), vp(db.ce0), vp(db.CI), vp(db.ci0), vp(db.x), vp(db.f),
        vp(db.status), vp(db.iters), None if u_null else vp(u), None if nact_null else vp(nact),
        ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc


def test_argument_rules(gpu):
    pr = dual_ref.case("lane_7_6_14")
    assert _raw_call(pr) == qpgpu.SUCCESS
    assert _raw_call(pr, flags=qpgpu.FLAG_FAST) == qpgpu.ERR_INVALID_ARGUMENT
    assert _raw_call(pr, u_null=True) == qpgpu.ERR_INVALID_ARGUMENT
    assert _raw_call(pr, nact_null=True) == qpgpu.SUCCESS
    assert _raw_call(dual_ref.case("degenerate_3_0_0"), u_null=True, nact_null=True) == qpgpu.SUCCESS
    big = dual_ref.case("wave_30_6_60")
    assert _raw_call(big, flags=qpgpu.FLAG_FORCE_LANE) == qpgpu.ERR_UNSUPPORTED_SHAPE
    assert _raw_call(big, flags=qpgpu.FLAG_FORCE_SUBGROUP) == qpgpu.ERR_UNSUPPORTED_SHAPE
    # nact == NULL changes nothing else
    got = run_dual(pr, nact_null=True)
    assert_matches_ref(got, dual_ref.reference("lane_7_6_14"), "nact NULL")


def test_step_cap_zeroes_u(gpu):
    cid = "edge_long_paths"
    ref = dual_ref.reference(cid, 1)
    got = run_dual(dual_ref.case(cid), max_iter=1)
    assert_matches_ref(got, ref, "max_iter = 1")
    capped = got[2] == qpgpu.QP_MAX_ITER
    assert capped.any()
    assert not np.any(got[4][capped].view(np.uint64)) and not np.any(got[5][capped])


def test_convenience_wrapper(gpu):
    cid = "subgroup_5_2_30"
    pr = dual_ref.case(cid)
    for layout in LAYOUTS:
        got = qpgpu.solve_batched_dual(pr, layout=layout)
        assert got[4].shape == (pr.batch, pr.p + pr.m)
        assert_matches_ref(got, dual_ref.reference(cid), f"solve_batched_dual {layout}")


def test_write_factor(gpu):
    """QPGPU_FLAG_WRITE_FACTOR works as in the plain entry and leaves u unchanged."""
    cid = "subgroup_14_10_28"
    assert_matches_ref(run_dual(dual_ref.case(cid), write_factor=True), dual_ref.reference(cid), "write_factor")


def test_graph_capture(gpu):
    """One capture and replay of the dual entry (as tests/test_gpu_graph.py): replay = eager."""
    import torch

    pr = qp_cases.make("general", 7, 6, 14, 128, seed=31)
    eager = run_dual(pr)
    dev = torch.device("cuda", 0)
    db = qpgpu.DeviceBatch(pr, dev)
    u = torch.full((128, 20), float("nan"), dtype=torch.float64, device=dev)
    nact = torch.full((128,), -7, dtype=torch.int32, device=dev)
    s = torch.cuda.Stream(dev)
    with torch.cuda.stream(s):
        db.solve(stream=s, dual_out=(u, nact))  # warm-up on the capturing stream
    s.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        db.solve(stream=s, dual_out=(u, nact))
    u.fill_(float("nan"))
    nact.fill_(-7)
    db.x.zero_()
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    x, f, st, it = db.results()
    assert_matches_ref((x, f, st, it, u.cpu().numpy(), nact.cpu().numpy()), eager, "graph replay")
