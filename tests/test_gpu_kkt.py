"""qpgpu_kkt_residuals / qpgpu_kkt_residuals_box on the GPU, bit for bit against the definition
(tests/kkt_ref.py).  The pairs (x, u) and the status words come from the CPU reference
(tests/dual_ref.py, tests/box_dual_ref.py), so only the new kernel is under test; the end-to-end
test is the one that runs a solve first.  NaN slots compare as NaN (payloads are not compared);
-0.0 and +0.0 are different values.  In the placement and graph tests r is pre-filled (a sentinel,
7.0), so a slot the kernel did not write shows.  All batches are small."""
import ctypes
import functools

import numpy as np
import pytest

import box_dual_ref
import box_ref
import dual_ref
import kkt_ref
import placement
import qp_cases
import qpgpu

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LAYOUTS = ("qp_major", "tiled64")
STATIONARITY_MAX = 1e-12
COMPLEMENTARITY_MAX = 1e-10
EQUALITY_MAX = 1e-10
INEQUALITY_MAX = 1e-10

# beyond dual_ref.GPU_SHAPES and the edge cases: one, a wave less one and a wave plus one QP at C1's
# shape, and two shapes with n > 256 (more than four 64-row blocks, the columns in a second sweep)
EXTRA = {
    "b1_7_6_14": (7, 6, 14, 1),
    "b63_7_6_14": (7, 6, 14, 63),
    "b65_7_6_14": (7, 6, 14, 65),
    "rt_257_1_3": (257, 1, 3, 2),
    "rt_300_2_10": (300, 2, 10, 2),
}


@functools.lru_cache(maxsize=None)
def extra_case(cid):
    n, p, m, B = EXTRA[cid]
    return qp_cases.make("general", n, p, m, B, seed=500 + n + B)


@functools.lru_cache(maxsize=None)
def pair(cid):
    """(problems, x, u, status, nact) of a named case from the CPU reference, left unchanged."""
    if cid in EXTRA:
        pr = extra_case(cid)
        x, f, st, it, u, nact = dual_ref.solve(pr, dual_ref.default_cap(pr.n, pr.p, pr.m))
    else:
        pr = dual_ref.case(cid)
        x, f, st, it, u, nact = dual_ref.reference(cid)
    return pr, x, u, st, nact


@functools.lru_cache(maxsize=None)
def want(cid, masked):
    pr, x, u, st, _ = pair(cid)
    r = kkt_ref.residuals(pr, x, u, st if masked else None)
    r.setflags(write=False)
    return r


def assert_bits(got, ref, label):
    assert got.shape == ref.shape, f"{label}: shape {got.shape} vs {ref.shape}"
    bad = kkt_ref.mismatches(got, ref)
    assert not bad, f"{label}: (QP, slot, gpu, definition) {bad}"


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("cid", sorted(dual_ref.gpu_cases()) + sorted(EXTRA))
def test_bitwise_against_definition(gpu, cid, layout):
    pr, x, u, st, _ = pair(cid)
    for masked in (True, False):
        got = qpgpu.kkt_residuals(pr, x, u if pr.p + pr.m else None, st if masked else None, layout=layout)
        assert_bits(got, want(cid, masked), f"{cid} {layout} {'masked' if masked else 'status NULL'}")


# ---- the box entry ---------------------------------------------------------------------------------
BOX_CASES = ("lane_7_0", "lane_7_3", "subgroup_16_0", "wave_lds_33_0", "box_65_2", "long_7_3", "inf_7_3")


@functools.lru_cache(maxsize=None)
def box_pair(cid):
    if cid == "box_65_2":  # two 64-row blocks, equalities in the second sweep
        bp = qpgpu.make_box_problems(65, 2, 0, 3, seed=565)
        bp.g0 *= box_ref.g0_scale(65)
        x, f, st, it, u, nact = dual_ref.solve(bp.to_dense(), box_ref.default_cap(65, 2))
    else:
        bp = box_ref.case(cid)
        x, f, st, it, u, nact = box_dual_ref.reference(cid)
    return bp, x, u, st


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("cid", BOX_CASES)
def test_box_entry_bitwise(gpu, cid, layout):
    bp, x, u, st = box_pair(cid)
    n, p = bp.n, bp.p
    if cid == "long_7_3":  # an upper and a lower bound active in the same QP
        assert np.any(np.any(u[:, p:p + n] != 0, axis=1) & np.any(u[:, p + n:] != 0, axis=1))
    if cid == "inf_7_3":
        assert np.isinf(bp.hi).any() and np.isinf(bp.lo).any()
    dense = bp.to_dense()
    for status in (st, None):
        ref = kkt_ref.residuals(dense, x, u, status)
        got = qpgpu.kkt_residuals(bp, x, u, status, layout=layout)
        assert_bits(got, ref, f"box {cid} {layout} vs the definition on to_dense()")
        assert_bits(got, qpgpu.kkt_residuals(dense, x, u, status, layout=layout), f"box {cid} {layout} vs the dense entry")
    ok = st == qpgpu.QP_OK
    assert ok.any() and not np.all(np.isnan(got[ok]))


# ---- solve, then check, on the device ---------------------------------------------------------------
def _solve_dual_then_check(pr, layout=None):
    import torch

    db = qpgpu.DeviceBatch(pr, DEV, layout=layout)
    B, E = pr.batch, pr.p + pr.m
    u = torch.full((db.x.shape[0], E), float("nan"), dtype=torch.float64, device=DEV) if E else None
    nact = torch.full((B,), -7, dtype=torch.int32, device=DEV)
    db.solve(dual_out=(u, nact))
    r = db.kkt_residuals(u)  # same stream, nothing copied back in between
    torch.cuda.synchronize()
    x, f, st, it = db.results()
    return db.kkt_rows(r), x, st, nact.cpu().numpy()


@pytest.mark.parametrize("cid", sorted(dual_ref.kkt_cases()))
def test_solve_then_check_on_the_device(gpu, cid):
    pr = dual_ref.case(cid)
    r, x, st, nact = _solve_dual_then_check(pr)
    assert np.all(np.isnan(r[st != qpgpu.QP_OK]))
    ok = (st == qpgpu.QP_OK) & np.all(np.isfinite(x), axis=1)
    if not ok.any():
        return
    g = r[ok]
    print(f"{cid}: {int(ok.sum())} QPs, stat {g[:, 0].max():.3e} eq {g[:, 2].max():.3e} ineq {g[:, 3].max():.3e} "
          f"comp {g[:, 4].max():.3e}")
    assert np.all(g[:, kkt_ref.STAT] <= STATIONARITY_MAX), f"{cid}: stationarity {g[:, kkt_ref.STAT].max():.3e}"
    assert np.all(g[:, kkt_ref.COMP] <= COMPLEMENTARITY_MAX), f"{cid}: complementarity {g[:, kkt_ref.COMP].max():.3e}"
    assert np.all(g[:, kkt_ref.EQ] <= EQUALITY_MAX), f"{cid}: equality residual {g[:, kkt_ref.EQ].max():.3e}"
    # a NaN limit in the data (edge_nan_limit) is reported as such, by definition: INEQ is NaN
    # there and held to the bar on every QP whose ci0 is free of NaN
    nan_limit = np.isnan(pr.ci0).any(axis=1)[ok]
    assert np.all(np.isnan(g[nan_limit, kkt_ref.INEQ]))
    assert np.all(g[~nan_limit, kkt_ref.INEQ] <= INEQUALITY_MAX), f"{cid}: inequality violation {g[:, kkt_ref.INEQ]}"
    assert not np.any(g[:, kkt_ref.UMIN].view(np.uint64)), f"{cid}: a negative multiplier"
    assert np.array_equal(g[:, kkt_ref.NNZ], nact[ok].astype(np.float64))


def test_tolerance_mode_x_is_feasible(gpu):
    """The n > 64 default (tolerance mode, plain entry): x from the device, u from the CPU
    reference; the primal slots stay under the bar."""
    import torch

    cid = "ws_100_20_200"
    pr, _, u, st, _ = pair(cid)
    db = qpgpu.DeviceBatch(pr, DEV)
    db.solve()
    ud = torch.from_numpy(np.array(u)).to(DEV)
    r = db.kkt_residuals(ud)
    torch.cuda.synchronize()
    r = db.kkt_rows(r)
    x, f, sd, it = db.results()
    assert np.array_equal(sd, st) and np.all(st == qpgpu.QP_OK)
    print(f"{cid}: eq {r[:, kkt_ref.EQ].max():.3e} ineq {r[:, kkt_ref.INEQ].max():.3e} stat {r[:, kkt_ref.STAT].max():.3e}")
    assert np.all(r[:, kkt_ref.EQ] < EQUALITY_MAX) and np.all(r[:, kkt_ref.INEQ] < INEQUALITY_MAX)


# ---- status ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("cid", ["edge_infeasible", "edge_not_pd", "edge_dependent"])
def test_status_handling(gpu, cid, layout):
    pr, x, u, st, _ = pair(cid)
    bad = st != qpgpu.QP_OK
    assert bad.all()
    masked = qpgpu.kkt_residuals(pr, x, u if pr.p + pr.m else None, st, layout=layout)
    assert np.all(np.isnan(masked[bad])) and not np.any(np.isnan(masked[~bad]))
    free = qpgpu.kkt_residuals(pr, x, u if pr.p + pr.m else None, None, layout=layout)
    assert_bits(free, want(cid, False), f"{cid} {layout} status NULL")
    assert bad.any() and not np.all(np.isnan(free[bad]))  # evaluated, not masked


# ---- placement ----------------------------------------------------------------------------------------
def kkt_specs(pr, x, u, st, layout):
    """placement.Spec of every array of the dense entry: nine inputs, r the one output."""
    B, n, p, m = pr.batch, pr.n, pr.p, pr.m
    rows = placement.rows_of(B, layout)
    conv = qpgpu.to_tiled64 if layout == "tiled64" else (lambda a: a)
    per_qp = {"G": n * n, "g0": n, "CE": n * p, "ce0": p, "CI": n * m, "ci0": m, "x": n, "u": p + m}
    specs = []
    for name, a in list(zip(placement.DENSE_INPUTS, pr.arrays())) + [("x", x), ("u", u)]:
        d = np.ascontiguousarray(conv(np.asarray(a, dtype=np.float64).reshape(B, -1))).reshape(-1)
        assert d.size == rows * per_qp[name]
        specs.append(placement.Spec(name, "f8", per_qp[name], d.size, d))
    specs.append(placement.Spec("status", "i4", 1, B, np.ascontiguousarray(st, dtype=np.int32)))
    specs.append(placement.Spec("r", "f8", qpgpu.KKT_NRES, rows * qpgpu.KKT_NRES))
    return specs


def call_in_arena(ar, pr, layout, b0=0, batch=None):
    """qpgpu_kkt_residuals with every pointer the arena's, advanced to QP b0; synchronises."""
    import torch

    batch = pr.batch if batch is None else batch
    d = qpgpu.ProblemDesc(pr.n, pr.p, pr.m, 0, batch, 0, qpgpu.LAYOUTS[layout])
    ptr = lambda name: ctypes.c_void_p(ar.address(name) + b0 * ar.specs[name].E * ar.specs[name].isz)
    names = list(placement.DENSE_INPUTS) + ["x", "u", "status", "r"]
    rc = qpgpu.LIB.qpgpu_kkt_residuals(ctypes.byref(d), *[ptr(k) for k in names],
                                       ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert rc == qpgpu.SUCCESS, rc
    return ar


def decoded(ar, B, layout):
    v = ar.values("r")
    return qpgpu.from_tiled64(v, B, (qpgpu.KKT_NRES,)) if layout == "tiled64" else v.reshape(B, qpgpu.KKT_NRES)


@functools.lru_cache(maxsize=None)
def placed_case(sid):
    """65 QPs (a TILED64 tile plus one: 63 padding slots) with QP 1 indefinite and QP 2 infeasible."""
    n, p, m = {"c1": (7, 6, 14), "wave": (30, 6, 60)}[sid]
    pr = qp_cases.make("general", n, p, m, 65, seed=900 + n)
    pr.G[1, n // 2, n // 2] = -1.0
    pr.CI[2, :, 1] = -pr.CI[2, :, 0]
    pr.ci0[2, 1] = -pr.ci0[2, 0] - 0.5
    x, f, st, it, u, nact = dual_ref.solve(pr, dual_ref.default_cap(n, p, m))
    assert st[1] == qpgpu.QP_NOT_POSITIVE_DEFINITE and st[2] == qpgpu.QP_INFEASIBLE
    return pr, x, u, st, kkt_ref.residuals(pr, x, u, st)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("sid", ["c1", "wave"])
def test_placement_odd_addresses_and_guard_bands(gpu, sid, layout):
    pr, x, u, st, ref = placed_case(sid)
    B = pr.batch
    bits = {}
    for pl in ("aligned", "odd"):
        ar = call_in_arena(placement.Arena(kkt_specs(pr, x, u, st, layout), pl, DEV), pr, layout)
        for name in ("G", "x", "u", "r"):
            assert ar.address(name) % 16 == placement.residue(pl, name, "f8")
        # guard bands, gaps and inputs untouched; every slot of the 65 QPs written, no padding slot
        assert ar.check({"r": placement.block_mask(qpgpu.KKT_NRES, layout, B)}) == [], f"{sid} {layout} {pl}"
        bits[pl] = ar.bits("r")
        assert_bits(decoded(ar, B, layout), ref, f"{sid} {layout} {pl}")
    assert np.array_equal(bits["aligned"], bits["odd"])


@pytest.mark.parametrize("layout,b0,B1", [("qp_major", 3, 70), ("qp_major", 65, 128), ("tiled64", 64, 70)])
def test_sub_range_of_a_batch(gpu, layout, b0, B1):
    """Pointers advanced to QP b0 of a 200-QP batch: the slice of the whole-batch result inside the
    range, the sentinel outside, inputs unchanged."""
    total = 200
    pr = qp_cases.make("general", 7, 6, 14, total, seed=40)
    x, f, st, it, u, nact = dual_ref.solve(pr, dual_ref.default_cap(7, 6, 14))
    ar = placement.Arena(kkt_specs(pr, x, u, st, layout), "aligned", DEV)
    whole = decoded(call_in_arena(ar, pr, layout), total, layout)
    assert_bits(whole, kkt_ref.residuals(pr, x, u, st), f"whole batch {layout}")
    ar.reset()
    call_in_arena(ar, pr, layout, b0=b0, batch=B1)
    if layout == "qp_major" and b0 % 2:
        assert (ar.address("G") + b0 * 49 * 8) % 16 == 8
    assert ar.check({"r": placement.block_mask(qpgpu.KKT_NRES, layout, total, b0, b0 + B1)}) == []
    assert_bits(decoded(ar, total, layout)[b0:b0 + B1], whole[b0:b0 + B1], f"QPs [{b0}, {b0 + B1}) {layout}")


# ---- hipGraph ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", ["b65_7_6_14", "ws_100_20_200"])
def test_first_call_captured_into_a_graph(gpu, cid):
    """No warm-up call: the capture is the first time this process enqueues the check on the
    stream.  One kernel node, a single chain.  Two replays, then the direct call: the same bits."""
    import torch

    pr, x, u, st, _ = pair(cid)
    db = qpgpu.DeviceBatch(pr, DEV, with_iters=False)
    up = lambda a: torch.from_numpy(np.array(a)).to(DEV)
    xd, ud = up(x), up(u)
    db.status.copy_(up(st))
    r = torch.full((pr.batch, qpgpu.KKT_NRES), 7.0, dtype=torch.float64, device=DEV)
    s = torch.cuda.Stream(DEV)
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        db.kkt_residuals(ud, r=r, x=xd, stream=s)
    torch.cuda.synchronize()
    assert torch.all(r == 7.0), "the capture itself must not run the kernel"
    for k in range(2):
        r.fill_(7.0)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert_bits(db.kkt_rows(r), want(cid, True), f"{cid} replay {k}")
    direct = db.kkt_rows(db.kkt_residuals(ud, x=xd))
    torch.cuda.synchronize()
    assert_bits(db.kkt_rows(r), direct, f"{cid} replay vs direct")
