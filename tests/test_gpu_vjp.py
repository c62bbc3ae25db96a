"""qpgpu_vjp / qpgpu_vjp_box on the GPU, bit for bit against the definition (tests/vjp_ref.py).  The
pairs (x, u) and the status words come from the CPU reference (tests/dual_ref.py,
tests/box_dual_ref.py), so only the new kernels are under test; the end-to-end tests are the ones
that run a solve first.  NaN compares as NaN (payloads are not compared); -0.0 and +0.0 are
different values.  gx comes from a fixed seed (vjp_ref.make_gx).  In the placement and graph tests
the gradients are pre-filled with a sentinel, so an element the kernel did not write shows.  All
batches are small."""
import ctypes
import functools

import numpy as np
import pytest

import box_dual_ref
import box_ref
import dual_ref
import placement
import qp_cases
import qpgpu
import vjp_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LAYOUTS = ("qp_major", "tiled64")

# beyond dual_ref.GPU_SHAPES and the edge cases: the first group-kernel shape, the first shape of the
# 64-lane group, and one, a wave less one and a wave plus one QP at C1's shape
EXTRA = {
    "group_9_2_20": (9, 2, 20, 9),
    "group_33_0_66": (33, 0, 66, 3),
    "b1_7_6_14": (7, 6, 14, 1),
    "b63_7_6_14": (7, 6, 14, 63),
    "b65_7_6_14": (7, 6, 14, 65),
}
CASES = sorted(c for c, pr in dual_ref.gpu_cases().items() if pr.n <= 64) + sorted(EXTRA)


@functools.lru_cache(maxsize=None)
def pair(cid):
    """(problems, x, u, status, gx) of a named case from the CPU reference, left unchanged."""
    if cid in EXTRA:
        n, p, m, B = EXTRA[cid]
        pr = qp_cases.make("box" if cid == "group_33_0_66" else "general", n, p, m, B, seed=500 + n + B)
        if cid == "group_33_0_66":
            pr.g0 *= box_ref.g0_scale(n)  # so that bounds bind
        x, f, st, it, u, nact = dual_ref.solve(pr, dual_ref.default_cap(n, p, m))
    else:
        pr = dual_ref.case(cid)
        x, f, st, it, u, nact = dual_ref.reference(cid)
    return pr, x, u, st, vjp_ref.make_gx(pr)


@functools.lru_cache(maxsize=None)
def want(cid, masked):
    pr, x, u, st, gx = pair(cid)
    return vjp_ref.vjp(pr, x, u, gx, st if masked else None)


def assert_bits(got, ref, label):
    bad = vjp_ref.mismatches(got, ref)
    assert not bad, f"{label}: (output, index, gpu, definition) {bad}"


def test_cases_cover_both_kernels_and_every_group_size():
    names = {qpgpu.kernel_name_vjp(pair(c)[0].n) for c in CASES}
    assert {"vjp_group_s16", "vjp_group_s32", "vjp_group_s64"} <= names
    assert sum("lane" in k for k in names) >= 5
    # the lists exercise active inequalities, q = n, masked QPs and q > n
    assert any(np.any(pair(c)[2][:, pair(c)[0].p:] != 0) for c in CASES)
    assert any(np.any(np.isnan(want(c, False)["dg0"])) for c in CASES)


def test_kernel_names(gpu):
    for n in (1, 7, 8):
        assert "lane" in qpgpu.kernel_name_vjp(n, 6, 14)
    for n in (9, 16, 17, 33, 64):
        assert "group" in qpgpu.kernel_name_vjp(n, 6, 14)
    assert qpgpu.kernel_name_vjp(65, 0, 0) == "" and qpgpu.kernel_name_vjp(256, 0, 512) == ""


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("cid", CASES)
def test_bitwise_against_definition(gpu, cid, layout):
    pr, x, u, st, gx = pair(cid)
    for masked in (True, False):
        got = qpgpu.vjp(pr, x, u if pr.p + pr.m else None, gx, st if masked else None, layout=layout)
        assert_bits(got, want(cid, masked), f"{cid} {layout} {'masked' if masked else 'status NULL'}")


# ---- the box entry ---------------------------------------------------------------------------------
BOX_CASES = ("lane_7_0", "lane_7_3", "subgroup_16_0", "wave_lds_33_0", "long_7_3", "inf_7_3")


@functools.lru_cache(maxsize=None)
def box_pair(cid):
    bp = box_ref.case(cid)
    x, f, st, it, u, nact = box_dual_ref.reference(cid)
    return bp, x, u, st, vjp_ref.make_gx(bp)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("cid", BOX_CASES)
def test_box_entry_bitwise(gpu, cid, layout):
    bp, x, u, st, gx = box_pair(cid)
    n, p = bp.n, bp.p
    if cid == "long_7_3":  # an upper and a lower bound active in the same QP
        assert np.any(np.any(u[:, p:p + n] != 0, axis=1) & np.any(u[:, p + n:] != 0, axis=1))
    dense = bp.to_dense()
    for status in (st, None):
        got = qpgpu.vjp(bp, x, u, gx, status, layout=layout)
        assert_bits(got, vjp_ref.vjp_box(bp, x, u, gx, status), f"box {cid} {layout} vs its own form")
        # against the definition on to_dense() and against the dense entry
        ref = vjp_ref.vjp(dense, x, u, gx, status)
        gd = qpgpu.vjp(dense, x, u, gx, status, layout=layout)
        assert_bits(gd, ref, f"dense entry on to_dense() of {cid} {layout}")
        for name, r in (("the definition", ref), ("the dense entry", gd)):
            on = r["dci0"][:, n:].view(np.uint64) != 0
            mapped = {"dG": r["dG"], "dg0": r["dg0"], "dCE": r["dCE"], "dce0": r["dce0"],
                      "dhi": r["dci0"][:, :n], "dlo": np.where(on, -r["dci0"][:, n:], 0.0)}
            assert_bits(got, mapped, f"box {cid} {layout} vs {name} on to_dense()")
    ok = st == qpgpu.QP_OK
    assert ok.any() and (np.any(got["dhi"][ok] != 0) or np.any(got["dlo"][ok] != 0))


# ---- NULL outputs ------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid,box", [("lane_7_6_14", False), ("subgroup_14_10_28", False), ("lane_7_3", True),
                                     ("subgroup_16_0", True)])
def test_null_outputs(gpu, cid, box):
    """Every single-output call equals the all-outputs call; the tensors of the outputs that were
    not asked for are not touched."""
    import torch

    pr, x, u, st, gx = box_pair(cid) if box else pair(cid)
    db = (qpgpu.DeviceBoxBatch if box else qpgpu.DeviceBatch)(pr, DEV, with_iters=False)
    up = lambda a: torch.from_numpy(np.array(a)).to(DEV)
    xd, ud, gd = up(x), up(u), up(gx)
    db.status.copy_(up(st))
    allo = db.vjp(ud, gd, x=xd)
    torch.cuda.synchronize()
    whole = db.vjp_rows(allo)
    assert_bits(whole, vjp_ref.vjp_box(pr, x, u, gx, st) if box else want(cid, True), f"{cid} all outputs")
    for name in db._VJP_OUTPUTS:
        pre = {k: torch.full_like(allo[k], 7.0) for k in db._VJP_OUTPUTS}
        res = db.vjp(ud, gd, outs={name: pre[name]}, x=xd)
        torch.cuda.synchronize()
        assert list(res) == [name]
        assert_bits(db.vjp_rows(res), {name: whole[name]}, f"{cid} only {name}")
        for k in db._VJP_OUTPUTS:
            if k != name:
                assert torch.all(pre[k] == 7.0), f"{cid}: {k} was written by a call that asked for {name} only"


# ---- placement ----------------------------------------------------------------------------------------
VJP_OUTPUTS = vjp_ref.DENSE_OUTPUTS


def vjp_specs(pr, x, u, st, gx, layout):
    """placement.Spec of every array of the dense entry: seven inputs, six outputs."""
    B, n, p, m = pr.batch, pr.n, pr.p, pr.m
    rows = placement.rows_of(B, layout)
    conv = qpgpu.to_tiled64 if layout == "tiled64" else (lambda a: a)
    per_qp = {"G": n * n, "CE": n * p, "CI": n * m, "x": n, "u": p + m, "gx": n,
              "dG": n * n, "dg0": n, "dCE": n * p, "dce0": p, "dCI": n * m, "dci0": m}
    specs = []
    for name, a in (("G", pr.G), ("CE", pr.CE), ("CI", pr.CI), ("x", x), ("u", u), ("gx", gx)):
        d = np.ascontiguousarray(conv(np.asarray(a, dtype=np.float64).reshape(B, -1))).reshape(-1)
        assert d.size == rows * per_qp[name]
        specs.append(placement.Spec(name, "f8", per_qp[name], d.size, d))
    specs.append(placement.Spec("status", "i4", 1, B, np.ascontiguousarray(st, dtype=np.int32)))
    for name in VJP_OUTPUTS:
        specs.append(placement.Spec(name, "f8", per_qp[name], rows * per_qp[name]))
    return specs


def call_in_arena(ar, pr, layout, b0=0, batch=None):
    """qpgpu_vjp with every pointer the arena's, advanced to QP b0; synchronises."""
    import torch

    batch = pr.batch if batch is None else batch
    d = qpgpu.ProblemDesc(pr.n, pr.p, pr.m, 0, batch, 0, qpgpu.LAYOUTS[layout])
    ptr = lambda name: ctypes.c_void_p(ar.address(name) + b0 * ar.specs[name].E * ar.specs[name].isz)
    names = ["G", "CE", "CI", "x", "u", "status", "gx"] + list(VJP_OUTPUTS)
    rc = qpgpu.LIB.qpgpu_vjp(ctypes.byref(d), *[ptr(k) for k in names],
                             ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert rc == qpgpu.SUCCESS, rc
    return ar


def decoded(ar, pr, layout, now=None):
    B, n, p, m = pr.batch, pr.n, pr.p, pr.m
    shapes = {"dG": (n, n), "dg0": (n,), "dCE": (n, p), "dce0": (p,), "dCI": (n, m), "dci0": (m,)}
    now = ar.download() if now is None else now
    out = {}
    for k in VJP_OUTPUTS:
        v = ar.values(k, now)
        out[k] = qpgpu.from_tiled64(v, B, shapes[k]) if layout == "tiled64" else v.reshape((B,) + shapes[k])
    return out


def masks(pr, layout, total, b0=0, b1=None):
    n, p, m = pr.n, pr.p, pr.m
    per_qp = {"dG": n * n, "dg0": n, "dCE": n * p, "dce0": p, "dCI": n * m, "dci0": m}
    return {k: placement.block_mask(per_qp[k], layout, total, b0, b1) for k in VJP_OUTPUTS}


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
    gx = vjp_ref.make_gx(pr)
    return pr, x, u, st, gx, vjp_ref.vjp(pr, x, u, gx, st)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("sid", ["c1", "wave"])
def test_placement_odd_addresses_and_guard_bands(gpu, sid, layout):
    pr, x, u, st, gx, ref = placed_case(sid)
    B = pr.batch
    bits = {}
    for pl in ("aligned", "odd"):
        ar = call_in_arena(placement.Arena(vjp_specs(pr, x, u, st, gx, layout), pl, DEV), pr, layout)
        for name in ("G", "x", "u", "gx", "dG", "dCI"):
            assert ar.address(name) % 16 == placement.residue(pl, name, "f8")
        # guard bands, gaps and inputs untouched; every element of the 65 QPs written, no padding slot
        assert ar.check(masks(pr, layout, B)) == [], f"{sid} {layout} {pl}"
        now = ar.download()
        bits[pl] = [ar.bits(k, now) for k in VJP_OUTPUTS]
        assert_bits(decoded(ar, pr, layout, now), ref, f"{sid} {layout} {pl}")
    assert all(np.array_equal(a, o) for a, o in zip(bits["aligned"], bits["odd"]))


@pytest.mark.parametrize("layout,b0,B1", [("qp_major", 3, 70), ("qp_major", 65, 128), ("tiled64", 64, 70)])
def test_sub_range_of_a_batch(gpu, layout, b0, B1):
    """Pointers advanced to QP b0 of a 200-QP batch: the slice of the whole-batch result inside the
    range, the sentinel outside, inputs unchanged."""
    total = 200
    pr = qp_cases.make("general", 7, 6, 14, total, seed=40)
    x, f, st, it, u, nact = dual_ref.solve(pr, dual_ref.default_cap(7, 6, 14))
    gx = vjp_ref.make_gx(pr)
    ar = placement.Arena(vjp_specs(pr, x, u, st, gx, layout), "aligned", DEV)
    whole = decoded(call_in_arena(ar, pr, layout), pr, layout)
    assert_bits(whole, vjp_ref.vjp(pr, x, u, gx, st), f"whole batch {layout}")
    ar.reset()
    call_in_arena(ar, pr, layout, b0=b0, batch=B1)
    if layout == "qp_major" and b0 % 2:
        assert (ar.address("G") + b0 * 49 * 8) % 16 == 8
    assert ar.check(masks(pr, layout, total, b0, b0 + B1)) == []
    part = decoded(ar, pr, layout)
    assert_bits({k: v[b0:b0 + B1] for k, v in part.items()}, {k: v[b0:b0 + B1] for k, v in whole.items()},
                f"QPs [{b0}, {b0 + B1}) {layout}")


# ---- hipGraph ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", ["b65_7_6_14", "wave_30_6_60", "wave_64_0_128"])
def test_first_call_captured_into_a_graph(gpu, cid):
    """The capture is the first time the test enqueues the backward step on the stream; it runs
    nothing.  Two replays, then the direct call: the same bits.  (64, 0, 128) is the shape whose
    kernel needs more than 64 KiB of LDS granted, here inside the capture."""
    import torch

    pr, x, u, st, gx = pair(cid)
    db = qpgpu.DeviceBatch(pr, DEV, with_iters=False)
    up = lambda a: torch.from_numpy(np.array(a)).to(DEV)
    xd, ud, gd = up(x), up(u), up(gx)
    db.status.copy_(up(st))
    outs = {k: torch.full((pr.batch, db._vjp_elems(k)), 7.0, dtype=torch.float64, device=DEV) for k in db._VJP_OUTPUTS}
    s = torch.cuda.Stream(DEV)
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        db.vjp(ud, gd, outs=outs, x=xd, stream=s)
    torch.cuda.synchronize()
    assert all(bool(torch.all(t == 7.0)) for t in outs.values()), "the capture itself must not run the kernel"
    for k in range(2):
        for t in outs.values():
            t.fill_(7.0)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert_bits(db.vjp_rows(outs), want(cid, True), f"{cid} replay {k}")
    direct = db.vjp(ud, gd, x=xd)
    torch.cuda.synchronize()
    assert_bits(db.vjp_rows(outs), db.vjp_rows(direct), f"{cid} replay vs direct")


# ---- solve, then differentiate, on the device ------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("cid", ["lane_7_6_14", "subgroup_14_10_28", "wave_30_6_60", "edge_infeasible"])
def test_solve_then_differentiate_on_the_device(gpu, cid, layout):
    import torch

    pr, x, u, st, gx = pair(cid)
    db = qpgpu.DeviceBatch(pr, DEV, layout=layout)
    B, E = pr.batch, pr.p + pr.m
    ud = torch.full((db.x.shape[0], E), float("nan"), dtype=torch.float64, device=DEV)
    conv = qpgpu.to_tiled64 if layout == "tiled64" else (lambda a: a)
    gd = torch.from_numpy(np.ascontiguousarray(conv(gx))).to(DEV)
    db.solve(dual_out=(ud, None))
    res = db.vjp(ud, gd)  # same stream, nothing copied back in between
    torch.cuda.synchronize()
    assert np.array_equal(db.results()[2], st)
    assert_bits(db.vjp_rows(res), want(cid, True), f"{cid} {layout} solve then vjp")


# ---- the autograd layers -----------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", ["lane_7_6_14", "subgroup_14_10_28"])
def test_qp_layer_backward_is_the_definition(gpu, cid):
    import torch

    pr, x, u, st, gx = pair(cid)
    B = min(pr.batch, 70)
    ins = [torch.from_numpy(np.array(a[:B])).to(DEV).requires_grad_(k != 1) for k, a in enumerate(pr.arrays())]
    xs = qpgpu.qp_layer(*ins)
    (xs * torch.from_numpy(gx[:B]).to(DEV)).sum().backward()
    torch.cuda.synchronize()
    assert np.array_equal(xs.detach().cpu().numpy().view(np.uint64), x[:B].view(np.uint64))
    ref = want(cid, True)
    assert ins[1].grad is None  # g0 did not require grad
    got = {k: t.grad.cpu().numpy() for k, t in zip(vjp_ref.DENSE_OUTPUTS, ins) if t.grad is not None}
    assert sorted(got) == sorted(k for k in vjp_ref.DENSE_OUTPUTS if k != "dg0")
    assert_bits(got, {k: ref[k][:B] for k in got}, f"qp_layer {cid}")


def test_qp_layer_box_backward_is_the_definition(gpu):
    import torch

    cid = "lane_7_3"
    bp, x, u, st, gx = box_pair(cid)
    ins = [torch.from_numpy(np.array(a)).to(DEV).requires_grad_(k != 2) for k, a in enumerate(bp.arrays())]
    xs = qpgpu.qp_layer_box(*ins)
    (xs * torch.from_numpy(gx).to(DEV)).sum().backward()
    torch.cuda.synchronize()
    ref = vjp_ref.vjp_box(bp, x, u, gx, st)
    assert ins[2].grad is None  # CE did not require grad
    got = {k: t.grad.cpu().numpy() for k, t in zip(vjp_ref.BOX_OUTPUTS, ins) if t.grad is not None}
    assert sorted(got) == sorted(k for k in vjp_ref.BOX_OUTPUTS if k != "dCE")
    assert_bits(got, {k: ref[k] for k in got}, f"qp_layer_box {cid}")


def test_qp_layer_with_failed_qps(gpu):
    """One indefinite and one infeasible QP in the batch: zeros there, finite gradients elsewhere."""
    import torch

    pr, x, u, st, gx, ref = placed_case("c1")
    ins = [torch.from_numpy(np.array(a)).to(DEV).requires_grad_(True) for a in pr.arrays()]
    xs = qpgpu.qp_layer(*ins)
    (xs * torch.from_numpy(gx).to(DEV)).sum().backward()
    torch.cuda.synchronize()
    got = {k: t.grad.cpu().numpy() for k, t in zip(vjp_ref.DENSE_OUTPUTS, ins)}
    bad = st != qpgpu.QP_OK
    assert bad.sum() == 2
    for k, v in got.items():
        assert not np.any(v[bad].view(np.uint64)), k
        assert np.all(np.isfinite(v[~bad])), k
    assert np.all(np.any(got["dg0"][~bad] != 0, axis=1))
    assert_bits(got, ref, "qp_layer with failed QPs")
