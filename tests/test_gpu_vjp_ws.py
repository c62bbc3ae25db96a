"""qpgpu_vjp_ws / qpgpu_vjp_box_ws on the GPU, bit for bit against the definition (tests/vjp_ref.py), on
the n > 64 cases of tests/vjp_ws_cases.py.  The pairs (x, u) and the status words come from the CPU
reference, so only the new kernel is under test; the end-to-end tests are the ones that run a solve
first.  NaN compares as NaN (payloads are not compared); -0.0 and +0.0 are different values.  In the
placement, NULL-output and graph tests the gradients are pre-filled with a sentinel, so an element
the kernel did not write shows.  All batches are one to three QPs."""
import ctypes

import numpy as np
import pytest

import box_ref
import dual_ref
import placement
import qpgpu
import vjp_ref
import vjp_ws_cases as W
from vjp_ws_cases import assert_bits

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LAYOUTS = ("qp_major", "tiled64")


def test_kernel_names(gpu):
    for cid in W.DENSE_CASES + (W.NAN_CASE,):
        pr = W.pair(cid)[0]
        assert "ws" in qpgpu.kernel_name_vjp_ws(pr.n, pr.p, pr.m) and qpgpu.kernel_name_vjp(pr.n, pr.p, pr.m) == ""


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("cid", W.DENSE_CASES + (W.NAN_CASE,) + W.EDGE_CASES)
def test_bitwise_against_definition(gpu, cid, layout):
    pr, x, u, st, gx = W.pair(cid)
    for masked in (True, False):
        got = qpgpu.vjp(pr, x, u if pr.p + pr.m else None, gx, st if masked else None, layout=layout)
        assert_bits(got, W.want(cid, masked), f"{cid} {layout} {'masked' if masked else 'status NULL'}")
    if cid == W.NAN_CASE:
        for k, v in got.items():  # status NULL: q > n, NaN from the arithmetic, finite
            assert np.all(np.isnan(v[0])) and not np.any(np.isnan(v[2])), k
        assert np.any(np.isnan(got["dg0"][1]))
        masked = qpgpu.vjp(pr, x, u, gx, st, layout=layout)
        assert all(not np.any(v[1].view(np.uint64)) for v in masked.values())  # +0.0 exactly


# ---- the box entry ---------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("cid", W.BOX_CASES)
def test_box_entry_bitwise(gpu, cid, layout):
    bp, x, u, st, gx = W.box_pair(cid)
    n = bp.n
    dense = box_ref.dense(cid)
    for masked in (True, False):
        status = st if masked else None
        got = qpgpu.vjp(bp, x, u, gx, status, layout=layout)
        assert_bits(got, W.box_want(cid, masked), f"box {cid} {layout} vs its own form")
        ref = W.box_dense_want(cid, masked)
        gd = qpgpu.vjp(dense, x, u, gx, status, layout=layout)
        assert_bits(gd, ref, f"dense entry on to_dense() of {cid} {layout}")
        assert_bits(got, W.box_as_dense(ref, n), f"box {cid} {layout} vs the definition on to_dense()")
        assert_bits(got, W.box_as_dense(gd, n), f"box {cid} {layout} vs the dense entry on to_dense()")
    assert np.all(np.any(got["dhi"] != 0, axis=1) & np.any(got["dlo"] != 0, axis=1))


# ---- the number of slots ---------------------------------------------------------------------------
@pytest.mark.parametrize("cid", ["ws_65_2_130", "g_129_70_40"])
def test_results_do_not_depend_on_the_slots(gpu, cid):
    """1 slot and 2 slots wrap the QP loop (B = 3: two laps and one and a half); `batch` slots do not."""
    pr, x, u, st, gx = W.pair(cid)
    for slots in (1, 2, pr.batch):
        got = qpgpu.vjp(pr, x, u, gx, st, slots=slots)
        assert_bits(got, W.want(cid, True), f"{cid} with {slots} slot(s)")


# ---- placement: the workspace in an arena ------------------------------------------------------------
OUTS = vjp_ref.DENSE_OUTPUTS
FILL = {"nan": 0xFF, "zero": 0x00}


def ws_specs(pr, x, u, st, gx, layout, slots, fill):
    """placement.Spec of every array of the dense entry, and the workspace of `slots` slots as an input
    filled with the byte `fill` (Arena.check(modified_ok=("ws",)) lets the call write it, and still
    holds its guard bands)."""
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
    for name in OUTS:
        specs.append(placement.Spec(name, "f8", per_qp[name], rows * per_qp[name]))
    per = qpgpu.vjp_workspace_bytes(n, p, m, 1) // 8
    ws = np.full(slots * per * 8, fill, dtype=np.uint8).view(np.float64)
    specs.append(placement.Spec("ws", "f8", per, slots * per, ws))
    return specs


def call_in_arena(ar, pr, layout, b0=0, batch=None):
    """qpgpu_vjp_ws with every pointer the arena's, advanced to QP b0; synchronises."""
    import torch

    batch = pr.batch if batch is None else batch
    d = qpgpu.ProblemDesc(pr.n, pr.p, pr.m, 0, batch, 0, qpgpu.LAYOUTS[layout])
    ptr = lambda name: ctypes.c_void_p(ar.address(name) + b0 * ar.specs[name].E * ar.specs[name].isz)
    names = ["G", "CE", "CI", "x", "u", "status", "gx"] + list(OUTS)
    s = ar.specs["ws"]
    rc = qpgpu.LIB.qpgpu_vjp_ws(ctypes.byref(d), *[ptr(k) for k in names], ctypes.c_void_p(ar.address("ws")),
                                s.count * 8, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert rc == qpgpu.SUCCESS, rc
    return ar


def decoded(ar, pr, layout):
    B, n, p, m = pr.batch, pr.n, pr.p, pr.m
    shapes = {"dG": (n, n), "dg0": (n,), "dCE": (n, p), "dce0": (p,), "dCI": (n, m), "dci0": (m,)}
    now = ar.download()
    out = {}
    for k in OUTS:
        v = ar.values(k, now)
        out[k] = qpgpu.from_tiled64(v, B, shapes[k]) if layout == "tiled64" else v.reshape((B,) + shapes[k])
    return out


def masks(pr, layout, total, b0=0, b1=None):
    n, p, m = pr.n, pr.p, pr.m
    per_qp = {"dG": n * n, "dg0": n, "dCE": n * p, "dce0": p, "dCI": n * m, "dci0": m}
    return {k: placement.block_mask(per_qp[k], layout, total, b0, b1) for k in OUTS}


def test_workspace_hygiene_tiled64(gpu):
    """B = 3 in TILED64 (61 padding slots), the workspace between guard bands: whatever it holds on
    entry, the same bits; the guards, the inputs and the padding slots untouched."""
    cid = "ws_65_2_130"
    pr, x, u, st, gx = W.pair(cid)
    bits = {}
    for fill in ("nan", "zero"):
        for slots in (pr.batch, 2):
            ar = placement.Arena(ws_specs(pr, x, u, st, gx, "tiled64", slots, FILL[fill]), "aligned", DEV)
            assert ar.address("ws") % 8 == 0
            call_in_arena(ar, pr, "tiled64")
            assert ar.check(masks(pr, "tiled64", pr.batch), modified_ok=("ws",)) == [], f"{fill} {slots} slots"
            now = ar.download()
            bits[fill, slots] = [ar.bits(k, now) for k in OUTS]
            assert_bits(decoded(ar, pr, "tiled64"), W.want(cid, True), f"{cid} tiled64, workspace of {fill} bytes")
    first = bits["nan", pr.batch]
    assert all(np.array_equal(a, o) for other in bits.values() for a, o in zip(first, other))


def test_workspace_hygiene_sub_range_qp_major(gpu):
    """Pointers advanced to QP 1 of the three: QPs [1, 3) written, QP 0 keeps the sentinel; one slot."""
    cid = "ws_65_2_130"
    pr, x, u, st, gx = W.pair(cid)
    ar = placement.Arena(ws_specs(pr, x, u, st, gx, "qp_major", 1, FILL["nan"]), "odd", DEV)
    assert ar.address("ws") % 16 == 8  # 8-byte aligned is enough
    call_in_arena(ar, pr, "qp_major", b0=1, batch=2)
    assert ar.check(masks(pr, "qp_major", pr.batch, 1, 3), modified_ok=("ws",)) == []
    part = decoded(ar, pr, "qp_major")
    ref = W.want(cid, True)
    assert_bits({k: v[1:] for k, v in part.items()}, {k: v[1:] for k, v in ref.items()}, f"{cid} QPs [1, 3)")


# ---- n <= 64 through the new entry ---------------------------------------------------------------------
@pytest.mark.parametrize("cid", ["lane_7_6_14", "wave_30_6_60"])
def test_on_chip_shapes_through_the_new_entry(gpu, cid):
    """NULL workspace, 0 bytes: the launch of qpgpu_vjp, the same bits."""
    import torch

    pr = dual_ref.case(cid)
    x, f, st, it, u, nact = dual_ref.reference(cid)
    gx = vjp_ref.make_gx(pr)
    assert qpgpu.kernel_name_vjp_ws(pr.n, pr.p, pr.m) == qpgpu.kernel_name_vjp(pr.n, pr.p, pr.m) != ""
    assert qpgpu.vjp_workspace_bytes(pr.n, pr.p, pr.m, 8) == 0
    db = qpgpu.DeviceBatch(pr, DEV, with_iters=False)
    up = lambda a: torch.from_numpy(np.array(a)).to(DEV)
    xd, ud, gd = up(x), up(u), up(gx)
    db.status.copy_(up(st))
    old = db.vjp(ud, gd, x=xd)
    new = {k: torch.full_like(t, 7.0) for k, t in old.items()}
    d = qpgpu.ProblemDesc(pr.n, pr.p, pr.m, 0, pr.batch, 0, 0)
    vp = lambda t: ctypes.c_void_p(t.data_ptr())
    rc = qpgpu.LIB.qpgpu_vjp_ws(ctypes.byref(d), vp(db.G), vp(db.CE), vp(db.CI), vp(xd), vp(ud), vp(db.status), vp(gd),
                                *[vp(new[k]) for k in db._VJP_OUTPUTS], None, 0,
                                ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert rc == qpgpu.SUCCESS
    assert_bits(db.vjp_rows(new), db.vjp_rows(old), f"{cid}: qpgpu_vjp_ws vs qpgpu_vjp")
    assert_bits(db.vjp_rows(new), vjp_ref.vjp(pr, x, u, gx, st), f"{cid}: qpgpu_vjp_ws vs the definition")


# ---- NULL outputs ------------------------------------------------------------------------------------
def test_null_outputs(gpu):
    """Every single-output call equals the all-outputs call; the tensors of the outputs that were
    not asked for are not touched."""
    import torch

    cid = "ws_65_2_130"
    pr, x, u, st, gx = W.pair(cid)
    db = qpgpu.DeviceBatch(pr, DEV, with_iters=False)
    up = lambda a: torch.from_numpy(np.array(a)).to(DEV)
    xd, ud, gd = up(x), up(u), up(gx)
    db.status.copy_(up(st))
    allo = db.vjp(ud, gd, x=xd)
    torch.cuda.synchronize()
    whole = db.vjp_rows(allo)
    assert_bits(whole, W.want(cid, True), f"{cid} all outputs")
    for name in db._VJP_OUTPUTS:
        pre = {k: torch.full_like(allo[k], 7.0) for k in db._VJP_OUTPUTS}
        res = db.vjp(ud, gd, outs={name: pre[name]}, x=xd)
        torch.cuda.synchronize()
        assert list(res) == [name]
        assert_bits(db.vjp_rows(res), {name: whole[name]}, f"{cid} only {name}")
        for k in db._VJP_OUTPUTS:
            if k != name:
                assert torch.all(pre[k] == 7.0), f"{cid}: {k} was written by a call that asked for {name} only"


# ---- hipGraph ------------------------------------------------------------------------------------------
def test_first_call_captured_into_a_graph(gpu):
    """The capture is the first time the test enqueues the backward step of this shape on the stream;
    it runs nothing.  Two replays, then the direct call: the same bits."""
    import torch

    cid = "ws_100_20_200"
    pr, x, u, st, gx = W.pair(cid)
    db = qpgpu.DeviceBatch(pr, DEV, with_iters=False)
    up = lambda a: torch.from_numpy(np.array(a)).to(DEV)
    xd, ud, gd = up(x), up(u), up(gx)
    db.status.copy_(up(st))
    outs = {k: torch.full((pr.batch, db._vjp_elems(k)), 7.0, dtype=torch.float64, device=DEV) for k in db._VJP_OUTPUTS}
    ws = torch.empty(qpgpu.vjp_workspace_bytes(pr.n, pr.p, pr.m, pr.batch), dtype=torch.uint8, device=DEV)
    s = torch.cuda.Stream(DEV)
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        db.vjp(ud, gd, outs=outs, x=xd, stream=s, workspace=ws)
    torch.cuda.synchronize()
    assert all(bool(torch.all(t == 7.0)) for t in outs.values()), "the capture itself must not run the kernel"
    for k in range(2):
        for t in outs.values():
            t.fill_(7.0)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert_bits(db.vjp_rows(outs), W.want(cid, True), f"{cid} replay {k}")
    direct = db.vjp(ud, gd, x=xd)
    torch.cuda.synchronize()
    assert_bits(db.vjp_rows(outs), db.vjp_rows(direct), f"{cid} replay vs direct")


# ---- solve, then differentiate, on the device ------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS)
def test_solve_then_differentiate_on_the_device(gpu, layout):
    import torch

    cid = "ws_65_2_130"
    pr, x, u, st, gx = W.pair(cid)
    db = qpgpu.DeviceBatch(pr, DEV, layout=layout)
    E = pr.p + pr.m
    ud = torch.full((db.x.shape[0], E), float("nan"), dtype=torch.float64, device=DEV)
    conv = qpgpu.to_tiled64 if layout == "tiled64" else (lambda a: a)
    gd = torch.from_numpy(np.ascontiguousarray(conv(gx))).to(DEV)
    db.solve(dual_out=(ud, None))
    res = db.vjp(ud, gd)  # same stream, nothing copied back in between
    torch.cuda.synchronize()
    assert np.array_equal(db.results()[2], st)
    assert_bits(db.vjp_rows(res), W.want(cid, True), f"{cid} {layout} solve then vjp")


# ---- the autograd layers -----------------------------------------------------------------------------------
def test_qp_layer_backward_is_the_definition(gpu):
    import torch

    cid = "ws_65_2_130"
    pr, x, u, st, gx = W.pair(cid)
    ins = [torch.from_numpy(np.array(a)).to(DEV).requires_grad_(k != 1) for k, a in enumerate(pr.arrays())]
    xs = qpgpu.qp_layer(*ins)
    (xs * torch.from_numpy(gx).to(DEV)).sum().backward()
    torch.cuda.synchronize()
    assert np.array_equal(xs.detach().cpu().numpy().view(np.uint64), x.view(np.uint64))
    ref = W.want(cid, True)
    assert ins[1].grad is None  # g0 did not require grad
    got = {k: t.grad.cpu().numpy() for k, t in zip(vjp_ref.DENSE_OUTPUTS, ins) if t.grad is not None}
    assert sorted(got) == sorted(k for k in vjp_ref.DENSE_OUTPUTS if k != "dg0")
    assert_bits(got, {k: ref[k] for k in got}, f"qp_layer {cid}")


def test_qp_layer_box_backward_is_the_definition(gpu):
    import torch

    cid = "wave_ws_65_0"
    bp, x, u, st, gx = W.box_pair(cid)
    ins = [torch.from_numpy(np.array(a)).to(DEV).requires_grad_(k != 3) for k, a in enumerate(bp.arrays())]
    xs = qpgpu.qp_layer_box(*ins)
    (xs * torch.from_numpy(gx).to(DEV)).sum().backward()
    torch.cuda.synchronize()
    assert np.array_equal(xs.detach().cpu().numpy().view(np.uint64), np.asarray(x).view(np.uint64))
    ref = W.box_want(cid, True)
    assert ins[3].grad is None  # ce0 did not require grad
    got = {k: t.grad.cpu().numpy() for k, t in zip(vjp_ref.BOX_OUTPUTS, ins) if t.grad is not None}
    assert sorted(got) == sorted(k for k in vjp_ref.BOX_OUTPUTS if k != "dce0")
    assert_bits(got, {k: ref[k] for k in got}, f"qp_layer_box {cid}")
