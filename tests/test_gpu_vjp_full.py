"""qpgpu_vjp_full / qpgpu_vjp_box_full on the GPU, bit for bit against the definition
(tests/vjp_full_ref.py), on the smallest shape of every code path: the lane kernel (dense and box),
the three group sizes, q = 0 and q = n, the workspace kernel (dense and box) and a batch with an
indefinite and an infeasible QP.  The pairs (x, u) and the status words come from the CPU reference,
so only the new kernels are under test; the layer tests run a solve first.  NaN compares as NaN;
-0.0 and +0.0 are different values.  gx, gu and gf come from fixed seeds.  Every case is a few QPs
(the lane case 70: a full wave and a partial one), computed once and shared."""
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
import vjp_full_ref as F
import vjp_ref
from vjp_ws_cases import assert_bits

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LAYOUTS = ("qp_major", "tiled64")
COTANGENTS = {"neither": (False, False), "gu": (True, False), "gf": (False, True), "both": (True, True)}

# id -> (source, case, QPs kept, the kind of kernel its name must carry)
CASES = {
    "lane_7_6_14": ("dual", "lane_7_6_14", 70, "lane"),
    "lane_8_0_16": ("dual", "lane_8_0_16", 5, "lane"),
    "lane_box_7_0": ("box", "lane_7_0", 5, "lane"),
    "group_s16_14_10_28": ("dual", "subgroup_14_10_28", 5, "group_s16"),
    "group_s32_30_6_60": ("dual", "wave_30_6_60", 3, "group_s32"),
    "group_s64_64_0_128": ("dual", "wave_64_0_128", 2, "group_s64"),
    "degenerate_3_0_0": ("dual", "degenerate_3_0_0", 5, "lane"),
    "degenerate_4_4_0": ("dual", "degenerate_4_4_0", 5, "lane"),
    "ws_65_2_130": ("dual", "ws_65_2_130", 3, "ws"),
    "ws_box_65_0": ("box", "wave_ws_65_0", 2, "ws"),
    "failed_7_6_14": ("failed", None, 70, "lane"),
}


@functools.lru_cache(maxsize=None)
def pair(cid):
    """(problems, x, u, status, gx, gu, gf) of a case, from the CPU reference; left unchanged."""
    src, name, B, _ = CASES[cid]
    if src == "failed":  # QP 1 indefinite, QP 2 infeasible; 70 QPs: a TILED64 tile and six more
        pr = qp_cases.make("general", 7, 6, 14, B, seed=907)
        pr.G[1, 3, 3] = -1.0
        pr.CI[2, :, 1] = -pr.CI[2, :, 0]
        pr.ci0[2, 1] = -pr.ci0[2, 0] - 0.5
        x, f, st, it, u, nact = dual_ref.solve(pr, dual_ref.default_cap(7, 6, 14))
        assert st[1] == qpgpu.QP_NOT_POSITIVE_DEFINITE and st[2] == qpgpu.QP_INFEASIBLE and (st != qpgpu.QP_OK).sum() == 2
    else:
        mod, ref = (box_ref, box_dual_ref) if src == "box" else (dual_ref, dual_ref)
        full = mod.case(name)
        B = min(B, full.batch)
        pr = full.slice(0, B)
        x, f, st, it, u, nact = [np.array(a[:B]) for a in ref.reference(name)]
    gu, gf = F.make_cotangents(pr)
    return pr, x, u, st, vjp_ref.make_gx(pr), gu, gf


def is_box(cid):
    return CASES[cid][0] == "box"


@functools.lru_cache(maxsize=None)
def want(cid, cot, masked=True):
    pr, x, u, st, gx, gu, gf = pair(cid)
    with_u, with_f = COTANGENTS[cot]
    fn = F.vjp_box_full if is_box(cid) else F.vjp_full
    return fn(pr, x, u if pr.p + pr.m else None, gx, gu if with_u else None, gf if with_f else None,
              st if masked else None)


def run(cid, cot, layout, masked=True, **kw):
    pr, x, u, st, gx, gu, gf = pair(cid)
    with_u, with_f = COTANGENTS[cot]
    if cot == "neither":  # the full entry with both cotangents NULL: qpgpu.vjp would take the old entry
        return full_call(cid, layout, None, None, masked, **kw)
    return qpgpu.vjp(pr, x, u if pr.p + pr.m else None, gx, st if masked else None, layout=layout,
                     gu=gu if with_u and pr.p + pr.m else None, gf=gf if with_f else None, **kw)


def full_call(cid, layout, gu, gf, masked=True, outs=None, slots=qpgpu.VJP_SLOTS):
    """qpgpu_vjp_full / qpgpu_vjp_box_full itself, whatever gu and gf are (numpy or None)."""
    import torch

    pr, x, u, st, gx, _, _ = pair(cid)
    db = (qpgpu.DeviceBoxBatch if is_box(cid) else qpgpu.DeviceBatch)(pr, DEV, with_iters=False, layout=layout)
    B, E = pr.batch, pr.p + pr.m
    conv = qpgpu.to_tiled64 if layout == "tiled64" else (lambda a: a)
    up = lambda a, cols: torch.from_numpy(np.array(conv(np.asarray(a, dtype=np.float64).reshape(B, cols)), order="C")).to(DEV)
    t = [getattr(db, k) for k in db._VJP_INPUTS] + [up(x, pr.n), up(u, E) if E else None,
                                                    torch.from_numpy(np.array(st)).to(DEV) if masked else None,
                                                    up(gx, pr.n), None if gu is None else up(gu, E),
                                                    None if gf is None else torch.from_numpy(np.array(gf)).to(DEV)]
    rows = placement.rows_of(B, layout)
    res = {k: torch.full((rows, db._vjp_elems(k)), 7.0, dtype=torch.float64, device=DEV)
           for k in (db._VJP_OUTPUTS if outs is None else outs)}
    ws = torch.empty(qpgpu.vjp_workspace_bytes(pr.n, pr.p, pr.m, max(1, min(B, slots))), dtype=torch.uint8, device=DEV)
    d = qpgpu.ProblemDesc(pr.n, pr.p, pr.m, 0, B, 0, qpgpu.LAYOUTS[layout])
    vp = lambda a: None if a is None or a.numel() == 0 else ctypes.c_void_p(a.data_ptr())
    entry = db._ENTRY_VJP + "_full"
    rc = getattr(qpgpu.LIB, entry)(ctypes.byref(d), *[vp(a) for a in t], *[vp(res.get(k)) for k in db._VJP_OUTPUTS],
                                   vp(ws), ws.numel(), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert rc == qpgpu.SUCCESS, (entry, rc)
    return db.vjp_rows(res)


def test_cases_are_what_they_are_named_for():
    for cid, (_, _, _, kind) in CASES.items():
        pr = pair(cid)[0]
        name = qpgpu.kernel_name_vjp_full(pr.n, pr.p, pr.m)
        assert "full" in name and kind in name, (cid, name)
    q = lambda cid: pair(cid)[0].p + (pair(cid)[2][:, pair(cid)[0].p:] != 0).sum(axis=1)
    assert np.all(q("degenerate_3_0_0") == 0) and np.all(q("degenerate_4_4_0") == 4)
    for cid in ("lane_7_6_14", "lane_box_7_0", "group_s32_30_6_60", "ws_65_2_130", "ws_box_65_0"):
        pr, x, u = pair(cid)[:3]
        assert np.any(u[:, pr.p:] != 0) and np.any(u[:, pr.p:] == 0), cid  # inequalities in W and outside it
    assert pair("lane_7_6_14")[0].batch == 70  # more than one wave, the last one partial


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("cot", sorted(COTANGENTS))
@pytest.mark.parametrize("cid", sorted(CASES))
def test_bitwise_against_definition(gpu, cid, cot, layout):
    got = run(cid, cot, layout)
    assert_bits(got, want(cid, cot), f"{cid} {cot} {layout}")
    if cid == "failed_7_6_14":
        st = pair(cid)[3]
        for k, v in got.items():
            assert not np.any(v[st != qpgpu.QP_OK].view(np.uint64)), k  # +0.0 exactly
            assert np.all(np.isfinite(v[st == qpgpu.QP_OK])), k


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("cid", sorted(CASES))
def test_null_cotangents_are_the_old_entries(gpu, cid, layout):
    """gu = gf = NULL through the full entry: the bits of qpgpu_vjp (n <= 64) / qpgpu_vjp_ws, called in
    the same process, and of tests/vjp_ref.py."""
    pr, x, u, st, gx, gu, gf = pair(cid)
    new = full_call(cid, layout, None, None)
    old = qpgpu.vjp(pr, x, u if pr.p + pr.m else None, gx, st, layout=layout)
    assert_bits(new, old, f"{cid} {layout}: the full entry with NULL cotangents vs the x-only entry")
    ref = (vjp_ref.vjp_box if is_box(cid) else vjp_ref.vjp)(pr, x, u if pr.p + pr.m else None, gx, st)
    assert_bits(new, ref, f"{cid} {layout}: the full entry with NULL cotangents vs tests/vjp_ref.py")


@pytest.mark.parametrize("cid", ["lane_7_6_14", "group_s16_14_10_28", "ws_65_2_130"])
def test_status_null_and_more_columns_than_variables(gpu, cid):
    """status NULL evaluates every QP; with every multiplier non-zero q = p + m > n: NaN everywhere."""
    got = run(cid, "both", "qp_major", masked=False)
    assert_bits(got, want(cid, "both", False), f"{cid} status NULL")
    pr, x, u, st, gx, gu, gf = pair(cid)
    ones = np.ones_like(u)
    got = qpgpu.vjp(pr, x, ones, gx, None, gu=gu, gf=gf)
    assert all(np.all(np.isnan(v)) for v in got.values())
    assert_bits(got, F.vjp_full(pr, x, ones, gx, gu, gf), f"{cid} q > n")


@pytest.mark.parametrize("cid", ["lane_7_6_14", "group_s32_30_6_60", "ws_65_2_130", "lane_box_7_0"])
def test_gu_outside_w_may_hold_nan(gpu, cid):
    pr, x, u, st, gx, gu, gf = pair(cid)
    poisoned = gu.copy()
    off = np.zeros(u.shape, dtype=bool)
    off[:, pr.p:] = u[:, pr.p:] == 0
    assert off.any()
    poisoned[off] = np.nan
    for layout in LAYOUTS:
        got = full_call(cid, layout, poisoned, gf)
        assert_bits(got, want(cid, "both"), f"{cid} {layout}: NaN in gu where u == 0")


@pytest.mark.parametrize("cid", ["lane_7_6_14", "group_s16_14_10_28", "ws_65_2_130", "lane_box_7_0"])
def test_null_outputs(gpu, cid):
    """Every single-output call equals the all-outputs call (a missing output would have failed to
    decode: only the named tensors exist)."""
    pr, x, u, st, gx, gu, gf = pair(cid)
    whole = want(cid, "both")
    for name in whole:
        got = full_call(cid, "qp_major", gu, gf, outs=(name,))
        assert list(got) == [name]
        assert_bits(got, {name: whole[name]}, f"{cid} only {name}")


def test_results_do_not_depend_on_the_slots(gpu):
    cid = "ws_65_2_130"
    pr, x, u, st, gx, gu, gf = pair(cid)
    assert pr.batch == 3
    a = full_call(cid, "qp_major", gu, gf, slots=1)
    b = full_call(cid, "qp_major", gu, gf, slots=3)
    assert_bits(a, b, f"{cid}: 1 slot vs 3 slots")
    assert_bits(a, want(cid, "both"), f"{cid}: 1 slot")


# ---- placement -------------------------------------------------------------------------------------
OUTS = F.DENSE_OUTPUTS


def specs(cid, layout):
    pr, x, u, st, gx, gu, gf = pair(cid)
    B, n, p, m = pr.batch, pr.n, pr.p, pr.m
    rows = placement.rows_of(B, layout)
    conv = qpgpu.to_tiled64 if layout == "tiled64" else (lambda a: a)
    per_qp = {"G": n * n, "CE": n * p, "CI": n * m, "x": n, "u": p + m, "gx": n, "gu": p + m,
              "dG": n * n, "dg0": n, "dCE": n * p, "dce0": p, "dCI": n * m, "dci0": m}
    out = []
    for name, a in (("G", pr.G), ("CE", pr.CE), ("CI", pr.CI), ("x", x), ("u", u), ("gx", gx), ("gu", gu)):
        d = np.ascontiguousarray(conv(np.asarray(a, dtype=np.float64).reshape(B, -1))).reshape(-1)
        assert d.size == rows * per_qp[name]
        out.append(placement.Spec(name, "f8", per_qp[name], d.size, d))
    out.append(placement.Spec("gf", "f8", 1, B, np.ascontiguousarray(gf)))  # one value per QP, no tiles
    out.append(placement.Spec("status", "i4", 1, B, np.ascontiguousarray(st, dtype=np.int32)))
    for name in OUTS:
        out.append(placement.Spec(name, "f8", per_qp[name], rows * per_qp[name]))
    return out


def call_in_arena(ar, pr, layout, b0=0, batch=None):
    import torch

    batch = pr.batch if batch is None else batch
    d = qpgpu.ProblemDesc(pr.n, pr.p, pr.m, 0, batch, 0, qpgpu.LAYOUTS[layout])
    ptr = lambda name: ctypes.c_void_p(ar.address(name) + b0 * ar.specs[name].E * ar.specs[name].isz)
    names = ["G", "CE", "CI", "x", "u", "status", "gx", "gu", "gf"] + list(OUTS)
    rc = qpgpu.LIB.qpgpu_vjp_full(ctypes.byref(d), *[ptr(k) for k in names], None, 0,
                                  ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
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


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("cid", ["failed_7_6_14", "group_s16_14_10_28"])
def test_gu_at_8_mod_16_and_guard_bands(gpu, cid, layout):
    """Every array at 8 mod 16, then gu alone: the same bits; guard bands round every output, the
    inputs and the TILED64 padding slots untouched."""
    pr = pair(cid)[0]
    for pl in ("odd", "only:gu"):
        ar = call_in_arena(placement.Arena(specs(cid, layout), pl, DEV), pr, layout)
        assert ar.address("gu") % 16 == 8
        assert ar.check(masks(pr, layout, pr.batch)) == [], f"{cid} {layout} {pl}"
        assert_bits(decoded(ar, pr, layout), want(cid, "both"), f"{cid} {layout} {pl}")


@pytest.mark.parametrize("layout,b0,B1", [("qp_major", 3, 66), ("tiled64", 64, 6)])
def test_sub_range_of_a_batch(gpu, layout, b0, B1):
    """Pointers advanced to QP b0 of the 70: the slice of the whole-batch result inside the range, the
    sentinel outside, inputs unchanged.  gf advances by b0 doubles in either layout."""
    cid = "failed_7_6_14"
    pr = pair(cid)[0]
    ar = placement.Arena(specs(cid, layout), "aligned", DEV)
    call_in_arena(ar, pr, layout, b0=b0, batch=B1)
    assert ar.check(masks(pr, layout, pr.batch, b0, b0 + B1)) == []
    part = decoded(ar, pr, layout)
    ref = want(cid, "both")
    assert_bits({k: v[b0:b0 + B1] for k, v in part.items()}, {k: v[b0:b0 + B1] for k, v in ref.items()},
                f"QPs [{b0}, {b0 + B1}) {layout}")


# ---- hipGraph ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", ["group_s64_64_0_128", "ws_65_2_130"])
def test_first_call_captured_into_a_graph(gpu, cid):
    """The capture enqueues the backward step and runs nothing; one replay gives the definition's bits."""
    import torch

    pr, x, u, st, gx, gu, gf = pair(cid)
    db = qpgpu.DeviceBatch(pr, DEV, with_iters=False)
    up = lambda a: torch.from_numpy(np.array(a)).to(DEV)
    xd, ud, gd, gud, gfd = up(x), up(u), up(gx), up(gu), up(gf)
    db.status.copy_(up(st))
    outs = {k: torch.full((pr.batch, db._vjp_elems(k)), 7.0, dtype=torch.float64, device=DEV) for k in db._VJP_OUTPUTS}
    ws = torch.empty(max(8, qpgpu.vjp_workspace_bytes(pr.n, pr.p, pr.m, pr.batch)), dtype=torch.uint8, device=DEV)
    s = torch.cuda.Stream(DEV)
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        db.vjp(ud, gd, outs=outs, x=xd, stream=s, workspace=ws, gu=gud, gf=gfd)
    torch.cuda.synchronize()
    assert all(bool(torch.all(t == 7.0)) for t in outs.values()), "the capture itself must not run the kernel"
    g.replay()
    torch.cuda.synchronize()
    assert_bits(db.vjp_rows(outs), want(cid, "both"), f"{cid} replay")


# ---- the autograd layers -----------------------------------------------------------------------------------
def layer_run(cid, use_x=True, use_u=True, use_f=True, full=True, skip=None):
    """Forward and backward of the layer on a case; (outputs, the six gradients as numpy or None)."""
    import torch

    pr, x, u, st, gx, gu, gf = pair(cid)
    box = is_box(cid)
    ins = [torch.from_numpy(np.array(a)).to(DEV).requires_grad_(k != skip) for k, a in enumerate(pr.arrays())]
    t = lambda a: torch.from_numpy(np.array(a)).to(DEV)
    if not full:
        xs = (qpgpu.qp_layer_box if box else qpgpu.qp_layer)(*ins)
        (xs * t(gx)).sum().backward()
        out = (xs,)
    else:
        out = (qpgpu.qp_layer_box_full if box else qpgpu.qp_layer_full)(*ins)
        xs, us, fs, ss = out
        loss = 0.0
        if use_x:
            loss = loss + (xs * t(gx)).sum()
        if use_u:
            loss = loss + (us * t(gu)).sum()
        if use_f:
            loss = loss + (fs * t(gf)).sum()
        loss.backward()
    torch.cuda.synchronize()
    names = F.BOX_OUTPUTS if box else F.DENSE_OUTPUTS
    return out, {k: (None if a.grad is None else a.grad.cpu().numpy()) for k, a in zip(names, ins)}


@pytest.mark.parametrize("cid", ["lane_7_6_14", "group_s16_14_10_28", "lane_box_7_0", "ws_65_2_130"])
def test_layer_backward_of_a_loss_on_x_u_and_f_is_the_definition(gpu, cid):
    import torch

    pr, x, u, st, gx, gu, gf = pair(cid)
    skip = 1 if cid == "lane_7_6_14" else None  # g0 does not require grad there: no dg0
    (xs, us, fs, ss), grads = layer_run(cid, skip=skip)
    assert np.array_equal(xs.detach().cpu().numpy().view(np.uint64), x.view(np.uint64))
    assert np.array_equal(us.detach().cpu().numpy().view(np.uint64), u.view(np.uint64))
    assert np.array_equal(ss.cpu().numpy(), st)
    assert ss.dtype == torch.int32 and not ss.requires_grad and ss.grad_fn is None  # status carries no grad
    assert xs.requires_grad and us.requires_grad and fs.requires_grad
    ref = want(cid, "both")
    if skip is not None:
        assert grads.pop("dg0") is None
    assert_bits(grads, {k: ref[k] for k in grads}, f"layer {cid}")


@pytest.mark.parametrize("cid,use", [("lane_7_6_14", "gu"), ("group_s16_14_10_28", "gf")])
def test_layer_backward_of_a_loss_on_u_or_f_alone(gpu, cid, use):
    """The output the loss does not use arrives as None: NULL to the entry, and gx becomes zeros."""
    pr, x, u, st, gx, gu, gf = pair(cid)
    _, grads = layer_run(cid, use_x=False, use_u=use == "gu", use_f=use == "gf")
    ref = F.vjp_full(pr, x, u, np.zeros_like(gx), gu if use == "gu" else None, gf if use == "gf" else None, st)
    assert_bits(grads, ref, f"layer {cid}, loss on {use} alone")


@pytest.mark.parametrize("cid", ["lane_7_6_14", "lane_box_7_0", "ws_65_2_130"])
def test_layer_loss_on_x_alone_gives_the_bits_of_qp_layer(gpu, cid):
    _, new = layer_run(cid, use_u=False, use_f=False)
    _, old = layer_run(cid, full=False)
    assert_bits(new, old, f"{cid}: qp_layer_full with a loss on x vs qp_layer")
    assert_bits(new, want(cid, "neither"), f"{cid}: qp_layer_full with a loss on x vs the definition")


def test_layer_with_failed_qps(gpu):
    """One indefinite and one infeasible QP in the batch: zeros there, finite gradients elsewhere."""
    cid = "failed_7_6_14"
    st = pair(cid)[3]
    (xs, us, fs, ss), grads = layer_run(cid)
    assert np.array_equal(ss.cpu().numpy(), st)
    bad = st != qpgpu.QP_OK
    for k, v in grads.items():
        assert not np.any(v[bad].view(np.uint64)), k
        assert np.all(np.isfinite(v[~bad])), k
    assert np.all(np.any(grads["dg0"][~bad] != 0, axis=1))
    assert_bits(grads, want(cid, "both"), "qp_layer_full with failed QPs")
