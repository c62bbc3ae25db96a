"""qpgpu_jvp / qpgpu_jvp_box on the GPU, bit for bit against the definition (tests/jvp_ref.py): NaN
compares as NaN, -0.0 and +0.0 are different values.  The pairs (x, u) and the status words come
from the CPU reference, so only the new kernels are under test; the end-to-end tests run a solve
first.  The tangents come from a fixed seed (jvp_ref.make_tangents).  Batches are small; a case's
reference is computed once and shared."""
import ctypes
import functools
import itertools

import numpy as np
import pytest

import box_dual_ref
import box_ref
import dual_ref
import jvp_ref
import placement
import qp_cases
import qpgpu
import vjp_full_ref
from test_jvp_cpu import ADJ_MAX
from vjp_ws_cases import assert_bits

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LAYOUTS = ("qp_major", "tiled64")
SENTINEL = 7.0

# (id, kind, n, p, m, B) beside dual_ref.gpu_cases() with n <= 64
EXTRA = [
    ("group_9_2_20", "general", 9, 2, 20, 9),
    ("box_33_0_66", "box", 33, 0, 66, 3),
    ("lane_7_6_14_x1", "general", 7, 6, 14, 1),
    ("lane_7_6_14_x63", "general", 7, 6, 14, 63),
    ("lane_7_6_14_x65", "general", 7, 6, 14, 65),
    ("qgt_3_0_8", "general", 3, 0, 8, 5),    # every multiplier of the even QPs set non-zero: q > n there
    ("qgt_9_2_20", "general", 9, 2, 20, 5),
]
CASES = sorted(c for c, pr in dual_ref.gpu_cases().items() if pr.n <= 64) + [e[0] for e in EXTRA]
BOX_CASES = ("lane_7_0", "lane_7_3", "subgroup_16_0", "wave_lds_33_0", "long_7_3", "inf_7_3")
BOX_QPS = 70  # a TILED64 tile and six more


@functools.lru_cache(maxsize=None)
def pair(cid):
    """(problems, x, u, status, tangents) of a case, from the CPU reference; left unchanged."""
    for eid, kind, n, p, m, B in EXTRA:
        if eid == cid:
            pr = qp_cases.make(kind, n, p, m, B, seed=311)
            if kind == "box":
                pr.g0 *= box_ref.g0_scale(n)  # so that bounds bind
            x, f, st, it, u, nact = dual_ref.solve(pr, dual_ref.default_cap(n, p, m))
            if cid.startswith("qgt"):
                u[::2] = 1.0
            break
    else:
        pr = dual_ref.case(cid)
        x, f, st, it, u, nact = dual_ref.reference(cid)
    return pr, x, u, st, jvp_ref.make_tangents(pr)


@functools.lru_cache(maxsize=None)
def want(cid, masked=True):
    pr, x, u, st, tan = pair(cid)
    return jvp_ref.jvp(pr, x, u if pr.p + pr.m else None, tan, st if masked else None)


@functools.lru_cache(maxsize=None)
def box_pair(cid):
    full = box_ref.case(cid)
    B = min(BOX_QPS, full.batch)
    bp = full.slice(0, B)
    x, f, st, it, u, nact = [np.array(a[:B]) for a in box_dual_ref.reference(cid)]
    return bp, x, u, st, jvp_ref.make_tangents(bp)


def run(cid, layout, masked=True, tangents=None, box=False, **kw):
    pr, x, u, st, tan = box_pair(cid) if box else pair(cid)
    return qpgpu.jvp(pr, x, u if pr.p + pr.m else None, tan if tangents is None else tangents,
                     st if masked else None, layout=layout, **kw)


def test_cases_cover_the_kernels():
    names = {cid: qpgpu.kernel_name_jvp(pair(cid)[0].n) for cid in CASES}
    assert all("jvp" in v for v in names.values())
    lane_n = {pair(cid)[0].n for cid, v in names.items() if "lane" in v}
    assert len(lane_n) >= 5, lane_n
    assert {v for v in names.values() if "group" in v} == {qpgpu.kernel_name_jvp(n) for n in (16, 32, 64)}
    q = lambda cid: pair(cid)[0].p + (pair(cid)[2][:, pair(cid)[0].p:] != 0).sum(axis=1)
    ok = lambda cid: pair(cid)[3] == qpgpu.QP_OK
    assert any(np.any((pair(cid)[2][:, pair(cid)[0].p:] != 0)[ok(cid)]) for cid in CASES)  # an active inequality
    assert np.any(pair("box_33_0_66")[2] != 0), "no bound binds on the box data"
    for cid in ("qgt_3_0_8", "qgt_9_2_20"):  # q > n beside q <= n, in a lane kernel and in a group kernel
        assert np.any(q(cid)[ok(cid)] > pair(cid)[0].n) and np.any(q(cid)[ok(cid)] <= pair(cid)[0].n), cid
        assert np.all(np.isnan(want(cid)["tx"][::2])) and not np.any(np.isnan(want(cid)["tx"][1::2]))
    assert any(np.any(~ok(cid)) for cid in CASES), "no case has a status that is not OK"
    assert {pair(c)[0].batch for c in ("lane_7_6_14_x1", "lane_7_6_14_x63", "lane_7_6_14_x65")} == {1, 63, 65}


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("masked", (True, False), ids=("masked", "status_null"))
@pytest.mark.parametrize("cid", CASES)
def test_bitwise_against_definition(gpu, cid, masked, layout):
    got = run(cid, layout, masked)
    assert_bits(got, want(cid, masked), f"{cid} {layout} masked={masked}")
    if masked:
        st = pair(cid)[3]
        for k, v in got.items():
            assert not np.any(v[st != qpgpu.QP_OK].view(np.uint64)), k  # +0.0 exactly


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("cid", ["lane_7_6_14", "subgroup_14_10_28", "wave_17_3_40", "wave_64_0_128"])
def test_more_columns_than_variables_is_nan(gpu, cid, layout):
    """Every multiplier non-zero on the even QPs: q = p + m > n there, NaN in every output element;
    the odd QPs keep their bits (a lane, and a group of a wave, beside a NaN one)."""
    pr, x, u, st, tan = pair(cid)
    B = min(pr.batch, 70)
    sub = pr.slice(0, B)
    u2 = np.array(u[:B])
    u2[::2] = 1.0
    tn = {k: v[:B] for k, v in tan.items()}
    got = qpgpu.jvp(sub, x[:B], u2, tn, None, layout=layout)
    ref = jvp_ref.jvp(sub, x[:B], u2, tn)
    assert all(np.all(np.isnan(v[::2])) for v in got.values())
    assert_bits(got, ref, f"{cid} {layout} q > n")


# ---- NULL arguments -----------------------------------------------------------------------------------
def entry_call(cid, layout, tangents, outs, box=False, masked=True):
    """The C entry itself with exactly the named tangents and outputs; all three output tensors exist
    and hold the sentinel first: ({name: numpy}, {name: untouched?})."""
    import torch

    pr, x, u, st, tan = box_pair(cid) if box else pair(cid)
    db = (qpgpu.DeviceBoxBatch if box else qpgpu.DeviceBatch)(pr, DEV, with_iters=False, layout=layout)
    B, E = pr.batch, pr.p + pr.m
    conv = qpgpu.to_tiled64 if layout == "tiled64" else (lambda a: a)
    up = lambda a: torch.from_numpy(np.array(conv(np.asarray(a, dtype=np.float64).reshape(B, -1)), order="C")).to(DEV)
    rows = placement.rows_of(B, layout)
    full = {"tx": torch.full((rows, pr.n), SENTINEL, dtype=torch.float64, device=DEV),
            "tu": torch.full((rows, E), SENTINEL, dtype=torch.float64, device=DEV),
            "tf": torch.full((B,), SENTINEL, dtype=torch.float64, device=DEV)}
    td = {k: up(tan[k]) for k in tangents if tan[k].size}
    res = db.jvp(up(u) if E else None, td, outs={k: full[k] for k in outs},
                 status=torch.from_numpy(np.array(st)).to(DEV) if masked else None, x=up(x))
    torch.cuda.synchronize()
    assert sorted(res) == sorted(outs)
    untouched = {k: bool(torch.all(full[k] == SENTINEL)) for k in full if k not in outs}
    return db.jvp_rows(res), untouched


NULL_CASES = ["lane_7_6_14", "subgroup_14_10_28", "wave_30_6_60"]


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("cid", NULL_CASES)
def test_null_tangents(gpu, cid, layout):
    """Each tangent NULL singly, and all of them NULL: the definition's bits with that tangent None."""
    pr, x, u, st, tan = pair(cid)
    for drop in [(k,) for k in jvp_ref.DENSE_TANGENTS] + [jvp_ref.DENSE_TANGENTS]:
        keep = [k for k in jvp_ref.DENSE_TANGENTS if k not in drop]
        got, _ = entry_call(cid, layout, keep, jvp_ref.OUTPUTS)
        ref = jvp_ref.jvp(pr, x, u, {k: tan[k] for k in keep}, st)
        assert_bits(got, ref, f"{cid} {layout} without {drop}")


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("cid", NULL_CASES)
def test_null_outputs(gpu, cid, layout):
    """Each output NULL singly and in pairs: the others keep their bits, and the tensor that was not
    passed still holds its sentinel everywhere."""
    whole = want(cid)
    for drop in [c for r in (1, 2) for c in itertools.combinations(jvp_ref.OUTPUTS, r)]:
        keep = [k for k in jvp_ref.OUTPUTS if k not in drop]
        got, untouched = entry_call(cid, layout, jvp_ref.DENSE_TANGENTS, keep)
        assert_bits(got, {k: whole[k] for k in keep}, f"{cid} {layout} without {drop}")
        assert untouched == {k: True for k in drop}


def test_all_outputs_null_writes_nothing(gpu):
    got, untouched = entry_call("lane_7_6_14", "qp_major", jvp_ref.DENSE_TANGENTS, ())
    assert got == {} and untouched == {"tx": True, "tu": True, "tf": True}


@pytest.mark.parametrize("cid", ["lane_7_6_14", "wave_30_6_60"])
def test_tangents_outside_w_may_hold_nan(gpu, cid):
    pr, x, u, st, tan = pair(cid)
    off = u[:, pr.p:] == 0
    assert off.any()
    tn = dict(tan)
    tn["CI"], tn["ci0"] = tan["CI"].copy(), tan["ci0"].copy()
    np.swapaxes(tn["CI"], 1, 2)[off] = np.nan
    tn["ci0"][off] = np.nan
    for layout in LAYOUTS:
        assert_bits(run(cid, layout, tangents=tn), want(cid), f"{cid} {layout}: NaN in tCI / tci0 outside W")


# ---- the box entry ------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("cid", BOX_CASES)
def test_box_entry(gpu, cid, layout):
    """Against jvp_box, and against the dense entry run on to_dense() with tCI = NULL and
    tci0 = [thi; -tlo]; masked and with status NULL; once more with tlo NULL."""
    bp, x, u, st, tan = box_pair(cid)
    dense = bp.to_dense()
    assert "jvp" in qpgpu.kernel_name_jvp(bp.n, bp.p, bp.m)
    for masked in (True, False):
        s = st if masked else None
        got = run(cid, layout, masked, box=True)
        assert_bits(got, jvp_ref.jvp_box(bp, x, u, tan, s), f"box {cid} {layout} masked={masked}")
        same = qpgpu.jvp(dense, x, u, jvp_ref.box_tangents_as_dense(bp, tan), s, layout=layout)
        assert_bits(got, same, f"box {cid} {layout} masked={masked}: the box entry vs the dense entry on to_dense()")
    tn = {k: v for k, v in tan.items() if k != "lo"}
    assert_bits(run(cid, layout, tangents=tn, box=True), jvp_ref.jvp_box(bp, x, u, tn, st), f"box {cid} {layout} tlo NULL")


def test_box_cases_are_what_they_are_named_for():
    kinds = {cid: qpgpu.kernel_name_jvp(box_pair(cid)[0].n) for cid in BOX_CASES}
    assert "lane" in kinds["lane_7_0"] and "group" in kinds["subgroup_16_0"] and "group" in kinds["wave_lds_33_0"]
    assert kinds["subgroup_16_0"] != kinds["wave_lds_33_0"]
    for cid in ("lane_7_0", "subgroup_16_0", "wave_lds_33_0", "long_7_3"):
        bp, x, u = box_pair(cid)[:3]
        assert np.any(u[:, bp.p:bp.p + bp.n] != 0) and np.any(u[:, bp.p + bp.n:] != 0), cid  # both kinds of bound


# ---- placement ----------------------------------------------------------------------------------------
PLACED = {"lane_70": ("lane_7_6_14", 70), "group_5": ("subgroup_14_10_28", 5)}


@functools.lru_cache(maxsize=None)
def placed_pair(pid):
    cid, B = PLACED[pid]
    pr, x, u, st, tan = pair(cid)
    st = np.array(st[:B])
    if pid == "lane_70":
        st[1] = qpgpu.QP_INFEASIBLE  # a masked QP inside the first tile
    sub = pr.slice(0, B)
    tn = {k: v[:B] for k, v in tan.items()}
    return sub, x[:B], u[:B], st, tn, jvp_ref.jvp(sub, x[:B], u[:B], tn, st)


def specs(pid, layout):
    pr, x, u, st, tan, _ = placed_pair(pid)
    B, n, p, m = pr.batch, pr.n, pr.p, pr.m
    rows = placement.rows_of(B, layout)
    conv = qpgpu.to_tiled64 if layout == "tiled64" else (lambda a: a)
    out = []
    for name, a in (("G", pr.G), ("CE", pr.CE), ("CI", pr.CI), ("x", x), ("u", u), ("tG", tan["G"]), ("tg0", tan["g0"]),
                    ("tCE", tan["CE"]), ("tce0", tan["ce0"]), ("tCI", tan["CI"]), ("tci0", tan["ci0"])):
        a = np.asarray(a, dtype=np.float64).reshape(B, -1)
        d = np.ascontiguousarray(conv(a)).reshape(-1)
        assert d.size == rows * a.shape[1]
        out.append(placement.Spec(name, "f8", a.shape[1], d.size, d))
    out.append(placement.Spec("status", "i4", 1, B, np.ascontiguousarray(st, dtype=np.int32)))
    out += [placement.Spec("tx", "f8", n, rows * n), placement.Spec("tu", "f8", p + m, rows * (p + m)),
            placement.Spec("tf", "f8", 1, B)]
    return out


ARENA_ORDER = ["G", "CE", "CI", "x", "u", "status", "tG", "tg0", "tCE", "tce0", "tCI", "tci0", "tx", "tu", "tf"]


def call_in_arena(ar, pr, layout, b0=0, batch=None):
    import torch

    batch = pr.batch if batch is None else batch
    d = qpgpu.ProblemDesc(pr.n, pr.p, pr.m, 0, batch, 0, qpgpu.LAYOUTS[layout])
    ptr = lambda name: ctypes.c_void_p(ar.address(name) + b0 * ar.specs[name].E * ar.specs[name].isz)
    rc = qpgpu.LIB.qpgpu_jvp(ctypes.byref(d), *[ptr(k) for k in ARENA_ORDER],
                             ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert rc == qpgpu.SUCCESS, rc
    return ar


def decoded(ar, pr, layout):
    B = pr.batch
    now = ar.download()
    shapes = {"tx": (pr.n,), "tu": (pr.p + pr.m,)}
    out = {"tf": ar.values("tf", now)}
    for k, sh in shapes.items():
        v = ar.values(k, now)
        out[k] = qpgpu.from_tiled64(v, B, sh) if layout == "tiled64" else v.reshape((B,) + sh)
    return out


def masks(pr, layout, b0=0, b1=None):
    return {"tx": placement.block_mask(pr.n, layout, pr.batch, b0, b1),
            "tu": placement.block_mask(pr.p + pr.m, layout, pr.batch, b0, b1),
            "tf": placement.scalar_mask(pr.batch, b0, b1)}


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("pid", sorted(PLACED))
def test_arrays_at_8_mod_16_and_guard_bands(gpu, pid, layout):
    """Every float64 array at 8 mod 16: the same bits; the guard bands round every array, the inputs
    and the TILED64 padding slots untouched."""
    pr, x, u, st, tan, ref = placed_pair(pid)
    ar = call_in_arena(placement.Arena(specs(pid, layout), "odd", DEV), pr, layout)
    assert all(ar.address(k) % 16 == 8 for k in ("G", "tG", "tCI", "tx", "tu", "tf"))
    assert ar.check(masks(pr, layout)) == [], f"{pid} {layout}"
    assert_bits(decoded(ar, pr, layout), ref, f"{pid} {layout} odd placement")


@pytest.mark.parametrize("layout,b0,B1", [("qp_major", 3, 66), ("tiled64", 64, 6)])
def test_sub_range_of_a_batch(gpu, layout, b0, B1):
    """Pointers advanced to QP b0 of the 70: the slice of the whole-batch result inside the range, the
    sentinel outside, inputs unchanged.  tf and status advance by b0 elements in either layout."""
    pid = "lane_70"
    pr, x, u, st, tan, ref = placed_pair(pid)
    ar = placement.Arena(specs(pid, layout), "aligned", DEV)
    call_in_arena(ar, pr, layout, b0=b0, batch=B1)
    assert ar.check(masks(pr, layout, b0, b0 + B1)) == []
    part = decoded(ar, pr, layout)
    assert_bits({k: v[b0:b0 + B1] for k, v in part.items()}, {k: v[b0:b0 + B1] for k, v in ref.items()},
                f"QPs [{b0}, {b0 + B1}) {layout}")


# ---- hipGraph, end to end --------------------------------------------------------------------------------
def _device_tangents(pr, tan):
    import torch

    return {k: torch.from_numpy(np.ascontiguousarray(v.reshape(pr.batch, -1))).to(DEV) for k, v in tan.items() if v.size}


@pytest.mark.parametrize("cid", ["lane_8_0_16", "wave_64_0_128"])
def test_call_captured_into_a_graph(gpu, cid):
    """The capture enqueues the entry and runs nothing; one replay gives the definition's bits."""
    import torch

    pr, x, u, st, tan = pair(cid)
    db = qpgpu.DeviceBatch(pr, DEV, with_iters=False)
    up = lambda a: torch.from_numpy(np.array(a)).to(DEV)
    xd, ud, td = up(x), up(u), _device_tangents(pr, tan)
    db.status.copy_(up(st))
    outs = {"tx": torch.full((pr.batch, pr.n), SENTINEL, dtype=torch.float64, device=DEV),
            "tu": torch.full((pr.batch, pr.p + pr.m), SENTINEL, dtype=torch.float64, device=DEV),
            "tf": torch.full((pr.batch,), SENTINEL, dtype=torch.float64, device=DEV)}
    s = torch.cuda.Stream(DEV)
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        db.jvp(ud, td, outs=outs, x=xd, stream=s)
    torch.cuda.synchronize()
    assert all(bool(torch.all(t == SENTINEL)) for t in outs.values()), "the capture itself must not run the kernel"
    g.replay()
    torch.cuda.synchronize()
    assert_bits(db.jvp_rows(outs), want(cid), f"{cid} replay")


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("cid", ["lane_7_6_14", "subgroup_14_10_28"])
def test_solve_then_jvp_on_one_stream(gpu, cid, layout):
    """DeviceBatch.solve with multipliers, then jvp on the same stream with no synchronisation between
    them: the definition on the device's own (x, u, status)."""
    import torch

    pr, _, _, _, tan = pair(cid)
    db = qpgpu.DeviceBatch(pr, DEV, layout=layout)
    rows = placement.rows_of(pr.batch, layout)
    u = torch.zeros((rows, pr.p + pr.m), dtype=torch.float64, device=DEV)
    conv = qpgpu.to_tiled64 if layout == "tiled64" else (lambda a: a)
    td = {k: torch.from_numpy(np.array(conv(v.reshape(pr.batch, -1)), order="C")).to(DEV) for k, v in tan.items()}
    db.solve(dual_out=(u, None))
    res = db.jvp(u, td)
    torch.cuda.synchronize()
    x, f, st, it = db.results()
    uh = u.cpu().numpy()
    uh = qpgpu.from_tiled64(uh.reshape(-1), pr.batch, (pr.p + pr.m,)) if layout == "tiled64" else uh
    assert_bits(db.jvp_rows(res), jvp_ref.jvp(pr, x, uh, tan, st), f"{cid} {layout}: solve, then jvp")


@pytest.mark.parametrize("box", (False, True), ids=("dense", "box"))
def test_qp_jvp_returns_the_solve_and_the_sensitivities(gpu, box):
    import torch

    if box:
        pr, x, u, st, tan = box_pair("lane_7_3")
    else:
        pr, x, u, st, tan = pair("lane_7_6_14")
    t = lambda a: torch.from_numpy(np.array(a)).to(DEV)
    names = jvp_ref.BOX_TANGENTS if box else jvp_ref.DENSE_TANGENTS
    ins = [t(a) for a in pr.arrays()]
    tn = {k: t(tan[k]) for k in names if k != "g0"}  # one name missing: a zero tangent
    xs, us, fs, ss, tx, tu, tf = (qpgpu.qp_jvp_box if box else qpgpu.qp_jvp)(*ins, tn)
    torch.cuda.synchronize()
    assert np.array_equal(xs.cpu().numpy().view(np.uint64), x.view(np.uint64))
    assert np.array_equal(us.cpu().numpy().view(np.uint64), u.view(np.uint64))
    assert np.array_equal(ss.cpu().numpy(), st) and fs.shape == (pr.batch,)
    ref = (jvp_ref.jvp_box if box else jvp_ref.jvp)(pr, x, u, {k: tan[k] for k in tn}, st)
    assert_bits({"tx": tx.cpu().numpy(), "tu": tu.cpu().numpy(), "tf": tf.cpu().numpy()}, ref, f"qp_jvp box={box}")


@pytest.mark.parametrize("cid", ["lane_7_6_14", "wave_30_6_60"])
def test_adjoint_identity_on_the_device(gpu, cid):
    """jvp and vjp(..., gu=, gf=) on the GPU: <gx, tx> + <gu, tu> + gf tf = <grad theta, t theta> within
    the bar measured on the CPU (tests/test_jvp_cpu.py), relative to the sum of the terms' sizes."""
    pr, x, u, st, tan = pair(cid)
    B = min(pr.batch, 16)
    sub = pr.slice(0, B)
    x, u, st = x[:B], u[:B], st[:B]
    tn = {k: v[:B] for k, v in tan.items()}
    assert np.all(st == qpgpu.QP_OK)
    rng = np.random.default_rng([pr.n, pr.p, pr.m, 43])
    gx, gu, gf = rng.standard_normal((B, pr.n)), rng.standard_normal((B, pr.p + pr.m)), rng.standard_normal(B)
    t = qpgpu.jvp(sub, x, u, tn, st)
    grads = qpgpu.vjp(sub, x, u, gx, st, gu=gu, gf=gf)
    inW = np.ones(u.shape, dtype=bool)
    inW[:, pr.p:] = u[:, pr.p:] != 0
    terms = [gx * t["tx"], np.where(inW, gu * t["tu"], 0.0), (gf * t["tf"])[:, None]]
    lhs = sum(a.sum(axis=1) for a in terms)
    size = sum(np.abs(a).sum(axis=1) for a in terms)
    rhs = np.zeros(B)
    for k, name in zip(vjp_full_ref.DENSE_OUTPUTS, jvp_ref.DENSE_TANGENTS):
        prod = (grads[k] * tn[name]).reshape(B, -1)
        rhs = rhs + prod.sum(axis=1)
        size = size + np.abs(prod).sum(axis=1)
    rel = np.abs(lhs - rhs) / size
    print(f"{cid}: adjoint identity on the device, worst {rel.max():.3e}")
    assert np.all(rel <= ADJ_MAX), f"{cid}: {rel.max():.3e}"


# ---- refusals -----------------------------------------------------------------------------------------
def test_refusals(gpu):
    import torch

    buf = torch.zeros(65 * 65 * 4, dtype=torch.float64, device=DEV)
    p = ctypes.c_void_p(buf.data_ptr())
    call = lambda fn, d, k: fn(ctypes.byref(d), *([p] * k), None)
    d = qpgpu.ProblemDesc(65, 0, 130, 0, 1, 0, 0)
    assert call(qpgpu.LIB.qpgpu_jvp, d, 15) == qpgpu.ERR_UNSUPPORTED_SHAPE
    assert call(qpgpu.LIB.qpgpu_jvp_box, d, 14) == qpgpu.ERR_UNSUPPORTED_SHAPE
    d = qpgpu.ProblemDesc(7, 0, 14, 0, 1, qpgpu.FLAG_EXACT, 0)
    assert call(qpgpu.LIB.qpgpu_jvp, d, 15) == qpgpu.ERR_INVALID_ARGUMENT
    assert call(qpgpu.LIB.qpgpu_jvp_box, d, 14) == qpgpu.ERR_INVALID_ARGUMENT
    d = qpgpu.ProblemDesc(7, 0, 13, 0, 1, 0, 0)
    assert call(qpgpu.LIB.qpgpu_jvp_box, d, 14) == qpgpu.ERR_INVALID_ARGUMENT
    torch.cuda.synchronize()
    assert bool(torch.all(buf == 0)), "a refused call wrote something"
