"""qpgpu_jvp_many / qpgpu_jvp_box_many on the GPU, bit for bit against the definition: direction k of
the entry is qpgpu_jvp on slice k (tests/jvp_many_ref.py restates it with the factorisation shared, and
tests/test_jvp_many_cpu.py checks that restatement against tests/jvp_ref.py slice by slice).  NaN
compares as NaN, -0.0 and +0.0 are different values.  The pairs (x, u) and the status words come from
the CPU reference, so only the new kernels are under test; the end-to-end tests run a solve first.
Direction k's tangents are jvp_ref.make_tangents(pr, seed=k).  Batches are small; a case's reference
is computed once and shared."""
import ctypes
import functools
import itertools

import numpy as np
import pytest

import box_dual_ref
import box_ref
import dual_ref
import jvp_many_ref
import jvp_ref
import placement
import qp_cases
import qpgpu
from vjp_ws_cases import assert_bits

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LAYOUTS = ("qp_major", "tiled64")
SENTINEL = 7.0

# (id, kind, n, p, m, B) beside dual_ref.gpu_cases() with n <= 64: tests/test_gpu_jvp.py's
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
KS = (1, 3, 17)  # 17: a partial chunk after full ones for chunks of 8 and of 16 directions
# K = 65 exceeds any chunk width: (case, QPs kept) for a lane kernel, the 16-lane and the 64-lane group kernel
WIDE = (("lane_8_0_16", 64), ("subgroup_14_10_28", 14), ("wave_64_0_128", 2))


@functools.lru_cache(maxsize=None)
def base_pair(cid):
    """(problems, x, u, status) of a case, from the CPU reference; left unchanged."""
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
    return pr, x, u, st


@functools.lru_cache(maxsize=None)
def pair(cid, K, B=None):
    """(problems, x, u, status, tangents (B, K, ...)) of the first B QPs of a case (default all)."""
    pr, x, u, st = base_pair(cid)
    if B is not None and B < pr.batch:
        pr, x, u, st = pr.slice(0, B), x[:B], u[:B], st[:B]
    return pr, x, u, st, jvp_many_ref.make_many_tangents(pr, K)


@functools.lru_cache(maxsize=None)
def want(cid, K, masked=True, B=None):
    pr, x, u, st, tan = pair(cid, K, B)
    return jvp_many_ref.jvp_many(pr, x, u if pr.p + pr.m else None, tan, K, st if masked else None)


@functools.lru_cache(maxsize=None)
def box_pair(cid, K):
    full = box_ref.case(cid)
    B = min(BOX_QPS, full.batch)
    bp = full.slice(0, B)
    x, f, st, it, u, nact = [np.array(a[:B]) for a in box_dual_ref.reference(cid)]
    return bp, x, u, st, jvp_many_ref.make_many_tangents(bp, K)


def run(cid, K, layout, masked=True, tangents=None, B=None, **kw):
    pr, x, u, st, tan = pair(cid, K, B)
    return qpgpu.jvp_many(pr, x, u if pr.p + pr.m else None, tan if tangents is None else tangents,
                          st if masked else None, layout=layout, ntan=K, **kw)


def check_blocks(cid, K, got, masked, B=None):
    """What the definition says about whole QPs, on the device's own output: masked QPs +0.0 exactly
    and q > n QPs NaN in all K blocks of every output."""
    pr, x, u, st, _ = pair(cid, K, B)
    for k, v in got.items():
        assert v.shape[:2] == (pr.batch, K), (k, v.shape)
        if masked:
            assert not np.any(v[st != qpgpu.QP_OK].view(np.uint64)), f"{cid} {k}: a masked QP is not +0.0"
    if cid.startswith("qgt"):
        for k, v in got.items():
            assert np.all(np.isnan(v[::2])), f"{cid} {k}: q > n is not NaN in all K blocks"
            assert np.all(np.isfinite(v[1::2])), f"{cid} {k}: a QP beside a NaN one"


def test_cases_cover_the_kernels():
    names = {cid: qpgpu.kernel_name_jvp_many(base_pair(cid)[0].n) for cid in CASES}
    assert all("jvp" in v and "many" in v for v in names.values())
    lane_n = {base_pair(cid)[0].n for cid, v in names.items() if "lane" in v}
    assert len(lane_n) >= 5 and 8 in lane_n, lane_n
    assert {v for v in names.values() if "group" in v} == {qpgpu.kernel_name_jvp_many(n) for n in (16, 32, 64)}
    group_n = {base_pair(cid)[0].n for cid, v in names.items() if "group" in v}
    assert {9, 14, 17, 30, 33, 64} <= group_n, group_n
    ok = lambda cid: base_pair(cid)[3] == qpgpu.QP_OK
    assert any(np.any(~ok(cid)) for cid in CASES), "no case has a status that is not OK"
    for cid in ("qgt_3_0_8", "qgt_9_2_20"):  # q > n beside q <= n, in a lane kernel and in a group kernel
        pr, x, u, st = base_pair(cid)
        q = pr.p + (u[:, pr.p:] != 0).sum(axis=1)
        assert np.all(q[::2] > pr.n) and np.all(q[1::2] <= pr.n) and np.all(st == qpgpu.QP_OK), cid
    assert {"lane", "group"} <= {("lane" if "lane" in qpgpu.kernel_name_jvp_many(base_pair(c)[0].n) else "group")
                                 for c, _ in WIDE}
    assert qpgpu.kernel_name_jvp_many(14) == qpgpu.kernel_name_jvp_many(16)


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("cid", CASES)
def test_bitwise_against_definition(gpu, cid, K):
    """Both layouts, masked and with status NULL."""
    for layout in LAYOUTS:
        for masked in (True, False):
            got = run(cid, K, layout, masked)
            assert_bits(got, want(cid, K, masked), f"{cid} K={K} {layout} masked={masked}")
            check_blocks(cid, K, got, masked)


@pytest.mark.parametrize("cid,B", WIDE)
def test_more_directions_than_any_chunk(gpu, cid, B):
    K = 65
    for layout in LAYOUTS:
        for masked in (True, False):
            got = run(cid, K, layout, masked, B=B)
            assert_bits(got, want(cid, K, masked, B), f"{cid} K={K} {layout} masked={masked}")
            check_blocks(cid, K, got, masked, B)


def test_results_do_not_depend_on_k(gpu):
    """Directions [0, 3) of the K = 17 call are the K = 3 call, on the device's own outputs."""
    for cid in ("lane_7_6_14", "wave_30_6_60"):
        a, b = run(cid, 3, "qp_major"), run(cid, 17, "qp_major")
        assert_bits({k: v[:, :3] for k, v in b.items()}, a, f"{cid}: K = 17 against K = 3")


# ---- against the device's own qpgpu_jvp ------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def made_pair(n, p, m, B):
    pr = qp_cases.make("general", n, p, m, B, seed=313)
    x, f, st, it, u, nact = dual_ref.solve(pr, dual_ref.default_cap(n, p, m))
    return pr, x, u, st


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("shape", [(7, 6, 14), (14, 10, 28), (17, 3, 40), "box_lane_7_3"], ids=str)
def test_one_launch_equals_k_single_direction_launches(gpu, shape, layout):
    """70 QPs (a tile and six), K = 5: five qpgpu_jvp launches on the slices, one qpgpu_jvp_many."""
    K = 5
    if isinstance(shape, str):
        pr, x, u, st, tan = box_pair("lane_7_3", K)
    else:
        pr, x, u, st = made_pair(*shape, 70)
        tan = jvp_many_ref.make_many_tangents(pr, K)
    assert pr.batch == 70 and np.any(st == qpgpu.QP_OK)
    many = qpgpu.jvp_many(pr, x, u, tan, st, layout=layout)
    for k in range(K):
        one = qpgpu.jvp(pr, x, u, jvp_many_ref.slice_tangents(tan, k), st, layout=layout)
        assert_bits({name: v[:, k] for name, v in many.items()}, one, f"{shape} {layout} direction {k}")


# ---- NULL arguments -----------------------------------------------------------------------------------
def entry_call(cid, K, layout, tangents, outs, masked=True):
    """The C entry itself with exactly the named tangents and outputs; all three output tensors exist
    and hold the sentinel first: ({name: numpy}, {name: untouched?})."""
    import torch

    pr, x, u, st, tan = pair(cid, K)
    db = qpgpu.DeviceBatch(pr, DEV, with_iters=False, layout=layout)
    B, E = pr.batch, pr.p + pr.m
    conv = qpgpu.to_tiled64 if layout == "tiled64" else (lambda a: a)
    up = lambda a: torch.from_numpy(np.array(conv(np.asarray(a, dtype=np.float64).reshape(B, -1)), order="C")).to(DEV)
    rows = placement.rows_of(B, layout)
    full = {"tx": torch.full((rows, K * pr.n), SENTINEL, dtype=torch.float64, device=DEV),
            "tu": torch.full((rows, K * E), SENTINEL, dtype=torch.float64, device=DEV),
            "tf": torch.full((rows, K), SENTINEL, dtype=torch.float64, device=DEV)}
    td = {k: up(tan[k]) for k in tangents if tan[k].size}
    res = db.jvp_many(up(u) if E else None, td, K, outs={k: full[k] for k in outs},
                      status=torch.from_numpy(np.array(st)).to(DEV) if masked else None, x=up(x))
    torch.cuda.synchronize()
    assert sorted(res) == sorted(outs)
    untouched = {k: bool(torch.all(full[k] == SENTINEL)) for k in full if k not in outs}
    return db.jvp_many_rows(res, K), untouched


NULL_CASES = ["lane_7_6_14", "subgroup_14_10_28", "wave_30_6_60"]


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("cid", NULL_CASES)
def test_null_tangents(gpu, cid, layout):
    """Each tangent NULL singly, and all of them NULL: the definition's bits with that tangent None."""
    K = 3
    pr, x, u, st, tan = pair(cid, K)
    for drop in [(k,) for k in jvp_ref.DENSE_TANGENTS] + [jvp_ref.DENSE_TANGENTS]:
        keep = [k for k in jvp_ref.DENSE_TANGENTS if k not in drop]
        got, _ = entry_call(cid, K, layout, keep, jvp_ref.OUTPUTS)
        ref = jvp_many_ref.jvp_many(pr, x, u, {k: tan[k] for k in keep}, K, st)
        assert_bits(got, ref, f"{cid} {layout} without {drop}")


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("cid", NULL_CASES)
def test_null_outputs(gpu, cid, layout):
    """Each output NULL singly and in pairs: the others keep their bits, and the tensor that was not
    passed still holds its sentinel everywhere."""
    K = 3
    whole = want(cid, K)
    for drop in [c for r in (1, 2) for c in itertools.combinations(jvp_ref.OUTPUTS, r)]:
        keep = [k for k in jvp_ref.OUTPUTS if k not in drop]
        got, untouched = entry_call(cid, K, layout, jvp_ref.DENSE_TANGENTS, keep)
        assert_bits(got, {k: whole[k] for k in keep}, f"{cid} {layout} without {drop}")
        assert untouched == {k: True for k in drop}


@pytest.mark.parametrize("cid", ["lane_7_6_14", "wave_30_6_60"])
def test_all_outputs_null_writes_nothing(gpu, cid):
    got, untouched = entry_call(cid, 3, "qp_major", jvp_ref.DENSE_TANGENTS, ())
    assert got == {} and untouched == {"tx": True, "tu": True, "tf": True}


@pytest.mark.parametrize("cid", ["lane_7_6_14", "wave_30_6_60"])
def test_tangents_outside_w_may_hold_nan(gpu, cid):
    """NaN in every direction's tCI column and tci0 entry of every inequality outside W."""
    K = 3
    pr, x, u, st, tan = pair(cid, K)
    off = u[:, pr.p:] == 0
    assert off.any()
    tn = dict(tan)
    tn["CI"], tn["ci0"] = tan["CI"].copy(), tan["ci0"].copy()
    for k in range(K):
        np.swapaxes(tn["CI"][:, k], 1, 2)[off] = np.nan
        tn["ci0"][:, k][off] = np.nan
    assert np.isnan(tn["CI"]).any() and np.isnan(tn["ci0"]).any()
    for layout in LAYOUTS:
        assert_bits(run(cid, K, layout, tangents=tn), want(cid, K), f"{cid} {layout}: NaN in tCI / tci0 outside W")


# ---- the box entry ------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("cid", BOX_CASES)
def test_box_entry(gpu, cid, layout):
    """Against jvp_box_many, masked and with status NULL; once more with tlo NULL."""
    K = 3
    bp, x, u, st, tan = box_pair(cid, K)
    assert "many" in qpgpu.kernel_name_jvp_many(bp.n, bp.p, bp.m)
    for masked in (True, False):
        s = st if masked else None
        got = qpgpu.jvp_many(bp, x, u, tan, s, layout=layout)
        assert_bits(got, jvp_many_ref.jvp_box_many(bp, x, u, tan, K, s), f"box {cid} {layout} masked={masked}")
    tn = {k: v for k, v in tan.items() if k != "lo"}
    assert_bits(qpgpu.jvp_many(bp, x, u, tn, st, layout=layout), jvp_many_ref.jvp_box_many(bp, x, u, tn, K, st),
                f"box {cid} {layout} tlo NULL")


def test_box_cases_are_what_they_are_named_for():
    kinds = {cid: qpgpu.kernel_name_jvp_many(box_ref.case(cid).n) for cid in BOX_CASES}
    assert "lane" in kinds["lane_7_0"] and "group" in kinds["subgroup_16_0"] and "group" in kinds["wave_lds_33_0"]
    assert kinds["subgroup_16_0"] != kinds["wave_lds_33_0"]


# ---- placement ----------------------------------------------------------------------------------------
PLACED = {"lane_70": ("lane_7_6_14", 70), "group_5": ("subgroup_14_10_28", 5)}
PK = 3  # odd: K * E is odd for odd E


@functools.lru_cache(maxsize=None)
def placed_pair(pid):
    cid, B = PLACED[pid]
    pr, x, u, st, tan = pair(cid, PK, B)
    st = np.array(st)
    if pid == "lane_70":
        st[1] = qpgpu.QP_INFEASIBLE  # a masked QP inside the first tile
    return pr, x, u, st, tan, jvp_many_ref.jvp_many(pr, x, u, tan, PK, st)


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
    out += [placement.Spec("tx", "f8", PK * n, rows * PK * n), placement.Spec("tu", "f8", PK * (p + m), rows * PK * (p + m)),
            placement.Spec("tf", "f8", PK, rows * PK)]
    return out


ARENA_ORDER = ["G", "CE", "CI", "x", "u", "status", "tG", "tg0", "tCE", "tce0", "tCI", "tci0", "tx", "tu", "tf"]


def call_in_arena(ar, pr, layout, b0=0, batch=None):
    import torch

    batch = pr.batch if batch is None else batch
    d = qpgpu.ProblemDesc(pr.n, pr.p, pr.m, 0, batch, 0, qpgpu.LAYOUTS[layout])
    ptr = lambda name: ctypes.c_void_p(ar.address(name) + b0 * ar.specs[name].E * ar.specs[name].isz)
    rc = qpgpu.LIB.qpgpu_jvp_many(ctypes.byref(d), PK, *[ptr(k) for k in ARENA_ORDER],
                                  ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert rc == qpgpu.SUCCESS, rc
    return ar


def decoded(ar, pr, layout):
    B = pr.batch
    now = ar.download()
    out = {}
    for k, sh in {"tx": (PK, pr.n), "tu": (PK, pr.p + pr.m), "tf": (PK,)}.items():
        v = ar.values(k, now)
        out[k] = qpgpu.from_tiled64(v, B, sh) if layout == "tiled64" else v.reshape((B,) + sh)
    return out


def masks(pr, layout, b0=0, b1=None):
    return {"tx": placement.block_mask(PK * pr.n, layout, pr.batch, b0, b1),
            "tu": placement.block_mask(PK * (pr.p + pr.m), layout, pr.batch, b0, b1),
            "tf": placement.block_mask(PK, layout, pr.batch, b0, b1)}


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
    """Pointers advanced to QP b0 of the 70 (K * E elements per QP, tf and its K included; status by b0
    words): the slice of the whole-batch result inside the range, the sentinel outside, inputs unchanged."""
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
def test_first_call_captured_into_a_graph(gpu, cid):
    """The capture enqueues the entry and runs nothing; one replay gives the definition's bits."""
    import torch

    K = 3
    pr, x, u, st, tan = pair(cid, K)
    db = qpgpu.DeviceBatch(pr, DEV, with_iters=False)
    up = lambda a: torch.from_numpy(np.array(a)).to(DEV)
    xd, ud, td = up(x), up(u), _device_tangents(pr, tan)
    db.status.copy_(up(st))
    outs = {"tx": torch.full((pr.batch, K * pr.n), SENTINEL, dtype=torch.float64, device=DEV),
            "tu": torch.full((pr.batch, K * (pr.p + pr.m)), SENTINEL, dtype=torch.float64, device=DEV),
            "tf": torch.full((pr.batch, K), SENTINEL, dtype=torch.float64, device=DEV)}
    s = torch.cuda.Stream(DEV)
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        db.jvp_many(ud, td, K, outs=outs, x=xd, stream=s)
    torch.cuda.synchronize()
    assert all(bool(torch.all(t == SENTINEL)) for t in outs.values()), "the capture itself must not run the kernel"
    g.replay()
    torch.cuda.synchronize()
    assert_bits(db.jvp_many_rows(outs), want(cid, K), f"{cid} replay")


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("cid", ["lane_7_6_14", "subgroup_14_10_28"])
def test_solve_then_jvp_many_on_one_stream(gpu, cid, layout):
    """DeviceBatch.solve with multipliers, then jvp_many on the same stream with no synchronisation
    between them: the definition on the device's own (x, u, status)."""
    import torch

    K = 3
    pr, _, _, _, tan = pair(cid, K)
    db = qpgpu.DeviceBatch(pr, DEV, layout=layout)
    rows = placement.rows_of(pr.batch, layout)
    u = torch.zeros((rows, pr.p + pr.m), dtype=torch.float64, device=DEV)
    conv = qpgpu.to_tiled64 if layout == "tiled64" else (lambda a: a)
    td = {k: torch.from_numpy(np.array(conv(v.reshape(pr.batch, -1)), order="C")).to(DEV) for k, v in tan.items()}
    db.solve(dual_out=(u, None))
    res = db.jvp_many(u, td, K)
    torch.cuda.synchronize()
    x, f, st, it = db.results()
    uh = u.cpu().numpy()
    uh = qpgpu.from_tiled64(uh.reshape(-1), pr.batch, (pr.p + pr.m,)) if layout == "tiled64" else uh
    assert_bits(db.jvp_many_rows(res), jvp_many_ref.jvp_many(pr, x, uh, tan, K, st), f"{cid} {layout}: solve, then jvp_many")


@pytest.mark.parametrize("box", (False, True), ids=("dense", "box"))
def test_qp_jvp_many_returns_the_solve_and_the_sensitivities(gpu, box):
    import torch

    K = 3
    if box:
        pr, x, u, st, tan = box_pair("lane_7_3", K)
    else:
        pr, x, u, st, tan = pair("lane_7_6_14", K)
    t = lambda a: torch.from_numpy(np.array(a)).to(DEV)
    names = jvp_ref.BOX_TANGENTS if box else jvp_ref.DENSE_TANGENTS
    ins = [t(a) for a in pr.arrays()]
    tn = {k: t(tan[k]) for k in names if k != "g0"}  # one name missing: a zero tangent
    xs, us, fs, ss, tx, tu, tf = (qpgpu.qp_jvp_box_many if box else qpgpu.qp_jvp_many)(*ins, tn)
    torch.cuda.synchronize()
    assert np.array_equal(xs.cpu().numpy().view(np.uint64), x.view(np.uint64))
    assert np.array_equal(us.cpu().numpy().view(np.uint64), u.view(np.uint64))
    assert np.array_equal(ss.cpu().numpy(), st) and fs.shape == (pr.batch,)
    assert tx.shape == (pr.batch, K, pr.n) and tu.shape == (pr.batch, K, pr.p + pr.m) and tf.shape == (pr.batch, K)
    ref = (jvp_many_ref.jvp_box_many if box else jvp_many_ref.jvp_many)(pr, x, u, {k: tan[k] for k in tn}, K, st)
    assert_bits({"tx": tx.cpu().numpy(), "tu": tu.cpu().numpy(), "tf": tf.cpu().numpy()}, ref, f"qp_jvp_many box={box}")


# ---- the Jacobian ------------------------------------------------------------------------------------
# dx* / dg0 two ways: forward with K = n identity directions of g0 (tx[b, k, j] = dx_j / dg0_k), and
# backward with gx = e_j (dg0_j[b, k] = dx_j / dg0_k): the adjoint identity of tests/test_jvp_cpu.py with
# one term on each side.  In exact arithmetic the Jacobian is -L^-T (I - P) L^-1 with P the projector
# on the range of M, so it is bounded by G^-1 and vanishes altogether on a QP whose W has n columns;
# there, and on every direction that W fixes, both modes return rounding of the size eps * |G^-1|, and
# the two sides' own magnitudes are no scale.  The measure is therefore per QP the largest
# |tx[b, k, j] - dg0_j[b, k]| over (j, k) relative to the largest entry of |G^-1| (np.linalg.inv of the
# symmetric G that the definition reads).  The bar is 100 x the worst value of the two CPU
# restatements (tests/jvp_many_ref.py and tests/vjp_ref.py) alone on the same data, every QP kept;
# jacobian_measure() below is what measured it: 1.13e-15 (lane_7_6_14, QP 5 of 16) and 3.4e-16
# (wave_30_6_60, 8 QPs).
JAC_CASES = {"lane_7_6_14": 16, "wave_30_6_60": 8}
JAC_MAX = 1.13e-13


def jacobian_measure(cid, forward, backward):
    """forward(pr, x, u, {"g0": (B, n, n) identities}, st) -> {"tx": (B, n, n)}; backward(pr, x, u, gx, st)
    -> {"dg0": (B, n)}.  The per-QP measure above, every QP of the case's head."""
    B = JAC_CASES[cid]
    pr, x, u, st = base_pair(cid)
    pr, x, u, st = pr.slice(0, B), x[:B], u[:B], st[:B]
    assert np.all(st == qpgpu.QP_OK)
    n = pr.n
    eye = np.broadcast_to(np.eye(n), (B, n, n)).copy()
    tx = forward(pr, x, u, {"g0": eye}, st)["tx"]
    jac = np.zeros((B, n, n))  # [b, k, j]
    for j in range(n):
        gx = np.zeros((B, n))
        gx[:, j] = 1.0
        jac[:, :, j] = backward(pr, x, u, gx, st)["dg0"]
    Gs = np.tril(pr.G) + np.swapaxes(np.tril(pr.G, -1), 1, 2)
    size = np.max(np.abs(np.linalg.inv(Gs)).reshape(B, -1), axis=1)
    return np.max(np.abs(tx - jac).reshape(B, -1), axis=1) / size


@pytest.mark.parametrize("cid", sorted(JAC_CASES))
def test_jacobian_forward_against_backward(gpu, cid):
    rel = jacobian_measure(cid, lambda pr, x, u, tan, st: qpgpu.jvp_many(pr, x, u, tan, st, outs=("tx",)),
                           lambda pr, x, u, gx, st: qpgpu.vjp(pr, x, u, gx, st, outs=("dg0",)))
    print(f"{cid}: dx/dg0 by qpgpu_jvp_many against qpgpu_vjp, worst {rel.max():.3e}")
    assert np.all(rel <= JAC_MAX), f"{cid}: {rel.max():.3e}"


# ---- refusals -----------------------------------------------------------------------------------------
def test_refusals(gpu):
    import torch

    buf = torch.zeros(65 * 65 * 4, dtype=torch.float64, device=DEV)
    p = ctypes.c_void_p(buf.data_ptr())
    call = lambda fn, d, ntan, k: fn(ctypes.byref(d), ntan, *([p] * k), None)
    d = qpgpu.ProblemDesc(65, 0, 130, 0, 1, 0, 0)
    assert call(qpgpu.LIB.qpgpu_jvp_many, d, 2, 15) == qpgpu.ERR_UNSUPPORTED_SHAPE
    assert call(qpgpu.LIB.qpgpu_jvp_box_many, d, 2, 14) == qpgpu.ERR_UNSUPPORTED_SHAPE
    d = qpgpu.ProblemDesc(7, 0, 14, 0, 1, qpgpu.FLAG_EXACT, 0)
    assert call(qpgpu.LIB.qpgpu_jvp_many, d, 2, 15) == qpgpu.ERR_INVALID_ARGUMENT
    assert call(qpgpu.LIB.qpgpu_jvp_box_many, d, 2, 14) == qpgpu.ERR_INVALID_ARGUMENT
    d = qpgpu.ProblemDesc(7, 0, 14, 0, 1, 0, 0)
    for ntan in (0, -1):
        assert call(qpgpu.LIB.qpgpu_jvp_many, d, ntan, 15) == qpgpu.ERR_INVALID_ARGUMENT
        assert call(qpgpu.LIB.qpgpu_jvp_box_many, d, ntan, 14) == qpgpu.ERR_INVALID_ARGUMENT
    assert call(qpgpu.LIB.qpgpu_jvp_many, d, 2 ** 30, 15) == qpgpu.ERR_UNSUPPORTED_SHAPE
    assert call(qpgpu.LIB.qpgpu_jvp_box_many, d, 2 ** 30, 14) == qpgpu.ERR_UNSUPPORTED_SHAPE
    d = qpgpu.ProblemDesc(7, 0, 13, 0, 1, 0, 0)
    assert call(qpgpu.LIB.qpgpu_jvp_box_many, d, 2, 14) == qpgpu.ERR_INVALID_ARGUMENT
    torch.cuda.synchronize()
    assert bool(torch.all(buf == 0)), "a refused call wrote something"
