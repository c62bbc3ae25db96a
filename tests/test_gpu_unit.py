"""qpgpu_solve_batched_unit on the GPU: x, f, status and iters — and the eq triple — of every kernel
family and both layouts, bit for bit against the oracle on the materialised problem with G = I
(tests/unit_ref.py; its case list is vetted on the CPU by tests/test_unit_cpu.py).  NaNs compare
equal to NaNs.  Float outputs are filled with NaN and integer ones with -7 before every solve, so a
slot the kernel did not write shows; in the TILED64 layout the padding entries of x must still hold
that NaN afterwards.  All batches are small."""
import ctypes

import numpy as np
import pytest

import placement
import qpgpu
import unit_ref

pytestmark = pytest.mark.gpu

LAYOUTS = ("qp_major", "tiled64")


def _bit_mismatch(a, b, show=6):
    a = np.ascontiguousarray(a, dtype=np.float64).ravel()
    b = np.ascontiguousarray(b, dtype=np.float64).ravel()
    assert a.shape == b.shape
    diff = (a.view(np.uint64) != b.view(np.uint64)) & ~(np.isnan(a) & np.isnan(b))
    return [(int(i), float(a[i]).hex(), float(b[i]).hex()) for i in np.where(diff)[0][:show]]


def _prefill(db, eq):
    for t in (db.x, db.f) + ((db.x_eq, db.f_eq) if eq else ()):
        t.fill_(float("nan"))
    for t in (db.status, db.iters) + ((db.status_eq,) if eq else ()):
        t.fill_(-7)


def run_unit(up, family=None, layout=None, max_iter=0, eq=False, stream=None):
    """One unit solve through DeviceUnitBatch: (x, f, status, iters[, x_eq, f_eq, status_eq])."""
    import torch

    db = qpgpu.DeviceUnitBatch(up, "cuda:0", layout=layout)
    if eq:
        db._eq_tensors()
    _prefill(db, eq)
    db.solve(max_iter=max_iter, family=family, eq=eq, stream=stream)
    torch.cuda.synchronize()
    if db.layout == qpgpu.LAYOUT_TILED64 and up.batch % 64:
        for t in (db.x,) + ((db.x_eq,) if eq else ()):
            xt = t.cpu().numpy().reshape(-1, up.n, 64)
            assert np.all(np.isnan(xt[-1][:, up.batch % 64:])), "a padding entry of x was written"
    return db.results() + (db.eq_results() if eq else ())


def assert_matches(got, ref, label):
    x, f, st, it = got[:4]
    xr, fr, sr, ir = ref[:4]
    assert np.array_equal(st, sr), f"{label}: status differs at {np.where(st != sr)[0][:8]}: {st[st != sr][:8]} vs {sr[st != sr][:8]}"
    assert np.array_equal(it, ir), f"{label}: l1 passes differ at {np.where(it != ir)[0][:8]}"
    assert not _bit_mismatch(f, fr), f"{label}: f (index, gpu, ref) {_bit_mismatch(f, fr)}"
    assert not _bit_mismatch(x, xr), f"{label}: x (index, gpu, ref) {_bit_mismatch(x, xr)}"
    if len(got) > 4:
        xe, fe, se = got[4:]
        xer, fer, ser = ref[4:]
        assert np.array_equal(se, ser), f"{label}: status_eq differs at {np.where(se != ser)[0][:8]}"
        assert not _bit_mismatch(fe, fer), f"{label}: f_eq {_bit_mismatch(fe, fer)}"
        assert not _bit_mismatch(xe, xer), f"{label}: x_eq {_bit_mismatch(xe, xer)}"


def full_reference(cid, max_steps=0):
    return tuple(unit_ref.reference(cid, max_steps)) + tuple(unit_ref.reference_eq(cid))


def _family_params():
    out = []
    for cid, up in unit_ref.cases().items():
        for fam in unit_ref.FAMILIES:
            if unit_ref.covers(fam, up.n, up.m):
                for lay in LAYOUTS:
                    out.append(pytest.param(cid, fam, lay, id=f"{cid}-{fam or 'default'}-{lay}"))
    return out


@pytest.mark.parametrize("cid,family,layout", _family_params())
def test_bitwise_against_oracle(gpu, cid, family, layout):
    """Four outputs, then again with the eq triple (seven outputs)."""
    up = unit_ref.case(cid)
    name = qpgpu.kernel_name_unit(up.n, up.p, up.m, qpgpu.FAMILY_FLAGS[family])
    assert "unit" in name
    if family:
        assert {"lane": "qp_lane", "subgroup": "qp_small", "wave": "qp_wave"}[family] in name
    ref = full_reference(cid)
    assert_matches(run_unit(up, family=family, layout=layout), ref[:4], f"{cid} {family} {layout}")
    assert_matches(run_unit(up, family=family, layout=layout, eq=True), ref, f"{cid} {family} {layout} eq")


@pytest.mark.parametrize("cid,family", [("lane_7_3_14", "lane"), ("subgroup_8_2_32", "subgroup"),
                                        ("wave_14_10_28", "wave"), ("crossed_30_6_60", "wave")])
def test_equals_dense_entries_in_the_same_process(gpu, cid, family):
    """The same bits as DeviceBatch.solve(exact=True) and as qpgpu_solve_batched_eq on to_dense()."""
    import torch

    up = unit_ref.case(cid)
    got = run_unit(up, family=family, eq=True)
    db = qpgpu.DeviceBatch(unit_ref.dense(cid), "cuda:0")
    db.solve(exact=True, family=family)
    torch.cuda.synchronize()
    assert_matches(got[:4], db.results(), f"{cid} {family} vs dense exact")
    eq_out = (torch.full_like(db.x, float("nan")), torch.full_like(db.f, float("nan")), torch.full_like(db.status, -7))
    db.solve(exact=True, family=family, eq_out=eq_out)
    torch.cuda.synchronize()
    dense = db.results() + (eq_out[0].cpu().numpy(), eq_out[1].cpu().numpy(), eq_out[2].cpu().numpy())
    assert_matches(got, dense, f"{cid} {family} vs dense eq")
    assert np.allclose(db.G.cpu().numpy(), np.eye(up.n))  # (the dense side did have its identity)


@pytest.mark.parametrize("cid,family", [("lane_7_3_14", "lane"), ("subgroup_8_2_32", "subgroup"),
                                        ("wave_30_6_60", "wave")])
def test_step_cap(gpu, cid, family):
    """max_iter = 3: the capped QPs match the oracle under the same cap."""
    ref = tuple(unit_ref.reference(cid, 3)) + tuple(unit_ref.reference_eq(cid))
    assert (ref[2] == qpgpu.QP_MAX_ITER).any()
    assert_matches(run_unit(unit_ref.case(cid), family=family, max_iter=3, eq=True), ref, f"max_iter = 3 {family}")


@pytest.mark.parametrize("family", ["lane", "subgroup", "wave"])
def test_null_ce_with_p0_and_null_ci_with_m0(gpu, family):
    """CE / ce0 may be NULL when p = 0 and CI / ci0 when m = 0 (a torch tensor of no elements has a
    NULL data_ptr; here the attributes are None)."""
    import torch

    cid = "lane_7_0_0"  # p = 0 and m = 0: all four NULL
    db = qpgpu.DeviceUnitBatch(unit_ref.case(cid), "cuda:0")
    db.CE = db.ce0 = db.CI = db.ci0 = None
    db._eq_tensors()
    _prefill(db, True)
    db.solve(family=family, eq=True)
    torch.cuda.synchronize()
    assert_matches(db.results() + db.eq_results(), full_reference(cid), f"all NULL {family}")
    cid = "lane_1_0_2"  # p = 0, m > 0
    db = qpgpu.DeviceUnitBatch(unit_ref.case(cid), "cuda:0")
    db.CE = db.ce0 = None
    _prefill(db, False)
    db.solve(family=family)
    torch.cuda.synchronize()
    assert_matches(db.results(), unit_ref.reference(cid), f"NULL CE {family}")


def _specs(up, layout, total=None):
    """placement.Spec list of the unit entry's arrays for `up` (the inputs in `layout`)."""
    B, n, p, m = up.batch, up.n, up.p, up.m
    rows = placement.rows_of(B, layout)
    conv = qpgpu.to_tiled64 if layout == "tiled64" else (lambda a: a)
    per = {"g0": n, "CE": n * p, "ce0": p, "CI": n * m, "ci0": m}
    specs = []
    for name, a in zip(("g0", "CE", "ce0", "CI", "ci0"), up.arrays()):
        d = np.ascontiguousarray(conv(np.asarray(a, dtype=np.float64))).reshape(-1)
        assert d.size == rows * per[name]
        specs.append(placement.Spec(name, "f8", per[name], d.size, d))
    specs += [placement.Spec("x", "f8", n, rows * n), placement.Spec("f", "f8", 1, B),
              placement.Spec("status", "i4", 1, B), placement.Spec("iters", "i4", 1, B),
              placement.Spec("x_eq", "f8", n, rows * n), placement.Spec("f_eq", "f8", 1, B),
              placement.Spec("status_eq", "i4", 1, B)]
    return specs


def _arena_solve(up, layout, place, family, b0=0, b1=None):
    """Solve QPs [b0, b1) of `up` in one arena at `place`; returns (arena, findings, outputs of
    the solved range as numpy in QP-major order)."""
    import torch

    b1 = up.batch if b1 is None else b1
    arena = placement.Arena(_specs(up, layout), place, device="cuda:0")
    db = qpgpu.DeviceUnitBatch(up.slice(0, 1), "cuda:0", layout=layout)
    eq = placement.attach(arena, db, b0=b0, batch=b1 - b0)
    db.x_eq, db.f_eq, db.status_eq = eq
    db.solve(family=family, eq=True)
    torch.cuda.synchronize()
    findings = arena.check(placement.written_masks(arena, layout, up.batch, b0, b1))
    now = arena.download()

    def rows(name, E):
        v = arena.values(name, now)
        if E is None:
            return v[b0:b1]
        full = qpgpu.from_tiled64(v, up.batch, (E,)) if layout == "tiled64" else v.reshape(-1, E)[:up.batch]
        return full[b0:b1]

    n = up.n
    return arena, findings, (rows("x", n), rows("f", None), rows("status", None), rows("iters", None),
                             rows("x_eq", n), rows("f_eq", None), rows("status_eq", None))


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("place", ["odd", "only:g0", "only:CE", "ci_aligned_rest_odd"])
def test_lane_unaligned_placement(gpu, layout, place):
    """g0 / CE at 8 mod 16: the lane family's unaligned build, the same bits, nothing else touched."""
    cid = "lane_7_3_14"
    up = unit_ref.case(cid)
    arena, findings, got = _arena_solve(up, layout, place, "lane")
    assert arena.address("g0") % 16 == (0 if place == "only:CE" else 8)
    assert not findings, findings
    assert_matches(got, full_reference(cid), f"{place} {layout}")


@pytest.mark.parametrize("cid,family", [("lane_7_3_14", "lane"), ("subgroup_forced_14_10_28", "subgroup"),
                                        ("wave_14_10_28", "wave")])
@pytest.mark.parametrize("layout,b0,b1", [("qp_major", 3, 60), ("qp_major", 1, 66), ("tiled64", 64, 66),
                                          ("tiled64", 0, 64)])
def test_sub_range_with_guard_bands(gpu, cid, family, layout, b0, b1):
    """A sub-range of a larger batch: only its QPs' outputs are written, every guard band holds."""
    up = unit_ref.case(cid)
    assert b1 <= up.batch
    _, findings, got = _arena_solve(up, layout, "aligned", family, b0, b1)
    assert not findings, findings
    assert_matches(got, tuple(a[b0:b1] for a in full_reference(cid)), f"{cid} [{b0}, {b1}) {layout}")


@pytest.mark.parametrize("cid,family", [("lane_5_2_9", "lane"), ("wave_14_1_28", "wave")])
def test_graph_capture_of_a_first_call(gpu, cid, family):
    """No workspace and no per-kernel grant: the very first call for a batch object is captured
    (on a side stream, as tests/test_gpu_graph.py captures), replay = the oracle."""
    import torch

    up = unit_ref.case(cid)
    dev = torch.device("cuda", 0)
    db = qpgpu.DeviceUnitBatch(up, dev)
    db._eq_tensors()
    s = torch.cuda.Stream(dev)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        db.solve(stream=s, family=family, eq=True)
    _prefill(db, True)
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    assert_matches(db.results() + db.eq_results(), full_reference(cid), f"graph replay {cid}")


def _raw_call(up, flags=0, n=None, m=None, eq=(True, True, True), iters=True):
    import torch

    db = qpgpu.DeviceUnitBatch(up, "cuda:0")
    e = db._eq_tensors()
    d = qpgpu.ProblemDesc(n or up.n, up.p, up.m if m is None else m, 0, up.batch, flags, 0)
    vp = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    rc = qpgpu.LIB.qpgpu_solve_batched_unit(
        ctypes.byref(d), vp(db.g0), vp(db.CE), vp(db.ce0), vp(db.CI), vp(db.ci0), vp(db.x), vp(db.f),
        vp(db.status), vp(db.iters) if iters else None, *[vp(t) if k else None for t, k in zip(e, eq)],
        ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc, db


def test_refusals_through_the_library(gpu):
    up = unit_ref.case("wave_14_10_28")
    inv, uns = qpgpu.ERR_INVALID_ARGUMENT, qpgpu.ERR_UNSUPPORTED_SHAPE
    assert _raw_call(up)[0] == qpgpu.SUCCESS
    assert _raw_call(up, flags=qpgpu.FLAG_EXACT)[0] == qpgpu.SUCCESS  # implied anyway
    assert _raw_call(up, eq=(False, False, False))[0] == qpgpu.SUCCESS
    # (n = 65 and m = 257 are refused from the descriptor: the arrays, sized for (14, 10, 28), are not read)
    assert _raw_call(up, n=65)[0] == uns
    assert _raw_call(up, m=257)[0] == uns
    assert _raw_call(up, flags=qpgpu.FLAG_FORCE_GENERIC)[0] == uns
    assert _raw_call(up, flags=qpgpu.FLAG_FORCE_LANE)[0] == uns
    assert _raw_call(up, flags=qpgpu.FLAG_FAST)[0] == inv
    assert _raw_call(up, flags=qpgpu.FLAG_WRITE_FACTOR)[0] == inv
    for mixed in ((True, False, False), (False, True, True), (True, True, False)):
        assert _raw_call(up, eq=mixed)[0] == inv
    # iters may be NULL: the other outputs are the same bits
    rc, db = _raw_call(up, iters=False)
    assert rc == qpgpu.SUCCESS
    x, f, st, _ = db.results()
    ref = full_reference("wave_14_10_28")
    assert_matches((x, f, st, ref[3]) + db.eq_results(), ref, "NULL iters")


def test_launcher_and_convenience_wrapper(gpu):
    import torch

    cid = "subgroup_6_0_20"
    db = qpgpu.DeviceUnitBatch(unit_ref.case(cid), "cuda:0", layout="tiled64")
    db._eq_tensors()
    _prefill(db, True)
    db.launcher(torch.cuda.current_stream(), eq=True)()
    torch.cuda.synchronize()
    assert_matches(db.results() + db.eq_results(), full_reference(cid), "launcher")
    for layout in LAYOUTS:
        got = qpgpu.solve_batched_unit(unit_ref.case(cid), layout=layout, eq=True)
        assert got[0].shape == (70, 6) and len(got) == 7
        assert_matches(got, full_reference(cid), f"wrapper {layout}")
        assert len(qpgpu.solve_batched_unit(unit_ref.case(cid), layout=layout)) == 4
