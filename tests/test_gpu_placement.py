"""Where the data lies: every entry point of the C-ABI with its arrays carved out of ONE device
allocation (tests/placement.py) at odd alignments, as sub-ranges of a larger batch, and between
guard bands — the way a host program's own arena hands them over (include/qpgpu.h: natural
alignment suffices, a pointer into a larger batch is legal).

Every case checks three things:
  * the arena is clean after the solve (placement.Arena.check: no guard band or gap touched, every
    input the bits that were uploaded, TILED64 padding and x of a not-positive-definite QP still
    the sentinel, every owed output element written);
  * every output is bit for bit what the same call gives at the `aligned` placement — arithmetic
    does not depend on where the data lies, QPGPU_FLAG_FAST and the n > 64 default mode included;
  * the `aligned` run itself meets the existing bar against the CPU reference (the rules of
    test_gpu_parity.assert_parity / assert_fast_parity, tests/dual_ref.py, tests/box_ref.py), so
    the comparison is anchored to the reference and not to the code under test.

The lane kernels are the ones with explicit 16-byte accesses through the caller's pointers: the
LDS-DMA staging of G, g0, CE, ce0 (aligned16 of those four: else the QPGPU_LANE_UNALIGNED builds
run), and CI's LDS-DMA copy, LDS-resident rows and double2 row loads (aligned16 of CI and ci0: else
scalar loads and the first scan fills the LDS copy).  `only:<array>` clears one array's alignment
at a time.  All batches are small; they cross a 64-QP tile wherever the kernel has a partial-wave
path.  QP 1 of every generated batch has an indefinite G (its x must stay unwritten), QP 2 a
contradictory pair of inequalities."""
import functools

import numpy as np
import pytest

import box_dual_ref
import box_ref
import dual_ref
import oracle
import placement
import qp_cases
import qpgpu
import test_gpu_parity as parity

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LAYOUTS = ("qp_major", "tiled64")

# id -> (n, p, m, B, forced family, exact): the smallest batch at which each instantiation or
# family is selected and, where it has one, its partial-wave path runs
SHAPES = {
    "lane_7_6_14": (7, 6, 14, 130, None, False),      # EXACT, p = 6 (C1's kernel)
    "lane_7_0_14": (7, 0, 14, 65, None, False),       # the p = 0 part (qp_lane_p0.hip)
    "lane_7_3_14": (7, 3, 14, 70, None, False),       # EXACT, run-time p
    "lane_5_2_9": (5, 2, 9, 70, None, False),         # run-time shape
    "lane_8_0_16": (8, 0, 16, 65, None, False),       # N = 8
    "subgroup_14_10_28": (14, 10, 28, 66, "subgroup", False),
    "subgroup_8_0_32": (8, 0, 32, 70, "subgroup", False),
    "wave_17_3_40": (17, 3, 40, 9, "wave", False),    # LDS variants
    "wave_30_6_60": (30, 6, 60, 33, "wave", False),
    "ws_65_5_130": (65, 5, 130, 3, None, False),      # workspace variant, tolerance mode
    "ws_65_5_130_exact": (65, 5, 130, 3, None, True),
    "generic_12_3_24": (12, 3, 24, 5, "generic", False),
    # (7, 6, 14) with a NaN in G of one QP per wave: under QPGPU_FLAG_FAST those waves re-solve
    # with the SAFE body
    "lane_7_6_14_nan": (7, 6, 14, 130, None, False),
    "eq_14_1_28": (14, 1, 28, 66, None, False),
}
LANE_IDS = [k for k in SHAPES if k.startswith("lane") and not k.endswith("nan")]
ONLY_DENSE = [f"only:{a}" for a in ("G", "g0", "CE", "ce0", "CI", "ci0", "x")]


@functools.lru_cache(maxsize=None)
def problems(sid):
    n, p, m, B, _, _ = SHAPES[sid]
    pr = qp_cases.make("general", n, p, m, B, seed=900 + n + p)
    pr.G[1, n // 2, n // 2] = -1.0  # indefinite: QPGPU_QP_NOT_POSITIVE_DEFINITE, x unwritten
    pr.CI[2, :, 1] = -pr.CI[2, :, 0]  # a^T x + c >= 0 and -(a^T x + c) - 0.5 >= 0
    pr.ci0[2, 1] = -pr.ci0[2, 0] - 0.5
    if sid.endswith("nan"):
        for b in (5, 70, 129):
            pr.G[b, 0, 1] = pr.G[b, 1, 0] = np.nan
    return pr  # shared between tests: left unchanged


def _cap(pr):
    return 1000 + 100 * (pr.n + pr.p + pr.m)


def _copy(pr):
    return qpgpu.Problems(pr.n, pr.p, pr.m, *[np.array(a) for a in pr.arrays()])


@functools.lru_cache(maxsize=None)
def oracle_ref(sid, write_factor=False):
    """(x, f, status, iters[, factor]) of the oracle, computed once and left unchanged."""
    prc = _copy(problems(sid))
    res = oracle.solve_batch(prc, write_factor=write_factor, max_steps=_cap(prc))
    return tuple(res) + ((prc.G,) if write_factor else ())


@functools.lru_cache(maxsize=None)
def oracle_eq_ref(sid):
    """The same QPs with the inequalities dropped (m = 0): what x_eq, f_eq, status_eq must be."""
    pr = problems(sid)
    B, n = pr.batch, pr.n
    pr0 = qpgpu.Problems(n, pr.p, 0, np.array(pr.G), np.array(pr.g0), np.array(pr.CE), np.array(pr.ce0),
                         np.zeros((B, n, 0)), np.zeros((B, 0)))
    return oracle.solve_batch(pr0, max_steps=_cap(pr0))


# ---- one solve inside an arena ---------------------------------------------------------------------
def solve_in_arena(pr, layout, pl, entry="plain", family=None, **kw):
    """Carve, upload, point a device batch at the arena, solve, synchronise.  Returns the arena."""
    import torch

    box = isinstance(pr, qpgpu.BoxProblems)
    ar = placement.Arena(placement.entry_specs(pr, layout, entry), pl, DEV)
    db = (qpgpu.DeviceBoxBatch if box else qpgpu.DeviceBatch)(pr, DEV, layout=layout)
    extra = placement.attach(ar, db)
    for name in ar.specs:  # the call really gets the arena's addresses
        if name in ("G", "g0", "x", "f", "status", "iters"):
            assert getattr(db, name).data_ptr() == ar.address(name)
            assert ar.address(name) % 16 == placement.residue(pl, name, ar.specs[name].dtype)
    if entry == "eq":
        kw["eq_out"] = extra
    elif entry == "dual":
        kw["dual_out"] = extra
    db.solve(family=family, **kw)
    torch.cuda.synchronize()
    return ar


def outputs(ar, B, layout, now=None):
    """name -> (raw bits as stored, values in QP-major (B, E) / (B,)) of every output, and of G."""
    now = ar.download() if now is None else now
    out = {}
    for name, s in ar.specs.items():
        if s.data is not None and name != "G":
            continue
        v = ar.values(name, now)
        if name not in placement.PER_QP_SCALARS:
            v = qpgpu.from_tiled64(v, B, (s.E,)) if layout == "tiled64" else v.reshape(B, s.E)
        out[name] = (ar.bits(name, now), v)
    return out


def clean(ar, B, layout, notpd, write_factor=False, b0=0, b1=None):
    masks = placement.written_masks(ar, layout, B, b0, b1, x_skip=notpd)
    return ar.check(masks, modified_ok=("G",) if write_factor else ())


def assert_same_bits(got, base, label):
    for name in base:
        if name == "G":
            continue
        a, b = got[name][0], base[name][0]
        bad = np.where(a != b)[0]
        assert bad.size == 0, (f"{label}: {name} differs from the aligned placement at {bad.size} element(s), "
                               f"e.g. [{bad[0]}] {a[bad[0]]:#x} vs {b[bad[0]]:#x}")


def assert_primal_bar(o, ref, pr, label, bitwise, fast=False):
    """test_gpu_parity.assert_parity's rules (assert_fast_parity's with fast) on decoded outputs."""
    xo, fo, so, io = ref[:4]
    x, f, st, it = (o[k][1] for k in ("x", "f", "status", "iters"))
    assert np.array_equal(so, st), f"{label}: status differs at {np.where(so != st)[0][:10]}"
    assert np.array_equal(io, it), f"{label}: iteration count differs at {np.where(io != it)[0][:10]}"
    if fast:
        ok = so == qpgpu.QP_OK
        sub = qpgpu.Problems(pr.n, pr.p, pr.m, pr.G[ok], pr.g0[ok], pr.CE[ok], pr.ce0[ok], pr.CI[ok], pr.ci0[ok])
        ex, efp, eft = parity._relerr(x[ok], xo[ok], f[ok], fo[ok], np.ones(int(ok.sum()), dtype=bool), sub)
        print(f"{label}: fast rel err x {ex:.3e} f vs its terms {eft:.3e}")
        assert ex <= parity.TOL and eft <= parity.TOL, f"{label}: rel err x {ex:.3e} f vs its terms {eft:.3e}"
        return
    ok = so != qpgpu.QP_NOT_POSITIVE_DEFINITE
    ex, ef, eft = parity._relerr(x, xo, f, fo, ok, pr)
    print(f"{label}: rel err x {ex:.3e} f {ef:.3e}")
    assert ex <= parity.TOL and ef <= parity.TOL, f"{label}: rel err x {ex:.3e} f {ef:.3e} (f vs its terms {eft})"
    if bitwise:
        bx, bf = parity._bit_mismatch(x[ok], xo[ok]), parity._bit_mismatch(f, fo)
        assert not bx and not bf, f"{label}: not bitwise: x (gpu, oracle) {bx}; f (gpu, oracle) {bf}"


def assert_bits(a, b, label):
    bad = parity._bit_mismatch(a, b)
    assert np.shape(a) == np.shape(b) and not bad, f"{label}: (gpu, reference) {bad}"


@functools.lru_cache(maxsize=None)
def aligned_plain(sid, layout, fast=False, entry="plain"):
    """The `aligned` run of a generated shape, held to the bar against the oracle, once."""
    n, p, m, B, family, exact = SHAPES[sid]
    pr, ref = problems(sid), oracle_ref(sid)
    label = f"{sid} {layout} aligned{' fast' if fast else ''} {entry}"
    kw = dict(exact=exact, fast=fast)
    ar = solve_in_arena(pr, layout, "aligned", entry=entry, family=family, **kw)
    notpd = ref[2] == qpgpu.QP_NOT_POSITIVE_DEFINITE
    assert notpd[1] and not notpd[0] and ref[2][2] == qpgpu.QP_INFEASIBLE
    assert clean(ar, B, layout, notpd) == [], label
    o = outputs(ar, B, layout)
    assert_primal_bar(o, ref, pr, label, parity.bitwise_expected(n, m, exact=exact), fast=fast)
    if entry == "eq":
        xe, fe, se, _ = oracle_eq_ref(sid)
        assert np.array_equal(o["status_eq"][1], se), label
        oke = se != qpgpu.QP_NOT_POSITIVE_DEFINITE
        assert_bits(o["x_eq"][1][oke], xe[oke], label + " x_eq")
        assert_bits(o["f_eq"][1], fe, label + " f_eq")
    return o


# ---- qpgpu_solve_batched ----------------------------------------------------------------------------
def _plain_params():
    out = []
    for sid in SHAPES:
        if sid.endswith("nan") or sid.startswith("eq"):
            continue
        for lay in LAYOUTS:
            for pl in ["odd", "ci_aligned_rest_odd"] + (ONLY_DENSE if sid in LANE_IDS else []):
                out.append(pytest.param(sid, lay, pl, False, id=f"{sid}-{lay}-{pl}"))
    for sid in ("lane_7_6_14_nan", "lane_8_0_16"):
        for lay in LAYOUTS:
            for pl in ("odd", "ci_aligned_rest_odd", "only:g0", "only:ci0"):
                out.append(pytest.param(sid, lay, pl, True, id=f"{sid}-{lay}-{pl}-fast"))
    return out


@pytest.mark.parametrize("sid,layout,pl,fast", _plain_params())
def test_plain_entry_placements(gpu, sid, layout, pl, fast):
    n, p, m, B, family, exact = SHAPES[sid]
    if sid.startswith("lane"):
        assert qpgpu.kernel_name(n, p, m, fast=fast).startswith("qp_lane_fast" if fast else "qp_lane")
    base = aligned_plain(sid, layout, fast)
    ar = solve_in_arena(problems(sid), layout, pl, family=family, exact=exact, fast=fast)
    label = f"{sid} {layout} {pl}{' fast' if fast else ''}"
    notpd = oracle_ref(sid)[2] == qpgpu.QP_NOT_POSITIVE_DEFINITE
    assert clean(ar, B, layout, notpd) == [], label
    assert_same_bits(outputs(ar, B, layout), base, label)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("sid", ["lane_7_6_14", "subgroup_14_10_28", "wave_30_6_60"])
def test_write_factor_placements(gpu, sid, layout):
    """QPGPU_FLAG_WRITE_FACTOR at `odd`: G receives the oracle's factor, bit for bit, padding
    untouched; the other inputs are unchanged; x, f, status, iters are the oracle's."""
    n, p, m, B, family, _ = SHAPES[sid]
    pr = problems(sid)
    ref = oracle_ref(sid, write_factor=True)
    notpd = ref[2] == qpgpu.QP_NOT_POSITIVE_DEFINITE
    label = f"{sid} {layout} write_factor"
    for pl in ("aligned", "odd"):
        ar = solve_in_arena(pr, layout, pl, family=family, write_factor=True)
        assert clean(ar, B, layout, notpd, write_factor=True) == [], f"{label} {pl}"
        o = outputs(ar, B, layout)
        assert_primal_bar(o, ref, pr, f"{label} {pl}", True)
        conv = qpgpu.to_tiled64 if layout == "tiled64" else (lambda a: a)
        want = np.ascontiguousarray(conv(ref[4])).reshape(-1)  # (TILED64: zero padding, as uploaded)
        assert_bits(o["G"][0].view(np.float64), want, f"{label} {pl} factor")


@pytest.mark.parametrize("pl", ["odd", "ci_aligned_rest_odd"])
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("sid", ["lane_7_6_14", "eq_14_1_28", "wave_30_6_60"])
def test_eq_entry_placements(gpu, sid, layout, pl):
    """qpgpu_solve_batched_eq with x_eq, f_eq, status_eq in the arena."""
    n, p, m, B, _, _ = SHAPES[sid]
    base = aligned_plain(sid, layout, entry="eq")
    ar = solve_in_arena(problems(sid), layout, pl, entry="eq")
    notpd = oracle_ref(sid)[2] == qpgpu.QP_NOT_POSITIVE_DEFINITE
    assert clean(ar, B, layout, notpd) == [], f"{sid} {layout} {pl}"
    assert_same_bits(outputs(ar, B, layout), base, f"{sid} {layout} {pl} eq")


# ---- qpgpu_solve_batched_dual ----------------------------------------------------------------------
DUAL_CASES = ("lane_7_6_14", "subgroup_14_10_28", "wave_30_6_60", "ws_65_2_130")
BOX_CASES = ("lane_7_0", "lane_7_3", "lane_5_2", "subgroup_9_1", "wave_lds_33_0", "wave_ws_65_0")


def assert_reference_bits(o, ref, label):
    """Bitwise against a tests/*_ref.py reference: (x, f, status, iters[, u, nact])."""
    xr, fr, sr, ir = ref[:4]
    assert np.array_equal(o["status"][1], sr), f"{label}: status differs at {np.where(o['status'][1] != sr)[0][:8]}"
    assert np.array_equal(o["iters"][1], ir), f"{label}: l1 passes differ at {np.where(o['iters'][1] != ir)[0][:8]}"
    ok = sr != qpgpu.QP_NOT_POSITIVE_DEFINITE
    assert_bits(o["f"][1], fr, label + " f")
    assert_bits(o["x"][1][ok], xr[ok], label + " x")
    if len(ref) > 4:
        assert_bits(o["u"][1], ref[4], label + " u")
        assert np.array_equal(o["nact"][1], ref[5]), f"{label}: nact differs"


@functools.lru_cache(maxsize=None)
def aligned_ref_case(kind, cid, family, layout):
    """The `aligned` run of a tests/dual_ref.py / box_ref.py case, bitwise against its reference."""
    if kind == "dual":
        pr, ref, entry = dual_ref.case(cid), dual_ref.reference(cid), "dual"
    elif kind == "box":
        pr, ref, entry = box_ref.case(cid), box_ref.reference(cid), "plain"
    else:
        pr, ref, entry = box_ref.case(cid), box_dual_ref.reference(cid), "dual"
    ar = solve_in_arena(pr, layout, "aligned", entry=entry, family=family)
    notpd = ref[2] == qpgpu.QP_NOT_POSITIVE_DEFINITE
    label = f"{kind} {cid} {family} {layout} aligned"
    assert clean(ar, pr.batch, layout, notpd) == [], label
    o = outputs(ar, pr.batch, layout)
    assert_reference_bits(o, ref, label)
    return pr, notpd, entry, o


def _ref_case_test(kind, cid, family, layout, pl):
    pr, notpd, entry, base = aligned_ref_case(kind, cid, family, layout)
    ar = solve_in_arena(pr, layout, pl, entry=entry, family=family)
    label = f"{kind} {cid} {family} {layout} {pl}"
    assert clean(ar, pr.batch, layout, notpd) == [], label
    assert_same_bits(outputs(ar, pr.batch, layout), base, label)


def _dual_params():
    import test_gpu_dual

    out = []
    for cid in DUAL_CASES:
        pr = dual_ref.case(cid)
        for fam in ("lane", "subgroup", "wave", "generic"):
            if test_gpu_dual.covers(fam, pr.n, pr.m):
                for lay in LAYOUTS:
                    for pl in ("odd", "only:u"):
                        out.append(pytest.param(cid, fam, lay, pl, id=f"{cid}-{fam}-{lay}-{pl}"))
    return out


@pytest.mark.parametrize("cid,family,layout,pl", _dual_params())
def test_dual_entry_placements(gpu, cid, family, layout, pl):
    _ref_case_test("dual", cid, family, layout, pl)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_generic_sub_batches_in_the_arena(gpu, layout):
    """launch_generic hands the generic kernel its sub-batches as pointers into the batch, each
    array advanced by its own per-QP size (u by p + m): a workspace cap of three QPs against 200
    (TILED64: one tile per launch), the arrays at `odd`."""
    import ctypes

    cid = "lane_7_6_14"
    pr = dual_ref.case(cid)
    wsb = qpgpu.LIB.qpk_generic_workspace_bytes
    wsb.restype, wsb.argtypes = ctypes.c_int64, [ctypes.c_int, ctypes.c_int, ctypes.c_int64]
    setcap = qpgpu.LIB.qpgpu_debug_set_generic_ws_cap
    setcap.argtypes = [ctypes.c_int64]
    setcap(3 * wsb(pr.n, pr.m, 1))
    try:
        _ref_case_test("dual", cid, "generic", layout, "odd")
    finally:
        setcap(0)


def _box_params():
    out = []
    for cid in BOX_CASES:
        fam = "wave" if cid.startswith("wave") else cid.split("_")[0]
        for kind in ("box", "box_dual"):
            for lay in LAYOUTS:
                for pl in ["odd"] + (["only:hi", "only:lo"] if fam == "lane" else []):
                    out.append(pytest.param(kind, cid, fam, lay, pl, id=f"{kind}-{cid}-{lay}-{pl}"))
    return out


@pytest.mark.parametrize("kind,cid,family,layout,pl", _box_params())
def test_box_entries_placements(gpu, kind, cid, family, layout, pl):
    name = (qpgpu.kernel_name_box_dual if kind == "box_dual" else qpgpu.kernel_name_box)
    bp = box_ref.case(cid)
    assert "box" in name(bp.n, bp.p, qpgpu.FAMILY_FLAGS[family])
    _ref_case_test(kind, cid, family, layout, pl)


# ---- a sub-range of a larger batch -----------------------------------------------------------------
SUB_TOTAL = 200
SUB_RANGES = {"qp_major": ((1, 64), (63, 70), (65, 128), (3, 1)), "tiled64": ((64, 70),)}
# id -> (n, p, m, forced family, entry); the box-dual one has m = 2n
SUB_SHAPES = {
    "lane_7_6_14": (7, 6, 14, "lane", "plain"),
    "lane_7_0_14": (7, 0, 14, "lane", "plain"),
    "subgroup_9_1_20": (9, 1, 20, "subgroup", "plain"),
    "wave_33_0_66": (33, 0, 66, "wave", "plain"),
    "box_dual_7_3": (7, 3, 14, None, "box_dual"),
}


@functools.lru_cache(maxsize=None)
def sub_case(sid):
    """The 200-QP batch and its reference; QPs 64 and 100 indefinite, 10 and 66 contradictory."""
    n, p, m, _, entry = SUB_SHAPES[sid]
    if entry == "box_dual":
        bp = qpgpu.make_box_problems(n, p, 0, SUB_TOTAL, seed=77)
        bp.g0 *= 3.0  # so that bounds bind
        bp.G[[64, 100], n // 2, n // 2] = -1.0
        bp.hi[[10, 66], 1], bp.lo[[10, 66], 1] = -0.5, 0.5  # lo > hi
        ref = dual_ref.solve(bp.to_dense(), box_ref.default_cap(n, p))
        return bp, ref
    pr = qp_cases.make("general", n, p, m, SUB_TOTAL, seed=33 + n)
    pr.G[[64, 100], n // 2, n // 2] = -1.0
    for b in (10, 66):
        pr.CI[b, :, 1] = -pr.CI[b, :, 0]
        pr.ci0[b, 1] = -pr.ci0[b, 0] - 0.5
    return pr, oracle.solve_batch(_copy(pr), max_steps=_cap(pr))


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("sid", list(SUB_SHAPES))
def test_sub_range_of_a_batch(gpu, sid, layout):
    """Every pointer advanced to QP b0 of one uploaded 200-QP batch, batch = B1: inside the range the
    reference's slice, outside it every output still the sentinel, inputs unchanged.  In QP-major an
    odd b0 moves G, g0 (E odd) to 8 mod 16 while CI, ci0 (E even) stay aligned."""
    import torch

    n, p, m, family, entry = SUB_SHAPES[sid]
    pr, ref = sub_case(sid)
    box = entry == "box_dual"
    assert set(np.where(ref[2] == qpgpu.QP_NOT_POSITIVE_DEFINITE)[0]) == {64, 100}
    assert ref[2][10] == ref[2][66] == qpgpu.QP_INFEASIBLE
    ar = placement.Arena(placement.entry_specs(pr, layout, "dual" if box else "plain"), "aligned", DEV)
    db = (qpgpu.DeviceBoxBatch if box else qpgpu.DeviceBatch)(pr, DEV, layout=layout)
    for b0, B1 in SUB_RANGES[layout]:
        label = f"{sid} {layout} QPs [{b0}, {b0 + B1})"
        ar.reset()
        extra = placement.attach(ar, db, b0=b0, batch=B1)
        if layout == "qp_major" and b0 % 2 and n % 2:
            assert db.g0.data_ptr() % 16 == 8 and db.G.data_ptr() % 16 == 8
        db.solve(family=family, **({"dual_out": extra} if box else {}))
        torch.cuda.synchronize()
        sl = slice(b0, b0 + B1)
        notpd = ref[2][sl] == qpgpu.QP_NOT_POSITIVE_DEFINITE
        assert clean(ar, SUB_TOTAL, layout, notpd, b0=b0, b1=b0 + B1) == [], label
        o = {k: (bits, v[sl]) for k, (bits, v) in outputs(ar, SUB_TOTAL, layout).items()}
        assert_reference_bits(o, tuple(r[sl] for r in ref), label)


# ---- hipGraph replay --------------------------------------------------------------------------------
def test_graph_replay_at_odd_placement(gpu):
    """One capture and one replay of (7, 6, 14, 128) at `ci_aligned_rest_odd` (CI's DMA paths on, the
    staging unaligned): replay = eager = oracle, the arena clean."""
    import torch

    sid, B, layout, pl = "lane_7_6_14", 128, "qp_major", "ci_aligned_rest_odd"
    pr = problems(sid).slice(0, B)
    ref = tuple(r[:B] for r in oracle_ref(sid))
    notpd = ref[2] == qpgpu.QP_NOT_POSITIVE_DEFINITE
    eager = outputs(solve_in_arena(pr, layout, pl), B, layout)
    assert_reference_bits(eager, ref, "eager")
    ar = placement.Arena(placement.entry_specs(pr, layout, "plain"), pl, DEV)
    db = qpgpu.DeviceBatch(pr, DEV, layout=layout)
    placement.attach(ar, db)
    s = torch.cuda.Stream(DEV)
    with torch.cuda.stream(s):
        db.solve(stream=s)  # warm-up on the capturing stream
    s.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        db.solve(stream=s)
    torch.cuda.synchronize()
    ar.reset()  # the outputs hold sentinels again: what is there afterwards, the replay wrote
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    assert clean(ar, B, layout, notpd) == []
    assert_same_bits(outputs(ar, B, layout), eager, "replay vs eager")
