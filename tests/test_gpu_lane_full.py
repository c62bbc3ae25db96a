"""The lane kernel's full-wave aligned kernels (qp_lane.hip: lane_body's FULL, qp_lane_full_kernel)
and the launch that splits a batch into its whole 64-QP blocks and the remaining QPs.

The full-wave kernels take the plain solves of the shapes (7, 6, 14) and (7, 0, 14) whose arrays
pass both 16-byte checks, without QPGPU_FLAG_WRITE_FACTOR and without a pass count (iters NULL);
the QPs past the last whole block go through the general kernel as a second launch with advanced
pointers, and every other launch runs the general kernels as before.  Which of the two was
enqueued is read from the test hook qpgpu_debug_lane_launches (qpgpu_kernel_name_flags names the
family's kernel for a shape and flags; it sees neither the addresses nor iters).

Every case is compared to the CPU oracle bit for bit — x, f, status, and the pass counts where they
are asked for — in both layouts, with every array inside one arena between guard bands
(tests/placement.py): a stray write of either launch, e.g. of the remainder launch past its QPs,
lands in a guard band or in a sentinel-filled output slot and is reported.

Batches: 1 and 63 (remainder only), 64 (one full wave), 65 (a full wave and a remainder of 1), 191
(two full waves and 63).  One lane of the first wave holds a QP with duplicated / zero inequality
columns and one a small-integer QP whose Givens steps meet |h| < eps (qp_cases._fuzz_qp's
"dup_zero_cols" and "integer_ties"), so that one wave runs both forms of the rotation; QP 1 has an
indefinite G (x unwritten), QP 2 a contradictory pair of inequalities."""
import ctypes
import functools

import numpy as np
import pytest

import oracle
import placement
import qp_cases
import qpgpu

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LAYOUTS = ("qp_major", "tiled64")
SHAPES = ((7, 6, 14), (7, 0, 14))
BATCHES = (1, 63, 64, 65, 191)
BMAX = max(BATCHES)
DUP_LANE, TIE_LANE = 5, 9  # both inside the first wave, beside ordinary QPs


def _cap(pr):
    return 1000 + 100 * (pr.n + pr.p + pr.m)


@functools.lru_cache(maxsize=None)
def problems(n, p, m):
    """BMAX QPs; every batch size solves the first B of them.  Shared: left unchanged."""
    pr = qp_cases.make("general", n, p, m, BMAX, seed=4100 + p)
    if BMAX > 2:
        pr.G[1, n // 2, n // 2] = -1.0
        pr.CI[2, :, 1] = -pr.CI[2, :, 0]
        pr.ci0[2, 1] = -pr.ci0[2, 0] - 0.5
    for lane, mode in ((DUP_LANE, "dup_zero_cols"), (TIE_LANE, "integer_ties")):
        q = qp_cases._fuzz_qp(np.random.default_rng([94, p, lane]), n, p, m, mode, False)
        for dst, src in zip(pr.arrays(), q):
            dst[lane] = src
    return pr


@functools.lru_cache(maxsize=None)
def oracle_ref(n, p, m, write_factor=False):
    """(x, f, status, iters[, factor]) of the oracle on all BMAX QPs, once (QPs are independent:
    the first B rows are the reference of every batch size)."""
    pr = problems(n, p, m)
    prc = qpgpu.Problems(pr.n, pr.p, pr.m, *[np.array(a) for a in pr.arrays()])
    res = oracle.solve_batch(prc, write_factor=write_factor, max_steps=_cap(prc))
    return tuple(res) + ((prc.G,) if write_factor else ())


def lane_launches(reset=True):
    fn = qpgpu.LIB.qpgpu_debug_lane_launches
    fn.argtypes = [ctypes.POINTER(ctypes.c_int64), ctypes.c_int]
    fn.restype = None
    out = (ctypes.c_int64 * 2)()
    fn(out, 1 if reset else 0)
    return out[0], out[1]


def solve(shape, B, layout, pl, with_iters, write_factor=False):
    """One solve of the first B QPs inside an arena.  Returns (arena, launches since the reset)."""
    import torch

    pr = problems(*shape).slice(0, B)
    specs = placement.entry_specs(pr, layout)
    if not with_iters:
        specs = [s for s in specs if s.name != "iters"]
    ar = placement.Arena(specs, pl, DEV)
    db = qpgpu.DeviceBatch(pr, DEV, with_iters=with_iters, layout=layout)
    placement.attach(ar, db)
    for name, s in ar.specs.items():  # the call really gets the arena's addresses
        if s.count == 0:  # (p = 0: CE and ce0 hold nothing, and an empty tensor has no address)
            continue
        assert getattr(db, name).data_ptr() == ar.address(name)
        assert ar.address(name) % 16 == placement.residue(pl, name, ar.specs[name].dtype)
    lane_launches(reset=True)
    db.solve(write_factor=write_factor)
    torch.cuda.synchronize()
    return ar, lane_launches(reset=True)


def check(ar, shape, B, layout, label, write_factor=False):
    """The arena is clean and every output is the oracle's, bit for bit."""
    n, p, m = shape
    ref = oracle_ref(n, p, m, write_factor)
    xo, fo, so, io = (np.asarray(a)[:B] for a in ref[:4])
    notpd = so == qpgpu.QP_NOT_POSITIVE_DEFINITE
    masks = placement.written_masks(ar, layout, B, x_skip=notpd)
    assert ar.check(masks, modified_ok=("G",) if write_factor else ()) == [], label
    now = ar.download()
    x = ar.values("x", now)
    x = qpgpu.from_tiled64(x, B, (n,)) if layout == "tiled64" else x.reshape(B, n)
    f, st = ar.values("f", now), ar.values("status", now)
    assert np.array_equal(st, so), f"{label}: status differs at {np.where(st != so)[0][:10]}"
    assert np.array_equal(f.view(np.uint64), fo.view(np.uint64)), \
        f"{label}: f differs at {np.where(f.view(np.uint64) != fo.view(np.uint64))[0][:10]}"
    ok = ~notpd
    bad = np.where((x[ok].view(np.uint64) != xo.reshape(B, n)[ok].view(np.uint64)).any(axis=1))[0]
    assert bad.size == 0, f"{label}: x differs at (ok-)QPs {bad[:10]}"
    if "iters" in ar.specs:
        it = ar.values("iters", now)
        assert np.array_equal(it, io), f"{label}: pass count differs at {np.where(it != io)[0][:10]}"
    if write_factor:
        G = ar.values("G", now)
        G = qpgpu.from_tiled64(G, B, (n * n,)) if layout == "tiled64" else G.reshape(B, n * n)
        fac = np.asarray(ref[4])[:B].reshape(B, n * n)
        assert np.array_equal(G[ok].view(np.uint64), fac[ok].view(np.uint64)), f"{label}: factor differs"


def test_the_special_lanes_do_what_they_are_there_for():
    """The data and the oracle's view of the two special lanes: both pass the setup and enter the
    loop; the small-integer lane has a diagonal G and, with p = 6, zeros in the last two entries of
    CE's first column, so d = J^T np ends in two exact zeros and the first Givens step of the
    equality phase meets h = 0 (the reference skips it) while the other lanes rotate."""
    for shape in SHAPES:
        pr, ref = problems(*shape), oracle_ref(*shape)
        assert ref[2][1] == qpgpu.QP_NOT_POSITIVE_DEFINITE and ref[2][2] == qpgpu.QP_INFEASIBLE
        assert ref[3][DUP_LANE] >= 1 and ref[3][TIE_LANE] >= 1
        assert np.count_nonzero(pr.CI[TIE_LANE] == 0.0) > 0
        assert np.array_equal(pr.G[TIE_LANE], np.diag(np.diag(pr.G[TIE_LANE])))
        if pr.p > 0:
            assert not pr.CE[TIE_LANE][-2:, 0].any() and pr.CE[TIE_LANE][:, 0].any()


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_aligned_without_pass_count_runs_full_waves_and_a_remainder(gpu, shape, B, layout):
    assert qpgpu.LIB.qpgpu_kernel_name_flags(*shape, 0).decode() == "qp_lane<N=7,M=14>"
    ar, (nfull, nrest) = solve(shape, B, layout, "aligned", with_iters=False)
    assert (nfull, nrest) == (1 if B >= 64 else 0, 1 if B % 64 else 0), (B, nfull, nrest)
    check(ar, shape, B, layout, f"{shape} B={B} {layout} aligned")


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_offset_by_8_bytes_falls_back(gpu, shape, B, layout):
    """Every array 8 bytes off a 16-byte boundary: neither check passes, the general kernels run."""
    assert qpgpu.LIB.qpgpu_kernel_name_flags(*shape, 0).decode() == "qp_lane<N=7,M=14>"
    ar, launches = solve(shape, B, layout, "odd", with_iters=False)
    assert launches == (0, 0), launches
    check(ar, shape, B, layout, f"{shape} B={B} {layout} odd")


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("pl", ["only:CI", "only:ci0", "only:G", "only:g0"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_one_array_off_falls_back(gpu, shape, pl, layout):
    """One array of either group off its 16-byte check is enough: the full-wave kernels assume both."""
    ar, launches = solve(shape, 65, layout, pl, with_iters=False)
    assert launches == (0, 0), (pl, launches)
    check(ar, shape, 65, layout, f"{shape} B=65 {layout} {pl}")


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("B", (65, 191))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_pass_count_requested_falls_back(gpu, shape, B, layout):
    ar, launches = solve(shape, B, layout, "aligned", with_iters=True)
    assert launches == (0, 0), launches
    check(ar, shape, B, layout, f"{shape} B={B} {layout} iters")


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("with_iters", (False, True))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_write_factor_falls_back(gpu, shape, with_iters, layout):
    name = qpgpu.LIB.qpgpu_kernel_name_flags(*shape, qpgpu.FLAG_WRITE_FACTOR).decode()
    assert name == "qp_lane<N=7,M=14>"
    ar, launches = solve(shape, 65, layout, "aligned", with_iters=with_iters, write_factor=True)
    assert launches == (0, 0), launches
    check(ar, shape, 65, layout, f"{shape} B=65 {layout} write_factor", write_factor=True)
