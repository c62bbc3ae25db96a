"""The lane kernels' LDS-DMA staging (qp_lane.hip: copy_chunk / copy_span, round_b, dma_ci_part).

Every copy names its LDS slot through M0 and the instruction's immediate offset, which the hardware
adds to the global address as well: G / g0 and CE / ce0 go in runs of up to four 1 KiB chunks on
one source address and one M0, CI's 16-byte pieces on one per-lane source address with an M0 per
piece.  A chunk or piece that lands in another slot, or comes from another address, changes what
some lane reads: the batches are qpgpu.make_problems', whose QPs all differ, and x, f and status
are compared with the CPU oracle bit for bit (the pass count is not asked for: with it the
full-wave kernels do not run, tests/test_gpu_lane_full.py).

Cases, in both layouts:
  * (7, 6, 14) and (7, 0, 14), B = 64, 65, 191: the full-wave kernels (unrolled spans, the G tail
    chunk) and the remainder launch (general kernels: whole waves by DMA, partial per lane);
  * (8, 6, 16), B = 65: the N = 8 instantiation (32 CI pieces, other span lengths);
  * (5, 3, 9), B = 65: a run-time shape, whose spans end inside a chunk (the tail guard is live);
  * the 191 QPs as QPs [64, 255) of a 320-QP allocation: every wave's base is not the array's;
  * QPGPU_FLAG_FAST at (7, 6, 14), B = 65, against the exact build's output of the same call;
  * qpgpu_solve_batched_unit at (7, 6, 14), B = 65."""
import functools

import numpy as np
import pytest

import oracle
import qpgpu
import test_gpu_parity as parity

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LAYOUTS = ("qp_major", "tiled64")
BMAX = 191
SEED = 7100


def _cap(n, p, m):
    return 1000 + 100 * (n + p + m)


@functools.lru_cache(maxsize=None)
def problems(n, p, m):
    """BMAX seeded QPs; every batch size solves the first B of them.  Shared: left unchanged."""
    return qpgpu.make_problems("general", n, p, m, 0, BMAX, seed=SEED + 10 * n + p)


@functools.lru_cache(maxsize=None)
def oracle_ref(n, p, m):
    """(x, f, status) of the oracle on all BMAX QPs, once (the QPs are independent)."""
    pr = problems(n, p, m)
    prc = qpgpu.Problems(n, p, m, *[np.array(a) for a in pr.arrays()])
    x, f, st, _ = oracle.solve_batch(prc, max_steps=_cap(n, p, m))
    for a in (x, f, st):
        a.setflags(write=False)
    return x.reshape(BMAX, n), f, st


def _prefill(db):
    db.x.fill_(float("nan"))
    db.f.fill_(float("nan"))
    db.status.fill_(-7)


def gpu_solve(pr, layout, **kw):
    """One solve without a pass count: (x (B, n), f, status)."""
    import torch

    db = qpgpu.DeviceBatch(pr, DEV, with_iters=False, layout=layout)
    _prefill(db)
    db.solve(**kw)
    torch.cuda.synchronize()
    x, f, st, _ = db.results()
    return x.reshape(pr.batch, pr.n), f, st


def assert_bits(got, ref, label):
    x, f, st = got
    xr, fr, sr = ref
    assert np.array_equal(st, sr), f"{label}: status differs at {np.where(st != sr)[0][:8]}"
    ok = sr != qpgpu.QP_NOT_POSITIVE_DEFINITE  # (x is unwritten on that exit)
    bf, bx = parity._bit_mismatch(f, fr), parity._bit_mismatch(x[ok], xr[ok])
    assert not bf, f"{label}: f (gpu, oracle) {bf}"
    assert not bx, f"{label}: x (gpu, oracle) {bx}"


def test_the_batches_are_solved_and_their_lanes_differ():
    """What the comparison rests on: no two QPs share the first entry of G, CE or CI, and the
    oracle solves every QP (so every x depends on all of its QP's staged data)."""
    for shape in ((7, 6, 14), (7, 0, 14), (8, 6, 16), (5, 3, 9)):
        pr, (x, f, st) = problems(*shape), oracle_ref(*shape)
        for a in (pr.G, pr.CE, pr.CI):
            flat = a.reshape(BMAX, -1)
            if flat.shape[1]:
                assert np.unique(flat[:, 0]).size == BMAX
        assert (st == qpgpu.QP_OK).all(), (shape, np.bincount(st))


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("B", (64, 65, 191))
@pytest.mark.parametrize("shape", ((7, 6, 14), (7, 0, 14)), ids=lambda s: "x".join(map(str, s)))
def test_full_wave_shapes(gpu, shape, B, layout):
    assert qpgpu.kernel_name(*shape) == "qp_lane<N=7,M=14>"
    ref = tuple(a[:B] for a in oracle_ref(*shape))
    assert_bits(gpu_solve(problems(*shape).slice(0, B), layout), ref, f"{shape} B={B} {layout}")


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("shape", ((8, 6, 16), (5, 3, 9)), ids=lambda s: "x".join(map(str, s)))
def test_n8_and_run_time_shape(gpu, shape, layout):
    assert qpgpu.kernel_name(*shape).startswith("qp_lane<N=")
    ref = tuple(a[:65] for a in oracle_ref(*shape))
    assert_bits(gpu_solve(problems(*shape).slice(0, 65), layout), ref, f"{shape} B=65 {layout}")


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("shape", ((7, 6, 14), (7, 0, 14)), ids=lambda s: "x".join(map(str, s)))
def test_sub_range_of_a_larger_allocation(gpu, shape, layout):
    """The 191 QPs as QPs [64, 255) of 320 uploaded ones, every pointer advanced to QP 64 and
    batch = 191: the copies' per-wave bases are 64 QPs past the arrays', the outputs outside the
    range stay as they were."""
    import torch

    n, p, m = shape
    b0, total = 64, 320
    pr = problems(*shape)
    fill = qpgpu.make_problems("general", n, p, m, 0, total, seed=SEED + 1)
    big = qpgpu.Problems(n, p, m, *[np.concatenate([f[:b0], a, f[b0 + BMAX:]]) for a, f in
                                    zip(pr.arrays(), fill.arrays())])
    db = qpgpu.DeviceBatch(big, DEV, with_iters=False, layout=layout)
    _prefill(db)
    whole = (db.x, db.f, db.status)
    per_qp = {"G": n * n, "g0": n, "CE": n * p, "ce0": p, "CI": n * m, "ci0": m, "x": n, "f": 1, "status": 1}
    for name, E in per_qp.items():  # (TILED64: QP 64 is the start of a tile)
        setattr(db, name, getattr(db, name).reshape(-1)[b0 * E:])
    db.batch = BMAX
    db.solve()
    torch.cuda.synchronize()
    db.x, db.f, db.status = whole
    db.batch = total
    x, f, st, _ = db.results()
    x = x.reshape(total, n)
    sl = slice(b0, b0 + BMAX)
    assert_bits((x[sl], f[sl], st[sl]), oracle_ref(*shape), f"{shape} QPs [64, 255) {layout}")
    out = np.r_[0:b0, b0 + BMAX:total]
    assert np.isnan(x[out]).all() and np.isnan(f[out]).all() and (st[out] == -7).all()


def test_fast_build_against_the_exact_build(gpu):
    """QPGPU_FLAG_FAST at (7, 6, 14), B = 65: the same statuses, x within 1e-10 relative and f within
    1e-10 of its terms (the fast build's bar, tests/test_gpu_parity.py) of the exact build's output
    of the same batch, which is the oracle's bit for bit."""
    shape = (7, 6, 14)
    pr = problems(*shape).slice(0, 65)
    for layout in LAYOUTS:
        xe, fe, se = gpu_solve(pr, layout)
        assert_bits((xe, fe, se), tuple(a[:65] for a in oracle_ref(*shape)), f"exact {layout}")
        assert qpgpu.kernel_name(*shape, fast=True).startswith("qp_lane_fast<")
        xf, ff, sf = gpu_solve(pr, layout, fast=True)
        assert np.array_equal(sf, se), f"fast {layout}: status differs at {np.where(sf != se)[0][:8]}"
        ok = se == qpgpu.QP_OK
        sub = qpgpu.Problems(*shape, *[a[ok] for a in pr.arrays()])
        ex, efp, eft = parity._relerr(xf[ok], xe[ok], ff[ok], fe[ok], np.ones(int(ok.sum()), dtype=bool), sub)
        print(f"fast {layout}: rel err x {ex:.3e}, f vs its terms {eft:.3e} (plain {efp:.3e})")
        assert ex <= parity.TOL and eft <= parity.TOL, (layout, ex, eft)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_unit_entry(gpu, layout):
    """qpgpu_solve_batched_unit at (7, 6, 14), B = 65, against the oracle on the dense problem with
    G = I materialised (what the entry is defined as)."""
    import torch

    n, p, m = 7, 6, 14
    up = qpgpu.make_unit_problems(n, p, m, 0, 65, seed=SEED + 2)
    assert qpgpu.kernel_name_unit(n, p, m).startswith("qp_lane_unit<")
    xo, fo, so, _ = oracle.solve_batch(up.to_dense(), max_steps=_cap(n, p, m))
    assert (so == qpgpu.QP_OK).all()
    db = qpgpu.DeviceUnitBatch(up, DEV, with_iters=False, layout=layout)
    _prefill(db)
    db.solve()
    torch.cuda.synchronize()
    x, f, st, _ = db.results()
    assert_bits((x.reshape(65, n), f, st), (xo.reshape(65, n), fo, so), f"unit {layout}")
