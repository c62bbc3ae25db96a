"""The definition of the multipliers qpgpu_solve_batched_dual returns, checked on the CPU.

tests/dual_ref.py builds the restatement with an export hook at `done:`.  Here: (i) the hook
changes nothing — x, f, status and iters of the variant are the unmodified oracle's, bit for bit,
on every case the dual tests use; (ii) on the well-posed list of DESIGN §3.5 the exported u is a
Lagrange multiplier vector in the header's sign convention: stationarity, complementarity,
non-negativity, and nact = the number of non-zero inequality multipliers.

The thresholds are properties of the definition, not of any code under test: 1e-12 and 1e-10 sit
three to four orders above what binary64 rounding leaves on these problems (measured maxima:
7.9e-16 and 3.9e-14) and twelve below what a sign or index error produces (O(1)).
"""
import numpy as np
import pytest

import dual_ref
import oracle
import qpgpu

STATIONARITY_MAX = 1e-12
COMPLEMENTARITY_MAX = 1e-10

ALL_IDS = sorted(set(dual_ref.gpu_cases()) | set(dual_ref.fuzz_cases()) | set(dual_ref.kkt_cases()))


def _same_bits(a, b):
    a = np.ascontiguousarray(a, dtype=np.float64).ravel()
    b = np.ascontiguousarray(b, dtype=np.float64).ravel()
    return bool(np.all((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))))


@pytest.mark.parametrize("cid", ALL_IDS)
def test_hook_changes_nothing(cid):
    pr = dual_ref.case(cid)
    x, f, st, it, u, nact = dual_ref.reference(cid)
    xo, fo, so, io = oracle.solve_batch(pr, max_steps=dual_ref.default_cap(pr.n, pr.p, pr.m))
    assert np.array_equal(st, so) and np.array_equal(it, io)
    assert _same_bits(x, xo) and _same_bits(f, fo)
    # every slot written, inactive ones and non-OK QPs exactly +0.0
    assert u.shape == (pr.batch, pr.p + pr.m) and not np.any(nact == -7)
    bad = st != qpgpu.QP_OK
    assert not np.any(u[bad].view(np.uint64)) and not np.any(nact[bad])


def test_hook_under_a_step_cap():
    cid = "edge_long_paths"
    pr = dual_ref.case(cid)
    x, f, st, it, u, nact = dual_ref.reference(cid, 1)
    xo, fo, so, io = oracle.solve_batch(pr, max_steps=1)
    assert np.array_equal(st, so) and np.array_equal(it, io) and _same_bits(x, xo) and _same_bits(f, fo)
    capped = st == qpgpu.QP_MAX_ITER
    assert capped.any() and not np.any(u[capped].view(np.uint64)) and not np.any(nact[capped])


@pytest.mark.parametrize("cid", sorted(dual_ref.kkt_cases()))
def test_kkt_on_well_posed(cid):
    pr = dual_ref.case(cid)
    x, f, st, it, u, nact = dual_ref.reference(cid)
    stat, comp, umin, cnt = dual_ref.kkt_measures(pr, x, st, u)
    print(f"{cid}: {cnt} QPs, stationarity {stat:.3e}, complementarity {comp:.3e}, min u[p:] {umin!r}")
    assert stat <= STATIONARITY_MAX, f"{cid}: scaled stationarity residual {stat:.3e}"
    assert comp <= COMPLEMENTARITY_MAX, f"{cid}: complementarity residual {comp:.3e}"
    ui = u[:, pr.p:]
    assert not np.any(ui < 0), f"{cid}: negative inequality multiplier {ui.min()!r}"
    assert np.array_equal(np.count_nonzero(ui, axis=1), nact), f"{cid}: nact != count_nonzero(u[p:])"
    bad = st != qpgpu.QP_OK
    assert not np.any(u[bad].view(np.uint64)), f"{cid}: non-zero u on a non-OK status"


def test_kkt_maxima_over_the_list():
    """The figures DESIGN §3.5 records (run with -s to see them)."""
    stat = comp = 0.0
    total = 0
    for cid in sorted(dual_ref.kkt_cases()):
        pr = dual_ref.case(cid)
        x, f, st, it, u, nact = dual_ref.reference(cid)
        s, c, _, cnt = dual_ref.kkt_measures(pr, x, st, u)
        stat, comp, total = max(stat, s), max(comp, c), total + cnt
    print(f"KKT over {total} status-OK QPs: max stationarity {stat:.3e}, max complementarity {comp:.3e}")
    assert total > 0 and stat <= STATIONARITY_MAX and comp <= COMPLEMENTARITY_MAX
