"""The one-free-dimension loop of the lane kernel (qp_lane.hip: lane_body's kOneFree, the select and
step of qp_lane_full_kernel<7, 14, T, 6>): with n - p = 1 the active set holds at most one inequality, and
the full-wave kernel of the shape (7, 6, 14) runs a two-state machine (slot empty / slot taken)
instead of the general select and step.

Every case is compared to the CPU oracle bit for bit on x, f and status, in both layouts, with
every array inside one arena between guard bands (tests/placement.py).  The batches 64, 65, 128
and 191 run the new loop on the whole 64-QP blocks and the unchanged general kernel on the
remaining QPs in the same call (qpgpu_debug_lane_launches says which kernels were enqueued), and
the same 191 QPs placed 8 bytes off a 16-byte boundary go to the general kernels altogether: both
calls must return identical bytes, which pins the new loop against the old one independently of
the oracle.

Lanes of the first wave hold QPs built to take every branch of the machine (the others are
ordinary qp_cases.make("general", ...) QPs); test_the_special_lanes_do_what_they_are_there_for
checks against the oracle that each one does what it is there for:

  NOTPD      indefinite G (x unwritten)
  PAIR       a contradictory pair of inequalities: infeasible with the slot taken (r <= 0)
  OPTIMAL    no inequality violated: optimal at the first scan
  ONE_ADD    one violated inequality, every other slack large: one add, optimal at the second scan
  DUP        duplicated / zero inequality columns (qp_cases "dup_zero_cols")
  LONG..     g0 scaled by 30 as in qp_cases "long_paths": add -> violated -> dual drop -> add chains
  TIES       small-integer data (qp_cases "integer_ties"): exact ties in the selection
  SPAN       the one violated inequality column lies in span(CE): z = J[:,6] d[6] vanishes to
             rounding, zz <= eps, infeasible with the slot empty
  DEPENDENT  CE's last column repeats its first: status DEPENDENT out of the equality phase
  ROLLBACK   the degenerate add: G = I, CE = 1e9 [e0 .. e5] (so J = +-I and R_norm = 1e9), one
             violated CI column whose e6 component is 1e-7 (zz = 1e-14 > eps, yet |d[6]| = 1e-7 <=
             eps R_norm = 2.2e-7: the add fails after the full step and x is rolled back), and a
             second, less violated column.  The re-select keeps the stale ss and with it the same
             ip, so the QP repeats the failing step until the step cap: status MAX_ITER.  (That this
             QP takes the rollback was confirmed once with a throw-away instrumented build of the
             oracle, which is not part of the repository.)

max_steps = 1 and 2 reach the kernel through the entry's max_iter argument."""
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
SHAPE = (7, 6, 14)
BATCHES = (64, 65, 128, 191)
BMAX = max(BATCHES)
# all inside the first wave, beside ordinary QPs
NOTPD, PAIR, OPTIMAL, ONE_ADD, DUP, TIES, SPAN, DEPENDENT, ROLLBACK = 1, 2, 3, 4, 5, 9, 10, 11, 12
LONG = (6, 7, 8, 13, 14, 15, 16, 17)
BIG = 1.0e3  # a slack no step of these QPs uses up


def _cap(pr):
    return 1000 + 100 * (pr.n + pr.p + pr.m)


@functools.lru_cache(maxsize=None)
def problems():
    """BMAX QPs; every batch size solves the first B of them.  Shared: left unchanged."""
    n, p, m = SHAPE
    pr = qp_cases.make("general", n, p, m, BMAX, seed=4206)
    for lane, mode in ((DUP, "dup_zero_cols"), (TIES, "integer_ties")):
        q = qp_cases._fuzz_qp(np.random.default_rng([95, p, lane]), n, p, m, mode, False)
        for dst, src in zip(pr.arrays(), q):
            dst[lane] = src
    pr.G[NOTPD, n // 2, n // 2] = -1.0
    pr.CI[PAIR, :, 1] = -pr.CI[PAIR, :, 0]
    pr.ci0[PAIR, 1] = -pr.ci0[PAIR, 0] - 0.5
    # the equality-constrained minimiser of a lane, to place slacks around it
    xeq = lambda b: _x_eq(pr.G[b], pr.g0[b], pr.CE[b], pr.ce0[b])
    for b in (OPTIMAL, ONE_ADD):
        pr.ci0[b] = -pr.CI[b].T @ xeq(b) + BIG
    pr.ci0[ONE_ADD, 4] -= BIG + 0.25  # s[4] = -0.25 at the equality-phase x
    for b in LONG:
        pr.g0[b] *= 30.0
    # SPAN: column 0 of CI = 2 CE[:, 0], so s[0] = -2 ce0[0] + ci0[0] on the equality manifold
    pr.ci0[SPAN] = -pr.CI[SPAN].T @ xeq(SPAN) + BIG
    pr.CI[SPAN, :, 0] = 2.0 * pr.CE[SPAN, :, 0]
    pr.ci0[SPAN, 0] = 2.0 * pr.ce0[SPAN, 0] - 1.0
    pr.CE[DEPENDENT, :, p - 1] = pr.CE[DEPENDENT, :, 0]
    # ROLLBACK (see the module's text)
    pr.G[ROLLBACK] = np.eye(n)
    pr.g0[ROLLBACK] = 0.0
    pr.CE[ROLLBACK] = 1.0e9 * np.eye(n)[:, :p]
    pr.ce0[ROLLBACK] = 0.0
    pr.CI[ROLLBACK] = 0.0
    pr.ci0[ROLLBACK] = BIG
    pr.CI[ROLLBACK, :, 3] = [0.5, -0.25, 0.0, 1.0, 0.0, 0.0, 1.0e-7]
    pr.ci0[ROLLBACK, 3] = -1.0
    pr.CI[ROLLBACK, n - 1, 8] = 1.0
    pr.ci0[ROLLBACK, 8] = -0.5
    return pr


def _x_eq(G, g0, CE, ce0):
    """argmin 1/2 x'Gx + g0'x  s.t.  CE'x + ce0 = 0 (float64 KKT solve; only places test data)."""
    n, p = CE.shape
    K = np.block([[G, CE], [CE.T, np.zeros((p, p))]])
    return np.linalg.solve(K, np.concatenate([-g0, -ce0]))[:n]


@functools.lru_cache(maxsize=None)
def oracle_ref(max_steps=0):
    """(x, f, status, iters) of the oracle on all BMAX QPs, once per step cap (0: the entry's
    default).  QPs are independent: the first B rows are the reference of every batch size."""
    pr = problems()
    prc = qpgpu.Problems(pr.n, pr.p, pr.m, *[np.array(a) for a in pr.arrays()])
    return tuple(oracle.solve_batch(prc, max_steps=max_steps or _cap(prc)))


def lane_launches(reset=True):
    fn = qpgpu.LIB.qpgpu_debug_lane_launches
    fn.argtypes = [ctypes.POINTER(ctypes.c_int64), ctypes.c_int]
    fn.restype = None
    out = (ctypes.c_int64 * 2)()
    fn(out, 1 if reset else 0)
    return out[0], out[1]


def solve(B, layout, pl, max_steps=0):
    """One solve of the first B QPs inside an arena, without a pass count (the full-wave kernels
    take only such calls).  Returns (arena, launches since the reset)."""
    import torch

    pr = problems().slice(0, B)
    specs = [s for s in placement.entry_specs(pr, layout) if s.name != "iters"]
    ar = placement.Arena(specs, pl, DEV)
    db = qpgpu.DeviceBatch(pr, DEV, with_iters=False, layout=layout)
    placement.attach(ar, db)
    for name, s in ar.specs.items():  # the call really gets the arena's addresses
        assert getattr(db, name).data_ptr() == ar.address(name)
        assert ar.address(name) % 16 == placement.residue(pl, name, s.dtype)
    lane_launches(reset=True)
    db.solve(max_iter=max_steps)
    torch.cuda.synchronize()
    return ar, lane_launches(reset=True)


def outputs(ar, B, layout):
    """(x (B, n), f, status) of an arena after a solve."""
    n = SHAPE[0]
    now = ar.download()
    x = ar.values("x", now)
    x = qpgpu.from_tiled64(x, B, (n,)) if layout == "tiled64" else x.reshape(B, n)
    return x, ar.values("f", now), ar.values("status", now)


def check(ar, B, layout, label, max_steps=0):
    """The arena is clean and every output is the oracle's, bit for bit."""
    n = SHAPE[0]
    xo, fo, so, _ = (np.asarray(a)[:B] for a in oracle_ref(max_steps))
    notpd = so == qpgpu.QP_NOT_POSITIVE_DEFINITE
    assert ar.check(placement.written_masks(ar, layout, B, x_skip=notpd)) == [], label
    x, f, st = outputs(ar, B, layout)
    assert np.array_equal(st, so), f"{label}: status differs at {np.where(st != so)[0][:10]}"
    assert np.array_equal(f.view(np.uint64), fo.view(np.uint64)), \
        f"{label}: f differs at {np.where(f.view(np.uint64) != fo.view(np.uint64))[0][:10]}"
    ok = ~notpd
    bad = np.where((x[ok].view(np.uint64) != xo.reshape(B, n)[ok].view(np.uint64)).any(axis=1))[0]
    assert bad.size == 0, f"{label}: x differs at (ok-)QPs {bad[:10]}"


def test_the_special_lanes_do_what_they_are_there_for():
    """The oracle's view of the special lanes (no GPU work): each one ends where it was built to."""
    pr = problems()
    _, _, st, it = oracle_ref()
    assert st[NOTPD] == qpgpu.QP_NOT_POSITIVE_DEFINITE
    assert st[PAIR] == qpgpu.QP_INFEASIBLE and it[PAIR] >= 2      # met with the slot taken
    assert st[OPTIMAL] == qpgpu.QP_OK and it[OPTIMAL] == 1
    assert st[ONE_ADD] == qpgpu.QP_OK and it[ONE_ADD] == 2
    assert st[SPAN] == qpgpu.QP_INFEASIBLE and it[SPAN] == 1      # at the first step, slot empty
    assert st[DEPENDENT] == qpgpu.QP_DEPENDENT
    assert st[ROLLBACK] == qpgpu.QP_MAX_ITER and it[ROLLBACK] == 1  # one scan, then re-selects only
    assert it[DUP] >= 1 and it[TIES] >= 1
    assert np.array_equal(pr.G[TIES], np.diag(np.diag(pr.G[TIES])))
    # swap chains: a QP with k passes added k - 1 times and dropped in between
    assert max(it[b] for b in LONG) >= 5 and all(st[b] == qpgpu.QP_OK for b in LONG), [it[b] for b in LONG]
    # the step caps cut QPs short in both states of the machine
    for cap in (1, 2):
        stc = oracle_ref(cap)[2]
        assert (stc[:64] == qpgpu.QP_MAX_ITER).sum() >= 8 and (stc[:64] == qpgpu.QP_OK).sum() >= 2, cap
    assert (oracle_ref(1)[2] != oracle_ref(2)[2]).any()


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("B", BATCHES)
def test_whole_blocks_run_the_onefree_loop_and_match_the_oracle(gpu, B, layout):
    assert qpgpu.LIB.qpgpu_kernel_name_flags(*SHAPE, 0).decode() == "qp_lane<N=7,M=14>"
    ar, (nfull, nrest) = solve(B, layout, "aligned")
    assert (nfull, nrest) == (1, 1 if B % 64 else 0), (B, nfull, nrest)
    check(ar, B, layout, f"B={B} {layout} aligned")


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("cap", (1, 2))
def test_step_cap_through_the_entry(gpu, cap, layout):
    ar, launches = solve(BMAX, layout, "aligned", max_steps=cap)
    assert launches == (1, 1), launches
    check(ar, BMAX, layout, f"max_steps={cap} {layout}", max_steps=cap)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_new_loop_and_general_loop_return_identical_bytes(gpu, layout):
    """The 191 QPs through the full-wave kernel (+ remainder) and, with every array 8 bytes off a
    16-byte boundary, through the general kernels alone."""
    new, launches = solve(BMAX, layout, "aligned")
    assert launches == (1, 1), launches
    old, launches = solve(BMAX, layout, "odd")
    assert launches == (0, 0), launches
    check(old, BMAX, layout, f"{layout} odd")
    for name in ("x", "f", "status"):
        assert np.array_equal(new.bits(name), old.bits(name)), f"{layout}: {name} differs between the loops"
