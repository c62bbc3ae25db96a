"""The resident CI rows of the QP-major one-free lane kernel (qp_lane.hip: lane_body's kResident,
lane_scan_kept; qp_lane_full_kernel<7, 14, 1, 6>).  Rows 5-6 of CI stay in VGPRs and ci0 in AGPRs
from the first l1 scan, which is peeled out of the loop, to the end of the solve: later scans issue
no global load, and the select picks np[5], np[6] out of the kept rows under its own `take`.

Every case is compared bit for bit on x, f and status against the CPU oracle, and against the same
QPs solved 8 bytes off a 16-byte boundary, which sends them to the unchanged general kernels.
QP-major only (the TILED64 kernel is not touched), batches 64, 128 and 191, every array in one
arena between guard bands (tests/placement.py); qpgpu_debug_lane_launches says that the full-wave
kernel ran the whole blocks.  The generators and the one-free test's special lanes are imported
from tests/test_gpu_lane_onefree.py and tests/qp_cases.py.

Two sets of 191 QPs, three 64-QP blocks each (the third is 63 QPs, the general kernel's):

  "special", block 0: the one-free test's lanes (ROLLBACK: the most violated column is excluded
      after a rollback and the re-select must keep ip and np; LONG: add -> violated -> dual drop
      -> re-add of the pending ip, np surviving a pass without a select) and, beside them,
        COL0..COL13  the only violated inequality is column i: ip = i, np[5], np[6] from position i
        DESC         s strictly descending over columns 0..13 at the first scan: `take` fires 14 times
        ASC          the same QP with s ascending: only `take` 0 fires
        BLOCKED      at the second scan the most violated column is the one in the slot (its column
                     scaled by 1e10, so that its rounding residue is below the -1e-7 of the one
                     other violated column): the select must pass over it
        BITS         -0.0 and a subnormal in rows 5 and 6 of the selected column, -0.0 and
                     subnormals in ci0 (the oracle sees the same bits; a flushed or re-signed copy
                     shows wherever the result depends on it)
  "special", block 1: 64 QPs that never scan (DEPENDENT and not positive definite, alternating): the
      peeled scan is skipped by the whole wave.
  "sparse", block 0: 63 such QPs and one ordinary QP in lane 37.
  "sparse", block 1: QPs that finish at passes 1, 2, 3, 4 and 5, interleaved.

test_the_cases_take_the_paths_they_are_built_for confirms the construction on the CPU, from the
oracle's pass counts and from s = CI^T x + ci0 evaluated in the kernel's order."""
import functools

import numpy as np
import pytest

import oracle
import placement
import qp_cases
import qpgpu
import test_gpu_lane_onefree as onefree

DEV = "cuda:0"
LAYOUT = "qp_major"
SHAPE = onefree.SHAPE
BATCHES = (64, 128, 191)
BMAX = max(BATCHES)
BIG = onefree.BIG
COL0 = 18                      # lanes COL0 .. COL0 + 13
DESC, ASC, BLOCKED, BITS = 32, 33, 34, 35
ORDINARY = 37                  # the one ordinary QP of the sparse set's block 0
SUB = 5e-324                   # the smallest subnormal


def _cap(pr):
    return 1000 + 100 * (pr.n + pr.p + pr.m)


def _oracle(pr, max_steps=0):
    prc = qpgpu.Problems(pr.n, pr.p, pr.m, *[np.array(a) for a in pr.arrays()])
    return tuple(oracle.solve_batch(prc, max_steps=max_steps or _cap(prc)))


def scan_s(CI, ci0, x):
    """s = CI^T x + ci0 as the kernel and the oracle sum it: j ascending from 0.0, then + ci0[i]."""
    n, m = CI.shape
    out = []
    for i in range(m):
        s = 0.0
        for j in range(n):
            s += float(CI[j, i]) * float(x[j])
        out.append(s + float(ci0[i]))
    return np.array(out)


def _never_scan_block(pr, lanes):
    """Make the QPs `lanes` end before the loop: DEPENDENT (CE's last column repeats its first) and
    not positive definite, alternating.  Whether the repeated column is caught is a matter of
    rounding, so a QP the oracle does not call DEPENDENT becomes a not positive definite one."""
    lanes = list(lanes)
    ce = pr.CE.copy()
    for b in lanes[0::2]:
        pr.CE[b, :, pr.p - 1] = pr.CE[b, :, 0]
    for b in lanes[1::2]:
        pr.G[b, pr.n // 2, pr.n // 2] = -1.0
    st = _oracle(pr)[2]
    for b in lanes[0::2]:
        if st[b] != qpgpu.QP_DEPENDENT:
            pr.CE[b] = ce[b]
            pr.G[b, pr.n // 2, pr.n // 2] = -1.0


def _one_violated(pr, b, col, by=0.25):
    xeq = onefree._x_eq(pr.G[b], pr.g0[b], pr.CE[b], pr.ce0[b])
    pr.ci0[b] = -pr.CI[b].T @ xeq + BIG
    pr.ci0[b, col] -= BIG + by
    return xeq


def _blocked_qp(n, p, m):
    """A QP whose second scan finds the slot's column the most violated one (see the module's
    text): candidates are drawn until the rounding residue of the scaled column has the sign and
    the size that are needed.  Returns its six arrays and the column in the slot."""
    col, other = 9, 3
    cand = qp_cases.make("general", n, p, m, 64, seed=7711)
    for b in range(cand.batch):
        _one_violated(cand, b, col)
        cand.CI[b, :, col] *= 1.0e10
        cand.ci0[b, col] *= 1.0e10
    x2, _, st, it = _oracle(cand)  # one add, optimal at the second scan: x2 is that scan's x
    for b in range(cand.batch):
        if st[b] != qpgpu.QP_OK or it[b] != 2:
            continue
        ci0 = cand.ci0[b].copy()
        ci0[other] = -float(cand.CI[b, :, other] @ x2[b]) - 1.0e-7
        s = scan_s(cand.CI[b], ci0, x2[b])
        rest = np.delete(s, [col, other])
        if s[col] < 2.0 * s[other] < 0.0 and s[other] < -0.5e-7 and (rest > 1.0).all():
            q = [a[b].copy() for a in cand.arrays()]
            q[5] = ci0
            return q, col, other, x2[b].copy()
    raise AssertionError("no candidate with a negative residue in the slot's column")


@functools.lru_cache(maxsize=None)
def problems(which):
    """The 191 QPs of a set; every batch size solves the first B of them.  Shared: left unchanged."""
    n, p, m = SHAPE
    if which == "special":
        src = onefree.problems()
        pr = qpgpu.Problems(n, p, m, *[np.array(a) for a in src.arrays()])
        for i in range(m):
            _one_violated(pr, COL0 + i, i)
        for b, sign in ((DESC, 1.0), (ASC, -1.0)):
            for dst, s in zip(pr.arrays(), pr.slice(DESC, DESC + 1).arrays()):
                dst[b] = s[0]
            xeq = onefree._x_eq(pr.G[b], pr.g0[b], pr.CE[b], pr.ce0[b])
            ramp = np.arange(1, m + 1) if sign > 0 else np.arange(m, 0, -1)
            pr.ci0[b] = -pr.CI[b].T @ xeq - 0.1 * ramp
        q, _, _, _ = _blocked_qp(n, p, m)
        for dst, s in zip(pr.arrays(), q):
            dst[BLOCKED] = s
        # BITS: column 6 is the one violated; its rows 5 and 6, and three entries of ci0
        pr.CI[BITS, 5, 6] = -0.0
        pr.CI[BITS, 6, 6] = SUB
        pr.CI[BITS, :, 2] = 0.0
        pr.CI[BITS, :, 11] = 0.0
        pr.CI[BITS, 5, 12] = -SUB
        pr.CI[BITS, 6, 12] = -0.0
        _one_violated(pr, BITS, 6)
        pr.ci0[BITS, 2] = -0.0   # s[2] = +0.0 + -0.0
        pr.ci0[BITS, 11] = SUB   # s[11] = the subnormal itself
        _never_scan_block(pr, range(64, 128))
        return pr
    assert which == "sparse"
    pr = qp_cases.make("general", n, p, m, BMAX, seed=5150)
    _never_scan_block(pr, [b for b in range(64) if b != ORDINARY])
    pr.g0[ORDINARY] *= 100.0  # (several passes, as the LONG lanes)
    # block 1: by pass count, out of a pool (most of it with g0 scaled by 100: longer chains, as
    # the LONG lanes'; a QP of 5 passes is about one in 500 there)
    pool = qp_cases.make("general", n, p, m, 2560, seed=5151)
    pool.g0[512:] *= 100.0
    _, _, st, it = _oracle(pool)
    by_passes = {k: [b for b in range(pool.batch) if st[b] == qpgpu.QP_OK and it[b] == k] for k in range(1, 6)}
    for lane in range(64):
        want = by_passes[lane % 5 + 1]
        b = want[(lane // 5) % len(want)]
        for dst, s in zip(pr.arrays(), pool.arrays()):
            dst[64 + lane] = s[b]
    return pr


@functools.lru_cache(maxsize=None)
def oracle_ref(which, max_steps=0):
    """(x, f, status, iters) of the oracle on a set's 191 QPs, once per step cap."""
    return _oracle(problems(which), max_steps)


def solve(which, B, pl, max_steps=0):
    """One QP-major solve of the first B QPs of a set inside an arena, without a pass count (the
    full-wave kernels take only such calls).  Returns (arena, launches since the reset)."""
    import torch

    pr = problems(which).slice(0, B)
    specs = [s for s in placement.entry_specs(pr, LAYOUT) if s.name != "iters"]
    ar = placement.Arena(specs, pl, DEV)
    db = qpgpu.DeviceBatch(pr, DEV, with_iters=False, layout=LAYOUT)
    placement.attach(ar, db)
    for name, s in ar.specs.items():  # the call really gets the arena's addresses
        assert getattr(db, name).data_ptr() == ar.address(name)
        assert ar.address(name) % 16 == placement.residue(pl, name, s.dtype)
    onefree.lane_launches(reset=True)
    db.solve(max_iter=max_steps)
    torch.cuda.synchronize()
    return ar, onefree.lane_launches(reset=True)


def check(ar, which, B, label, max_steps=0):
    """The arena is clean and every output is the oracle's, bit for bit."""
    n = SHAPE[0]
    xo, fo, so, _ = (np.asarray(a)[:B] for a in oracle_ref(which, max_steps))
    notpd = so == qpgpu.QP_NOT_POSITIVE_DEFINITE
    assert ar.check(placement.written_masks(ar, LAYOUT, B, x_skip=notpd)) == [], label
    now = ar.download()
    x, f, st = ar.values("x", now).reshape(B, n), ar.values("f", now), ar.values("status", now)
    assert np.array_equal(st, so), f"{label}: status differs at {np.where(st != so)[0][:10]}"
    assert np.array_equal(f.view(np.uint64), fo.view(np.uint64)), \
        f"{label}: f differs at {np.where(f.view(np.uint64) != fo.view(np.uint64))[0][:10]}"
    ok = ~notpd
    bad = np.where((x[ok].view(np.uint64) != xo.reshape(B, n)[ok].view(np.uint64)).any(axis=1))[0]
    assert bad.size == 0, f"{label}: x differs at (ok-)QPs {bad[:10]}"


def test_the_cases_take_the_paths_they_are_built_for():
    """No GPU work: the oracle's pass counts and the scans' s say that each case is what it is for."""
    n, p, m = SHAPE
    pr = problems("special")
    x, _, st, it = oracle_ref("special")
    x = np.asarray(x).reshape(BMAX, n)
    xeq = lambda b: onefree._x_eq(pr.G[b], pr.g0[b], pr.CE[b], pr.ce0[b])
    # every column selected once: one violated column at the first scan, one add, optimal at the second
    for i in range(m):
        b = COL0 + i
        s = scan_s(pr.CI[b], pr.ci0[b], xeq(b))
        assert s.argmin() == i and s[i] < -0.2 and (np.delete(s, i) > 1.0).all(), (i, s)
        assert st[b] == qpgpu.QP_OK and it[b] == 2, (i, st[b], it[b])
    # the chains: 14 takes and 1 take at the first select (the gaps of 0.1 are far above rounding)
    sd, sa = scan_s(pr.CI[DESC], pr.ci0[DESC], xeq(DESC)), scan_s(pr.CI[ASC], pr.ci0[ASC], xeq(ASC))
    assert sd[0] < -0.05 and (np.diff(sd) < -0.05).all(), sd
    assert sa[0] < -1.0 and (np.diff(sa) > 0.05).all() and sa[-1] < -0.05, sa
    assert it[DESC] >= 2 and it[ASC] >= 2
    for a, b in zip(pr.slice(DESC, DESC + 1).arrays()[:5], pr.slice(ASC, ASC + 1).arrays()[:5]):
        assert np.array_equal(a, b)  # the same QP but for ci0
    # the blocked minimum: the slot's column is the most violated one at the second scan, one other
    # column is violated, and the solve goes on past that scan (its select ran)
    q, col, other, x2 = _blocked_qp(n, p, m)
    for a, b in zip(pr.slice(BLOCKED, BLOCKED + 1).arrays(), q):
        assert np.array_equal(a[0], b)
    s1 = scan_s(q[4], q[5], onefree._x_eq(q[0], q[1], q[2], q[3]))
    assert s1.argmin() == col and s1[col] < 1.0e3 * s1[other], s1  # the first pass adds `col`
    s2 = scan_s(q[4], q[5], x2)
    assert s2.argmin() == col and s2[col] < s2[other] < 0.0 and (np.delete(s2, [col, other]) > 0).all(), s2
    assert it[BLOCKED] >= 3, it[BLOCKED]
    # the excluded minimum, the passes without a select: the one-free test's lanes, unchanged
    for a, b in zip(pr.slice(0, COL0).arrays(), onefree.problems().slice(0, COL0).arrays()):
        assert np.array_equal(a, b)
    assert st[onefree.ROLLBACK] == qpgpu.QP_MAX_ITER and it[onefree.ROLLBACK] == 1
    assert max(it[b] for b in onefree.LONG) >= 5 and all(st[b] == qpgpu.QP_OK for b in onefree.LONG)
    # the bit patterns are in the arrays the kernel gets, in the column it selects
    assert it[BITS] == 2 and st[BITS] == qpgpu.QP_OK
    assert scan_s(pr.CI[BITS], pr.ci0[BITS], xeq(BITS)).argmin() == 6
    bits = lambda v: np.float64(v).view(np.uint64)
    assert bits(pr.CI[BITS, 5, 6]) == bits(-0.0) and bits(pr.CI[BITS, 6, 6]) == 1
    assert bits(pr.ci0[BITS, 2]) == bits(-0.0) and bits(pr.ci0[BITS, 11]) == 1
    # lanes that never scan
    never = (qpgpu.QP_DEPENDENT, qpgpu.QP_NOT_POSITIVE_DEFINITE)
    assert all(s in never for s in st[64:128]) and (it[64:128] == 0).all()
    assert (st[64:128] == qpgpu.QP_DEPENDENT).sum() >= 16 and (st[64:128] == never[1]).sum() >= 16
    _, _, st2, it2 = oracle_ref("sparse")
    rest = np.delete(np.arange(64), ORDINARY)
    assert all(s in never for s in st2[rest]) and (it2[rest] == 0).all()
    assert st2[ORDINARY] == qpgpu.QP_OK and it2[ORDINARY] >= 2
    # a block whose lanes finish at passes 1 through 5
    assert (st2[64:128] == qpgpu.QP_OK).all()
    for k in range(1, 6):
        assert (it2[64:128] == k).sum() >= 8, (k, np.bincount(it2[64:128]))
    # the step caps cut QPs short in both states of the machine
    for cap in (1, 2):
        stc = oracle_ref("special", cap)[2]
        assert (stc[:64] == qpgpu.QP_MAX_ITER).sum() >= 8 and (stc[:64] == qpgpu.QP_OK).sum() >= 2, cap
    assert (oracle_ref("special", 1)[2] != oracle_ref("special", 2)[2]).any()


@pytest.mark.gpu
@pytest.mark.parametrize("which", ("special", "sparse"))
@pytest.mark.parametrize("B", BATCHES)
def test_whole_blocks_run_the_resident_kernel_and_match_the_oracle(gpu, B, which):
    assert qpgpu.LIB.qpgpu_kernel_name_flags(*SHAPE, 0).decode() == "qp_lane<N=7,M=14>"
    ar, (nfull, nrest) = solve(which, B, "aligned")
    assert (nfull, nrest) == (1, 1 if B % 64 else 0), (B, nfull, nrest)
    check(ar, which, B, f"{which} B={B} aligned")


@pytest.mark.gpu
@pytest.mark.parametrize("cap", (1, 2))
def test_step_cap_through_the_entry(gpu, cap):
    ar, launches = solve("special", BMAX, "aligned", max_steps=cap)
    assert launches == (1, 1), launches
    check(ar, "special", BMAX, f"max_steps={cap}", max_steps=cap)


@pytest.mark.gpu
@pytest.mark.parametrize("which", ("special", "sparse"))
def test_resident_and_general_kernels_return_identical_bytes(gpu, which):
    """The 191 QPs through the full-wave kernel (+ remainder) and, with every array 8 bytes off a
    16-byte boundary, through the general kernels alone."""
    new, launches = solve(which, BMAX, "aligned")
    assert launches == (1, 1), launches
    old, launches = solve(which, BMAX, "odd")
    assert launches == (0, 0), launches
    check(old, which, BMAX, f"{which} odd")
    for name in ("x", "f", "status"):
        assert np.array_equal(new.bits(name), old.bits(name)), f"{which}: {name} differs between the kernels"
