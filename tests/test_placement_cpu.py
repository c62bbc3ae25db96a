"""The arena helper of tests/placement.py on CPU tensors: a helper that placed nothing where it
says, or a checker that reported nothing, would make tests/test_gpu_placement.py vacuous.  Also the
host side of the alignment contract (include/qpgpu.h): which 16-byte paths the solve entries
license from the addresses they are given (qpgpu_api.cpp alignment_flags, through its test hook)."""
import ctypes

import numpy as np
import pytest

import placement
import qp_cases
import qpgpu

ARRAYS = ("G", "g0", "CE", "ce0", "CI", "ci0", "x", "u")
ALL_PLACEMENTS = placement.PLACEMENTS + tuple(f"only:{a}" for a in ARRAYS) + ("only:hi", "only:lo")


def _arena(pl, layout="qp_major", entry="dual", B=70, box=False):
    if box:
        pr = qpgpu.make_box_problems(5, 2, 0, B, seed=3)
    else:
        pr = qp_cases.make("general", 5, 2, 9, B)
    return pr, placement.Arena(placement.entry_specs(pr, layout, entry), pl, "cpu")


def _fake_solve(ar, masks, value=1.0):
    """Write every element the call must write (and nothing else), as a correct kernel does."""
    for name, w in masks.items():
        v = ar.view(name).numpy()  # shares the arena's memory
        v[np.asarray(w)] = value if v.dtype == np.float64 else 3


@pytest.mark.parametrize("box", [False, True])
@pytest.mark.parametrize("layout", ["qp_major", "tiled64"])
@pytest.mark.parametrize("pl", ALL_PLACEMENTS)
def test_residues_guards_and_no_overlap(pl, layout, box):
    _, ar = _arena(pl, layout, box=box)
    specs = sorted(ar.specs.values(), key=lambda s: s.start)
    names = {s.name for s in specs}
    assert {"x", "f", "status", "iters", "u", "nact", "G", "g0", "CE", "ce0"} <= names
    assert ({"hi", "lo"} if box else {"CI", "ci0"}) <= names
    prev_end = 0
    for s in specs:
        want = placement.residue(pl, s.name, s.dtype)
        assert ar.address(s.name) % 16 == want, (s.name, ar.address(s.name) % 16, want)
        assert ar.view(s.name).data_ptr() == ar.address(s.name)
        assert ar.view(s.name).numel() == s.count
        g = placement.guard_elems(s.E) * s.isz
        assert placement.guard_elems(s.E) >= 64 and placement.guard_elems(s.E) >= 64 * s.E
        assert s.guard == g
        # this array's band before it starts where the previous array's band after it ended, or later
        assert s.start - g >= prev_end, f"{s.name} or its guard overlaps its neighbour"
        prev_end = s.end + g
    assert prev_end <= ar.buf.numel()
    # the residues the placement promises
    for s in specs:
        odd = 8 if s.dtype == "f8" else 4
        r = ar.address(s.name) % 16
        if pl == "aligned":
            assert r == 0
        elif pl == "odd":
            assert r == odd and (s.dtype == "f8" or ar.address(s.name) % 8 == 4)
        elif pl == "ci_aligned_rest_odd":
            assert r == (0 if s.name in ("CI", "ci0") else odd)
        else:
            assert r == (odd if s.name == pl[5:] else 0)
    # everything but the inputs holds the sentinels, outputs included
    now = ar.download()
    for s in specs:
        band = now[s.start - s.guard:s.start].view(s.npdtype)
        assert band.size == placement.guard_elems(s.E) and np.all(band == s.sentinel)
        assert np.all(now[s.end:s.end + s.guard].view(s.npdtype) == s.sentinel)
        if s.data is None:
            assert np.all(ar.bits(s.name) == s.sentinel)
        else:
            assert np.array_equal(ar.bits(s.name), np.ascontiguousarray(s.data).view(np.uint64))


def test_sentinels_are_what_the_contract_says():
    v = np.array([placement.F64_SENTINEL]).view(np.float64)[0]
    assert np.isnan(v) and int(placement.F64_SENTINEL) & 0x0008_0000_0000_0000  # quiet
    assert int(placement.F64_SENTINEL) & 0x0007_FFFF_FFFF_FFFF  # non-zero payload
    assert int(placement.F64_SENTINEL) != np.array([np.nan]).view(np.uint64)[0]
    assert not (-8 <= int(placement.I32_SENTINEL) <= 1 << 24)  # no status, count or pass number


@pytest.mark.parametrize("layout", ["qp_major", "tiled64"])
@pytest.mark.parametrize("pl", ["aligned", "odd"])
def test_checker_is_silent_on_a_correct_solve_and_on_an_untouched_arena(pl, layout):
    pr, ar = _arena(pl, layout)
    skip = np.zeros(pr.batch, dtype=bool)
    skip[1] = True
    masks = placement.written_masks(ar, layout, pr.batch, x_skip=skip)
    nothing = {k: np.zeros_like(v) for k, v in masks.items()}
    assert ar.check(nothing) == []
    _fake_solve(ar, masks)
    assert ar.check(masks) == []
    # ... and the masks mean what they say: 70 QPs, x of one left alone, padding left alone
    assert int(masks["x"].sum()) == 69 * 5 and int(masks["u"].sum()) == 70 * 11
    assert int(masks["f"].sum()) == 70 and masks["x"].size == (128 if layout == "tiled64" else 70) * 5


def _one_finding(ar, masks, needle, **kw):
    f = ar.check(masks, **kw)
    assert len(f) == 1 and needle in f[0], f
    return f[0]


@pytest.mark.parametrize("layout", ["qp_major", "tiled64"])
@pytest.mark.parametrize("pl", ["aligned", "odd"])
def test_checker_reports_what_is_inflicted(pl, layout):
    def fresh():
        pr, ar = _arena(pl, layout)
        skip = np.zeros(pr.batch, dtype=bool)
        skip[1] = True
        masks = placement.written_masks(ar, layout, pr.batch, x_skip=skip)
        _fake_solve(ar, masks)
        return pr, ar, masks

    raw = lambda ar: ar.buf.numpy()
    # a guard element before an array, and after one: the nearest and the farthest of each band
    for name in ("x", "status", "G", "f"):
        for where in ("before", "after"):
            for far in (False, True):
                pr, ar, masks = fresh()
                s = ar.specs[name]
                k = (s.guard - s.isz if far else 0)
                off = s.start - s.isz - k if where == "before" else s.end + k
                raw(ar)[off] ^= 0x01
                _one_finding(ar, masks, f"guard {where} {name}")
    # one modified element of every input; G is forgiven only when the factor is asked for
    for name in placement.DENSE_INPUTS:
        pr, ar, masks = fresh()
        v = ar.view(name).numpy()
        v[v.size - 1] = np.nextafter(v[v.size - 1], np.inf)
        _one_finding(ar, masks, f"input {name}")
        if name == "G":
            assert ar.check(masks, modified_ok=("G",)) == []
        else:
            _one_finding(ar, masks, f"input {name}", modified_ok=("G",))
    # x of the not-positive-definite QP written; an element the call owed left unwritten
    pr, ar, masks = fresh()
    ar.view("x").numpy()[int(np.argmin(masks["x"]))] = 0.0
    _one_finding(ar, masks, "output x")
    pr, ar, masks = fresh()
    ar.view("nact").numpy()[5] = placement.I32_SENTINEL
    _one_finding(ar, masks, "output nact: 1 element(s) not written")
    # a byte between two arrays' bands
    pr, ar, masks = fresh()
    covered = np.zeros(ar.buf.numel(), dtype=bool)
    for s in ar.specs.values():
        covered[s.start - s.guard:s.end + s.guard] = True
    gaps = np.where(~covered)[0]
    assert gaps.size
    raw(ar)[gaps[0]] = 0
    _one_finding(ar, masks, "between the guard bands")
    if layout == "tiled64":
        # a written padding slot: QP 70 of the second tile, in x, u and nothing else
        for name in ("x", "u"):
            pr, ar, masks = fresh()
            E = ar.specs[name].E
            slot = 64 * E + (E - 1) * 64 + (70 - 64)
            assert not masks[name][slot] and masks[name][slot - 1]
            ar.view(name).numpy()[slot] = 0.0
            _one_finding(ar, masks, f"output {name}")


def test_sub_range_masks_and_pointers():
    """A call on QPs [b0, b1) of a larger batch: the pointers advance by whole QP blocks (QP-major)
    or whole tiles (TILED64), and only that range may be written."""
    pr, ar = _arena("odd", "qp_major", entry="plain", B=200)
    m = placement.written_masks(ar, "qp_major", 200, 63, 133)
    assert m["x"].reshape(200, 5)[63:133].all() and not m["x"].reshape(200, 5)[:63].any()
    assert not m["x"].reshape(200, 5)[133:].any() and int(m["status"].sum()) == 70
    assert ar.view("CI")[63 * 45:].data_ptr() == ar.address("CI") + 63 * 45 * 8
    pr, ar = _arena("odd", "tiled64", entry="plain", B=200)
    m = placement.written_masks(ar, "tiled64", 200, 64, 134)
    t = m["x"].reshape(4, 5, 64)
    assert not t[0].any() and t[1].all() and t[2][:, :6].all() and not t[2][:, 6:].any() and not t[3].any()
    _fake_solve(ar, m)
    assert ar.check(m) == []
    ar.view("f").numpy()[63] = 0.0  # the QP just before the range
    _one_finding(ar, m, "output f")


def test_host_licenses_16_byte_paths_per_array_group():
    """alignment_flags: bit 0 (CI's on-chip copy and double2 row loads) needs CI and ci0 aligned,
    bit 1 (the LDS-DMA staging) needs G, g0 and, with p > 0, CE and ce0; either array of a group
    clears its bit alone, and neither group touches the other's bit."""
    fn = qpgpu.LIB.qpgpu_debug_alignment_bits
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_void_p] * 6 + [ctypes.c_int32]
    base = 0x7F00_0000_1000
    names = ("G", "g0", "CE", "ce0", "CI", "ci0")
    call = lambda odd, p: fn(*[base + 0x1000 * i + (8 if n in odd else 0) for i, n in enumerate(names)], p)
    assert call((), 6) == 3 and call((), 0) == 3
    for n in ("CI", "ci0"):
        assert call((n,), 6) == 2, n
    for n in ("G", "g0", "CE", "ce0"):
        assert call((n,), 6) == 1, n
    for n in ("CE", "ce0"):
        assert call((n,), 0) == 3, n  # p = 0: never read, never staged
    assert call(names, 6) == 0
    assert call(("G", "g0", "CE", "ce0"), 6) == 1  # ci_aligned_rest_odd: CI's paths stay on
    # the box entries pass no CI / ci0 (NULL), an empty CE / ce0 may be NULL
    assert fn(base, base, None, None, None, None, 0) == 3
    assert fn(base + 8, base, None, None, None, None, 0) == 1
