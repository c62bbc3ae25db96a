"""Arena placement of a solve's device arrays (TEST INFRASTRUCTURE ONLY).

include/qpgpu.h takes plain pointers: natural alignment is enough for every entry and a pointer
into the middle of a larger batch is legal.  The parity tests place every array in a fresh
allocation of its own (512-byte aligned, QP 0 first, nothing of ours beside it); this helper places
them the other ways a host program's own arena does:

  * ONE allocation per solve, carved into the entry's arrays, all of it filled with sentinels
    before the arrays are written into it;
  * every array at a requested residue of its base ADDRESS mod 16 (float64: 0 or 8; int32: 0 or
    4, i.e. 4 mod 8), by a named placement (PLACEMENTS, `only:<array>`);
  * a guard band of max(64, 64 * E) elements before and after every array (E its per-QP element
    count), so that a whole stray 64-QP tile still lands inside a guard;
  * outputs pre-filled with the same sentinels, the TILED64 padding slots included.

Sentinels: for float64 one fixed quiet-NaN bit pattern with a payload no arithmetic produces,
compared as uint64; for int32 a value that is no status, count or pass number.

Arena.check() downloads the whole allocation once and returns a list of findings (strings), empty
when every guard band and every byte between the bands is what was uploaded, every input is
bit-identical to what was uploaded, every output element the call must not write (TILED64 padding,
QPs outside the solved range, x of a not-positive-definite QP) still holds the sentinel, and every
element it must write no longer does.  tests/test_placement_cpu.py runs all of this on CPU tensors.
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

F64_SENTINEL = np.uint64(0x7FF8_5EA7_1E55_C0DE)  # quiet NaN, non-zero payload
I32_SENTINEL = np.int32(-1515870811)             # 0xA5A5A5A5
SLACK_BYTE = 0xEE                                # the few bytes between two arrays' guard bands

PLACEMENTS = ("aligned", "odd", "ci_aligned_rest_odd")
DENSE_INPUTS = ("G", "g0", "CE", "ce0", "CI", "ci0")
BOX_INPUTS = ("G", "g0", "CE", "ce0", "hi", "lo")
PER_QP_SCALARS = ("f", "status", "iters", "f_eq", "status_eq", "nact")  # one value per QP, no tiles


def residue(placement: str, name: str, dtype: str) -> int:
    """The residue mod 16 of array `name`'s base address under a named placement."""
    odd = 8 if dtype == "f8" else 4
    if placement == "aligned":
        return 0
    if placement == "odd":
        return odd
    if placement == "ci_aligned_rest_odd":
        return 0 if name in ("CI", "ci0") else odd
    if placement.startswith("only:"):
        return odd if name == placement[5:] else 0
    raise ValueError(f"unknown placement {placement!r}")


def guard_elems(E: int) -> int:
    return max(64, 64 * E)


@dataclass
class Spec:
    """One array of the entry: `count` elements of `dtype` ("f8" / "i4"), E per QP.  `data` (flat
    numpy, the device layout) makes it an input; None an output."""
    name: str
    dtype: str
    E: int
    count: int
    data: np.ndarray | None = None
    # filled in by Arena: byte offsets from the allocation's base
    start: int = field(default=0, repr=False)
    guard: int = field(default=0, repr=False)  # bytes, each side

    @property
    def isz(self) -> int:
        return 8 if self.dtype == "f8" else 4

    @property
    def end(self) -> int:
        return self.start + self.count * self.isz

    @property
    def npdtype(self):
        return np.uint64 if self.dtype == "f8" else np.int32

    @property
    def sentinel(self):
        return F64_SENTINEL if self.dtype == "f8" else I32_SENTINEL


class Arena:
    """One allocation on `device` ("cpu" for the helper's own test) holding `specs` at `placement`.
    view(name) is a 1-D torch tensor of the array inside the allocation (float64 / int32)."""

    def __init__(self, specs, placement: str, device="cpu"):
        import torch

        self.specs = {s.name: s for s in specs}
        assert len(self.specs) == len(specs), "array names must be unique"
        self.placement = placement
        total = 16
        for s in specs:
            total += 2 * guard_elems(s.E) * s.isz + s.count * s.isz + 16
        self.buf = torch.empty(total, dtype=torch.uint8, device=device)
        base = self.buf.data_ptr()
        assert base % 8 == 0
        cur = 0
        for s in specs:
            s.guard = guard_elems(s.E) * s.isz
            s.start = cur + s.guard
            s.start += (residue(placement, s.name, s.dtype) - (base + s.start)) % 16
            cur = s.end + s.guard
        assert cur <= total
        self.base = base
        img = np.full(total, SLACK_BYTE, dtype=np.uint8)
        for s in specs:
            lo, hi = s.start - s.guard, s.end + s.guard
            img[lo:hi].view(s.npdtype)[:] = s.sentinel
            if s.data is not None:
                d = np.ascontiguousarray(s.data).reshape(-1)
                assert d.size == s.count and d.dtype.itemsize == s.isz, s.name
                img[s.start:s.end] = d.view(np.uint8)
        self.image = img  # what was uploaded
        self.buf.copy_(torch.from_numpy(img))
        self._tdtype = {"f8": torch.float64, "i4": torch.int32}

    def reset(self):
        """Upload the initial image again: inputs as given, sentinels everywhere else."""
        import torch

        self.buf.copy_(torch.from_numpy(self.image))

    def address(self, name: str) -> int:
        return self.base + self.specs[name].start

    def view(self, name: str):
        s = self.specs[name]
        return self.buf[s.start:s.end].view(self._tdtype[s.dtype])

    def download(self) -> np.ndarray:
        return self.buf.cpu().numpy().copy()

    def bits(self, name: str, now: np.ndarray | None = None) -> np.ndarray:
        """The array's current content as raw uint64 / int32 (a copy)."""
        s = self.specs[name]
        now = self.download() if now is None else now
        return now[s.start:s.end].view(s.npdtype).copy()

    def values(self, name: str, now: np.ndarray | None = None) -> np.ndarray:
        b = self.bits(name, now)
        return b.view(np.float64) if self.specs[name].dtype == "f8" else b

    def check(self, written: dict, modified_ok=()) -> list:
        """Findings after a solve.  written[name] is, per output, a boolean mask over its elements:
        True where the call must have written, False where it must not have.  `modified_ok` names
        inputs the call may overwrite (G with QPGPU_FLAG_WRITE_FACTOR)."""
        now = self.download()
        out = []
        diff = now != self.image
        covered = np.zeros(now.size, dtype=bool)

        def first(lo, hi, s):
            k = lo + int(np.argmax(diff[lo:hi]))
            e = (k - s.start) // s.isz  # floor: negative before the array
            v = now[s.start + e * s.isz:s.start + (e + 1) * s.isz].view(s.npdtype)[0]
            return e, v

        for s in self.specs.values():
            lo, hi = s.start - s.guard, s.end + s.guard
            covered[lo:hi] = True
            if diff[lo:s.start].any():
                e, v = first(lo, s.start, s)
                n = int(diff[lo:s.start].reshape(-1, s.isz).any(axis=1).sum())
                out.append(f"guard before {s.name}: {n} element(s) written, e.g. element {e} = {v:#x}")
            if diff[s.end:hi].any():
                e, v = first(s.end, hi, s)
                n = int(diff[s.end:hi].reshape(-1, s.isz).any(axis=1).sum())
                out.append(f"guard after {s.name}: {n} element(s) written, e.g. element {e} "
                           f"(count {s.count}) = {v:#x}")
            if s.data is not None:
                if s.name not in modified_ok and diff[s.start:s.end].any():
                    e, v = first(s.start, s.end, s)
                    n = int(diff[s.start:s.end].reshape(-1, s.isz).any(axis=1).sum())
                    out.append(f"input {s.name}: {n} element(s) modified, e.g. element {e} = {v:#x}")
                continue
            assert s.name in written, f"no written-mask for output {s.name}"
            w = np.asarray(written[s.name], dtype=bool).reshape(-1)
            assert w.size == s.count, s.name
            held = now[s.start:s.end].view(s.npdtype) == s.sentinel
            bad = ~w & ~held
            if bad.any():
                out.append(f"output {s.name}: {int(bad.sum())} element(s) written that the call must leave "
                           f"alone, e.g. element {int(np.argmax(bad))}")
            miss = w & held
            if miss.any():
                out.append(f"output {s.name}: {int(miss.sum())} element(s) not written, e.g. element "
                           f"{int(np.argmax(miss))}")
        stray = diff & ~covered
        if stray.any():
            out.append(f"between the guard bands: {int(stray.sum())} byte(s) written, e.g. offset {int(np.argmax(stray))}")
        return out


# ---- masks ----------------------------------------------------------------------------------------
def rows_of(batch: int, layout) -> int:
    """QP slots a per-QP array holds: whole 64-QP tiles in the TILED64 layout."""
    return (batch + 63) // 64 * 64 if layout == "tiled64" else batch


def block_mask(E: int, layout, total: int, b0: int = 0, b1: int | None = None, skip=None) -> np.ndarray:
    """Mask over a per-QP array of E elements per QP holding QPs [0, total) in `layout`: True on the
    elements of QPs [b0, b1) (default: all `total`), except the QPs flagged in `skip` (a boolean
    array over [b0, b1)).  TILED64 padding slots are False."""
    b1 = total if b1 is None else b1
    qp = np.zeros(rows_of(total, layout), dtype=bool)
    qp[b0:b1] = True
    if skip is not None:
        qp[b0:b1] &= ~np.asarray(skip, dtype=bool)
    if layout == "tiled64":
        return np.repeat(qp.reshape(-1, 1, 64), E, axis=1).reshape(-1)
    return np.repeat(qp, E)


def scalar_mask(total: int, b0: int = 0, b1: int | None = None) -> np.ndarray:
    return block_mask(1, None, total, b0, b1)


# ---- the entries' arrays ---------------------------------------------------------------------------
ENTRY_OUTPUTS = {
    "plain": (),
    "eq": (("x_eq", "f8", "n"), ("f_eq", "f8", 1), ("status_eq", "i4", 1)),
    "dual": (("u", "f8", "p+m"), ("nact", "i4", 1)),
}


def entry_specs(pr, layout, entry: str = "plain") -> list:
    """Specs of every array of one entry for the batch `pr` (qpgpu.Problems, or qpgpu.BoxProblems
    for the box entries, whose "dual" is qpgpu_solve_batched_box_dual), inputs in `layout`."""
    import qpgpu

    B, n, p, m = pr.batch, pr.n, pr.p, pr.m
    rows = rows_of(B, layout)
    conv = qpgpu.to_tiled64 if layout == "tiled64" else (lambda a: a)
    names = BOX_INPUTS if isinstance(pr, qpgpu.BoxProblems) else DENSE_INPUTS
    per_qp = {"G": n * n, "g0": n, "CE": n * p, "ce0": p, "CI": n * m, "ci0": m, "hi": n, "lo": n}
    specs = []
    for name, a in zip(names, pr.arrays()):
        d = np.ascontiguousarray(conv(np.asarray(a, dtype=np.float64))).reshape(-1)
        assert d.size == rows * per_qp[name]
        specs.append(Spec(name, "f8", per_qp[name], d.size, d))
    specs += [Spec("x", "f8", n, rows * n), Spec("f", "f8", 1, B), Spec("status", "i4", 1, B),
              Spec("iters", "i4", 1, B)]
    for name, dt, e in ENTRY_OUTPUTS[entry]:
        E = {"n": n, "p+m": p + m, 1: 1}[e]
        specs.append(Spec(name, dt, E, B if name in PER_QP_SCALARS else rows * E))
    return specs


def attach(arena: Arena, db, b0: int = 0, batch: int | None = None):
    """Point a qpgpu.DeviceBatch / DeviceBoxBatch at the arena's arrays (its solve() takes
    data_ptr() of whatever tensors it holds), advanced to QP b0 (QP-major: b0 * E elements;
    TILED64: whole tiles, b0 a multiple of 64) with `batch` QPs.  Returns the extra outputs as the
    tuple solve() takes (eq_out or dual_out), or None."""
    import qpgpu

    tiled = db.layout == qpgpu.LAYOUT_TILED64
    assert not (tiled and b0 % 64), "a TILED64 sub-range starts at a whole tile"
    for name, s in arena.specs.items():
        if name in ("x_eq", "f_eq", "status_eq", "u", "nact"):
            continue
        setattr(db, name, arena.view(name)[b0 * s.E:])
    if batch is not None:
        db.batch = batch
    adv = lambda name: arena.view(name)[b0 * arena.specs[name].E:]
    if "x_eq" in arena.specs:
        return (adv("x_eq"), adv("f_eq"), adv("status_eq"))
    if "u" in arena.specs:
        return (adv("u"), adv("nact"))
    return None


def written_masks(arena: Arena, layout, total: int, b0: int = 0, b1: int | None = None, x_skip=None) -> dict:
    """The written-masks of every output in the arena for a call on QPs [b0, b1) of `total`;
    x_skip flags the QPs of that range whose x (and x_eq) the contract leaves unwritten
    (QPGPU_QP_NOT_POSITIVE_DEFINITE: the reference throws before x exists)."""
    out = {}
    for name, s in arena.specs.items():
        if s.data is not None:
            continue
        if name in PER_QP_SCALARS:
            out[name] = scalar_mask(total, b0, b1)
        else:
            out[name] = block_mask(s.E, layout, total, b0, b1, skip=x_skip if name in ("x", "x_eq") else None)
    return out
