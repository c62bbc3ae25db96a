"""CPU tests of the kernel selection: which kernel the library names for (n, p, m, flags, mode) and
what the seven solve entries return for calls that are decided before any device work, against a
table recorded from the library as it was before the selection was gathered into one function
(tests/golden/dispatch_table.json).  The table is data: `record()` below wrote it, run once with
QPGPU_LIB_PATH naming a build of that earlier commit; no test regenerates it.

No family's choice reads p (iq never exceeds n, so any p fits a variant that n fits): the table
stores one row per (flags, n, m) and every test checks it for p = 0 and p = 6.

Return codes come in two columns.  `nodev` was recorded where no GPU is visible, `dev` on an
MI355X; they differ only for qpgpu_solve_batched_multi, which needs the device count to check
its device list and so reports QPGPU_ERR_NO_DEVICE ahead of its later rules.  Every recorded call
returns before a pointer is read through: the arrays are one host buffer that no kernel sees.
"""
import ctypes
import json
import os

import pytest

import qpgpu

TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dispatch_table.json")

NS = (0, 1, 7, 8, 9, 16, 17, 32, 33, 64, 65, 256, 257, 300, 50000)
MS = (0, 14, 16, 17, 32, 33, 64, 65, 128, 129, 256, 257, 1024, 1025, "2n")
PS = (0, 6)
_FAM = (qpgpu.FLAG_FORCE_LANE, qpgpu.FLAG_FORCE_SUBGROUP, qpgpu.FLAG_FORCE_WAVE, qpgpu.FLAG_FORCE_GENERIC)
FLAGS = ((0,) + _FAM + tuple(f | qpgpu.FLAG_FAST for f in (0,) + _FAM)
         + (qpgpu.FLAG_EXACT, qpgpu.FLAG_WRITE_FACTOR)
         # rejected: FAST with EXACT / WRITE_FACTOR, two families, an unknown bit
         + (qpgpu.FLAG_FAST | qpgpu.FLAG_EXACT, qpgpu.FLAG_FAST | qpgpu.FLAG_WRITE_FACTOR,
            qpgpu.FLAG_FORCE_LANE | qpgpu.FLAG_FORCE_WAVE, 0x1000))


def _m(n, m):
    return 2 * n if m == "2n" else m


def _name_flags(lib, n, p, m, flags):
    return lib.qpgpu_kernel_name_flags(n, p, m, flags).decode()


def _name_box(lib, n, p, flags):
    return lib.qpgpu_kernel_name_box(n, p, flags).decode()


def _name_box_dual(lib, n, p, flags):
    return lib.qpgpu_kernel_name_box_dual(n, p, flags).decode()


# ---- return codes: the calls -----------------------------------------------------------------------
# pointer arguments of each entry after the descriptor (and, for multi, after ndev and devices),
# the stream excluded: it is always NULL
ENTRIES = {
    "plain": ("qpgpu_solve_batched", ("G", "g0", "CE", "ce0", "CI", "ci0", "x", "f", "status", "iters")),
    "eq": ("qpgpu_solve_batched_eq", ("G", "g0", "CE", "ce0", "CI", "ci0", "x", "f", "status", "iters",
                                      "x_eq", "f_eq", "status_eq")),
    "dual": ("qpgpu_solve_batched_dual", ("G", "g0", "CE", "ce0", "CI", "ci0", "x", "f", "status", "iters",
                                          "u", "nact")),
    "box": ("qpgpu_solve_batched_box", ("G", "g0", "CE", "ce0", "hi", "lo", "x", "f", "status", "iters")),
    "box_dual": ("qpgpu_solve_batched_box_dual", ("G", "g0", "CE", "ce0", "hi", "lo", "x", "f", "status",
                                                  "iters", "u", "nact")),
    "host": ("qpgpu_solve_batched_host", ("G", "g0", "CE", "ce0", "CI", "ci0", "x", "f", "status", "iters")),
    "multi": ("qpgpu_solve_batched_multi", ("G", "g0", "CE", "ce0", "CI", "ci0", "x", "f", "status", "iters")),
}
_HAS_STREAM = {"plain", "eq", "dual", "box", "box_dual"}
_BUF = (ctypes.c_double * 8192)()  # what every non-NULL pointer points at; never read through


def rc_rows():
    """(label, entry, desc or None, names of the non-NULL pointer arguments, ndev, devices)."""
    rows = []
    C1 = (7, 6, 14)
    for e, (_, names) in ENTRIES.items():
        full = frozenset(names)
        # what the entry's own rules ask for ahead of the common checks
        need = frozenset({"eq": ("x_eq", "f_eq", "status_eq"), "dual": ("u",), "box_dual": ("u",)}.get(e, ()))

        def add(label, desc, have, ndev=1, devs=(0,)):
            rows.append((f"{e}: {label}", e, desc, frozenset(have), ndev, devs))

        def D(n=C1[0], p=C1[1], m=C1[2], batch=4, flags=0, layout=0):
            return (n, p, m, 0, batch, flags, layout)

        # a bad descriptor
        add("NULL descriptor", None, full)
        add("n = 0", D(n=0), full)
        add("p < 0", D(p=-1), full)
        add("m < 0", D(m=-1), full)
        add("batch < 0", D(batch=-1), full)
        add("unknown layout", D(layout=7), full)
        # a flag-rule violation
        add("FAST | EXACT", D(flags=qpgpu.FLAG_FAST | qpgpu.FLAG_EXACT), full)
        add("FAST | WRITE_FACTOR", D(flags=qpgpu.FLAG_FAST | qpgpu.FLAG_WRITE_FACTOR), full)
        add("two families", D(flags=qpgpu.FLAG_FORCE_LANE | qpgpu.FLAG_FORCE_WAVE), full)
        add("unknown flag bit", D(flags=0x1000), full)
        # the entry's own rule
        if e == "eq":
            for k in need:
                add(f"NULL {k}", D(), full - {k})
        if e in ("dual", "box", "box_dual"):
            add("FAST refused", D(flags=qpgpu.FLAG_FAST), full)
            add("FAST refused, batch = 0", D(batch=0, flags=qpgpu.FLAG_FAST), full)
        if e in ("dual", "box_dual"):
            add("NULL u", D(), full - {"u"})
            add("NULL u, batch = 0", D(batch=0), full - {"u"})
        if e in ("box", "box_dual"):
            add("m != 2n", D(m=13), full)
            add("m != 2n, batch = 0", D(m=13, batch=0), full)
            add("NULL hi", D(), full - {"hi"})
            add("NULL lo", D(), full - {"lo"})
        if e == "multi":
            add("ndev = 0", D(), full, ndev=0)
            add("ndev = 65", D(), full, ndev=65, devs=(0,) * 65)
            add("NULL devices", D(), full, devs=None)
            add("device id out of range", D(), full, devs=(99,))
            add("negative device id", D(), full, devs=(-1,))
        # batch == 0: success with every array NULL (but what the entry's own rule asks for)
        add("batch = 0, arrays NULL", D(batch=0), need)
        add("batch = 0", D(batch=0), full)
        if e == "dual":
            add("batch = 0, p + m = 0, NULL u", D(p=0, m=0, batch=0), full - {"u"})
        # NULL common arrays with batch > 0
        own = need | ({"hi", "lo"} & full)
        add("arrays NULL", D(), own)
        for k in ("G", "g0", "x", "f", "status", "CE", "ce0") + (("CI", "ci0") if "CI" in full else ()):
            add(f"NULL {k}", D(), full - {k})
        # no kernel covers the shape: a forced family that lacks it, and no family at all
        shapes = (("FORCE_LANE", qpgpu.FLAG_FORCE_LANE, 30), ("FORCE_SUBGROUP", qpgpu.FLAG_FORCE_SUBGROUP, 30),
                  ("FORCE_WAVE", qpgpu.FLAG_FORCE_WAVE, 300), ("FORCE_GENERIC", qpgpu.FLAG_FORCE_GENERIC, 50000),
                  ("no family", 0, 50000))
        for label, fl, n in shapes:
            add(f"{label} does not cover n = {n}", D(n=n, p=0, m=2 * n, flags=fl), full)
        if e in ("plain", "eq", "host", "multi"):
            add("FAST | FORCE_LANE does not cover n = 30",
                D(n=30, p=0, m=60, flags=qpgpu.FLAG_FAST | qpgpu.FLAG_FORCE_LANE), full)
    return rows


def _call(lib, row):
    _, e, desc, have, ndev, devs = row
    sym, names = ENTRIES[e]
    fn = getattr(lib, sym)
    buf = ctypes.cast(_BUF, ctypes.c_void_p)
    d = None if desc is None else ctypes.byref(qpgpu.ProblemDesc(*desc))
    args = [buf if k in have else None for k in names]
    if e == "multi":
        dv = None if devs is None else (ctypes.c_int32 * len(devs))(*devs)
        return fn(d, ndev, None if dv is None else ctypes.cast(dv, ctypes.c_void_p), *args)
    if e in _HAS_STREAM:
        args.append(None)
    return fn(d, *args)


# ---- the generator of the table (run once against a build of the commit before the refactor) -------
def record(path=TABLE):
    """Write the table from the loaded library.  The name grid is written whole; the return codes
    fill the column of this machine (`dev` where a GPU is visible, `nodev` otherwise) and keep the
    other column of an existing file."""
    lib = qpgpu.LIB
    names = [""]

    def idx(s):
        if s not in names:
            names.append(s)
        return names.index(s)

    def same_for_every_p(fn):
        got = [fn(p) for p in PS]
        assert all(g == got[0] for g in got), got
        return got[0]

    t = {"names": names, "n": list(NS), "m": list(MS), "p": list(PS), "flags": list(FLAGS)}
    t["name_flags"] = [[[idx(same_for_every_p(lambda p: _name_flags(lib, n, p, _m(n, m), fl))) for m in MS]
                        for n in NS] for fl in FLAGS]
    t["name_box"] = [[idx(same_for_every_p(lambda p: _name_box(lib, n, p, fl))) for n in NS] for fl in FLAGS]
    t["name_box_dual"] = [[idx(same_for_every_p(lambda p: _name_box_dual(lib, n, p, fl))) for n in NS]
                          for fl in FLAGS]
    for n in NS:  # qpgpu_kernel_name is the flags = 0 slab
        for m in MS:
            for p in PS:
                assert lib.qpgpu_kernel_name(n, p, _m(n, m)).decode() == _name_flags(lib, n, p, _m(n, m), 0)
    col = "dev" if qpgpu.device_count() > 0 else "nodev"
    old = json.load(open(path)).get("rc", {}) if os.path.exists(path) else {}
    rows = rc_rows()
    t["rc"] = {r[0]: dict(old.get(r[0], {}), **{col: _call(lib, r)}) for r in rows}
    assert len(t["rc"]) == len(rows), "row labels must be unique"
    with open(path, "w") as f:
        f.write("{\n" + ",\n".join(f"{json.dumps(k)}: {json.dumps(v)}" for k, v in t.items() if k != "rc"))
        f.write(',\n"rc": {\n' + ",\n".join(f"{json.dumps(k)}: {json.dumps(v)}" for k, v in t["rc"].items()))
        f.write("\n}\n}\n")


# ---- the tests -------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def table():
    t = json.load(open(TABLE))
    assert tuple(t["n"]) == NS and tuple(t["m"]) == MS and tuple(t["p"]) == PS and tuple(t["flags"]) == FLAGS
    return t


def test_table_holds_every_kernel_name(table):
    """39 distinct answers, the empty name included: every name the four functions can return."""
    used = set()
    for key in ("name_flags", "name_box", "name_box_dual"):
        flat = json.dumps(table[key]).replace("[", " ").replace("]", " ").replace(",", " ").split()
        used |= {int(v) for v in flat}
    assert used == set(range(len(table["names"])))
    assert len(set(table["names"])) == len(table["names"]) == 39
    assert table["names"][0] == ""


@pytest.mark.parametrize("p", PS)
def test_kernel_name_flags_is_the_recorded_selection(table, p):
    lib, names = qpgpu.LIB, table["names"]
    for fi, fl in enumerate(FLAGS):
        for ni, n in enumerate(NS):
            for mi, m in enumerate(MS):
                want = names[table["name_flags"][fi][ni][mi]]
                got = _name_flags(lib, n, p, _m(n, m), fl)
                assert got == want, f"qpgpu_kernel_name_flags({n}, {p}, {_m(n, m)}, {fl:#x})"


@pytest.mark.parametrize("p", PS)
def test_kernel_name_is_the_flagless_selection(table, p):
    lib, names = qpgpu.LIB, table["names"]
    for ni, n in enumerate(NS):
        for mi, m in enumerate(MS):
            want = names[table["name_flags"][0][ni][mi]]
            assert lib.qpgpu_kernel_name(n, p, _m(n, m)).decode() == want, f"qpgpu_kernel_name({n}, {p}, {_m(n, m)})"


@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("which", ("name_box", "name_box_dual"))
def test_box_kernel_names_are_the_recorded_selection(table, which, p):
    fn = _name_box if which == "name_box" else _name_box_dual
    names = table["names"]
    for fi, fl in enumerate(FLAGS):
        for ni, n in enumerate(NS):
            want = names[table[which][fi][ni]]
            assert fn(qpgpu.LIB, n, p, fl) == want, f"qpgpu_kernel_{which}({n}, {p}, {fl:#x})"


@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_return_codes_decided_before_any_device_work(table, entry):
    col = "dev" if qpgpu.device_count() > 0 else "nodev"
    rows = [r for r in rc_rows() if r[1] == entry]
    assert rows and {r[0] for r in rc_rows()} == set(table["rc"])
    for r in rows:
        assert _call(qpgpu.LIB, r) == table["rc"][r[0]][col], r[0]
