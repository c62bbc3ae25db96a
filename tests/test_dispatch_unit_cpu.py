"""CPU test of the unit-Hessian entry's kernel selection: which kernel qpgpu_kernel_name_unit names
for (n, p, m, flags), variant and all, against a table recorded from the library as it was while the
unit selection was a function of its own beside the main one (tests/golden/dispatch_unit_table.json).
tests/test_unit_cpu.py checks the family word of a name only.  The table is data: `record()` below
wrote it, run once with QPGPU_LIB_PATH naming a build of that earlier commit; no test regenerates it.

The grid is tests/test_dispatch_cpu.py's; as there, no family's choice reads p, so the table stores
one row per (flags, n, m) and the test checks it for every p.
"""
import json
import os

import pytest

import qpgpu
from test_dispatch_cpu import MS, NS, PS, _m

TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dispatch_unit_table.json")

FLAGS = ((0, qpgpu.FLAG_FORCE_LANE, qpgpu.FLAG_FORCE_SUBGROUP, qpgpu.FLAG_FORCE_WAVE, qpgpu.FLAG_EXACT)
         # refused: no fast unit form, no G to write a factor to, no generic unit kernel, two families,
         # an unknown bit
         + (qpgpu.FLAG_FAST, qpgpu.FLAG_WRITE_FACTOR, qpgpu.FLAG_FORCE_GENERIC,
            qpgpu.FLAG_FORCE_LANE | qpgpu.FLAG_FORCE_WAVE, 0x1000))


def _name_unit(lib, n, p, m, flags):
    return lib.qpgpu_kernel_name_unit(n, p, m, flags).decode()


# ---- the generator of the table (run once against a build of the commit before the refactor) -------
def record(path=TABLE):
    """Write the table from the loaded library."""
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
    t["name_unit"] = [[[idx(same_for_every_p(lambda p: _name_unit(lib, n, p, _m(n, m), fl))) for m in MS]
                       for n in NS] for fl in FLAGS]
    with open(path, "w") as f:
        f.write("{\n" + ",\n".join(f"{json.dumps(k)}: {json.dumps(v)}" for k, v in t.items()) + "\n}\n")


# ---- the tests -------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def table():
    t = json.load(open(TABLE))
    assert tuple(t["n"]) == NS and tuple(t["m"]) == MS and tuple(t["p"]) == PS and tuple(t["flags"]) == FLAGS
    return t


def test_table_holds_every_unit_kernel_name(table):
    """The empty name and one name per size class of the three families' unit builds: 2 lane, 4
    subgroup, 5 wave."""
    flat = json.dumps(table["name_unit"]).replace("[", " ").replace("]", " ").replace(",", " ").split()
    assert {int(v) for v in flat} == set(range(len(table["names"])))
    assert len(set(table["names"])) == len(table["names"]) == 12
    assert table["names"][0] == ""
    assert all("_unit<" in s for s in table["names"][1:])


@pytest.mark.parametrize("p", PS)
def test_kernel_name_unit_is_the_recorded_selection(table, p):
    lib, names = qpgpu.LIB, table["names"]
    for fi, fl in enumerate(FLAGS):
        for ni, n in enumerate(NS):
            for mi, m in enumerate(MS):
                want = names[table["name_unit"][fi][ni][mi]]
                got = _name_unit(lib, n, p, _m(n, m), fl)
                assert got == want, f"qpgpu_kernel_name_unit({n}, {p}, {_m(n, m)}, {fl:#x})"
