"""usage: asm_diff.py new.s parent.s   -- filtered whole-file and per-kernel comparison of two gfx950 .s files"""
import re
import sys


def load(path):
    out = []
    for ln in open(path):
        ln = ln.rstrip("\n")
        s = ln.split(";", 1)[0].rstrip() if ";" in ln and not ln.lstrip().startswith(".") else ln
        t = s.strip()
        if not t or t.startswith(("//", ";")):
            continue
        if t.startswith((".file", ".ident", ".section", ".loc")) or "__hip_cuid_" in t:
            continue
        out.append(s)
    return out


def split(lines):
    """kernel name -> its lines (label .. .Lfunc_end), plus the rest in order"""
    ker, rest, name, cur = {}, [], None, None
    order = []
    for ln in lines:
        m = re.match(r"^(_Z\w+):", ln)
        if m and name is None:
            name, cur = m.group(1), []
            order.append(name)
            continue
        if name is not None:
            cur.append(ln)
            if ln.startswith(".Lfunc_end"):
                ker[name] = cur
                name = None
            continue
        rest.append(ln)
    if name is not None:  # a device variable's label after the last function: no .Lfunc_end follows
        order.pop()
        rest += [name + ":"] + cur
    return ker, rest, order


def meta(path):
    txt = open(path).read()
    m = txt[txt.index("amdhsa.kernels:"):]
    out = {}
    for blk in re.split(r"\n  - ", m)[1:]:
        f = dict(re.findall(r"\.(\w+):\s+(\S+)", blk))
        if "vgpr_count" in f:
            keys = ("sgpr_count", "vgpr_count", "agpr_count", "group_segment_fixed_size",
                    "private_segment_fixed_size", "kernarg_segment_size", "wavefront_size")
            out[f["name"]] = tuple(f.get(k, "0") for k in keys)
    return out


new, par = load(sys.argv[1]), load(sys.argv[2])
kn, rn, on = split(new)
kp, rp, op = split(par)
mn, mp = meta(sys.argv[1]), meta(sys.argv[2])
print(f"filtered lines: new {len(new)} parent {len(par)}; whole files identical: {new == par}")
print(f"kernels: new {len(kn)} parent {len(kp)}; same set: {set(kn) == set(kp)}; same emission order: {on == op}")
tot = bad = 0
for k in op:
    a, b = kn.get(k), kp[k]
    if a is None:
        print(k, "MISSING in new")
        bad += 1
        continue
    d = sum(1 for x, y in zip(a, b) if x != y) + abs(len(a) - len(b))
    tot += len(a)
    bad += d
    print(f"{k} lines {len(a)} parent {len(b)} differing {d} sgpr {mn[k][0]} vgpr {mn[k][1]} agpr {mn[k][2]} lds {mn[k][3]} "
          f"scratch {mn[k][4]} kernarg {mn[k][5]} metadata {'equal' if mn[k] == mp[k] else 'DIFFERENT'}")
print(f"total: {tot} kernel lines, differing lines {bad}")
print("outside kernels:", "identical" if rn == rp else "DIFFERENT")
