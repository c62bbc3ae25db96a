"""Every kernel of one or two gfx950 .s files (hipcc -S / -save-temps): static instruction totals,
f64 count, registers and scratch on one line per kernel, and with two files what moved.
usage: python tools/isa_census.py after.s [before.s] [op ...]
Each `op` (an instruction mnemonic, e.g. v_lshl_add_u64) is counted per kernel as well."""
import collections
import re
import sys


def kernels(path):
    txt = open(path).read()
    meta = txt[txt.index("amdhsa.kernels:"):]
    regs = {}
    for blk in re.split(r"\n  - ", meta)[1:]:
        f = dict(re.findall(r"\.(\w+):\s+(\S+)", blk))
        if "vgpr_count" not in f:  # (the lists that follow the kernels: amdhsa.version)
            continue
        regs[f["name"]] = (int(f["vgpr_count"]), int(f.get("agpr_count", 0)), int(f["private_segment_fixed_size"]))
    out, name, cnt = {}, None, None
    for ln in txt.split("\n"):
        m = re.match(r"^([A-Za-z_]\w*):", ln)
        if m and m.group(1) in regs:
            name, cnt = m.group(1), collections.Counter()
            continue
        if name is None:
            continue
        if ln.startswith("\t.size") or ln.startswith(".Lfunc_end"):
            out[name] = (cnt, regs[name])
            name = None
            continue
        s = ln.strip()
        if not s or s.startswith((";", ".", "//")) or s.endswith(":"):
            continue
        cnt[s.split()[0]] += 1
    return out


def row(cnt, regs, ops):
    tot = sum(cnt.values())
    f64 = sum(v for k, v in cnt.items() if k.startswith("v_") and "f64" in k)
    return (tot, f64) + regs + tuple(cnt[o] for o in ops)


files = [a for a in sys.argv[1:] if a.endswith(".s")]
ops = [a for a in sys.argv[1:] if not a.endswith(".s")]
after = kernels(files[0])
before = kernels(files[1]) if len(files) > 1 else None
print("kernel: total f64 vgpr agpr scratch " + " ".join(ops))
for name, (cnt, regs) in after.items():
    r = row(cnt, regs, ops)
    line = f"{name[:72]:72s} " + " ".join(str(v) for v in r)
    if before is not None:
        if name not in before:
            line += "   (not in the other file)"
        else:
            rb = row(*before[name], ops)
            line += "   was " + " ".join(str(v) for v in rb) if rb != r else "   unchanged"
    print(line)
