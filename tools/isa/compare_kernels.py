"""Per-kernel comparison of two builds' device code:  python tools/isa/compare_kernels.py OLD NEW
OLD and NEW are `llvm-objdump -d --no-show-raw-insn` listings (see README.md) or directories of them (*.s): a kernel is
looked up in whichever listing of its side holds it.  Instruction lines are compared with the trailing `// address` comment
removed and the `...` padding lines dropped.  Per kernel of OLD: instruction count on both sides, SAME / DIFF, and for a
DIFF the number of differing lines and the opcodes whose counts differ.  Exit 1 when a kernel of OLD is missing in NEW."""
import collections, difflib, glob, os, re, sys


def kernels(path):
    out = {}
    for f in sorted(glob.glob(os.path.join(path, "*.s"))) if os.path.isdir(path) else [path]:
        name = None
        for line in open(f):
            m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
            if m:
                name = m.group(1)
                out[name] = []
            elif name and line.strip() and line.strip() != "...":
                out[name].append(re.sub(r"\s*//.*$", "", line.strip()))
    return out


old, new = kernels(sys.argv[1]), kernels(sys.argv[2])
missing = 0
for k in sorted(old):
    a = old[k]
    if k not in new:
        print("%-90s %6d %6s MISSING" % (k[:90], len(a), "-"))
        missing += 1
        continue
    b = new[k]
    if a == b:
        print("%-90s %6d %6d SAME" % (k[:90], len(a), len(b)))
        continue
    lo = next(i for i, (x, y) in enumerate(zip(a, b)) if x != y) if a[:min(len(a), len(b))] != b[:min(len(a), len(b))] else min(len(a), len(b))
    hi = 0
    while hi < min(len(a), len(b)) - lo and a[-1 - hi] == b[-1 - hi]:
        hi += 1
    sm = difflib.SequenceMatcher(None, a[lo:len(a) - hi], b[lo:len(b) - hi], autojunk=False)   # between the common ends only
    changed = sum(max(i2 - i1, j2 - j1) for tag, i1, i2, j1, j2 in sm.get_opcodes() if tag != "equal")
    ha, hb = (collections.Counter(l.split()[0] for l in x) for x in (a, b))
    ops = ", ".join("%s %d/%d" % (o, ha[o], hb[o]) for o in sorted(set(ha) | set(hb)) if ha[o] != hb[o])
    print("%-90s %6d %6d DIFF %d lines; opcode counts: %s" % (k[:90], len(a), len(b), changed, ops or "equal"))
sys.exit(1 if missing else 0)
