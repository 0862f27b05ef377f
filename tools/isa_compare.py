"""Kernel-by-kernel comparison of two gfx950 assembly files of one source (hipcc <build.py's FLAGS> -save-temps -c FILE.hip, before and after a
change; no GPU needed):  python tools/isa_compare.py parent.s child.s > profiles/<change>_isa.txt
Per kernel symbol: VGPR / SGPR / LDS bytes / scratch bytes of both sides and whether the instruction streams are identical once comments, labels
and symbol names are stripped; for a stream that differs, which opcodes' counts changed and whether the floating-point opcodes keep their order."""
import collections, re, subprocess, sys


def kernels(path):
    asm = open(path).read()
    res = {}
    for entry in asm[asm.index("amdhsa.kernels:"):].split("\n  - .agpr_count")[1:]:      # one metadata entry per kernel
        f = dict(re.findall(r"\.(name|vgpr_count|sgpr_count|group_segment_fixed_size|private_segment_fixed_size):\s+(\S+)", entry))
        res[f["name"]] = tuple(int(f[k]) for k in ("vgpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size"))
    out = {}
    for name in res:
        body = re.search(r"^%s:[^\n]*\n(.*?)^\.Lfunc_end\d+:" % re.escape(name), asm, re.S | re.M).group(1)
        ins = []
        for line in body.split("\n"):
            line = line.split(";")[0].strip()
            if not line or line.startswith(".") or line.endswith(":"):
                continue
            ins.append(re.sub(r"_Z\w+|\.LBB\w+|\.L\w+", "SYM", line))       # symbol names and branch targets
        out[name] = (res[name], ins)
    return out


def demangle(names):
    return dict(zip(names, subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")))


a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
pretty = demangle(sorted(set(a) | set(b)))
print(f"# kernels: parent {len(a)}, child {len(b)}; symbol sets {'equal' if set(a) == set(b) else 'DIFFER: ' + str(sorted(set(a) ^ set(b)))}")
print("# vgpr / sgpr / LDS bytes / scratch bytes, parent -> child (one value: unchanged)")
same = 0
for name in sorted(set(a) & set(b), key=lambda n: pretty[n]):
    (ra, ia), (rb, ib) = a[name], b[name]
    if ia == ib:
        verdict = "identical"
        same += 1
    else:       # what moved: the opcodes whose counts changed (none: registers / operands / order only) and whether the floating-point opcodes still come in the same order
        ops = lambda ins: [x.split()[0] for x in ins]
        ca, cb = collections.Counter(ops(ia)), collections.Counter(ops(ib))
        delta = ", ".join(f"{k} {cb[k] - ca[k]:+d}" for k in sorted(set(ca) | set(cb)) if ca[k] != cb[k]) or "none"
        fp = lambda ins: [x for x in ops(ins) if re.match(r"v_(pk_)?(add|sub|mul|fma|fmac|mac|max|min|rsq|rcp|exp|sqrt|cvt)\w*_(f|bf)", x) or "mfma" in x]
        verdict = f"DIFFERS ({len(ia)} -> {len(ib)} instructions; opcode counts changed: {delta}; floating-point opcode sequence {'equal' if fp(ia) == fp(ib) else 'DIFFERS'})"
    r = " ".join(str(x) if x == y else f"{x}->{y}" for x, y in zip(ra, rb))
    print(f"{pretty[name].replace('void ', '').split('(')[0]:60s} {r:22s} {verdict}")
print(f"# {same} of {len(set(a) & set(b))} instruction streams identical")
