#!/usr/bin/env python3
"""Per-kernel comparison of two device-assembly listings of one translation unit (a refactor's before / after):
    hipcc <the Makefile's FLAGS> --cuda-device-only -S x.hip -o x.s -Rpass-analysis=kernel-resource-usage 2> x.remarks
    tools/isa_compare.py old.s old.remarks new.s new.remarks [old-name-regex=new-name-template ...]
Prints instruction count, VGPRs, scratch and waves per SIMD of every kernel in both builds and whether the instruction streams are
identical (labels renumbered, symbol names ignored).  Renamed kernels are paired by the regex arguments (on demangled names)."""
import re, subprocess, sys


def demangle(names):
    # (binutils' c++filt does not know the 16-bit float manglings DF16_ / DF16b: two unused builtin codes stand in for them)
    names = [n.replace("DF16_", "Dh").replace("DF16b", "De") for n in names]
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
    out = [re.sub(r"\bhalf\b", "_Float16", o).replace("decimal128", "__bf16").replace("> >", ">>").replace("> >", ">>") for o in out]
    return [re.sub(r"^void ", "", re.sub(r"\(.*", "", o)).replace("nsa::", "") for o in out]


def kernels(asm, remarks):
    body, cur = {}, None
    for line in open(asm):
        m = re.match(r"\s*\.type\s+(\S+),@function", line)
        if m:
            cur = m.group(1)
            body[cur] = []
            continue
        if cur is None:
            continue
        if re.match(r"\.Lfunc_end", line):
            cur = None
            continue
        t = line.split(";")[0].strip()
        if not t or t.startswith(".") and not t.endswith(":") or t == cur + ":":
            continue
        body[cur].append(re.sub(r"\.LBB\d+_", ".LBB_", t))
    res, cur = {}, None
    for line in open(remarks):
        m = re.search(r"remark:\s+(.*?)\s*\[-Rpass", line)
        if not m:
            continue
        k, _, v = m.group(1).partition(":")
        if k == "Function Name":
            cur = v.strip()
            res[cur] = {}
        elif cur:
            res[cur][k.strip()] = v.strip()
    names = [n for n in body if n in res]
    out = {}
    for n, d in zip(names, demangle(names)):
        ins = [t for t in body[n] if not t.endswith(":")]
        r = res[n]
        out[d] = dict(n=len(ins), text=body[n], vgpr=r.get("VGPRs"), scratch=r.get("ScratchSize [bytes/lane]"), occ=r.get("Occupancy [waves/SIMD]"))
    return out


def main():
    old, new = kernels(sys.argv[1], sys.argv[2]), kernels(sys.argv[3], sys.argv[4])
    maps = [a.split("=", 1) for a in sys.argv[5:]]
    same, rows = [], []
    for name, o in old.items():
        to = name
        for pat, tmpl in maps:
            if re.fullmatch(pat, name):
                to = re.sub(pat, tmpl, name)
        b = new.get(to)
        if b is None:
            rows.append(f"{name}\n    -> (gone)")
            continue
        ident = o["text"] == b["text"]
        if ident:
            same.append(name if to == name else f"{name} -> {to}")
        flags = "".join([" SCRATCH+" if int(b["scratch"]) > int(o["scratch"]) else "", " OCC-" if int(b["occ"]) < int(o["occ"]) else ""])
        rows.append(f"{name}" + (f"\n    -> {to}" if to != name else "") +
                    f"\n    instr {o['n']} -> {b['n']}  vgpr {o['vgpr']} -> {b['vgpr']}  scratch {o['scratch']} -> {b['scratch']}  waves/SIMD {o['occ']} -> {b['occ']}"
                    f"  {'identical' if ident else 'differs'}{flags}")
    print("\n".join(rows))
    print(f"\nidentical instruction streams ({len(same)} of {len(old)} kernels):")
    print("\n".join("  " + s for s in same))


main()
