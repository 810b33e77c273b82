#!/usr/bin/env python3
"""Per-kernel comparison of two device-assembly listings of one translation unit (a refactor's before / after):
    hipcc <the Makefile's FLAGS> --cuda-device-only -S x.hip -o x.s -Rpass-analysis=kernel-resource-usage 2> x.remarks
    tools/isa_compare.py old.s old.remarks new.s new.remarks [old-name-regex=new-name-template ...]
Prints instruction count, VGPRs, scratch, LDS and waves per SIMD of every kernel in both builds and whether the instruction streams are
identical (labels renumbered, symbol names ignored).  A kernel that differs also gets the verdict on its loops: "loops same" when every
loop block (tools/isa_loop.py's blocks, in order) keeps its VALU / SALU / DS / VMEM / MFMA counts, so that the difference lies outside the
loops or in the order inside a block.  Flags: SCRATCH+, OCC-, VGPR+, LDS!=, LOOPS!=.  Renamed kernels are paired by the regex arguments
(on demangled names)."""
import re, subprocess, sys


def demangle(names):
    # (binutils' c++filt does not know the 16-bit float manglings DF16_ / DF16b: two unused builtin codes stand in for them)
    names = [n.replace("DF16_", "Dh").replace("DF16b", "De") for n in names]
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
    out = [re.sub(r"\bhalf\b", "_Float16", o).replace("decimal128", "__bf16").replace("> >", ">>").replace("> >", ">>") for o in out]
    return [re.sub(r"^void ", "", re.sub(r"\(.*", "", o)).replace("nsa::", "") for o in out]


def kind(op):
    return 4 if op.startswith("v_mfma") else 0 if op.startswith("v_") else 1 if op.startswith("s_") else 2 if op.startswith("ds_") else \
        3 if op.startswith(("global_", "buffer_", "flat_", "scratch_")) else 5


def kernels(asm, remarks):
    body, loops, cur = {}, {}, None
    for line in open(asm):
        m = re.match(r"\s*\.type\s+(\S+),@function", line)
        if m:
            cur = m.group(1)
            body[cur], loops[cur], mix = [], [], None
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
        if t.endswith(":"):  # a block label: the blocks of a loop say so in the label's comment
            mix = [0] * 6 if ("Loop" in line or "Depth" in line) else None
            if mix is not None:
                loops[cur].append(mix)
        elif mix is not None:
            mix[kind(t.split()[0])] += 1
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
        out[d] = dict(n=len(ins), text=body[n], loops=[m[:5] for m in loops[n]], vgpr=r.get("VGPRs"), scratch=r.get("ScratchSize [bytes/lane]"),
                      occ=r.get("Occupancy [waves/SIMD]"), lds=r.get("LDS Size [bytes/block]"))
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
        flags = "".join([" SCRATCH+" if int(b["scratch"]) > int(o["scratch"]) else "", " OCC-" if int(b["occ"]) < int(o["occ"]) else "",
                         " VGPR+" if int(b["vgpr"]) > int(o["vgpr"]) else "", " LDS!=" if b["lds"] != o["lds"] else ""])
        if not ident:
            flags = ("  loops same" if o["loops"] == b["loops"] else " LOOPS!=") + flags
        rows.append(f"{name}" + (f"\n    -> {to}" if to != name else "") +
                    f"\n    instr {o['n']} -> {b['n']}  vgpr {o['vgpr']} -> {b['vgpr']}  scratch {o['scratch']} -> {b['scratch']}  lds {o['lds']} -> {b['lds']}  waves/SIMD {o['occ']} -> {b['occ']}"
                    f"  {'identical' if ident else 'differs'}{flags}")
    print("\n".join(rows))
    print(f"\nidentical instruction streams ({len(same)} of {len(old)} kernels):")
    print("\n".join("  " + s for s in same))


main()
