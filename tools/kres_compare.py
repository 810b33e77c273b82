#!/usr/bin/env python3
"""Kernel resources of one .hip file on two trees, side by side (no GPU): -Rpass-analysis=kernel-resource-usage for gfx950 with the
library's flags (csrc/Makefile), per instantiation VGPRs, AGPRs, scratch, VGPR spills, occupancy and SGPRs, and the verdict on the
instantiations both trees have.

    git archive HEAD nsa_vibe_amd/csrc include | tar -x -C /tmp/parent
    python tools/kres_compare.py /tmp/parent/nsa_vibe_amd/csrc/layer_fused.hip nsa_vibe_amd/csrc/layer_fused.hip \
        > profiles/layer_decode_paged/resources.txt

Trailing template flags at their default (false) are dropped from the names, so a flag added at the end of a parameter list keeps the
parent's name for the instantiations the parent has."""
import argparse
import re
import subprocess

FLAGS = ["-O3", "-std=c++17", "--offload-arch=gfx950", "-fPIC", "-fvisibility=hidden", "-ffp-contract=off", "-mllvm", "-amdgpu-mfma-vgpr-form=1",
         "-fno-slp-vectorize"]
KEYS = (("VGPRs", "VGPRs"), ("AGPRs", "AGPRs"), ("ScratchSize [bytes/lane]", "B scratch"), ("VGPRs Spill", "VGPR spills"),
        ("Occupancy [waves/SIMD]", "occupancy"), ("TotalSGPRs", "SGPRs"), ("LDS Size [bytes/block]", "B LDS"))
HARD = ("VGPRs", "AGPRs", "ScratchSize [bytes/lane]", "VGPRs Spill", "Occupancy [waves/SIMD]")


def resources(src):
    err = subprocess.run(["/opt/rocm/bin/hipcc", *FLAGS, "-c", src, "-o", "/dev/null", "-Rpass-analysis=kernel-resource-usage"], capture_output=True,
                         text=True).stderr
    names, rows, cur = [], {}, None
    for line in err.splitlines():
        m = re.search(r"remark:\s+(.*?)\s*\[-Rpass", line)
        if not m:
            continue
        t = m.group(1)
        if t.startswith("Function Name:"):
            cur = t.split(":", 1)[1].strip()
            names.append(cur)
            rows[cur] = {}
        elif cur and ":" in t:
            k, v = t.split(":", 1)
            rows[cur][k.strip()] = v.strip()
    # (binutils' c++filt does not know the 16-bit float types DF16b / DF16_: demangle with the half type in their place -- a builtin like
    # them, so the back references keep their numbers -- and put the element type's name back afterwards)
    half = [n.replace("DF16b", "Dh").replace("DF16_", "Dh") for n in names]
    plain = subprocess.run(["c++filt"], input="\n".join(half), capture_output=True, text=True).stdout.splitlines()
    out = {}
    for mangled, name in zip(names, plain):
        elt = "bf16" if "DF16b" in mangled else "f16 "
        name = re.sub(r"^void ", "", name).replace("nsa::", "").replace("half", elt)
        depth, cut = 0, len(name)
        for i, ch in enumerate(name):  # cut the parameter list: the first '(' outside the template arguments
            depth += ch == "<"
            depth -= ch == ">"
            if ch == "(" and depth == 0:
                cut = i
                break
        name = name[:cut]
        while re.search(r", false\s*>", name):  # trailing flags at their default: a flag added at the end of a list keeps the parent's name
            name = re.sub(r", false\s*>", ">", name)
        out[name] = rows[mangled]
    return out


def line(r):
    return ", ".join(f"{r.get(k, '?'):>4} {label}" for k, label in KEYS)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("parent")
    ap.add_argument("now")
    a = ap.parse_args()
    parent, now = resources(a.parent), resources(a.now)
    padded = parent
    hard = soft = True
    for name in sorted(set(padded) | set(now)):
        print(name)
        if name in padded:
            print(f"    parent: {line(padded[name])}")
        if name in now:
            print(f"    {'now   ' if name in padded else 'new   '}: {line(now[name])}")
        if name in padded and name in now:
            hard &= all(padded[name].get(k) == now[name].get(k) for k in HARD)
            soft &= all(padded[name].get(k) == now[name].get(k) for k, _ in KEYS)
        elif name in padded:
            print("    (gone)")
            hard = False
    print()
    print(f"all existing instantiations keep VGPRs, AGPRs, scratch, VGPR spills and occupancy: {hard}")
    print(f"all existing instantiations keep SGPRs and LDS as well: {soft}")


if __name__ == "__main__":
    main()
