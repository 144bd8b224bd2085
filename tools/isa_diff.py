#!/usr/bin/env python3
"""Compare the gfx950 device assembly of two builds of one .hip file, kernel by kernel (CPU only).

    hipcc $(CXXFLAGS) --offload-device-only -S old/kernels_x.hip -o old.s      (likewise new.s)
    tools/isa_diff.py old.s new.s [--rename 'fused_bf16p_kernel<false, =fused_bf16p_kernel<']

Two compiles of the same source differ only in the __hip_cuid_ symbol, so "identical" below means the instruction
stream, the registers, the scratch and the LDS of a kernel are unchanged.  Kernels are matched by demangled name;
--rename OLD=NEW rewrites a substring of the OLD file's names first (a template parameter that was dropped).
The number of a function within its file is taken out of every block label, with or without the .L prefix: the loop
comments of the assembly ("Loop: Header=BB31_3") carry it too, and a kernel added or removed earlier in the file shifts it
for every later kernel, which would otherwise all report DIFFERS.
Exit status 1 if any kernel differs or is missing on either side.
"""
import argparse
import difflib
import re
import subprocess
import sys

FILT = "c++filt"
RES = ("next_free_vgpr", "accum_offset", "next_free_sgpr", "private_segment_fixed_size", "group_segment_fixed_size")


def kernels(path, renames):
    text = open(path).read()
    names = sorted(set(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, re.M)), key=len, reverse=True)
    dem = subprocess.run([FILT] + names, capture_output=True, text=True, check=True).stdout.split("\n") if names else []
    out = {}
    for mangled, d in zip(names, dem):
        d = re.sub(r"\(.*$", "", d).replace("void ", "")
        for old, new in renames:
            d = d.replace(old, new)
        body = re.search(r"^%s:[^\n]*\n(.*?)^\.Lfunc_end\d+:" % re.escape(mangled), text, re.M | re.S).group(1)
        desc = re.search(r"\.amdhsa_kernel\s+%s\n(.*?)\.end_amdhsa_kernel" % re.escape(mangled), text, re.S).group(1)
        norm = lambda s: re.sub(r"BB\d+_", "BB_", s.replace(mangled, "KERNEL"))
        res = {k: re.search(r"\.amdhsa_%s\s+(\S+)" % k, desc).group(1) for k in RES}
        out[d] = (norm(body).split("\n"), norm(desc).split("\n"), res)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--rename", action="append", default=[], help="OLD=NEW substring rewrite of the old file's demangled names")
    ap.add_argument("--show", type=int, default=0, help="print up to this many diff lines per differing kernel")
    a = ap.parse_args()
    old = kernels(a.old, [r.split("=", 1) for r in a.rename])
    new = kernels(a.new, [])
    bad = 0
    for name in sorted(set(old) | set(new)):
        if name not in old or name not in new:
            print("%-9s %s" % ("only-old" if name in old else "only-new", name))
            bad += 1
            continue
        (ob, od, ores), (nb, nd, nres) = old[name], new[name]
        same = ob == nb and od == nd
        bad += not same
        fmt = lambda r: "vgpr+agpr %s (acc at %s) sgpr %s scratch %s lds %s" % tuple(r[k] for k in RES)
        print("%-9s %s\n          %s%s" % ("identical" if same else "DIFFERS", name, fmt(nres), "" if ores == nres else "   was: " + fmt(ores)))
        if not same:
            d = [l for l in difflib.unified_diff(ob + od, nb + nd, lineterm="", n=0) if not l.startswith(("---", "+++", "@@"))]
            print("          %d diff lines, %d -> %d instructions-and-labels" % (len(d), len(ob), len(nb)))
            for l in d[: a.show]:
                print("          " + l)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
