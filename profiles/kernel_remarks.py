#!/usr/bin/env python3
"""One sorted line per kernel from the compiler's own resource remarks (no GPU needed): VGPRs, AGPRs, SGPRs, SGPR / VGPR spills, scratch,
LDS and waves per SIMD -- what kernel_resources.py cannot read from a code object's metadata (AGPRs apart, SGPR spills, occupancy).
usage: hipcc <the flags of _lib.HIPCC_FLAGS> -c UNIT.hip -o /dev/null -Rpass-analysis=kernel-resource-usage 2> UNIT.txt   (per unit)
       kernel_remarks.py SUBSTRING UNIT.txt [UNIT.txt ...]      lines of the kernels whose mangled name contains SUBSTRING"""
import re
import subprocess
import sys

KEYS = ("VGPRs", "AGPRs", "TotalSGPRs", "SGPRs Spill", "VGPRs Spill", "ScratchSize [bytes/lane]", "LDS Size [bytes/block]", "Occupancy [waves/SIMD]")
LABELS = ("vgpr", "agpr", "sgpr", "sgpr_spill", "vgpr_spill", "scratch", "lds", "waves")

if __name__ == "__main__":
    pat = re.compile(r"remark:\s+(Function Name|%s): (\S+)" % "|".join(re.escape(k) for k in KEYS))
    rows, cur = [], None
    for path in sys.argv[2:]:
        for line in open(path, errors="replace"):
            m = pat.search(line)
            if m and m.group(1) == "Function Name":
                cur = {"name": m.group(2)}
                rows.append(cur)
            elif m and cur is not None:
                cur[m.group(1)] = m.group(2)
    rows = [r for r in rows if sys.argv[1] in r["name"]]
    # binutils' c++filt does not know DF16b (__bf16): the builtin Dh (half) stands in for it, __half is a class and keeps its name
    dem = subprocess.run(["c++filt"] + [r["name"].replace("DF16b", "Dh") for r in rows], capture_output=True, text=True, check=True).stdout.splitlines()
    out = []
    for r, d in zip(rows, dem):
        d = re.sub(r"\(.*$", "", re.sub(r"^void pea::(\(anonymous namespace\)::)?", "", d)).replace("half", "__bf16").replace("____bf16", "__half")
        out.append(d + "  " + " ".join("%s %s" % (lab, r[k]) for lab, k in zip(LABELS, KEYS)))
    print("\n".join(sorted(out)))
