#!/usr/bin/env python3
"""Did a refactor move an f32 rounding?  Per kernel of libpea_hip.so the MULTISET of its floating-point VALU instructions (v_fma_f32,
v_mul_f32, v_sub_f32, v_pk_fma_f32, ...), two libraries compared.  The forwards leave expressions such as u * m - t * m to the default
contraction: whether the compiler makes it one fma or two products and a subtraction is decided per kernel, and shows in the bits as
soon as a mask holds anything but 0 and 1.  Equal code bytes (kernel_resources.py --digest) imply equal multisets; where the bytes
moved, equal multisets say that no product gained or lost its rounding (packed and scalar forms count apart: v_pk_fma_f32 is two
v_fma_f32).

usage: kernel_fp_mix.py PARENT/libpea_hip.so [THIS/libpea_hip.so] [--show N]"""
import os
import re
import shutil
import subprocess
import sys
import tempfile
from collections import Counter

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernel_resources as kr  # noqa: E402

FP = re.compile(r"^v_(pk_)?(fma|fmac|mul|sub|subrev|add|mad|mac|max|min|rcp|rsq|sqrt|log|exp|div_\w+|cvt|ldexp|frexp_\w+|dot\w*)_?\w*(f32|f16|f64|bf16)\w*")
UNPACK = {"v_pk_fma_f32": ("v_fma_f32", 2), "v_pk_mul_f32": ("v_mul_f32", 2), "v_pk_add_f32": ("v_add_f32", 2),
          "v_cvt_pk_f16_f32": ("v_cvt_f16_f32", 2), "v_cvt_f16_f32_e32": ("v_cvt_f16_f32", 1), "v_cvt_f16_f32_sdwa": ("v_cvt_f16_f32", 1)}
ALIAS = {"v_fmac_f32_e32": "v_fma_f32", "v_fmac_f32_e64": "v_fma_f32", "v_mul_f32_e32": "v_mul_f32", "v_mul_f32_e64": "v_mul_f32",
         "v_add_f32_e32": "v_add_f32", "v_add_f32_e64": "v_add_f32", "v_sub_f32_e32": "v_sub_f32", "v_sub_f32_e64": "v_sub_f32",
         "v_subrev_f32_e32": "v_sub_f32", "v_subrev_f32_e64": "v_sub_f32", "v_fmac_f32_dpp": "v_fma_f32"}


def objdump():
    return shutil.which("llvm-objdump") or os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "llvm-objdump")


def mixes(so):
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for co in kr.code_objects(so, tmp):
            text = subprocess.run([objdump(), "-d", "--no-show-raw-insn", co], capture_output=True, text=True, check=True).stdout
            cur = None
            for line in text.splitlines():
                m = re.match(r"^[0-9a-f]+ <(\S+)>:", line)
                if m:
                    cur = out.setdefault(m.group(1), Counter())
                    continue
                t = line.split()
                if cur is not None and t and FP.match(t[0]):
                    name, n = UNPACK.get(t[0], (ALIAS.get(t[0], t[0]), 1))
                    if t[0] == "v_pk_add_f32" and "neg_lo:[" in line:  # a negated source in both halves: a - b as a + (-b), or
                        neg = re.search(r"neg_lo:\[([01,]+)\] neg_hi:\[\1\]", line)  # (-a) + (-0), the packed form of a sign flip
                        if neg and neg.group(1) in ("0,1", "1,0"):
                            name = "v_sub_f32"
                        elif neg and neg.group(1) == "1,1" and t[3].rstrip(",") == "0":
                            continue
                    cur[name] += n
    return out


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    show = int(sys.argv[sys.argv.index("--show") + 1]) if "--show" in sys.argv else 10
    if "--show" in sys.argv:
        args.remove(str(show))
    here = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "pixel-embedded-affinity_amd", "csrc", "libpea_hip.so")
    a, b = mixes(args[0]), mixes(args[1] if len(args) > 1 else here)
    only = sorted(set(a) ^ set(b))
    moved = sorted(k for k in set(a) & set(b) if a[k] != b[k])
    print("%d kernels, %d in one library only, %d with another floating-point multiset" % (len(set(a) | set(b)), len(only), len(moved)))
    for k in moved[:show]:
        print(k)
        print("   first only: %s   second only: %s" % (dict(a[k] - b[k]), dict(b[k] - a[k])))
    return 1 if moved or only else 0


if __name__ == "__main__":
    sys.exit(main())
