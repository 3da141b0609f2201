#!/usr/bin/env python3
"""Did a refactor change a hand-off?  Per kernel of libpea_hip.so: the count of LDS-DMA loads (buffer loads with the `lds` modifier),
the count of s_barrier, and the MULTISET of vmcnt immediates over all s_waitcnt that name vmcnt (and, apart, over those with an
s_barrier right behind them: the hand-offs, which the compiler neither writes nor moves) -- two libraries compared.  The
LDS-staged kernels hand their ring buffers over with `s_waitcnt vmcnt(N); s_barrier` for a literal N that counts the loads still
allowed in flight (csrc/pea_stage.h): where the code bytes moved (kernel_resources.py --digest), equal censuses say that every wait
still names the count it named, that no DMA and no barrier was gained or lost.  A difference is to be read in the disassembly: the
compiler may merge or split a wait of its own; an immediate that one of the hand-off functions produced must not move.

usage: kernel_sync_mix.py PARENT/libpea_hip.so [THIS/libpea_hip.so] [--show N]"""
import os
import re
import subprocess
import sys
import tempfile
from collections import Counter

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernel_fp_mix as fm  # noqa: E402
import kernel_resources as kr  # noqa: E402

VMCNT = re.compile(r"vmcnt\((\d+)\)")


def census(so):
    """kernel -> Counter over 'lds_dma', 'barrier', 'vmcnt(N)' and 'handoff(N)'"""
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for co in kr.code_objects(so, tmp):
            text = subprocess.run([fm.objdump(), "-d", "--no-show-raw-insn", co], capture_output=True, text=True, check=True).stdout
            cur, last_wait = None, None
            for line in text.splitlines():
                m = re.match(r"^[0-9a-f]+ <(\S+)>:", line)
                if m:
                    cur, last_wait = out.setdefault(m.group(1), Counter()), None
                    continue
                t = line.split()
                if cur is None or not t:
                    continue
                if t[0].startswith("buffer_load") and "lds" in t[1:]:
                    cur["lds_dma"] += 1
                elif t[0] == "s_barrier":
                    cur["barrier"] += 1
                elif t[0] == "s_waitcnt":
                    m = VMCNT.search(line)
                    if m:
                        cur["vmcnt(%s)" % m.group(1)] += 1
                        last_wait = m.group(1)
                        continue
                if t[0] == "s_barrier" and last_wait is not None:
                    cur["handoff(%s)" % last_wait] += 1  # a counted wait with the barrier right behind it: a hand-off, not a wait of the compiler's
                last_wait = None
    return out


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    show = int(sys.argv[sys.argv.index("--show") + 1]) if "--show" in sys.argv else 10
    if "--show" in sys.argv:
        args.remove(str(show))
    here = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "pixel-embedded-affinity_amd", "csrc", "libpea_hip.so")
    a, b = census(args[0]), census(args[1] if len(args) > 1 else here)
    only = sorted(set(a) ^ set(b))
    moved = sorted(k for k in set(a) & set(b) if a[k] != b[k])
    hand = [k for k in moved if any(x.startswith(("handoff", "lds_dma", "barrier")) for x in (a[k] - b[k]) + (b[k] - a[k]))]
    print("%d kernels, %d in one library only, %d with another synchronisation census (%d of them in the DMA, the barriers or the hand-offs)"
          % (len(set(a) | set(b)), len(only), len(moved), len(hand)))
    moved = hand + [k for k in moved if k not in hand]
    for k in only[:show]:
        print("only in the %s: %s" % ("first" if k in a else "second", k))
    for k in moved[:show]:
        print(k)
        print("   first only: %s   second only: %s" % (dict(a[k] - b[k]), dict(b[k] - a[k])))
    return 1 if moved or only else 0


if __name__ == "__main__":
    sys.exit(main())
