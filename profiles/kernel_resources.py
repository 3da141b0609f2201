#!/usr/bin/env python3
"""VGPR / LDS / spill figures of every kernel in libpea_hip.so, from the code objects' metadata (no GPU needed).
The library is linked from several translation units, so its .hip_fatbin section holds one offload bundle per unit.
usage: kernel_resources.py [substring of the demangled name]
       kernel_resources.py --digest | --digest-families [path of another libpea_hip.so]
--digest prints one sorted line per kernel: mangled name, code size, SHA-256 of its code bytes, vgpr, sgpr, LDS, spill, scratch.  Two builds
whose listings are equal run the same device code with the same resources (what a host-side change has to show).
--digest-families condenses that listing (190 KB for 815 kernels) to one line per kernel template: name, instantiations, their code bytes,
SHA-256 of their --digest lines -- equal exactly where the full listings are equal; this is the form kept under profiles/."""
import hashlib, os, shutil, subprocess, sys, tempfile

LLVM = "/opt/rocm/lib/llvm/bin"
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


def code_objects(so, tmp):
    """paths of the gfx950 code objects unbundled from `so` (one per translation unit)"""
    fat = os.path.join(tmp, "fat.bin")
    subprocess.check_call([shutil.which("objcopy"), "-O", "binary", "--only-section=.hip_fatbin", so, fat])
    blob = open(fat, "rb").read()
    starts = []
    i = blob.find(MAGIC)
    while i >= 0:
        starts.append(i)
        i = blob.find(MAGIC, i + 1)
    out = []
    for n, s in enumerate(starts):
        e = starts[n + 1] if n + 1 < len(starts) else len(blob)
        part, co = os.path.join(tmp, "b%d.bin" % n), os.path.join(tmp, "k%d.co" % n)
        open(part, "wb").write(blob[s:e])
        subprocess.check_call([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", "--input=" + part,
                               "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--output=" + co])
        if os.path.getsize(co) > 0:
            out.append(co)
    return out


def code_bytes(co):
    """{symbol: bytes} of the functions in the .text of code object `co` (by the symbols' value and size)"""
    readelf = lambda flag: subprocess.run([os.path.join(LLVM, "llvm-readelf"), flag, "--wide", co], capture_output=True, text=True, check=True).stdout
    text = None  # (index, address, file offset) of .text
    for line in readelf("--sections").splitlines():
        f = line.replace("[", " ").replace("]", " ").split()
        if len(f) > 5 and f[1] == ".text":
            text = (f[0], int(f[3], 16), int(f[4], 16))
    blob, out = open(co, "rb").read(), {}
    for line in readelf("--symbols").splitlines():
        f = line.split()  # Num: Value Size Type Bind Vis Ndx Name
        if len(f) == 8 and f[3] == "FUNC" and text and f[6] == text[0]:
            start = text[2] + int(f[1], 16) - text[1]
            out[f[7]] = blob[start:start + int(f[2])]
    return out


def kernels(so, code=False):
    """[{name, vgpr, sgpr, lds, spill, scratch}] over all code objects of `so`; code: also `code`, the kernel's code bytes"""
    res = []
    with tempfile.TemporaryDirectory() as tmp:
        for co in code_objects(so, tmp):
            first, text = len(res), code_bytes(co) if code else {}
            notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", co], capture_output=True, text=True, check=True).stdout
            cur = None
            for line in notes.splitlines():
                line = line.strip()
                if line.startswith("- .agpr_count:") or line.startswith("- .args:"):
                    cur = {}
                    res.append(cur)
                if cur is None or ":" not in line:
                    continue
                k, v = line.lstrip("- ").split(":", 1)
                v = v.strip()
                key = {".name": "name", ".vgpr_count": "vgpr", ".sgpr_count": "sgpr", ".group_segment_fixed_size": "lds",
                       ".vgpr_spill_count": "spill", ".private_segment_fixed_size": "scratch", ".agpr_count": "agpr"}.get(k)
                if key and key not in cur:
                    cur[key] = v if key == "name" else int(v)
            for r in res[first:]:
                if code and "name" in r:
                    r["code"] = text[r["name"]]
    return [r for r in res if "name" in r and "vgpr" in r]


def family(mangled):
    """the kernel template's name: the length-prefixed identifiers at the head of the mangled name (L: internal linkage)"""
    if not mangled.startswith("_Z"):
        return mangled
    i, ids = 3 if mangled.startswith("_ZN") else 2, []
    while mangled[i:i + 1].isdigit() or mangled[i:i + 1] == "L":
        j = i = i + (mangled[i] == "L")
        while mangled[j].isdigit():
            j += 1
        i = j + int(mangled[i:j])
        ids.append(mangled[j:i])
    return "::".join(x for x in ids if x != "_GLOBAL__N_1")


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import __graft_entry__ as ge
    so = ge.load_package()._lib.SO_PATH
    if sys.argv[1:2] in (["--digest"], ["--digest-families"]):
        rows = ["%s %d %s vgpr %d sgpr %d lds %d spill %d scratch %d" % (k["name"], len(k["code"]), hashlib.sha256(k["code"]).hexdigest(),
                                                                         k["vgpr"], k["sgpr"], k["lds"], k["spill"], k.get("scratch", 0))
                for k in kernels(sys.argv[2] if len(sys.argv) > 2 else so, code=True)]
        rows.sort()
        if sys.argv[1] == "--digest-families":
            fams = {}
            for r in rows:
                fams.setdefault(family(r.split()[0]), []).append(r)
            rows = ["%s kernels %d bytes %d sha256 %s" % (f, len(rs), sum(int(r.split()[1]) for r in rs), hashlib.sha256("\n".join(rs).encode()).hexdigest())
                    for f, rs in sorted(fams.items())]
            rows.append("all kernels %d" % sum(len(rs) for rs in fams.values()))
        print("\n".join(rows))
        sys.exit(0)
    ks = kernels(so)
    dem = subprocess.run(["c++filt"] + [k["name"] for k in ks], capture_output=True, text=True).stdout.splitlines() if shutil.which("c++filt") else [k["name"] for k in ks]
    pat = sys.argv[1] if len(sys.argv) > 1 else ""
    print("%d kernels" % len(ks))
    for k, d in zip(ks, dem):
        if pat in d:
            print("vgpr %3d  spill %2d  scratch %3d  %s" % (k["vgpr"], k["spill"], k.get("scratch", 0), d[:150]))
