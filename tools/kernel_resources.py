#!/usr/bin/env python3
"""Per-kernel resources of the gfx950 code objects in libdiffpool_hip.so: code bytes, VGPRs, AGPRs, VGPR / SGPR spills
and scratch (private segment) bytes per lane.  Needs only the ROCm LLVM tools, no GPU:

    llvm-objcopy --dump-section .hip_fatbin=F libdiffpool_hip.so     (one offload bundle per translation unit)
    clang-offload-bundler --unbundle --type=o --targets=hipv4-amdgcn-amd-amdhsa--gfx950
    llvm-readelf --notes (kernel metadata)  and  -s (code symbol sizes)

    python3 tools/kernel_resources.py [--lib PATH] [--filter SUBSTRING]
"""
import argparse
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULT_LIB = os.path.join(ROOT, "graph_pooling_amd", "libdiffpool_hip.so")
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"
BUNDLE_MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"
TOOLS = ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf")
NOTE_KEYS = {".vgpr_count": "vgprs", ".agpr_count": "agprs", ".vgpr_spill_count": "vgpr_spills",
             ".sgpr_spill_count": "sgpr_spills", ".private_segment_fixed_size": "scratch", ".sgpr_count": "sgprs",
             ".group_segment_fixed_size": "lds_static"}


def find_tool(name):
    """The ROCm LLVM tool `name` (ROCM_PATH/llvm/bin first, then PATH), or None."""
    for d in (os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin"),):
        p = os.path.join(d, name)
        if os.access(p, os.X_OK):
            return p
    return shutil.which(name)


def tools_available():
    return all(find_tool(t) for t in TOOLS)


def _run(args):
    return subprocess.run(args, check=True, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True).stdout


def demangle_short(sym):
    """_ZN2dp12_GLOBAL__N_112k_level0_fwdILi3EEEvNS0_6L0ArgsE -> k_level0_fwd<3> (enough for this project's names)."""
    s = sym                                    # the length-prefixed name after the (anonymous) namespace
    pos = s.find("_GLOBAL__N_1")
    pos = pos + len("_GLOBAL__N_1") if pos >= 0 else (s.find("N2dp") + 4 if s.find("N2dp") >= 0 else -1)
    if pos < 0:
        return sym
    mm = re.match(r"(\d+)", s[pos:])
    if not mm:
        return sym
    n = int(mm.group(1))
    start = pos + len(mm.group(1))
    name = s[start:start + n]
    rest = s[start + n:]
    targs = re.match(r"I((?:Li-?\d+E|Lb[01]E)+)E", rest)
    if targs:
        vals = re.findall(r"L[ib](-?\d+)E", targs.group(1))
        name += "<" + ",".join(vals) + ">"
    return name


def _parse_notes(text):
    """kernel metadata maps of `llvm-readelf --notes` -> {symbol (no .kd): {field: int}}."""
    out = {}
    entries = re.split(r"\n  - ", text)
    for e in entries:
        fields, sym = {}, None
        for line in e.splitlines():
            m = re.match(r"\s*(\.[a-z_]+):\s+(\S+)\s*$", line)
            if not m:
                continue
            k, v = m.group(1), m.group(2)
            if k == ".symbol" and v.endswith(".kd"):
                sym = v[:-3]
            elif k in NOTE_KEYS and line.startswith("    ") and not line.startswith("      "):
                fields[NOTE_KEYS[k]] = int(v)
        if sym:
            out[sym] = fields
    return out


def _parse_symbols(text):
    """FUNC symbols of `llvm-readelf -s --wide` -> {symbol: code bytes}."""
    out = {}
    for line in text.splitlines():
        p = line.split()
        if len(p) >= 8 and p[3] == "FUNC":
            out[p[7]] = int(p[2], 0)
    return out


def kernel_resources(lib=DEFAULT_LIB):
    """{mangled kernel symbol: {"name", "code_bytes", "vgprs", "agprs", "vgpr_spills", "sgpr_spills", "scratch", ...}}
    over every gfx950 code object bundled into `lib`."""
    objcopy, bundler, readelf = (find_tool(t) for t in TOOLS)
    res = {}
    with tempfile.TemporaryDirectory() as td:
        fat = os.path.join(td, "fatbin")
        _run([objcopy, "--dump-section", ".hip_fatbin=" + fat, lib, os.path.join(td, "stripped")])
        data = open(fat, "rb").read()
        offs = [m.start() for m in re.finditer(re.escape(BUNDLE_MAGIC), data)] + [len(data)]
        for i in range(len(offs) - 1):
            bpath, cpath = os.path.join(td, "b%d" % i), os.path.join(td, "c%d" % i)
            with open(bpath, "wb") as f:
                f.write(data[offs[i]:offs[i + 1]])
            listed = _run([bundler, "--list", "--type=o", "--input=" + bpath]).split()
            if TARGET not in listed:
                continue
            _run([bundler, "--unbundle", "--type=o", "--targets=" + TARGET, "--input=" + bpath, "--output=" + cpath])
            notes = _parse_notes(_run([readelf, "--notes", cpath]))
            sizes = _parse_symbols(_run([readelf, "-s", "--wide", cpath]))
            for sym, fields in notes.items():
                d = dict(fields)
                d["code_bytes"] = sizes.get(sym, 0)
                d["name"] = demangle_short(sym)
                res[sym] = d
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--lib", default=DEFAULT_LIB)
    ap.add_argument("--filter", default="", help="only kernels whose short name contains this")
    args = ap.parse_args()
    if not tools_available():
        sys.exit("kernel_resources: the ROCm LLVM tools (%s) were not found" % ", ".join(TOOLS))
    res = kernel_resources(args.lib)
    rows = sorted((d for d in res.values() if args.filter in d["name"]), key=lambda d: d["name"])
    print("%-40s %10s %6s %6s %11s %11s %8s" % ("kernel", "code_B", "vgpr", "agpr", "vgpr_spill", "sgpr_spill", "scratch"))
    for d in rows:
        print("%-40s %10d %6d %6d %11d %11d %8d" % (d["name"][:40], d["code_bytes"], d.get("vgprs", 0), d.get("agprs", 0),
                                                   d.get("vgpr_spills", 0), d.get("sgpr_spills", 0), d.get("scratch", 0)))


if __name__ == "__main__":
    main()
