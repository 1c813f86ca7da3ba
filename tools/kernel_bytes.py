#!/usr/bin/env python3
"""kernel_bytes.py A B [--find NAME ...] -- "the kernels did not change", stated on the CPU.

A and B are shared libraries or object files built by csrc/Makefile.  Every gfx950 code object is unbundled from their
.hip_fatbin section (a linked library holds one bundle a translation unit), and every kernel of it is read twice: its
machine code, by its symbol, and its descriptor figures from the code object's notes (VGPRs, AGPRs, SGPRs, LDS bytes,
scratch bytes, spills, kernel-argument bytes).  Four groups are printed: the kernels identical in both, those whose
bytes or figures differ, those only in A, those only in B; the exit status is 0 only when all but the first are empty.

Bytes and names are compared, nothing is disassembled.  Kernels of an anonymous namespace may carry one name in several
units, so a library holds a MULTISET of (name, bytes, figures): copies of A are paired with equal copies of B first, the
rest of a name pairwise as "differ", and what is left over is "only in".

--find NAME: NAME (a substring of a mangled kernel name) must occur in both; a name that is missing is an error.

Needs llvm-objcopy, clang-offload-bundler and llvm-readelf of the ROCm tree ($ROCM_PATH, default /opt/rocm); no GPU.
"""
import argparse
import hashlib
import os
import re
import subprocess
import sys
import tempfile
from collections import defaultdict

LLVM = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "llvm", "bin")
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"
FIGURES = ("vgpr_count", "agpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size",
           "vgpr_spill_count", "sgpr_spill_count", "kernarg_segment_size")


def tool(name, *args):
    return subprocess.run([os.path.join(LLVM, name), *args], check=True, capture_output=True, text=True).stdout


def code_objects(path, tmp):
    """the gfx950 code objects of `path`, as files under tmp"""
    fat = os.path.join(tmp, "fatbin")
    tool("llvm-objcopy", "-O", "binary", "--only-section=.hip_fatbin", path, fat)
    data = open(fat, "rb").read() if os.path.exists(fat) else b""
    starts = [m.start() for m in re.finditer(re.escape(MAGIC), data)]
    if not starts:
        sys.exit(f"{path}: no offload bundle in .hip_fatbin")
    out = []
    for k, (lo, hi) in enumerate(zip(starts, starts[1:] + [len(data)])):
        bundle, co = os.path.join(tmp, f"bundle{k}"), os.path.join(tmp, f"code{k}.co")
        with open(bundle, "wb") as fh:
            fh.write(data[lo:hi])
        if TARGET not in tool("clang-offload-bundler", "--list", "--type=o", f"--input={bundle}").split():
            continue
        tool("clang-offload-bundler", "--unbundle", "--type=o", f"--targets={TARGET}", f"--input={bundle}", f"--output={co}")
        if os.path.getsize(co):
            out.append(co)
    return out


def kernels_of(co):
    """[(name, sha256 of the machine code, size, {figure: value})] of one code object"""
    figures, name, cur = {}, None, {}
    for line in tool("llvm-readelf", "--notes", co).splitlines():
        m = re.match(r"\s+(- )?\.(\w+):\s+(\S+)\s*$", line)
        if not m:
            continue
        if m.group(1) and line.startswith("  - "):      # the first key of the next kernel
            if name:
                figures[name] = cur
            name, cur = None, {}
        if m.group(2) == "name" and line.startswith("    .name:"):
            name = m.group(3)
        elif m.group(2) in FIGURES and (line.startswith("    .") or line.startswith("  - .")):
            cur[m.group(2)] = int(m.group(3))
    if name:
        figures[name] = cur
    sections = {}
    for line in tool("llvm-readelf", "-S", "-W", co).splitlines():
        m = re.match(r"\s*\[\s*(\d+)\]\s+\S+\s+\S+\s+([0-9a-f]+)\s+([0-9a-f]+)\s+([0-9a-f]+)", line)
        if m:
            sections[int(m.group(1))] = (int(m.group(2), 16), int(m.group(3), 16), int(m.group(4), 16))
    blob = open(co, "rb").read()
    found = {}
    for line in tool("llvm-readelf", "-s", "-W", co).splitlines():
        f = line.split()
        if len(f) == 8 and f[3] == "FUNC" and f[7] in figures and f[6].isdigit():
            addr, off, size = sections[int(f[6])]
            at, n = int(f[1], 16) - addr + off, int(f[2])
            found[f[7]] = (hashlib.sha256(blob[at:at + n]).hexdigest(), n)
    missing = set(figures) - set(found)
    if missing:
        sys.exit(f"{co}: no code symbol for {sorted(missing)}")
    return [(k, found[k][0], found[k][1], figures[k]) for k in figures]


def kernels(path):
    with tempfile.TemporaryDirectory() as tmp:
        return [k for co in code_objects(path, tmp) for k in kernels_of(co)]


def describe(k):
    return f"{k[2]} B " + " ".join(f"{f}={k[3].get(f)}" for f in FIGURES) + f" sha256={k[1][:12]}"


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("a")
    ap.add_argument("b")
    ap.add_argument("--find", action="append", default=[], metavar="NAME")
    ap.add_argument("--quiet", action="store_true", help="counts alone for the identical group")
    args = ap.parse_args()
    by_name = [defaultdict(list), defaultdict(list)]
    for side, path in enumerate((args.a, args.b)):
        for k in kernels(path):
            by_name[side][k[0]].append(k)
    same, differ, only_a, only_b = [], [], [], []
    for name in sorted(set(by_name[0]) | set(by_name[1])):
        a, b = list(by_name[0][name]), list(by_name[1][name])
        for k in list(a):
            twin = next((x for x in b if x[1:] == k[1:]), None)
            if twin:
                a.remove(k)
                b.remove(twin)
                same.append(k)
        while a and b:
            differ.append((a.pop(0), b.pop(0)))
        only_a += a
        only_b += b
    print(f"identical: {len(same)}")
    if not args.quiet:
        for k in same:
            print(f"  {k[0]}  {describe(k)}")
    print(f"differ: {len(differ)}")
    for ka, kb in differ:
        print(f"  {ka[0]}\n    A: {describe(ka)}\n    B: {describe(kb)}")
    for title, group in (("only in A", only_a), ("only in B", only_b)):
        print(f"{title}: {len(group)}")
        for k in group:
            print(f"  {k[0]}  {describe(k)}")
    status = 1 if differ or only_a or only_b else 0
    for want in args.find:
        for side, label in enumerate("AB"):
            if not any(want in name for name in by_name[side] if by_name[side][name]):
                print(f"not found in {label}: {want}")
                status = 1
    return status


if __name__ == "__main__":
    sys.exit(main())
