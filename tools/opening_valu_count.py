#!/usr/bin/env python3
"""opening_valu_count.py [LIB] [--kernel SUBSTRING] [--json] -- the VALU count of the deferred opening, on the CPU.

LIB (default: the built product library) is unbundled the way kernel_bytes.py does it, the gfx950 code object that
holds the kernel is disassembled with llvm-objdump, and the kernel's text is cut into straight-line blocks as the labels
of a compiler listing cut it (tools/isa_blocks.py): a block begins at every branch target and after s_branch, s_endpgm
or s_setpc.  A conditional branch that only skips a masked region when no lane is in it (s_cbranch_execz over a park)
does not end a block: the wave falls through it nearly always and issues the region's instructions.

The lock-step deferred opening (connect_kernels.hip: open_games_deferred) is inlined where the grouped rollout kernel
opens games: inside a step (seven calls of eight at 512 games a wave) and, further down in the text, where a wave
moves on to the next step.  Stage 1 of a copy is a block with the three philox calls (>= 40 of v_mad_u64_u32 /
v_mul_hi_u32; nothing else in the kernel comes near), stage 2 the next block with the three sub-draw multiplies
(v_mul_lo_u32).  Printed: the VALU counts of the two blocks of every copy -- the count of v_* mnemonics, nothing else --
and the sum; "the opening's count" is the first copy's.

Needs llvm-objcopy, clang-offload-bundler, llvm-readelf and llvm-objdump of the ROCm tree ($ROCM_PATH, default
/opt/rocm); no GPU.
"""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernel_bytes  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULT_LIB = os.path.join(REPO, "board-game-simulator-python_amd", "libbgs.so")
# k_connect_rollout_opened_steps<Geo<1,6,7,4>, 3, true>: the kernel the executor launches for the bench
DEFAULT_KERNEL = "k_connect_rollout_opened_stepsINS0_3GeoILi1ELi6ELi7ELi4EEELi3ELb1EEE"
WIDE_MULTIPLIES = ("v_mad_u64_u32", "v_mul_hi_u32")
BLOCK_ENDS = ("s_branch", "s_endpgm", "s_setpc")
PHILOX_MULTIPLIES = 40   # three calls of ten rounds of two; a refetch (one call) and the plies stay far below


def kernel_text(lib, want):
    """[(address, mnemonic, operands)] of the one kernel of `lib` whose mangled name contains `want`"""
    with tempfile.TemporaryDirectory() as tmp:
        for co in kernel_bytes.code_objects(lib, tmp):
            names = [k[0] for k in kernel_bytes.kernels_of(co) if want in k[0]]
            if not names:
                continue
            if len(names) > 1:
                sys.exit(f"{lib}: {want} names {len(names)} kernels")
            out = subprocess.run([os.path.join(kernel_bytes.LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn",
                                  f"--disassemble-symbols={names[0]}", co], check=True, capture_output=True, text=True).stdout
            text = []
            for line in out.splitlines():
                m = re.match(r"\s+(\S+)((?:\s+[^/]*)?)//\s*([0-9A-Fa-f]+):", line)
                if m and re.match(r"[a-z]\w*$", m.group(1)):
                    text.append((int(m.group(3), 16), m.group(1), m.group(2).strip()))
            if not text:
                sys.exit(f"{lib}: no instructions read for {names[0]}")
            return names[0], text
    sys.exit(f"{lib}: no kernel named *{want}*")


def straight_line_blocks(text):
    """the kernel's text cut in front of every branch target and after every unconditional transfer"""
    targets = set()
    for addr, mnem, ops in text:
        if mnem.startswith(("s_branch", "s_cbranch")):
            # llvm-objdump resolves the target: "s_cbranch_scc1 65532 <symbol+0x1234>"; without a symbol: the 16-bit offset
            m = re.search(r"<[^>+]*\+0x([0-9A-Fa-f]+)>", ops)
            if m:
                targets.add(("off", int(m.group(1), 16)))
            else:
                imm = int(ops.split()[-1], 0)
                imm = imm - 0x10000 if imm >= 0x8000 else imm
                targets.add(("abs", addr + 4 + 4 * imm))
    base = text[0][0]
    starts = {a if kind == "abs" else base + a for kind, a in targets}
    blocks, cur = [], []
    for addr, mnem, ops in text:
        if addr in starts and cur:
            blocks.append(cur)
            cur = []
        cur.append((addr, mnem, ops))
        if mnem.startswith(BLOCK_ENDS):
            blocks.append(cur)
            cur = []
    if cur:
        blocks.append(cur)
    return blocks


def valu(block):
    return sum(1 for _, mnem, _ in block if mnem.startswith("v_"))


def opening_blocks(lib, want=DEFAULT_KERNEL):
    """(kernel name, [(VALU of stage 1's block, VALU of stage 2's block) of every copy, in text order])"""
    name, text = kernel_text(lib, want)
    copies, stage1 = [], None
    for block in straight_line_blocks(text):
        wide = sum(1 for _, mnem, _ in block if mnem.startswith(WIDE_MULTIPLIES))
        subdraws = sum(1 for _, mnem, _ in block if mnem.startswith("v_mul_lo_u32"))
        if wide >= PHILOX_MULTIPLIES:
            if stage1 is not None:
                sys.exit(f"{lib}: {name}: two philox blocks in a row, no stage 2 between them")
            stage1 = valu(block)
        elif stage1 is not None and subdraws >= 3:
            copies.append((stage1, valu(block)))
            stage1 = None
    if not copies or stage1 is not None:
        sys.exit(f"{lib}: {name}: no complete copy of the deferred opening found")
    return name, copies


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("lib", nargs="?", default=DEFAULT_LIB)
    ap.add_argument("--kernel", default=DEFAULT_KERNEL, help="substring of the mangled kernel name")
    ap.add_argument("--json", action="store_true")
    args = ap.parse_args()
    name, copies = opening_blocks(args.lib, args.kernel)
    if args.json:
        print(json.dumps({"kernel": name, "copies": [list(c) for c in copies], "sum": sum(copies[0])}))
    else:
        print(name)
        for k, (one, two) in enumerate(copies):
            print(f"  opening copy {k}, VALU: {one} + {two} = {one + two}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
