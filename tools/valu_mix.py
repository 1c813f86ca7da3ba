#!/usr/bin/env python3
"""Issue cost of a kernel's instruction mix: the VALU instructions of its two hot basic blocks (the opening stage and the
rollout loop body of K2o; tools/collect_profiles.py weights them by how often each runs) weighted by the per-instruction issue costs measured on gfx950 with tools/ubench.hip (4 waves per SIMD; committed as
profiles/r01_ubench_valu_issue.txt).  mix_cycles_per_instruction feeds bench.py's `valu_issue.mix_ceiling`: the rate
the VALU could sustain on THIS mix, as opposed to the guide's 2-cycle SIMD-32 peak that only plain VOP2 streams reach.

    python tools/valu_mix.py            (compiles connect_kernels.hip to ISA with hipcc, prints JSON)
    python tools/valu_mix.py DIR        (the same for the csrc directory of another checkout, e.g. the parent commit's)"""
import json, os, re, subprocess, sys, tempfile
from collections import Counter

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from isa_blocks import blocks  # noqa: E402

# cycles per wave64 instruction per SIMD at 4 waves per SIMD (profiles/r01_ubench_valu_issue.txt); classes not
# measured individually take the cost of their class's measured member
COST = {
    "v_add_u32": 2.85, "v_sub_u32": 2.85, "v_subrev_u32": 2.85, "v_and_b32": 2.79, "v_or_b32": 2.79, "v_xor_b32": 2.79,
    "v_not_b32": 2.79, "v_mov_b32": 2.79, "v_lshrrev_b32": 2.58, "v_lshlrev_b32": 2.58, "v_ashrrev_i32": 2.58,
    "v_alignbit_b32": 4.46, "v_bcnt_u32_b32": 4.45, "v_mul_lo_u32": 4.73, "v_mul_hi_u32": 4.42, "v_bfe_u32": 4.25,
    "v_ffbl_b32": 4.23, "v_ffbh_u32": 4.23, "v_bitop3_b32": 4.06, "v_and_or_b32": 4.49, "v_or3_b32": 4.49,
    "v_lshl_add_u32": 4.55, "v_lshl_or_b32": 4.55, "v_add3_u32": 4.55, "v_add_lshl_u32": 4.55, "v_mad_u32_u24": 4.90,
    "v_mul_u32_u24": 4.90, "v_perm_b32": 4.75, "v_xad_u32": 4.73, "v_lshrrev_b64": 4.60, "v_lshlrev_b64": 4.73,
    "v_mad_u64_u32": 5.25, "v_lshl_add_u64": 4.85, "v_mov_b64": 4.39, "v_cndmask_b32": 3.5, "v_readfirstlane_b32": 4.0,
    "v_mbcnt_lo_u32_b32": 4.45, "v_mbcnt_hi_u32_b32": 4.45, "v_add_co_u32": 4.0, "v_addc_co_u32": 4.0,
}
CMP_COST = 3.5  # v_cmp_* (+ its v_cndmask partner: 7.09 per pair measured)
DEFAULT = 4.4   # unlisted VOP3


def block_mix(body):
    ops = Counter()
    for line in body:
        op = line.split()[0]
        if op.startswith("v_"):
            ops[re.sub(r"_(e32|e64|dpp|sdwa)$", "", op)] += 1
    total = sum(ops.values())
    cycles = sum(n * (CMP_COST if op.startswith("v_cmp") else COST.get(op, DEFAULT)) for op, n in ops.items())
    return {"valu_instructions": total, "mix_cycles_per_instruction": cycles / total, "top_opcodes": dict(ops.most_common(12))}


def straight_line_region(all_blocks, first):
    """The blocks a wave runs through from block `first` on without a scalar decision: a block is followed by the next
    one in layout as long as its only branch is an `s_cbranch_execz` to that next block -- a store under the lane mask
    (the deferred opening parks its games that way: its stages are one region, not one basic block)."""
    region = [first]
    while region[-1] + 1 < len(all_blocks):
        name_next = all_blocks[region[-1] + 1][0]
        branches = [l.split() for l in all_blocks[region[-1]][1] if l.startswith(("s_cbranch", "s_branch", "s_setpc", "s_endpgm"))]
        if not branches or any(b[0] != "s_cbranch_execz" or b[1] != name_next for b in branches):
            break
        region.append(region[-1] + 1)
    return region


def mix(path, sym):
    """The two hot pieces of K2o: the opening stage (run once per 64 games; since the deferred opening a straight-line
    region of several basic blocks) and the 4-ply loop body (the largest block outside it)."""
    all_blocks = blocks(path, sym)
    order = sorted(range(len(all_blocks)), key=lambda i: -len(all_blocks[i][1]))
    region = straight_line_region(all_blocks, order[0])
    second = next(i for i in order if i not in region)
    opening = block_mix([l for i in region for l in all_blocks[i][1]])
    loop = block_mix(all_blocks[second][1])
    if opening["valu_instructions"] < loop["valu_instructions"]:
        opening, loop = loop, opening
    else:
        opening["basic_blocks"] = {all_blocks[i][0]: block_mix(all_blocks[i][1])["valu_instructions"] for i in region}
    return {"opening_block": opening, "loop_body": loop,
            # (kept for readers of round-2 files: the loop body's figures under the old names)
            "valu_instructions_in_loop_body": loop["valu_instructions"],
            "mix_cycles_per_instruction": loop["mix_cycles_per_instruction"]}


BRANCHES = ("s_cbranch", "s_branch", "s_setpc", "s_endpgm")


def basic_blocks(path, sym):
    """True basic blocks of a kernel: isa_blocks splits at labels only, this splits after every branch as well.  Returns
    (names, bodies, successors): a block that ends in a conditional branch goes on to its target and to the next block."""
    names, bodies, labels = [], [], {}
    for name, body in blocks(path, sym):
        labels[name] = len(names)
        part, k = [], 0
        for line in body:
            part.append(line)
            if line.startswith(BRANCHES):
                names.append(name if k == 0 else f"{name}+{k}"); bodies.append(part); part = []; k += 1
        if part or k == 0:
            names.append(name if k == 0 else f"{name}+{k}"); bodies.append(part)
    succ = []
    for i, body in enumerate(bodies):
        last = body[-1].split() if body else [""]
        nxt = [i + 1] if i + 1 < len(bodies) else []
        if last[0] == "s_branch":
            succ.append([labels[last[1]]])
        elif last[0].startswith("s_cbranch"):
            succ.append([labels[last[1]]] + nxt)
        elif last[0].startswith(("s_endpgm", "s_setpc")):
            succ.append([])
        else:
            succ.append(nxt)
    return names, bodies, succ


def iteration_path(path, sym):
    """The VALU instructions a wave issues in ONE iteration of the refill loop in its steady state (docs/EXPERIMENTS.md §29):
    idle lanes take a game out of the pool (no opening), the block of four plies is played (no refetch), some lane's game
    ends and leaves its outcome byte (no board goes to memory where the kernel can tell that none does), nothing is
    flushed.  Found as the cheapest cycle, in VALU instructions, through three kinds of basic block:
      * a `take`: two ds_read_b128 of a pool slot's words, at most 30 VALU;
      * the loop body: four full plies, i.e. four v_mad_u64_u32;
      * the game-end block: a ds_write_b8 of the outcome byte behind the popcounts of the planes, at most 30 VALU.
    Every other block on the cycle is there because control passes through it whatever the lanes decide."""
    names, bodies, succ = basic_blocks(path, sym)
    ops = [[l.split()[0] for l in b] for b in bodies]
    valu = [sum(1 for o in b if o.startswith("v_")) for b in ops]
    takes = [i for i, b in enumerate(ops) if b.count("ds_read_b128") >= 2 and valu[i] <= 30]
    loops = [i for i, b in enumerate(ops) if b.count("v_mad_u64_u32") == 4]
    ends = [i for i, b in enumerate(ops) if "ds_write_b8" in b and b.count("v_bcnt_u32_b32") >= 4 and valu[i] <= 30]

    def cheapest(src):
        """(cost, predecessor) from src to every block: the VALU of the blocks entered, src's own not counted"""
        import heapq
        dist, prev, heap = {}, {}, [(0, src, None)]
        first = True
        while heap:
            d, i, frm = heapq.heappop(heap)
            if not first and i in dist:
                continue
            if not first:
                dist[i], prev[i] = d, frm
            first = False
            for j in succ[i]:
                if j not in dist:
                    heapq.heappush(heap, (d + valu[j], j, i))
        return dist, prev

    def walk(prev, src, dst):
        out = [dst]
        while prev[out[-1]] != src:
            out.append(prev[out[-1]])
        return out[::-1]

    best = None
    reach = {i: cheapest(i) for i in set(takes + loops + ends)}
    for t in takes:
        for b in loops:
            for e in ends:
                try:
                    cost = reach[t][0][b] + reach[b][0][e] + reach[e][0][t]
                except KeyError:
                    continue
                if best is None or cost < best[0]:
                    best = (cost, t, b, e)
    cost, t, b, e = best
    cycle = walk(reach[t][1], t, b) + walk(reach[b][1], b, e) + walk(reach[e][1], e, t)
    assert cost == sum(valu[i] for i in cycle)
    return {"valu_instructions": cost, "take": names[t], "loop_body": names[b], "game_end": names[e],
            "blocks": [[names[i], valu[i]] for i in cycle if valu[i]]}


def resources(path, sym):
    """VGPRs, scratch, LDS and occupancy of a kernel as the compiler states them in the listing (the comment block behind the
    kernel's code; LDS is the static part -- the outcome slices are dynamic and sized by the launcher)"""
    out, inside = {}, False
    for line in open(path):
        f = line.replace(":", " ").split()
        if len(f) >= 2 and f[0] == ".size" and f[1].rstrip(",").startswith(sym):
            inside = True
        elif inside and len(f) == 3 and f[0] == ";" and f[1] in ("NumVgprs", "NumAgprs", "TotalNumVgprs", "ScratchSize", "Occupancy", "NumSgprs"):
            out[f[1]] = int(f[2])
            if f[1] == "Occupancy":
                break
        elif inside and len(f) >= 3 and f[0] == ";" and f[1] == "LDSByteSize":
            out["LDSByteSize"] = int(f[2])
    return out


if __name__ == "__main__":
    csrc = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "board-game-simulator-python_amd", "csrc")
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "connect.s")
        subprocess.check_call(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-S",
                               os.path.join(csrc, "connect_kernels.hip"), "-o", out, "-Wno-unused-function", "-mllvm", "-enable-post-misched=0"],
                              stderr=subprocess.DEVNULL)
        # the bench kernel: Connect4(6,7,4), uncapped, from the initial state, 3 opening blocks, outcome codes fused
        # (template arguments: geometry, opening blocks, codes, RNG contract [, drain merge]: a prefix of the mangled name)
        sym = "_ZN3bgs12_GLOBAL__N_124k_connect_rollout_openedINS0_3GeoILi1ELi6ELi7ELi4EEELi3ELb1ELb0E"
        result = mix(out, sym)
        # additive (profiles/*.json keep their fields): the steady-state iteration of the refill loop of the bench's two
        # kernels -- the one-step launch and the grouped form -- and what the compiler says they occupy
        steps_sym = "_ZN3bgs12_GLOBAL__N_130k_connect_rollout_opened_stepsINS0_3GeoILi1ELi6ELi7ELi4EEELi3ELb1E"
        result["iteration_path"] = {"one_step": iteration_path(out, sym), "grouped": iteration_path(out, steps_sym)}
        result["resources"] = {"one_step": resources(out, sym), "grouped": resources(out, steps_sym)}
        print(json.dumps(result, indent=1))
