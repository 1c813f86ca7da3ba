#!/usr/bin/env python3
"""What a launch of the batched UCT tree search for Bounce costs, how often the default edge pool runs dry, and the
sequential-halving launch at the same playouts a root for context.

For n = 256 and 4096 roots of the default 9x6 board at mixed mid-game plies and both playout policies, two launches are
timed in one process, alternating, `--rounds` times `--reps` launches each after one untimed launch (device events on the
batch's stream, outputs and workspace left on the device):
  * search   -- search_moves_tensor(iterations = 256, leaf_playouts = 64, edges = None: the default pool);
  * halving  -- evaluate_moves_halving_tensor(budget = 256 * 64) on the same roots.
Per launch: the time (median over the rounds, and the rounds' least and greatest), the playouts played (search: the sum
of `visits`; halving: the sum of `given`), playouts/s, the env-steps counted on the device, and for the search the nodes
made a root, the edges in use a root, the workspace's size and `pool_dry_share`: the share of the running roots with
used + BGS_BOUNCE_SEARCH_MIN_EDGES > edges, that is, whose pool could no longer take a node of the most arms.  One
256-lane workgroup owns a root, so n = 256 fills the chip's CUs once and shows the launch's latency more than its rate.

Every (n, policy) step is a process of its own under its own time limit, started one after the other by this script,
which itself never opens the GPU; the first step that fails or runs out of time ends the run, and the file says so.

    python tools/search_bounce_rate.py [--rounds R] [--reps K] [--out profiles/search_bounce_rate.json]
Prints one JSON object (and writes it to --out)."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "board-game-simulator-python_amd")]

SEED = 0x0123456789ABCDEF
ITERATIONS, LEAF_PLAYOUTS = 256, 64
MAX_PLIES = 1024
ROOTS = (256, 4096)
POLICIES = ("uniform", "decisive")
STEP_SECONDS = 240


def roots(n, seed):
    """n boards of the default grid at mixed plies: board i is played uniformly at random for 1 + i % 12 plies (or to its
    end) (evaluate_bounce_halving_rate.py's)"""
    import numpy as np

    from simulator.batch import BounceBatch

    grid = np.zeros((9, 6), dtype=np.int8)
    grid[1] = grid[7] = [1, 2, 3, 3, 2, 1]
    b = BounceBatch(grid, n, use_torch=True)
    target = 1 + np.arange(n) % 12
    for ply in range(int(target.max())):
        g, p, w, pl = b.grid, b.player, b.winner, b.plies
        b.step_random(seed=seed + ply)
        keep = target <= ply     # boards past their target go back to where they were
        if keep.any():
            g2, p2, w2, pl2 = b.grid, b.player, b.winner, b.plies
            g2[keep], p2[keep], w2[keep], pl2[keep] = g[keep], p[keep], w[keep], pl[keep]
            assert (b.write_state(g2, p2, w2, pl2) == 0).all()
    return b


def device_ms(fn, reps):
    import torch

    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn()   # (untimed: the variant before this one in the round may leave the chip in another clock state)
    torch.cuda.synchronize()
    start.record()
    for _ in range(reps):
        fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) / reps


def step(n, policy, rounds, reps):
    """one (n, policy) measurement, in this process"""
    import torch

    from simulator.game import _abi

    b = roots(n, seed=4096 + ITERATIONS)
    h, w = b.height, b.width
    budget = ITERATIONS * LEAF_PLAYOUTS
    edges, least = b.search_default_edges(ITERATIONS), b.search_min_edges()
    slots = (n, w, h * w)
    search_out = [torch.empty(s, dtype=torch.int32, device="cuda:0") for s in (slots + (3,), slots, (n,), (n,), (n,))]
    halving_out = [torch.empty(s, dtype=torch.int32, device="cuda:0") for s in (slots + (3,), slots, (n,))]
    workspace = torch.empty(b.search_moves_workspace_bytes(ITERATIONS, edges), dtype=torch.uint8, device="cuda:0")
    calls = {
        "search": lambda: b.search_moves_tensor(*search_out, seed=SEED, iterations=ITERATIONS, leaf_playouts=LEAF_PLAYOUTS,
                                                max_plies=MAX_PLIES, policy=policy, edges=edges, workspace=workspace),
        "halving": lambda: b.evaluate_moves_halving_tensor(*halving_out, seed=SEED, budget=budget, max_plies=MAX_PLIES, policy=policy),
    }
    res = {}
    for name, call in calls.items():
        call()   # (warm-up)
        b.reset_steps()
        call()
        torch.cuda.synchronize()
        played = int((search_out if name == "search" else halving_out)[1].sum())
        res[name] = {"env_steps": b.steps, "playouts_played": played, "round_ms": []}
    running = search_out[2] >= 0
    used = search_out[4][running].float()
    res["search"]["mean_nodes_a_root"] = round(float(search_out[3][running].float().mean()), 2)
    res["search"]["mean_edges_used_a_root"] = round(float(used.mean()), 2)
    res["search"]["edges"] = edges
    res["search"]["min_edges"] = least
    res["search"]["pool_dry_share"] = round(float((used + least > edges).float().mean()), 4)
    res["search"]["workspace_bytes"] = workspace.numel()
    for _ in range(rounds):
        for name, call in calls.items():
            res[name]["round_ms"].append(round(device_ms(call, reps), 4))
    for v in res.values():
        ms = v["round_ms"]
        v["device_ms"] = statistics.median(ms)
        v["device_ms_least"], v["device_ms_greatest"] = min(ms), max(ms)
        v["playouts_per_s_device"] = v["playouts_played"] / (v["device_ms"] * 1e-3)
        v["env_steps_per_s_device"] = v["env_steps"] / (v["device_ms"] * 1e-3)
    row = {"geometry": f"{h}x{w}", "roots": n, "policy": policy, "iterations": ITERATIONS, "leaf_playouts": LEAF_PLAYOUTS,
           "halving_budget": budget, "max_plies": MAX_PLIES, "running_roots": int(running.sum()),
           "device": torch.cuda.get_device_name(0), "build_id": _abi.build_id(),
           "unit_ids": {**_abi.unit_ids(), **_abi.extra_unit_ids()}, **res,
           "search_vs_halving_ms": round(res["search"]["device_ms"] / res["halving"]["device_ms"], 3)}
    b.close()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--out", default="")
    ap.add_argument("--step", nargs=2, metavar=("ROOTS", "POLICY"), help="(internal) measure one step in this process")
    args = ap.parse_args()
    if args.step:
        print(json.dumps(step(int(args.step[0]), args.step[1], args.rounds, args.reps)))
        return
    res = {"tool": "tools/search_bounce_rate.py", "rounds": args.rounds, "reps": args.reps, "cases": [], "stopped": None}
    for n in ROOTS:
        for policy in POLICIES:
            cmd = [sys.executable, os.path.abspath(__file__), "--rounds", str(args.rounds), "--reps", str(args.reps), "--step", str(n), policy]
            try:
                out = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=STEP_SECONDS)
            except subprocess.TimeoutExpired:
                res["stopped"] = f"step {n} roots, {policy}: no result within {STEP_SECONDS} s"
                break
            if out.returncode != 0:
                res["stopped"] = f"step {n} roots, {policy}: exit status {out.returncode}"
                break
            row = json.loads(out.stdout.strip().splitlines()[-1])
            for key in ("device", "build_id", "unit_ids"):
                res[key] = row.pop(key)
            res["cases"].append(row)
        if res["stopped"]:
            break               # nothing more is started on the GPU after a step that failed
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")
    sys.exit(1 if res["stopped"] else 0)


if __name__ == "__main__":
    main()
