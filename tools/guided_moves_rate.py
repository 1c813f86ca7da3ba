#!/usr/bin/env python3
"""What one step of the Bounce guided search costs: bgs_bounce_guided_step with CONSTANT evaluator tensors (uniform
priors, zero values, no network), so the time is the library's alone -- the application of the pending leaves (their arms
made again, their priors quantised), the report, the descent with its move search at the leaf, and the leaf grids.

The sibling of tools/guided_search_rate.py, whose warm-up, rounds and timing it takes over: for n = 64, 4096 and 65536
roots of the default 9x6 board at mixed mid-game plies, one search is `begin`, SIMULATIONS - 1 `step`s and `finish` with
nodes = SIMULATIONS + 1 and the default edge pool.  After one untimed search, `--rounds` searches are timed with device
events on the batch's stream (one pair around the whole search: 1 + SIMULATIONS enqueues, nothing between them on the
host but the ctypes calls).  Per n: the microseconds a step (the search's time / (1 + SIMULATIONS); median over the
rounds, and the rounds' least and greatest), and beside it what the step's cost depends on: the mean length of a pending
path (one more untimed search, in which word 13 of every tree's share -- the edges of the pending path, see the layout
above k_bounce_search_guided -- is added up on the device after every call), the arms a node (pool edges in use / nodes in
use at the end), the nodes a root and the bytes of the trees.  One wave owns a tree, so n = 64 shows a launch's latency and
n = 65536 the chip's rate.  CONNECT_US_A_STEP holds the figures of profiles/guided_search_rate.json as context: another
game, paths of another length, 7 arms a node.

Every n is a process of its own under its own time limit, started one after the other by this script, which itself never
opens the GPU; the first step that fails or runs out of time ends the run, and the file says so.

    python tools/guided_moves_rate.py [--rounds R] [--out profiles/guided_bounce_rate.json]
Prints one JSON object (and writes it to --out)."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "board-game-simulator-python_amd")]

SIMULATIONS = 128
CPUCT = 320
ROOTS = (64, 4096, 65536)
STEP_SECONDS = 240
PATH_WORD = 13                      # of a tree's share: the edges of the pending path
CONNECT_US_A_STEP = {64: 8.7, 4096: 11.7, 65536: 80.0}     # profiles/guided_search_rate.json: Connect4, context only


def default_grid():
    import numpy as np

    grid = np.zeros((9, 6), dtype=np.int8)
    grid[1] = grid[7] = [1, 2, 3, 3, 2, 1]
    return grid


def roots(n, seed):
    """n boards of the default grid in the middle of the game: board i is played uniformly at random to 4 + i % 12 plies (or
    its end)"""
    import numpy as np

    from simulator.batch import BounceBatch

    b = BounceBatch(default_grid(), n, use_torch=True)
    target = 4 + np.arange(n) % 12
    state = [b.grid, b.player, b.winner, b.plies]
    for ply in range(1, int(target.max()) + 1):
        b.step_random(seed + ply)
        now = [b.grid, b.player, b.winner, b.plies]
        for kept, new in zip(state, now):
            kept[target >= ply] = new[target >= ply]
    assert (b.write_state(*state) == 0).all()
    b.reset_steps()
    return b


def step(n, rounds):
    """one n, in this process"""
    import torch

    from simulator.game import _abi

    b = roots(n, seed=4096 + SIMULATIONS)
    h, w = b.height, b.width
    guided = b.guided_moves_search(SIMULATIONS + 1, cpuct=CPUCT)
    priors = torch.full((n, w, h * w), 1.0 / (w * h * w), dtype=torch.float32, device="cuda:0")
    values = torch.zeros(n, dtype=torch.float32, device="cuda:0")
    share_words = guided._buffer.numel() // 4 // n
    path_words = guided._buffer.view(torch.int32).view(n, share_words)[:, PATH_WORD]
    path_sum = torch.zeros((), dtype=torch.int64, device="cuda:0")

    def search(count_paths=False):
        guided.begin()
        for _ in range(SIMULATIONS - 1):
            guided.step(priors, values)
            if count_paths:
                path_sum.add_(path_words.sum())
        return guided.finish(priors, values)

    outs = search()   # (warm-up, untimed)
    torch.cuda.synchronize()
    round_us = []
    for _ in range(rounds):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        search()
        end.record()
        torch.cuda.synchronize()
        round_us.append(round(start.elapsed_time(end) * 1e3 / (1 + SIMULATIONS), 3))
    outs = search(count_paths=True)   # (untimed: the pending paths of SIMULATIONS - 1 descents a running root)
    torch.cuda.synchronize()
    running = int((outs[7] + outs[8] > 0).sum())        # (a root with arms holds its own edges)
    nodes_in_use = float((outs[7][outs[8] > 0] + 1).sum())
    row = {"grid": "default 9x6", "roots": n, "running_roots": running, "simulations": SIMULATIONS, "cpuct": CPUCT,
           "nodes": guided.nodes, "edges": guided.edges, "trees_bytes": guided._buffer.numel(), "round_us_a_step": round_us,
           "us_a_step": statistics.median(round_us), "us_a_step_least": min(round_us), "us_a_step_greatest": max(round_us),
           "connect_us_a_step": CONNECT_US_A_STEP[n] if n in CONNECT_US_A_STEP else None,
           "visits_a_running_root": round(float(outs[4].sum()) / max(1, running), 2),
           "mean_path_edges": round(float(path_sum) / max(1, running * (SIMULATIONS - 1)), 3),
           "mean_arms_a_node": round(float(outs[8].sum()) / max(1.0, nodes_in_use), 2),
           "mean_nodes_a_root": round(float(outs[7].float().mean()), 2),
           "device": torch.cuda.get_device_name(0), "build_id": _abi.build_id(), "unit_ids": {**_abi.unit_ids(), **_abi.extra_unit_ids()}}
    row["tree_steps_per_s"] = round(running / (row["us_a_step"] * 1e-6))
    guided.close()
    b.close()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default="")
    ap.add_argument("--step", metavar="ROOTS", help="(internal) measure one n in this process")
    args = ap.parse_args()
    if args.step:
        print(json.dumps(step(int(args.step), args.rounds)))
        return
    res = {"tool": "tools/guided_moves_rate.py", "rounds": args.rounds, "evaluator": "constant tensors: uniform priors, zero values",
           "cases": [], "stopped": None}
    for n in ROOTS:
        cmd = [sys.executable, os.path.abspath(__file__), "--rounds", str(args.rounds), "--step", str(n)]
        try:
            out = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=STEP_SECONDS)
        except subprocess.TimeoutExpired:
            res["stopped"] = f"step {n} roots: no result within {STEP_SECONDS} s"
            break
        if out.returncode != 0:
            res["stopped"] = f"step {n} roots: exit status {out.returncode}"
            break               # nothing more is started on the GPU after a step that failed
        row = json.loads(out.stdout.strip().splitlines()[-1])
        for key in ("device", "build_id", "unit_ids"):
            res[key] = row.pop(key)
        res["cases"].append(row)
    if "unit_ids" in res:
        res["unit"] = {"search": res["unit_ids"]["search"]}      # the unit whose kernel this file describes
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")
    sys.exit(1 if res["stopped"] else 0)


if __name__ == "__main__":
    main()
