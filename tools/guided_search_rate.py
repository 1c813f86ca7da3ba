#!/usr/bin/env python3
"""What one step of the guided search costs: bgs_connect_guided_step with CONSTANT evaluator tensors (uniform priors,
zero values, no network), so the time is the library's alone -- the application of the pending leaves, the report, the
descent and the leaf grids.

For n = 64, 4096 and 65536 roots of Connect4 at mixed mid-game plies, one search is `begin`, SIMULATIONS - 1 `step`s and
`finish` with capacity = SIMULATIONS + 1.  After one untimed search, `--rounds` searches are timed with device events on
the batch's stream (one pair around the whole search: 1 + SIMULATIONS enqueues, nothing between them on the host but the
ctypes calls).  Per n: the microseconds a step (the search's time / (1 + SIMULATIONS); median over the rounds, and the
rounds' least and greatest), the nodes a root at the end and the bytes of the trees.  One wave owns a tree, so n = 64
shows a launch's latency and n = 65536 the chip's rate.  The trees deepen from step to step, so a step's cost is an
average over the search, not a constant.

Every n is a process of its own under its own time limit, started one after the other by this script, which itself never
opens the GPU; the first step that fails or runs out of time ends the run, and the file says so.

    python tools/guided_search_rate.py [--rounds R] [--out profiles/guided_search_rate.json]
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
GEOMETRY = (6, 7, 4)
ROOTS = (64, 4096, 65536)
STEP_SECONDS = 240


def roots(n, seed):
    """n Connect4 boards in the middle of the game: board i is played uniformly at random to 6 + i % 15 plies (or its end)"""
    import numpy as np

    from simulator.batch import ConnectBatch

    h, w, k = GEOMETRY
    b = ConnectBatch(h, w, k, n, use_torch=True)
    rng = np.random.default_rng(seed)
    target = 6 + np.arange(n) % 15
    for ply in range(int(target.max())):
        legal = b.legal.astype(bool)
        pick = (rng.random((n, w)) * legal).argmax(axis=1).astype(np.int32)
        cols = np.where((target > ply) & legal.any(axis=1), pick, -1).astype(np.int32)
        b.step_actions(cols, want_status=False)
    return b


def step(n, rounds):
    """one n, in this process"""
    import torch

    from simulator.game import _abi

    h, w, k = GEOMETRY
    b = roots(n, seed=4096 + SIMULATIONS)
    guided = b.guided_search(SIMULATIONS + 1, CPUCT)
    priors = torch.full((n, w), 1.0 / w, dtype=torch.float32, device="cuda:0")
    values = torch.zeros(n, dtype=torch.float32, device="cuda:0")

    def search():
        guided.begin()
        for _ in range(SIMULATIONS - 1):
            guided.step(priors, values)
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
    running = int((b.winner == -1).sum())
    row = {"geometry": "x".join(map(str, GEOMETRY)), "roots": n, "running_roots": running, "simulations": SIMULATIONS, "cpuct": CPUCT,
           "capacity": SIMULATIONS + 1, "trees_bytes": guided._buffer.numel(), "round_us_a_step": round_us,
           "us_a_step": statistics.median(round_us), "us_a_step_least": min(round_us), "us_a_step_greatest": max(round_us),
           "visits_a_running_root": round(float(outs[3].sum()) / max(1, running), 2),
           "mean_nodes_a_root": round(float(outs[6].float().mean()), 2),
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
    res = {"tool": "tools/guided_search_rate.py", "rounds": args.rounds, "evaluator": "constant tensors: uniform priors, zero values",
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
