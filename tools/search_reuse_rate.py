#!/usr/bin/env python3
"""What keeping the search trees between moves costs and gives: the advance launch beside the search launch of the same
batch, the nodes carried into a search, and the score of the agent that keeps its trees against the one that does not.

Launch times (one process): n = 4096 roots of Connect4 at mixed mid-game plies, the agent's default sizes (iterations =
256, leaf_playouts = 64, capacity = 2 * iterations + 1), uniform playouts.  The forest is searched once, advanced by the
best column, the boards are stepped by it and the forest is searched again.  Three launches are timed, alternating,
`--rounds` times `--reps` launches each after one untimed launch, by device events on the batch's stream:
  * search   -- search_actions_tensor on the boards after the step (the plain search the agent makes without reuse);
  * advance  -- advance_tensor by the best column, on the forest as the first search left it;
  * carried  -- search_tensor on the advanced forest (the search the reuse agent makes).
The advance and the carried search change the forest, so before each timed launch the forest is copied back from a
snapshot (outside the timed window: a launch is timed by events of its own and the times are summed).
`advance_share_of_saved` is advance_ms / (search_ms * mean_carried / iterations): the advance's cost over the part of a
search that the carried nodes stand for, a node counted as an iteration.

The match (a process of its own): examples/tree_reuse_match.py --json at `--games`, `--iterations`, `--leaf-playouts`.

    python tools/search_reuse_rate.py [--rounds R] [--reps K] [--games G] [--out profiles/search_reuse_rate.json]
Prints one JSON object (and writes it to --out)."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "board-game-simulator-python_amd"), os.path.join(ROOT, "tools")]

SEED = 0x0123456789ABCDEF
ITERATIONS, LEAF_PLAYOUTS = 256, 64
ROOTS = 4096
STEP_SECONDS = 300


def timed(prepare, fn, reps):
    """mean device ms of `fn` over `reps` launches, `prepare` before each one and outside its window"""
    import torch

    total = 0.0
    for rep in range(reps + 1):         # (the first launch is not counted)
        prepare()
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        fn()
        end.record()
        torch.cuda.synchronize()
        total += start.elapsed_time(end) if rep else 0.0
    return total / reps


def launches(rounds, reps):
    import torch

    from search_rate import roots
    from simulator.game import _abi

    n, capacity = ROOTS, 2 * ITERATIONS + 1
    kw = dict(iterations=ITERATIONS, leaf_playouts=LEAF_PLAYOUTS, policy="uniform")
    b = roots(n, seed=4096 + ITERATIONS)
    forest = b.search_forest(capacity)
    first = forest.search_tensor(seed=SEED, **kw)
    best = first[2].clone()
    searched = forest._buffer.clone()
    kept = forest.advance_tensor(best)
    advanced = forest._buffer.clone()
    b.step_actions_observe(best, b.legal_tensor())
    second = forest.search_tensor(seed=SEED + 1, **kw)
    torch.cuda.synchronize()
    running = second[2] >= 0
    workspace = torch.empty(b.search_workspace_bytes(ITERATIONS), dtype=torch.uint8, device="cuda:0")
    plain_out = [torch.empty_like(x) for x in first[:4]]
    calls = {
        "search": (lambda: None, lambda: b.search_actions_tensor(*plain_out, seed=SEED + 1, workspace=workspace, **kw)),
        "advance": (lambda: forest._buffer.copy_(searched), lambda: forest.advance_tensor(best, kept)),
        "carried": (lambda: forest._buffer.copy_(advanced), lambda: forest.search_tensor(*second, seed=SEED + 1, **kw)),
    }
    res = {name: {"round_ms": []} for name in calls}
    for _ in range(rounds):
        for name, (prepare, fn) in calls.items():
            res[name]["round_ms"].append(round(timed(prepare, fn, reps), 4))
    for v in res.values():
        v["device_ms"] = statistics.median(v["round_ms"])
        v["device_ms_least"], v["device_ms_greatest"] = min(v["round_ms"]), max(v["round_ms"])
    mean_carried = float(second[4][running].float().mean())
    saved_ms = res["search"]["device_ms"] * mean_carried / ITERATIONS
    out = {"geometry": "6x7x4", "roots": n, "running_roots_searched_again": int(running.sum()), "iterations": ITERATIONS,
           "leaf_playouts": LEAF_PLAYOUTS, "capacity": capacity, "policy": "uniform", "forest_bytes": forest._buffer.numel(),
           "mean_nodes_after_first_search": round(float(first[3].float().mean()), 2),
           "mean_kept_by_advance": round(float(kept[running].float().mean()), 2), "mean_carried": round(mean_carried, 2),
           "mean_nodes_after_second_search": round(float(second[3][running].float().mean()), 2), **res,
           "saved_ms_estimate": round(saved_ms, 4),
           "advance_share_of_saved": round(res["advance"]["device_ms"] / saved_ms, 4) if saved_ms else None,
           "device": torch.cuda.get_device_name(0), "build_id": _abi.build_id(), "unit_ids": {**_abi.unit_ids(), **_abi.extra_unit_ids()}}
    forest.close()
    b.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--games", type=int, default=512)
    ap.add_argument("--iterations", type=int, default=64)
    ap.add_argument("--leaf-playouts", type=int, default=16)
    ap.add_argument("--out", default="")
    ap.add_argument("--step", action="store_true", help="(internal) time the launches in this process")
    args = ap.parse_args()
    if args.step:
        print(json.dumps(launches(args.rounds, args.reps)))
        return
    me = [sys.executable, os.path.abspath(__file__), "--rounds", str(args.rounds), "--reps", str(args.reps), "--step"]
    match = [sys.executable, os.path.join(ROOT, "board-game-simulator-python_amd", "examples", "tree_reuse_match.py"), "--json",
             "--games", str(args.games), "--iterations", str(args.iterations), "--leaf-playouts", str(args.leaf_playouts)]
    res = {"tool": "tools/search_reuse_rate.py", "measured": True, "rounds": args.rounds, "reps": args.reps, "stopped": None}
    for name, cmd in (("launches", me), ("match", match)):
        try:
            out = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=STEP_SECONDS)
        except subprocess.TimeoutExpired:
            res["stopped"] = f"{name}: no result within {STEP_SECONDS} s"
            break               # nothing more is started on the GPU after a step that failed
        if out.returncode != 0:
            res["stopped"] = f"{name}: exit status {out.returncode}"
            break
        res[name] = json.loads(out.stdout.strip().splitlines()[-1])
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")
    sys.exit(1 if res["stopped"] else 0)


if __name__ == "__main__":
    main()
