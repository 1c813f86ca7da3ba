#!/usr/bin/env python3
"""What proving in the Bounce search tree costs where nothing is proved, what it saves where things are, what it is worth
in play, and whether the plain launch is what it was.

Measurements, each a process of its own under its own time limit, started one after the other by this script, which
itself never opens the GPU; the first step that fails or runs out of time ends the run, and the file says so.

  * nothing_proved -- 4096 start positions of the default 9x6 board, iterations = 64, leaf_playouts = 16, uniform
    playouts: the proving launch (search_moves_proving_tensor) beside the plain launch (search_moves_tensor) of the same
    build on the same roots and workspace, alternating, `--rounds` times `--reps` launches each after one untimed launch,
    by device events on the batch's stream.  The yardstick is the plain launch and its own spread over the rounds:
    `slower_by_ms` is the difference of the medians, `plain_spread_ms` the plain launch's greatest round minus its least.
  * proved -- the same pair on 4096 boards played uniformly at random for 8, 16, 24 and 32 plies (boards that ended on the
    way stay in the batch and are not searched), with the mean of done / T over the running roots, the share of them
    decided and the root moves proved.
  * match -- examples/tree_prove_match_bounce.py --json at `--games`, `--iterations`, `--leaf-playouts`, both policies.
  * plain_against_parent (only with --parent-tree DIR, a built checkout of the parent commit) -- tools/search_bounce_rate.py
    --step of this tree and of DIR in alternation, `--ab-rounds` times, for 256 and 4096 roots and both policies: the
    plain launch's device ms of every run.  The launches of this build must lie inside the parent's run-to-run range.

    python tools/search_bounce_prove_rate.py [--rounds R] [--reps K] [--games G] [--parent-tree DIR]
        [--out profiles/search_bounce_prove_rate.json]
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
ITERATIONS, LEAF_PLAYOUTS = 64, 16
MAX_PLIES = 1024
ROOTS = 4096
DEPTHS = (8, 16, 24, 32)
AB_ROOTS = (256, 4096)
POLICIES = ("uniform", "decisive")
STEP_SECONDS = 300


def played(n, plies, seed):
    """n boards of the default grid played uniformly at random for `plies` plies, or to their end"""
    import numpy as np

    from simulator.batch import BounceBatch

    grid = np.zeros((9, 6), dtype=np.int8)
    grid[1] = grid[7] = [1, 2, 3, 3, 2, 1]
    b = BounceBatch(grid, n, use_torch=True)
    for ply in range(plies):
        b.step_random(seed=seed + ply)
    return b


def pair(b, rounds, reps):
    """the plain and the proving launch on batch `b`, alternating: {"plain": .., "proving": .., ..}"""
    import torch

    from search_bounce_rate import device_ms

    n, h, w = b.n, b.height, b.width
    edges = b.search_default_edges(ITERATIONS)
    kw = dict(seed=SEED, iterations=ITERATIONS, leaf_playouts=LEAF_PLAYOUTS, policy="uniform", max_plies=MAX_PLIES, edges=edges)
    workspace = torch.empty(b.search_moves_workspace_bytes(ITERATIONS, edges), dtype=torch.uint8, device="cuda:0")
    slots = (n, w, h * w)
    shapes = (slots + (3,), slots, (n,), (n,), (n,))
    plain_out = [torch.empty(s, dtype=torch.int32, device="cuda:0") for s in shapes]
    proving_out = [torch.empty(s, dtype=torch.int32, device="cuda:0") for s in shapes]
    proving_out += [torch.empty(slots, dtype=torch.int8, device="cuda:0"), torch.empty((n,), dtype=torch.int32, device="cuda:0")]
    calls = {
        "plain": lambda: b.search_moves_tensor(*plain_out, workspace=workspace, **kw),
        "proving": lambda: b.search_moves_proving_tensor(*proving_out, workspace=workspace, **kw),
    }
    res = {}
    for name, call in calls.items():
        call()   # (warm-up)
        b.reset_steps()
        call()
        torch.cuda.synchronize()
        res[name] = {"env_steps": b.steps, "round_ms": []}
    for _ in range(rounds):
        for name, call in calls.items():
            res[name]["round_ms"].append(round(device_ms(call, reps), 4))
    for v in res.values():
        ms = v["round_ms"]
        v["device_ms"] = statistics.median(ms)
        v["device_ms_least"], v["device_ms_greatest"] = min(ms), max(ms)
    proved, done = proving_out[5], proving_out[6]
    running = plain_out[2] >= 0
    res["running_roots"] = int(running.sum())
    res["mean_done_share"] = round(float(done[running].float().mean()) / ITERATIONS, 4) if res["running_roots"] else None
    res["decided_share"] = round(float((done[running] < ITERATIONS).float().mean()), 4) if res["running_roots"] else None
    res["proved_moves"] = {"win": int((proved == 1).sum()), "draw": int((proved == 0).sum()), "loss": int((proved == -1).sum())}
    res["outputs_equal_plain"] = all(bool((x == y).all()) for x, y in zip(plain_out, proving_out[:5]))
    res["best_differs"] = int((plain_out[2] != proving_out[2]).sum())
    res["slower_by_ms"] = round(res["proving"]["device_ms"] - res["plain"]["device_ms"], 4)
    res["plain_spread_ms"] = round(res["plain"]["device_ms_greatest"] - res["plain"]["device_ms_least"], 4)
    res["proving_over_plain"] = round(res["proving"]["device_ms"] / res["plain"]["device_ms"], 4)
    return res


def launches(rounds, reps):
    import torch

    from simulator.game import _abi

    out = {"geometry": "9x6 default", "roots": ROOTS, "iterations": ITERATIONS, "leaf_playouts": LEAF_PLAYOUTS, "policy": "uniform",
           "max_plies": MAX_PLIES}
    b = played(ROOTS, 0, 0)
    out["nothing_proved"] = pair(b, rounds, reps)
    b.close()
    out["proved"] = []
    for plies in DEPTHS:
        b = played(ROOTS, plies, 0x501E ^ plies)
        out["proved"].append({"plies": plies, **pair(b, rounds, reps)})
        b.close()
    out.update(device=torch.cuda.get_device_name(0), build_id=_abi.build_id(), unit_ids={**_abi.unit_ids(), **_abi.extra_unit_ids()})
    return out


def run(cmd, name, res):
    """the last line of `cmd`'s output as JSON, or None with res["stopped"] saying why"""
    print(f"step: {name}", file=sys.stderr, flush=True)     # (a sign of life: the result is printed at the end)
    try:
        out = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=STEP_SECONDS)
    except subprocess.TimeoutExpired:
        res["stopped"] = f"{name}: no result within {STEP_SECONDS} s"
        return None
    if out.returncode != 0:
        res["stopped"] = f"{name}: exit status {out.returncode}"
        return None
    return json.loads(out.stdout.strip().splitlines()[-1])


def against_parent(parent_tree, ab_rounds, res):
    """the plain launch of this tree and of the parent's, alternating, a process a run"""
    rows = []
    for n in AB_ROOTS:
        for policy in POLICIES:
            row = {"roots": n, "policy": policy, "this_ms": [], "parent_ms": []}
            for _ in range(ab_rounds):
                for key, tree in (("this_ms", ROOT), ("parent_ms", parent_tree)):
                    step = run([sys.executable, os.path.join(tree, "tools", "search_bounce_rate.py"), "--rounds", "3", "--reps", "2", "--step",
                                str(n), policy], f"plain_against_parent {n} {policy}", res)
                    if step is None:
                        return rows     # nothing more is started on the GPU after a step that failed
                    row[key].append(step["search"]["device_ms"])
                    # (a parent tree from before the search unit was split off holds k_bounce_search in its evaluate unit)
                    row[key.replace("_ms", "_search_unit")] = step["unit_ids"].get("search", step["unit_ids"].get("evaluate"))
            row["this_inside_parent_range"] = min(row["parent_ms"]) <= statistics.median(row["this_ms"]) <= max(row["parent_ms"])
            rows.append(row)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--games", type=int, default=512)
    ap.add_argument("--iterations", type=int, default=64)
    ap.add_argument("--leaf-playouts", type=int, default=16)
    ap.add_argument("--parent-tree", default="", help="a built checkout of the parent commit: the plain launch is timed against it")
    ap.add_argument("--ab-rounds", type=int, default=3)
    ap.add_argument("--out", default="")
    ap.add_argument("--step", action="store_true", help="(internal) time the launches in this process")
    args = ap.parse_args()
    if args.step:
        print(json.dumps(launches(args.rounds, args.reps)))
        return
    me = [sys.executable, os.path.abspath(__file__), "--rounds", str(args.rounds), "--reps", str(args.reps), "--step"]
    match = [sys.executable, os.path.join(ROOT, "board-game-simulator-python_amd", "examples", "tree_prove_match_bounce.py"), "--json",
             "--games", str(args.games), "--iterations", str(args.iterations), "--leaf-playouts", str(args.leaf_playouts)]
    res = {"tool": "tools/search_bounce_prove_rate.py", "measured": True, "rounds": args.rounds, "reps": args.reps, "stopped": None}
    steps = (("launches", me), ("match_uniform", match + ["--policy", "uniform"]), ("match_decisive", match + ["--policy", "decisive"]))
    for name, cmd in steps:
        got = run(cmd, name, res)
        if got is None:
            break               # nothing more is started on the GPU after a step that failed
        res[name] = got
    if args.parent_tree and not res["stopped"]:
        res["plain_against_parent"] = against_parent(os.path.abspath(args.parent_tree), args.ab_rounds, res)
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")
    sys.exit(1 if res["stopped"] else 0)


if __name__ == "__main__":
    main()
