#!/usr/bin/env python3
"""What keeping the Bounce search trees between moves costs and gives: the forest search beside the plain search at the
same shape, the advance launch beside the search launch, the nodes and edges carried after one ply and after two, and the
score of the agent that keeps its trees against the one that does not.

Launch times (one process): n = 1024 roots of the default grid at mixed mid-game plies (tools/search_bounce_rate.py's),
T = 256 iterations of P = 64 playouts, uniform playouts, the cap of 1024 plies.  Four launches are timed, alternating,
`--rounds` times `--reps` launches each after one untimed launch, by device events on the batch's stream:
  * search   -- search_moves_tensor (bgs_bounce_search_moves) with the default pool of T iterations: the baseline;
  * restart  -- search_tensor(restart=True) on a forest of C = T + 1 nodes and the same pool: the same work, bit for bit;
  * advance  -- advance_tensor by the best slot, on a forest of C = 2 T + 1 nodes as a first search left it;
  * carried  -- search_tensor on that forest after the advance and the step (the search the reuse agent makes).
The advance and the carried search change the forest, so before each timed launch the forest is copied back from a
snapshot (outside the timed window).  The baseline's run-to-run spread is its least and greatest round.
Carried: the forest of C = 2 T + 1 is searched and advanced by the best slot (one ply); the boards are stepped, the forest
is searched again and advanced by that search's best slot (the second ply); the mean nodes kept over the roots that still
run, and the edges in use after one further iteration of one playout (the edges carried plus at most one node's arms:
the advance reports nodes, and the tool does not read the forest's layout).

The match (a process of its own): examples/tree_reuse_match_bounce.py --json at `--games`, `--iterations`,
`--leaf-playouts`.

    python tools/search_bounce_reuse_rate.py [--rounds R] [--reps K] [--games G] [--out profiles/search_bounce_reuse_rate.json]
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
MAX_PLIES = 1024
ROOTS = 1024
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

    from search_bounce_rate import roots
    from simulator.game import _abi

    n, capacity = ROOTS, 2 * ITERATIONS + 1
    kw = dict(iterations=ITERATIONS, leaf_playouts=LEAF_PLAYOUTS, policy="uniform", max_plies=MAX_PLIES)
    b = roots(n, seed=4096 + ITERATIONS)
    h, w = b.height, b.width
    edges = b.search_default_edges(ITERATIONS)
    plain_out = [torch.empty(s, dtype=torch.int32, device="cuda:0") for s in ((n, w, h * w, 3), (n, w, h * w), (n,), (n,), (n,))]
    workspace = torch.empty(b.search_moves_workspace_bytes(ITERATIONS, edges), dtype=torch.uint8, device="cuda:0")
    same = b.search_moves_forest(ITERATIONS + 1, edges)
    same_out = same.search_tensor(seed=SEED, restart=True, **kw)
    b.search_moves_tensor(*plain_out, seed=SEED, edges=edges, workspace=workspace, **kw)
    torch.cuda.synchronize()
    equal = all(bool((x == y).all()) for x, y in zip(plain_out, same_out[:5]))
    forest = b.search_moves_forest(capacity)
    first = forest.search_tensor(seed=SEED, **kw)
    best = first[2].clone()
    searched = forest._buffer.clone()
    kept = forest.advance_tensor(best).clone()
    advanced = forest._buffer.clone()
    b.step_actions_observe(b.slots_to_moves_tensor(best), b.targets_tensor())

    def probe():
        """the edges in use after ONE further iteration of one playout on the forest as it stands: the edges carried plus
        at most one node's arms (the advance reports nodes only, and the forest's layout is not read here)"""
        return forest.search_tensor(seed=SEED + 7, iterations=1, leaf_playouts=1, policy="uniform", max_plies=MAX_PLIES)[4].clone()

    used_one = probe()
    forest._buffer.copy_(advanced)
    second = forest.search_tensor(seed=SEED + 1, **kw)
    after_second = forest._buffer.clone()
    reply = second[2].clone()
    torch.cuda.synchronize()
    running = second[2] >= 0
    calls = {
        "search": (lambda: None, lambda: b.search_moves_tensor(*plain_out, seed=SEED + 1, edges=edges, workspace=workspace, **kw)),
        "restart": (lambda: None, lambda: same.search_tensor(*same_out, seed=SEED + 1, restart=True, **kw)),
        "advance": (lambda: forest._buffer.copy_(searched), lambda: forest.advance_tensor(best)),
        "carried": (lambda: forest._buffer.copy_(advanced), lambda: forest.search_tensor(*second, seed=SEED + 1, **kw)),
    }
    res = {name: {"round_ms": []} for name in calls}
    for _ in range(rounds):
        for name, (prepare, fn) in calls.items():
            res[name]["round_ms"].append(round(timed(prepare, fn, reps), 4))
    for v in res.values():
        v["device_ms"] = statistics.median(v["round_ms"])
        v["device_ms_least"], v["device_ms_greatest"] = min(v["round_ms"]), max(v["round_ms"])

    # two plies, after the timed launches (they need the boards one ply on): the reply is the best slot of the second search
    forest._buffer.copy_(after_second)
    kept_two = forest.advance_tensor(reply).clone()
    b.step_actions_observe(b.slots_to_moves_tensor(reply), b.targets_tensor())
    used_two = probe()
    torch.cuda.synchronize()

    def mean(x, rows):
        return round(float(x[rows].float().mean()), 2)

    again = reply >= 0
    out = {"geometry": "9x6 default", "roots": n, "roots_running_after_one_ply": int(running.sum()),
           "iterations": ITERATIONS, "leaf_playouts": LEAF_PLAYOUTS, "capacity": capacity, "edges": forest.edges, "policy": "uniform",
           "forest_bytes": forest._buffer.numel(), "restart_equals_search_moves": equal,
           "mean_nodes_after_first_search": mean(first[3], first[2] >= 0), "mean_edges_after_first_search": mean(first[4], first[2] >= 0),
           "mean_nodes_kept_after_one_ply": mean(kept, running), "mean_edges_in_use_one_iteration_after_one_ply": mean(used_one, running),
           "mean_nodes_carried_into_second_search": mean(second[5], running),
           "mean_nodes_after_second_search": mean(second[3], running),
           "mean_nodes_kept_after_two_plies": mean(kept_two, again), "mean_edges_in_use_one_iteration_after_two_plies": mean(used_two, again),
           "two_plies_note": "the second ply is the best slot of a full second search on the stepped boards, so the tree it "
                             "re-roots holds that search's nodes too; edges are read as `used` after one further iteration of "
                             "one playout: the edges carried plus at most one node's arms", **res,
           "restart_over_search": round(res["restart"]["device_ms"] / res["search"]["device_ms"], 4),
           "advance_over_search": round(res["advance"]["device_ms"] / res["search"]["device_ms"], 4),
           "device": torch.cuda.get_device_name(0), "build_id": _abi.build_id(), "unit_ids": {**_abi.unit_ids(), **_abi.extra_unit_ids()}}
    for f in (forest, same):
        f.close()
    b.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--games", type=int, default=256)
    ap.add_argument("--iterations", type=int, default=64)
    ap.add_argument("--leaf-playouts", type=int, default=16)
    ap.add_argument("--out", default="")
    ap.add_argument("--step", action="store_true", help="(internal) time the launches in this process")
    args = ap.parse_args()
    if args.step:
        print(json.dumps(launches(args.rounds, args.reps)))
        return
    me = [sys.executable, os.path.abspath(__file__), "--rounds", str(args.rounds), "--reps", str(args.reps), "--step"]
    match = [sys.executable, os.path.join(ROOT, "board-game-simulator-python_amd", "examples", "tree_reuse_match_bounce.py"), "--json",
             "--games", str(args.games), "--iterations", str(args.iterations), "--leaf-playouts", str(args.leaf_playouts)]
    res = {"tool": "tools/search_bounce_reuse_rate.py", "measured": True, "rounds": args.rounds, "reps": args.reps, "stopped": None}
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
