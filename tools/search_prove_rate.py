#!/usr/bin/env python3
"""What proving in the tree costs where nothing is proved, what it saves where things are, and what it is worth in play.

Three measurements, each a process of its own under its own time limit, started one after the other by this script,
which itself never opens the GPU; the first step that fails or runs out of time ends the run, and the file says so.

  * nothing_proved -- 4096 start-position roots of Connect4, iterations = 64, leaf_playouts = 16, uniform playouts: the
    proving launch (search_actions_proving_tensor) beside the plain launch (search_actions_tensor) of the same build,
    alternating, `--rounds` times `--reps` launches each after one untimed launch, by device events on the batch's
    stream.  The yardstick is the plain launch and its own spread over the rounds: `slower_by` is the difference of the
    medians, `plain_spread` the plain launch's greatest round minus its least.
  * proved -- the same pair on mid- and end-game roots: 4096 running positions of random games at 26, 18 and 12 empty
    cells (the stepped boards of tools/solve_rate.py), with the mean of done / T, the share of roots decided and the
    root columns proved.
  * match -- examples/tree_prove_match.py --json at `--games`, `--iterations`, `--leaf-playouts`, both policies.

    python tools/search_prove_rate.py [--rounds R] [--reps K] [--games G] [--out profiles/search_prove_rate.json]
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
ROOTS = 4096
EMPTIES = (26, 18, 12)
STEP_SECONDS = 300


def pair(b, rounds, reps):
    """the plain and the proving launch on batch `b`, alternating: {"plain": .., "proving": .., ..}"""
    import torch

    from search_rate import device_ms

    n, w = b.n, b.width
    kw = dict(seed=SEED, iterations=ITERATIONS, leaf_playouts=LEAF_PLAYOUTS, policy="uniform")
    workspace = torch.empty(b.search_workspace_bytes(ITERATIONS), dtype=torch.uint8, device="cuda:0")
    plain_out = [torch.empty(s, dtype=torch.int32, device="cuda:0") for s in ((n, w, 3), (n, w), (n,), (n,))]
    proving_out = [torch.empty(s, dtype=torch.int32, device="cuda:0") for s in ((n, w, 3), (n, w), (n,), (n,))]
    proving_out += [torch.empty((n, w), dtype=torch.int8, device="cuda:0"), torch.empty((n,), dtype=torch.int32, device="cuda:0")]
    calls = {
        "plain": lambda: b.search_actions_tensor(*plain_out, workspace=workspace, **kw),
        "proving": lambda: b.search_actions_proving_tensor(*proving_out, workspace=workspace, **kw),
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
    proved, done = proving_out[4], proving_out[5]
    running = plain_out[2] >= 0
    res["running_roots"] = int(running.sum())
    res["mean_done_share"] = round(float(done[running].float().mean()) / ITERATIONS, 4) if res["running_roots"] else None
    res["decided_share"] = round(float((done[running] < ITERATIONS).float().mean()), 4) if res["running_roots"] else None
    res["proved_columns"] = {"win": int((proved == 1).sum()), "draw": int((proved == 0).sum()), "loss": int((proved == -1).sum())}
    res["best_differs"] = int((plain_out[2] != proving_out[2]).sum())
    res["slower_by_ms"] = round(res["proving"]["device_ms"] - res["plain"]["device_ms"], 4)
    res["plain_spread_ms"] = round(res["plain"]["device_ms_greatest"] - res["plain"]["device_ms_least"], 4)
    res["proving_over_plain"] = round(res["proving"]["device_ms"] / res["plain"]["device_ms"], 4)
    return res


def launches(rounds, reps):
    import torch

    from simulator.batch import ConnectBatch
    from simulator.game import _abi
    from solve_rate import positions

    out = {"geometry": "6x7x4", "roots": ROOTS, "iterations": ITERATIONS, "leaf_playouts": LEAF_PLAYOUTS, "policy": "uniform"}
    b = ConnectBatch(6, 7, 4, ROOTS, use_torch=True)
    out["nothing_proved"] = pair(b, rounds, reps)
    b.close()
    out["proved"] = []
    for empty in EMPTIES:
        g, p, wn, pl = positions(ROOTS, empty, 0x501E ^ empty, 16 * ROOTS)
        b = ConnectBatch(6, 7, 4, g.shape[0], use_torch=True)
        assert (b.write_state(g, p, wn, pl) == 0).all()
        out["proved"].append({"empty": empty, "boards": int(g.shape[0]), **pair(b, rounds, reps)})
        b.close()
    out.update(device=torch.cuda.get_device_name(0), build_id=_abi.build_id(), unit_ids={**_abi.unit_ids(), **_abi.extra_unit_ids()})
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
    match = [sys.executable, os.path.join(ROOT, "board-game-simulator-python_amd", "examples", "tree_prove_match.py"), "--json",
             "--games", str(args.games), "--iterations", str(args.iterations), "--leaf-playouts", str(args.leaf_playouts)]
    res = {"tool": "tools/search_prove_rate.py", "measured": True, "rounds": args.rounds, "reps": args.reps, "stopped": None}
    steps = (("launches", me), ("match_uniform", match + ["--policy", "uniform"]), ("match_decisive", match + ["--policy", "decisive"]))
    for name, cmd in steps:
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
