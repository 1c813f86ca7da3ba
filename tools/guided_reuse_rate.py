#!/usr/bin/env python3
"""What keeping the guided trees across moves costs and what it keeps: bgs_connect_guided_advance beside
bgs_connect_guided_step, and self-played games on a GuidedForest.

1. The launch.  For n = 64, 4096 and 65536 roots of Connect4 at mixed mid-game plies and SIMULATIONS = 128 and 512, with
   capacity = 2 * SIMULATIONS + 1 and CONSTANT evaluator tensors (uniform priors, zero values: the time is the library's
   alone): one round is `begin`, SIMULATIONS - 1 `step`s and `finish`, timed with one pair of device events on the batch's
   stream, then ONE `advance` by every tree's `best`, timed with a pair of its own.  The boards are not stepped, so the
   next round's `begin` starts every tree anew: the rounds are alike.  After one untimed round, `--rounds` rounds; per case
   the microseconds a step (the search's time / (1 + SIMULATIONS)) and the microseconds of the advance, each as the median
   over the rounds with the least and the greatest, the advance in steps, and the nodes kept a tree.  An advance is one
   launch of tens of microseconds between two events: its figure includes the launch's latency, as a step's does.
2. Self-play.  GAMES games of Connect4 against themselves to the end on a GuidedForest under a small untrained MLP (the
   numbers say how much of a tree survives a move under SOME evaluator, not under a trained one), SELFPLAY_SIMULATIONS
   simulations a move, the most visited column played: per move of a running game, the nodes kept by the advance and the
   share of the next search's final root visits that were there when it resumed.  `--repeats` runs with different seeds
   of the network; the median over the runs, the least and the greatest.

Every case is a process of its own under its own time limit, started one after the other by this script, which itself never
opens the GPU; the first case that fails or runs out of time ends the run, and the file says so.

    python tools/guided_reuse_rate.py [--rounds R] [--repeats K] [--out profiles/guided_reuse_rate.json]
Prints one JSON object (and writes it to --out)."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "board-game-simulator-python_amd"), os.path.join(ROOT, "tools")]

CPUCT = 320
GEOMETRY = (6, 7, 4)
ROOTS = (64, 4096, 65536)
SIMULATIONS = (128, 512)
GAMES, SELFPLAY_SIMULATIONS = 256, 128
CASE_SECONDS = 240


def spread(values):
    return {"median": statistics.median(values), "least": min(values), "greatest": max(values)}


def launch(n, simulations, rounds):
    """one (n, simulations), in this process"""
    import torch

    from guided_search_rate import roots
    from simulator.batch import GuidedForest
    from simulator.game import _abi

    h, w, k = GEOMETRY
    b = roots(n, seed=4096 + simulations)
    forest = GuidedForest(b, 2 * simulations + 1, CPUCT)
    priors = torch.full((n, w), 1.0 / w, dtype=torch.float32, device="cuda:0")
    values = torch.zeros(n, dtype=torch.float32, device="cuda:0")
    kept = torch.zeros(n, dtype=torch.int32, device="cuda:0")
    columns = torch.zeros(n, dtype=torch.int32, device="cuda:0")

    def one_round():
        events = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        events[0].record()
        forest.begin()
        for _ in range(simulations - 1):
            forest.step(priors, values)
        outs = forest.finish(priors, values)
        events[1].record()
        columns.copy_(outs[5])
        events[2].record()
        forest.advance(columns, kept)
        events[3].record()
        torch.cuda.synchronize()
        return events[0].elapsed_time(events[1]) * 1e3 / (1 + simulations), events[2].elapsed_time(events[3]) * 1e3, outs

    one_round()     # (warm-up, untimed)
    step_us, advance_us = [], []
    for _ in range(rounds):
        s, a, outs = one_round()
        step_us.append(round(s, 3))
        advance_us.append(round(a, 3))
    running = int((b.winner == -1).sum())
    row = {"geometry": "x".join(map(str, GEOMETRY)), "roots": n, "running_roots": running, "simulations": simulations, "cpuct": CPUCT,
           "capacity": 2 * simulations + 1, "trees_bytes": forest._buffer.numel(), "round_us_a_step": step_us, "round_us_advance": advance_us,
           "us_a_step": spread(step_us), "us_advance": spread(advance_us),
           "advance_in_steps": round(statistics.median(advance_us) / statistics.median(step_us), 2),
           "mean_nodes_before": round(float(outs[6].float().sum()) / max(1, running), 2),
           "mean_nodes_kept": round(float(kept.float().sum()) / max(1, running), 2),
           "device": torch.cuda.get_device_name(0), "build_id": _abi.build_id(), "unit_ids": {**_abi.unit_ids(), **_abi.extra_unit_ids()}}
    forest.close()
    b.close()
    return row


def selfplay(seed):
    """GAMES games to the end, in this process: nodes kept a move and the carried share of the root's visits"""
    import torch

    from simulator.batch import ConnectBatch, GuidedForest

    h, w, k = GEOMETRY
    n, simulations = GAMES, SELFPLAY_SIMULATIONS
    torch.manual_seed(seed)
    net = torch.nn.Sequential(torch.nn.Linear(2 * h * w, 64), torch.nn.ReLU(), torch.nn.Linear(64, 64), torch.nn.ReLU(),
                              torch.nn.Linear(64, w + 1)).to("cuda:0").eval()

    @torch.no_grad()
    def evaluate(grid, player):
        mover = player.view(-1, 1, 1)
        out = net(torch.stack([grid == mover, grid == 1 - mover], dim=1).to(torch.float32).flatten(1))
        return torch.softmax(out[:, :w], dim=1).contiguous(), torch.tanh(out[:, w]).contiguous()

    games = ConnectBatch(h, w, k, n, use_torch=True)
    forest = GuidedForest(games, 2 * simulations + 1, CPUCT)
    legal = games.legal_tensor()
    ended = torch.zeros(n, dtype=torch.uint8, device="cuda:0")
    kept = torch.zeros(n, dtype=torch.int32, device="cuda:0")
    totals = torch.zeros(4, dtype=torch.float64, device="cuda:0")    # moves, nodes kept, carried visits, final visits
    outs = forest.run(evaluate, simulations)
    for _ in range(h * w):
        running = ended == 0
        if not bool(running.any()):
            break
        columns = torch.where(running, outs[5], torch.full_like(outs[5], -1)).contiguous()
        games.step_actions_observe(columns, legal, ended=ended)
        forest.advance(columns, kept)
        still = ended == 0          # the games that are searched again
        carried = forest.resume()[3].sum(dim=1).clone()
        for t in range(simulations):
            outs = (forest.finish if t == simulations - 1 else forest.step)(*evaluate(outs[0], outs[1]))
        totals += torch.stack([still.sum(), (kept * still).sum(), (carried * still).sum(), (outs[3].sum(dim=1) * still).sum()]).to(torch.float64)
    moves, nodes, carried, final = (float(x) for x in totals)
    forest.close()
    games.close()
    return {"seed": seed, "searched_moves": int(moves), "nodes_kept_a_move": round(nodes / max(1.0, moves), 2),
            "carried_share_of_root_visits": round(carried / max(1.0, final), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default="")
    ap.add_argument("--case", nargs="+", metavar="ARG", help="(internal) one case in this process: launch N S | selfplay SEED")
    args = ap.parse_args()
    if args.case:
        row = launch(int(args.case[1]), int(args.case[2]), args.rounds) if args.case[0] == "launch" else selfplay(int(args.case[1]))
        print(json.dumps(row))
        return
    res = {"tool": "tools/guided_reuse_rate.py", "rounds": args.rounds, "evaluator": "launch: constant tensors; selfplay: an untrained MLP",
           "launch": [], "selfplay": {"games": GAMES, "simulations": SELFPLAY_SIMULATIONS, "capacity": 2 * SELFPLAY_SIMULATIONS + 1, "runs": []},
           "stopped": None}
    cases = [("launch", n, s) for s in SIMULATIONS for n in ROOTS] + [("selfplay", 1 + r) for r in range(args.repeats)]
    for case in cases:
        cmd = [sys.executable, os.path.abspath(__file__), "--rounds", str(args.rounds), "--case", *map(str, case)]
        try:
            out = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=CASE_SECONDS)
        except subprocess.TimeoutExpired:
            res["stopped"] = f"case {case}: no result within {CASE_SECONDS} s"
            break
        if out.returncode != 0:
            res["stopped"] = f"case {case}: exit status {out.returncode}"
            break               # nothing more is started on the GPU after a case that failed
        row = json.loads(out.stdout.strip().splitlines()[-1])
        if case[0] == "launch":
            for key in ("device", "build_id", "unit_ids"):
                res[key] = row.pop(key)
            res["launch"].append(row)
        else:
            res["selfplay"]["runs"].append(row)
    runs = res["selfplay"]["runs"]
    if runs:
        res["selfplay"]["nodes_kept_a_move"] = spread([r["nodes_kept_a_move"] for r in runs])
        res["selfplay"]["carried_share_of_root_visits"] = spread([r["carried_share_of_root_visits"] for r in runs])
    if "unit_ids" in res:
        res["unit"] = {"search": res["unit_ids"]["search"]}      # the unit whose kernels this file describes
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")
    sys.exit(1 if res["stopped"] else 0)


if __name__ == "__main__":
    main()
