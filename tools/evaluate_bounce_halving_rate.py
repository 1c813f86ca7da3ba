#!/usr/bin/env python3
"""What sequential halving costs a Bounce launch next to the flat evaluation of the same build, on the same roots and at
the same playouts a position.

Default 9x6 board, mixed-ply roots (evaluate_bounce_rate.py's), max_plies 1024, budget 1024, for n = 4096, 256, 64 and 1
roots (one team of lanes owns a root: few roots leave most of the chip idle) and both playout policies.  Two variants
are timed in one process, alternating, `--rounds` times `--reps` launches each after one untimed launch (device events on
the batch's stream, outputs left on the device):
  * flat     -- evaluate_moves(playouts = budget // mean legal moves of the running roots);
  * halving  -- evaluate_moves_halving(budget).
Per variant: the launch time (median over the rounds, and the rounds' least and greatest), the env-steps of one launch
(counted on the device, first moves included), env-steps/s, the playouts played and the mean plies a playout.  The
halving rows also say how many roots the budget was too small for (best = HALVING_SHORT).

    python tools/evaluate_bounce_halving_rate.py [--rounds R] [--reps K] [--budget B] [--out profiles/evaluate_bounce_halving_rate.json]
Prints one JSON object (and writes it to --out)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "board-game-simulator-python_amd")]
import numpy as np
import torch

from simulator.batch import HALVING_SHORT, BounceBatch
from simulator.game import _abi

SEED = 0x0123456789ABCDEF
GRID = np.zeros((9, 6), dtype=np.int8)
GRID[1] = GRID[7] = [1, 2, 3, 3, 2, 1]
ROOTS = [4096, 256, 64, 1]
CAP = 1024


def roots(n, seed):
    """n boards at mixed plies: board i is played uniformly at random for 1 + i % 12 plies (or to its end)
    (evaluate_bounce_rate.py's)"""
    b = BounceBatch(GRID, n, use_torch=True)
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
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn()   # (untimed: the variant before this one in the round may leave the chip in another clock state)
    torch.cuda.synchronize()
    start.record()
    for _ in range(reps):
        fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) / reps


def case(n, budget, policy, rounds, reps):
    b = roots(n, seed=4096)
    t = b.targets[:, :6]
    moves = np.array([[bin(int(m)).count("1") for m in row] for row in t]).sum(axis=1) * (b.winner == -1)
    running = int((moves > 0).sum())
    mean_moves = float(moves.sum()) / max(1, running)
    flat_playouts = max(1, int(budget // max(1.0, mean_moves)))
    slots = (n, 6, 54)
    flat_out = torch.empty(slots + (3,), dtype=torch.int32, device="cuda:0")
    outs = [torch.empty(s, dtype=torch.int32, device="cuda:0") for s in (slots + (3,), slots, (n,))]
    calls = {
        "flat": lambda: b.evaluate_moves_tensor(flat_out, seed=SEED, playouts=flat_playouts, max_plies=CAP, policy=policy),
        "halving": lambda: b.evaluate_moves_halving_tensor(*outs, seed=SEED, budget=budget, max_plies=CAP, policy=policy),
    }
    res = {}
    for name, call in calls.items():
        call()   # (warm-up)
        b.reset_steps()
        call()
        torch.cuda.synchronize()
        played = int(moves.sum()) * flat_playouts if name == "flat" else int(outs[1].sum())
        res[name] = {"env_steps": b.steps, "playouts_played": played,
                     "mean_plies_a_playout": round(b.steps / max(1, played), 3), "round_ms": []}
    res["halving"]["short_roots"] = int((outs[2] == HALVING_SHORT).sum())
    for _ in range(rounds):
        for name, call in calls.items():
            res[name]["round_ms"].append(round(device_ms(call, reps), 4))
    for v in res.values():
        ms = v["round_ms"]
        v["device_ms"] = statistics.median(ms)
        v["device_ms_least"], v["device_ms_greatest"] = min(ms), max(ms)
        v["env_steps_per_s_device"] = v["env_steps"] / (v["device_ms"] * 1e-3)
    row = {"roots": n, "running_roots": running, "mean_legal_moves": round(mean_moves, 3), "policy": policy, "budget": budget,
           "flat_playouts": flat_playouts, "max_plies": CAP, **res,
           "halving_vs_flat_ms": round(res["halving"]["device_ms"] / res["flat"]["device_ms"], 3)}
    b.close()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--budget", type=int, default=1024)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    res = {"tool": "tools/evaluate_bounce_halving_rate.py", "device": torch.cuda.get_device_name(0), "build_id": _abi.build_id(),
           "unit_ids": {**_abi.unit_ids(), **_abi.extra_unit_ids()}, "rounds": args.rounds, "reps": args.reps,
           "cases": [case(n, args.budget, policy, args.rounds, args.reps) for n in ROOTS for policy in ("uniform", "decisive")]}
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
