#!/usr/bin/env python3
"""What sequential halving costs a launch next to the flat evaluation of the same build, on the same roots and at the
same playouts a root.

For the two shapes of profiles/evaluate_rate.json (Connect4 and 12x13x5, 4096 roots at mixed plies x 256 playouts a
column) and for n = 1 and n = 64 roots of each (one team of lanes owns a root: few roots leave most of the chip idle),
two variants are timed in one process, alternating, `--rounds` times `--reps` launches each after one untimed launch
(device events on the batch's stream, outputs left on the device):
  * flat     -- evaluate_actions(playouts = budget // width);
  * halving  -- evaluate_actions_halving(budget), budget = 256 * width.
Per variant: the launch time (median over the rounds, and the rounds' least and greatest), the env-steps of one launch
(counted on the device, first moves included), env-steps/s, and the mean plies a playout (env-steps over the playouts
played: halving, the sum of `given`).

    python tools/evaluate_halving_rate.py [--rounds R] [--reps K] [--policy uniform] [--geometry H W K] [--out profiles/evaluate_halving_rate.json]
--geometry H W K: that board at 4096 roots in place of the case list (a two-word board, say: 6 12 4).
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

from simulator.batch import ConnectBatch
from simulator.game import _abi

SEED = 0x0123456789ABCDEF
PLAYOUTS = 256
CASES = [((6, 7, 4), 4096), ((12, 13, 5), 4096), ((6, 7, 4), 64), ((12, 13, 5), 64), ((6, 7, 4), 1), ((12, 13, 5), 1)]


def roots(h, w, k, n, seed):
    """n boards at mixed plies: board i is played uniformly at random to min(i % (h * w / 3), its end) (evaluate_rate.py's)"""
    b = ConnectBatch(h, w, k, n, use_torch=True)
    rng = np.random.default_rng(seed)
    target = np.arange(n) % max(1, h * w // 3)
    for ply in range(int(target.max())):
        legal = b.legal.astype(bool)
        pick = (rng.random((n, w)) * legal).argmax(axis=1).astype(np.int32)
        cols = np.where((target > ply) & legal.any(axis=1), pick, -1).astype(np.int32)
        b.step_actions(cols, want_status=False)
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


def case(geom, n, policy, rounds, reps):
    h, w, k = geom
    b = roots(h, w, k, n, seed=4096 + PLAYOUTS)
    budget = PLAYOUTS * w
    flat_out = torch.empty((n, w, 3), dtype=torch.int32, device="cuda:0")
    outs = [torch.empty(s, dtype=torch.int32, device="cuda:0") for s in ((n, w, 3), (n, w), (n,))]
    calls = {
        "flat": lambda: b.evaluate_actions_tensor(flat_out, seed=SEED, playouts=budget // w, policy=policy),
        "halving": lambda: b.evaluate_actions_halving_tensor(*outs, seed=SEED, budget=budget, policy=policy),
    }
    res = {}
    for name, call in calls.items():
        call()   # (warm-up)
        b.reset_steps()
        call()
        torch.cuda.synchronize()
        played = int(b.legal.astype(bool).sum()) * (budget // w) if name == "flat" else int(outs[1].sum())
        res[name] = {"env_steps": b.steps, "playouts_played": played,
                     "mean_plies_a_playout": round(b.steps / max(1, played), 3), "round_ms": []}
    for _ in range(rounds):
        for name, call in calls.items():
            res[name]["round_ms"].append(round(device_ms(call, reps), 4))
    for v in res.values():
        ms = v["round_ms"]
        v["device_ms"] = statistics.median(ms)
        v["device_ms_least"], v["device_ms_greatest"] = min(ms), max(ms)
        v["env_steps_per_s_device"] = v["env_steps"] / (v["device_ms"] * 1e-3)
    row = {"geometry": "x".join(map(str, geom)), "roots": n, "budget": budget, "flat_playouts": budget // w, **res,
           "halving_vs_flat_ms": round(res["halving"]["device_ms"] / res["flat"]["device_ms"], 3),
           "halving_vs_flat_env_steps_per_s": round(res["halving"]["env_steps_per_s_device"] / res["flat"]["env_steps_per_s_device"], 3)}
    b.close()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=4)
    ap.add_argument("--policy", default="uniform", choices=("uniform", "decisive"))
    ap.add_argument("--geometry", type=int, nargs=3, metavar=("H", "W", "K"))
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    cases = [(tuple(args.geometry), 4096)] if args.geometry else CASES
    res = {"tool": "tools/evaluate_halving_rate.py", "device": torch.cuda.get_device_name(0), "build_id": _abi.build_id(),
           "unit_ids": {**_abi.unit_ids(), **_abi.extra_unit_ids()}, "rounds": args.rounds, "reps": args.reps, "policy": args.policy,
           "cases": [case(g, n, args.policy, args.rounds, args.reps) for g, n in cases]}
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
