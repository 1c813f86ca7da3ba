#!/usr/bin/env python3
"""Playout policies of the Bounce flat Monte-Carlo evaluation on one GPU: what the decisive policy does to a launch, and
that the uniform policy costs the same through either entry point.

For the two shapes of profiles/evaluate_bounce_rate.json (default 9x6 board, mixed-ply roots, max_plies 1024: 256 roots x
256 playouts and 4096 x 64) three variants are timed in one process, alternating, `--rounds` times `--reps` launches each
after one untimed launch (device events on the batch's stream, counts left on the device):
  * uniform_old  -- bgs_bounce_evaluate_moves;
  * uniform_new  -- bgs_bounce_evaluate_moves_policy(BGS_POLICY_UNIFORM);
  * decisive     -- bgs_bounce_evaluate_moves_policy(BGS_POLICY_DECISIVE).
Per variant: the launch time (median over the rounds, and the rounds' least and greatest: the run-to-run spread), the
env-steps of one launch (counted on the device, first moves included), env-steps/s, playouts/s (the figure to compare
across policies: decisive playouts are shorter) and the mean plies a playout (env-steps over the playouts that start:
legal moves of running roots x playouts).  A library without the policy entry point (the parent commit's, for the
same-day comparison) gives uniform_old alone.

    python tools/evaluate_bounce_policy_rate.py [--rounds R] [--reps K] [--out FILE]
Prints one JSON object (and writes it to --out)."""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "board-game-simulator-python_amd")]
import numpy as np
import torch

from simulator.batch import BounceBatch
from simulator.game import _abi

SEED = 0x0123456789ABCDEF
GRID = np.zeros((9, 6), dtype=np.int8)
GRID[1] = GRID[7] = [1, 2, 3, 3, 2, 1]
CASES = [(256, 256), (4096, 64)]
CAP = 1024
POLICY_UNIFORM, POLICY_DECISIVE = 0, 1


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


def variants(lib):
    def old(b, out, seed, playouts):
        _abi.check(lib.bgs_bounce_evaluate_moves(b._handle, ctypes.c_uint64(seed), playouts, CAP, ctypes.c_void_p(out.data_ptr()), 1))

    def new(policy):
        def call(b, out, seed, playouts):
            _abi.check(lib.bgs_bounce_evaluate_moves_policy(b._handle, ctypes.c_uint64(seed), playouts, CAP, policy,
                                                            ctypes.c_void_p(out.data_ptr()), 1))
        return call

    out = {"uniform_old": old}
    if hasattr(lib, "bgs_bounce_evaluate_moves_policy"):
        out["uniform_new"] = new(POLICY_UNIFORM)
        out["decisive"] = new(POLICY_DECISIVE)
    return out


def device_ms(fn, reps):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn(-1)   # (untimed: the variant before this one in the round may leave the chip in another clock state)
    torch.cuda.synchronize()
    start.record()
    for r in range(reps):
        fn(r)
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) / reps


def case(n, playouts, rounds, reps, calls):
    b = roots(n, seed=n + playouts)
    h, w = GRID.shape
    t = b.targets[:, :w]
    legal = (((t[..., None] >> np.arange(h * w, dtype=np.uint64)) & np.uint64(1)) != 0) & (b.winner == -1)[:, None, None]
    started = int(legal.sum()) * playouts
    out = torch.empty((n, w, h * w, 3), dtype=torch.int32, device="cuda:0")
    res, counts = {}, {}
    for name, call in calls.items():
        call(b, out, SEED, playouts)   # (warm-up)
        b.reset_steps()
        call(b, out, SEED, playouts)
        torch.cuda.synchronize()
        res[name] = {"env_steps": b.steps, "mean_plies_a_playout": round(b.steps / started, 3), "round_ms": []}
        counts[name] = out.cpu().numpy()
    for r in range(rounds):
        for name, call in calls.items():
            res[name]["round_ms"].append(round(device_ms(lambda i: call(b, out, SEED, playouts), reps), 4))
    for name, v in res.items():
        ms = v["round_ms"]
        v["device_ms"] = statistics.median(ms)
        v["device_ms_least"], v["device_ms_greatest"] = min(ms), max(ms)
        v["env_steps_per_s_device"] = v["env_steps"] / (v["device_ms"] * 1e-3)
        v["playouts_per_s_device"] = started / (v["device_ms"] * 1e-3)
        v["capped_playouts"] = int(started - counts[name].sum())
    row = {"board": "9x6 default", "roots": n, "playouts": playouts, "max_plies": CAP, "playouts_started": started, **res}
    if "uniform_new" in res:
        row["uniform_counts_equal"] = bool(np.array_equal(counts["uniform_old"], counts["uniform_new"]))
        row["uniform_steps_equal"] = res["uniform_old"]["env_steps"] == res["uniform_new"]["env_steps"]
        row["uniform_new_vs_old_ms"] = round(res["uniform_new"]["device_ms"] / res["uniform_old"]["device_ms"], 4)
        row["decisive_vs_uniform_ms"] = round(res["decisive"]["device_ms"] / res["uniform_old"]["device_ms"], 3)
        row["decisive_vs_uniform_playouts_per_s"] = round(res["uniform_old"]["device_ms"] / res["decisive"]["device_ms"], 3)
        row["decisive_vs_uniform_plies"] = round(res["decisive"]["env_steps"] / res["uniform_old"]["env_steps"], 3)
    b.close()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=4)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    calls = variants(_abi.lib())
    units = {**_abi.unit_ids(), **_abi.extra_unit_ids()}
    res = {"tool": "tools/evaluate_bounce_policy_rate.py", "device": torch.cuda.get_device_name(0), "build_id": _abi.build_id(),
           "unit_ids": units, "evaluate_unit_id": units.get("evaluate"), "rounds": args.rounds, "reps": args.reps,
           "variants": list(calls), "cases": [case(n, p, args.rounds, args.reps, calls) for n, p in CASES]}
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")
    if not all(c.get("uniform_counts_equal", True) and c.get("uniform_steps_equal", True) for c in res["cases"]):
        sys.exit("the uniform policy's counts differ between the two entry points")


if __name__ == "__main__":
    main()
