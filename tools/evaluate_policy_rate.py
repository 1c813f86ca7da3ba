#!/usr/bin/env python3
"""Playout policies of the flat Monte-Carlo evaluation on one GPU: what the decisive policy costs a launch, and that the
uniform policy costs the same through either entry point.

For the two shapes of profiles/evaluate_rate.json (Connect4 and 12x13x5, 4096 roots at mixed plies x 256 playouts) three
variants are timed in one process, alternating, `--rounds` times `--reps` launches each after one untimed launch (device
events on the batch's stream, counts left on the device):
  * uniform_old  -- bgs_connect_evaluate_actions;
  * uniform_new  -- bgs_connect_evaluate_actions_policy(BGS_POLICY_UNIFORM);
  * decisive     -- bgs_connect_evaluate_actions_policy(BGS_POLICY_DECISIVE).
Per variant: the launch time (median over the rounds, and the rounds' least and greatest: the run-to-run spread), the
env-steps of one launch (counted on the device, first moves included), env-steps/s, and the mean plies a playout (env-steps
over the playouts that start: legal columns of running roots x playouts).  A library without the policy entry point (the
parent commit's, for the same-day comparison) gives uniform_old alone.

    python tools/evaluate_policy_rate.py [--rounds R] [--reps K] [--geometry H W K] [--out FILE]
--geometry H W K: that board at 4096 roots x 256 playouts in place of the two shapes (a two-word board, say: 6 12 4).
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

from simulator.batch import ConnectBatch
from simulator.game import _abi

SEED = 0x0123456789ABCDEF
CASES = [((6, 7, 4), 4096, 256), ((12, 13, 5), 4096, 256)]
POLICY_UNIFORM, POLICY_DECISIVE = 0, 1


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


def variants(lib):
    def old(b, out, seed, playouts):
        _abi.check(lib.bgs_connect_evaluate_actions(b._handle, ctypes.c_uint64(seed), playouts, 2**31 - 1, ctypes.c_void_p(out.data_ptr()), 1))

    def new(policy):
        def call(b, out, seed, playouts):
            _abi.check(lib.bgs_connect_evaluate_actions_policy(b._handle, ctypes.c_uint64(seed), playouts, 2**31 - 1, policy,
                                                               ctypes.c_void_p(out.data_ptr()), 1))
        return call

    out = {"uniform_old": old}
    if hasattr(lib, "bgs_connect_evaluate_actions_policy"):
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


def case(geom, n, playouts, rounds, reps, calls):
    h, w, k = geom
    b = roots(h, w, k, n, seed=n + playouts)
    started = int(b.legal.astype(bool).sum()) * playouts   # (an ended board has no legal column)
    out = torch.empty((n, w, 3), dtype=torch.int32, device="cuda:0")
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
    row = {"geometry": "x".join(map(str, geom)), "roots": n, "playouts": playouts, "playouts_started": started, **res}
    if "uniform_new" in res:
        row["uniform_counts_equal"] = bool(np.array_equal(counts["uniform_old"], counts["uniform_new"]))
        row["uniform_steps_equal"] = res["uniform_old"]["env_steps"] == res["uniform_new"]["env_steps"]
        row["uniform_new_vs_old_ms"] = round(res["uniform_new"]["device_ms"] / res["uniform_old"]["device_ms"], 4)
        row["decisive_vs_uniform_ms"] = round(res["decisive"]["device_ms"] / res["uniform_old"]["device_ms"], 3)
        row["decisive_vs_uniform_env_steps_per_s"] = round(res["decisive"]["env_steps_per_s_device"] / res["uniform_old"]["env_steps_per_s_device"], 3)
        row["decisive_vs_uniform_plies"] = round(res["decisive"]["env_steps"] / res["uniform_old"]["env_steps"], 3)
    b.close()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=4)
    ap.add_argument("--geometry", type=int, nargs=3, metavar=("H", "W", "K"))
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    cases = [(tuple(args.geometry), 4096, 256)] if args.geometry else CASES
    calls = variants(_abi.lib())
    res = {"tool": "tools/evaluate_policy_rate.py", "device": torch.cuda.get_device_name(0), "build_id": _abi.build_id(),
           "unit_ids": {**_abi.unit_ids(), **_abi.extra_unit_ids()}, "rounds": args.rounds, "reps": args.reps,
           "variants": list(calls), "cases": [case(g, n, p, args.rounds, args.reps, calls) for g, n, p in cases]}
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
