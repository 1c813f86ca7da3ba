#!/usr/bin/env python3
"""Flat Monte-Carlo evaluation (bgs_connect_evaluate_actions) on one GPU against what a user builds without it.

For each geometry and (roots n, playouts P), on n roots at mixed plies:
  * evaluate   -- the one-launch kernel: device time (events on the batch's stream, counts left on the device) and end to
                  end (counts in a host array);
  * composed   -- replicate every root W * P times (write_state), step_actions(column), rollout(seed, first_game * W * P),
                  read the winners, count in numpy: end to end, and the rollout launch's device time alone;
  * rollout    -- a plain from-the-start rollout() of n * W * P boards (the README's fused-rollout figure), device time.
Rates are env-steps per second, counted on the device (the evaluation's and the composed path's steps include the first
moves).  The composed counts must equal the kernel's (same game ids, same draws): `counts_equal` says whether they did;
the two env-step totals are reported side by side (`steps_equal`).

    python tools/evaluate_rate.py [--reps R] [--out FILE] [--kernel-only]
Prints one JSON object (and writes it to --out).  --kernel-only times the kernel alone and skips the composed path and the
plain rollout (A/B runs of two libraries through BGS_LIBRARY)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "board-game-simulator-python_amd")]
import numpy as np
import torch

from simulator.batch import ConnectBatch
from simulator.game import _abi

SEED = 0x0123456789ABCDEF
CASES = [((6, 7, 4), 4096, 256), ((6, 7, 4), 1 << 16, 16), ((12, 13, 5), 4096, 256), ((12, 13, 5), 1 << 16, 16)]


def roots(h, w, k, n, seed):
    """n boards at mixed plies: board i is played uniformly at random to min(i % (h * w / 3), its end)"""
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
    torch.cuda.synchronize()
    start.record()
    for r in range(reps):
        fn(r)
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) / reps


def host_s(fn, reps):
    best = float("inf")
    for r in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn(r)
        best = min(best, time.perf_counter() - t0)
    return best


def case(geom, n, playouts, reps, kernel_only):
    h, w, k = geom
    b = roots(h, w, k, n, seed=n + playouts)
    grid, player, winner, plies = b.grid, b.player, b.winner, b.plies
    out = torch.empty((n, w, 3), dtype=torch.int32, device="cuda:0")
    # ---- the kernel
    b.evaluate_actions_tensor(out, seed=SEED, playouts=playouts)   # (warm-up)
    b.reset_steps()
    b.evaluate_actions_tensor(out, seed=SEED, playouts=playouts)
    torch.cuda.synchronize()
    steps = b.steps
    counts = out.cpu().numpy()
    ms = device_ms(lambda r: b.evaluate_actions_tensor(out, seed=SEED + 1 + r, playouts=playouts), reps)
    e2e = host_s(lambda r: b.evaluate_actions(seed=SEED + 1 + r, playouts=playouts), reps)
    if kernel_only:
        b.close()
        return {"geometry": "x".join(map(str, geom)), "roots": n, "playouts": playouts,
                "evaluate": {"env_steps": steps, "device_ms": round(ms, 4), "env_steps_per_s_device": steps / (ms * 1e-3),
                             "end_to_end_ms": round(e2e * 1e3, 3), "env_steps_per_s_end_to_end": steps / e2e}}

    # ---- the composed path: replicate, step, rollout, count
    m = n * w * playouts
    rep = ConnectBatch(h, w, k, m, use_torch=True)
    cols = np.tile(np.repeat(np.arange(w, dtype=np.int32), playouts), n)
    roll_ms = []

    def composed(seed):
        rep.write_state(np.repeat(grid, w * playouts, axis=0), np.repeat(player, w * playouts),
                        np.repeat(winner, w * playouts), np.repeat(plies, w * playouts))
        ok = rep.step_actions(cols) == 0
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        rep.set_first_game(0)
        rep.rollout(seed)
        end.record()
        win = rep.winner.reshape(n, w, playouts)
        roll_ms.append(start.elapsed_time(end))
        okr = ok.reshape(n, w, playouts)
        mv = player.astype(np.int16)[:, None, None]
        return np.stack([(okr & (win == mv)).sum(-1), (okr & (win == 2)).sum(-1), (okr & (win == 1 - mv)).sum(-1)], -1)

    rep.reset_steps()
    composed_counts = composed(SEED)
    composed_steps = rep.steps
    composed_e2e = host_s(lambda r: composed(SEED + 1 + r), max(1, reps // 4))
    rollout_ms = min(roll_ms)
    # ---- a plain from-the-start rollout of the same number of games
    rep.rollout(SEED, from_initial=True)
    rep.reset_steps()
    rep.rollout(SEED + 1, from_initial=True)
    torch.cuda.synchronize()
    plain_steps = rep.steps
    plain_ms = device_ms(lambda r: rep.rollout(SEED + 1, from_initial=True), reps)
    rep.close()
    return {
        "geometry": "x".join(map(str, geom)), "roots": n, "playouts": playouts, "games": m,
        "evaluate": {"env_steps": steps, "device_ms": round(ms, 4), "env_steps_per_s_device": steps / (ms * 1e-3),
                     "end_to_end_ms": round(e2e * 1e3, 3), "env_steps_per_s_end_to_end": steps / e2e},
        "composed": {"env_steps": composed_steps, "end_to_end_ms": round(composed_e2e * 1e3, 3),
                     "env_steps_per_s_end_to_end": composed_steps / composed_e2e, "rollout_launch_ms": round(rollout_ms, 4)},
        "plain_rollout_from_start": {"env_steps": plain_steps, "device_ms": round(plain_ms, 4),
                                     "env_steps_per_s_device": plain_steps / (plain_ms * 1e-3)},
        "counts_equal": bool(np.array_equal(counts, composed_counts)), "steps_equal": steps == composed_steps,
        "evaluate_vs_plain_rollout_device": round((steps / ms) / (plain_steps / plain_ms), 3),
        "evaluate_vs_composed_end_to_end": round(composed_e2e / e2e, 2),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=8)
    ap.add_argument("--out", default="")
    ap.add_argument("--kernel-only", action="store_true")
    args = ap.parse_args()
    res = {"tool": "tools/evaluate_rate.py", "device": torch.cuda.get_device_name(0), "build_id": _abi.build_id(),
           "unit_ids": {**_abi.unit_ids(), **_abi.extra_unit_ids()}, "reps": args.reps,
           "cases": [case(g, n, p, args.reps, args.kernel_only) for g, n, p in CASES]}
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")
    if not args.kernel_only and not all(c["counts_equal"] for c in res["cases"]):
        sys.exit("the composed path's counts differ from the kernel's")


if __name__ == "__main__":
    main()
