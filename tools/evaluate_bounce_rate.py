#!/usr/bin/env python3
"""Flat Monte-Carlo evaluation of Bounce boards (bgs_bounce_evaluate_moves) on one GPU against what a user builds without it.

On the default 9x6 board, for each (roots n, playouts P), on n mid-game roots, max_plies 1024:
  * evaluate   -- the one-launch kernel: device time per launch (events on the batch's stream, counts left on the device;
                  the longest launch seen is reported too) and end to end (counts in a host array);
  * tail       -- the same launches with the cap at 256 plies: (t(1024) - t(256)) / t(1024) is the share of a launch spent
                  on the few games that outlive 256 plies (1 in 10^4 of random games; the ones that never end run to the cap);
  * composed   -- replicate every root S * P times (S = W * H * W slots; the copies of illegal slots loaded as ended),
                  write_state, step_actions(slot move), rollout(seed, first_game * S * P, 1024), read the winners, count in
                  numpy: end to end, and the rollout launch's device time alone on the stepped boards.
Rates are env-steps per second counted on the device (the first moves included).  The composed counts and steps must equal
the kernel's (same game ids, same draws): `counts_equal`, `steps_equal`.

    python tools/evaluate_bounce_rate.py [--reps R] [--out FILE] [--kernel-only]
Prints one JSON object (and writes it to --out).  --kernel-only skips the composed path (A/B of launch settings through
BGS_EXPERIMENT with BGS_LIBRARY=libbgs_test.so: bounce_static_geom=0, bounce_eval_wps=N)."""
import argparse
import json
import os
import sys
import time

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
CAP, SHORT_CAP = 1024, 256


def roots(n, seed):
    """n boards at mixed plies: board i is played uniformly at random for 1 + i % 12 plies (or to its end)"""
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


def launch_ms(fn, reps):
    """per-launch device times (ms) of `reps` launches"""
    out = []
    for r in range(reps):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        fn(r)
        end.record()
        end.synchronize()
        out.append(start.elapsed_time(end))
    return out


def host_s(fn, reps):
    best = float("inf")
    for r in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn(r)
        best = min(best, time.perf_counter() - t0)
    return best


def case(n, playouts, reps, kernel_only):
    b = roots(n, seed=n + playouts)
    h, w = GRID.shape
    S = w * h * w
    grid, player, winner, plies = b.grid, b.player, b.winner, b.plies
    out = torch.empty((n, w, h * w, 3), dtype=torch.int32, device="cuda:0")
    # ---- the kernel
    b.evaluate_moves_tensor(out, seed=SEED, playouts=playouts, max_plies=CAP)   # (warm-up)
    b.reset_steps()
    b.evaluate_moves_tensor(out, seed=SEED, playouts=playouts, max_plies=CAP)
    torch.cuda.synchronize()
    steps = b.steps
    counts = out.cpu().numpy()
    times = launch_ms(lambda r: b.evaluate_moves_tensor(out, seed=SEED + 1 + r, playouts=playouts, max_plies=CAP), reps)
    short = launch_ms(lambda r: b.evaluate_moves_tensor(out, seed=SEED + 1 + r, playouts=playouts, max_plies=SHORT_CAP), reps)
    ms = float(np.median(times))
    e2e = host_s(lambda r: b.evaluate_moves(seed=SEED + 1 + r, playouts=playouts, max_plies=CAP), reps)
    legal_slots = int((counts.sum(-1) > 0).sum())
    res = {
        "board": "9x6 default", "roots": n, "playouts": playouts, "max_plies": CAP, "legal_slots": legal_slots,
        "evaluate": {"env_steps": steps, "device_ms_median": round(ms, 4), "device_ms_longest": round(max(times), 4),
                     "env_steps_per_s_device": steps / (ms * 1e-3), "end_to_end_ms": round(e2e * 1e3, 3),
                     "env_steps_per_s_end_to_end": steps / e2e,
                     "capped_playouts": int(legal_slots * playouts - counts.sum())},
        "tail": {"device_ms_median_cap_256": round(float(np.median(short)), 4),
                 "share_beyond_256_plies": round(1.0 - float(np.median(short)) / ms, 3)},
    }
    if kernel_only:
        b.close()
        return res
    # ---- the composed path: replicate, step, rollout, count
    m = n * S * playouts
    rep = BounceBatch(GRID, m, use_torch=True)
    t = b.targets
    rows = t[:, w].astype(np.int64)
    rows[rows > 64] = 0
    s = np.arange(S)
    x, c = s // (h * w), s % (h * w)
    legal = ((t[:, x] >> c.astype(np.uint64)) & np.uint64(1)) != 0          # [n, S]
    moves = np.stack([np.broadcast_to(x, (n, S)), np.broadcast_to(rows[:, None], (n, S)), np.broadcast_to(c % w, (n, S)),
                      np.broadcast_to(c // w, (n, S))], -1).astype(np.int32)
    moves = np.repeat(moves.reshape(n * S, 4), playouts, axis=0)
    ended = np.repeat(~legal.reshape(-1), playouts)
    roll = {}

    def composed(seed):
        rw = np.repeat(winner, S * playouts)
        rw[ended] = 2                       # illegal slots: loaded as ended, they drop out of the step and the rollout
        rep.write_state(np.repeat(grid, S * playouts, axis=0), np.repeat(player, S * playouts), rw, np.repeat(plies, S * playouts))
        rep.reset_steps()
        ok = rep.step_actions(moves) == 0
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        rep.set_first_game(0)
        rep.rollout(seed, max_plies=CAP)
        end.record()
        win = rep.winner.reshape(n, S, playouts)
        roll["ms"] = start.elapsed_time(end)
        roll["steps"] = rep.steps - int(ok.sum())
        okr = ok.reshape(n, S, playouts)
        mv = player.astype(np.int16)[:, None, None]
        cnt = np.stack([(okr & (win == mv)).sum(-1), (okr & (win == 2)).sum(-1), (okr & (win == 1 - mv)).sum(-1)], -1)
        return cnt.reshape(n, w, h * w, 3).astype(np.int32), rep.steps

    t0 = time.perf_counter()
    composed_counts, composed_steps = composed(SEED)
    composed_e2e = time.perf_counter() - t0
    rep.close()
    res["composed"] = {"games": m, "env_steps": composed_steps, "end_to_end_ms": round(composed_e2e * 1e3, 1),
                       "env_steps_per_s_end_to_end": composed_steps / composed_e2e,
                       "rollout_launch_ms": round(roll["ms"], 4), "rollout_env_steps": roll["steps"],
                       "rollout_env_steps_per_s_device": roll["steps"] / (roll["ms"] * 1e-3)}
    res["counts_equal"] = bool(np.array_equal(counts, composed_counts))
    res["steps_equal"] = steps == composed_steps
    res["evaluate_vs_composed_end_to_end"] = round(composed_e2e / e2e, 1)
    res["evaluate_vs_rollout_on_stepped_boards_device"] = round((steps / (ms * 1e-3)) / res["composed"]["rollout_env_steps_per_s_device"], 3)
    b.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=8)
    ap.add_argument("--out", default="")
    ap.add_argument("--kernel-only", action="store_true")
    args = ap.parse_args()
    res = {"tool": "tools/evaluate_bounce_rate.py", "device": torch.cuda.get_device_name(0), "build_id": _abi.build_id(),
           "unit_ids": {**_abi.unit_ids(), **_abi.extra_unit_ids()}, "reps": args.reps,
           "experiment": os.environ.get("BGS_EXPERIMENT", ""),
           "cases": [case(n, p, args.reps, args.kernel_only) for n, p in CASES]}
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")
    if not args.kernel_only and not all(c["counts_equal"] and c["steps_equal"] for c in res["cases"]):
        sys.exit("the composed path's counts or steps differ from the kernel's")


if __name__ == "__main__":
    main()
