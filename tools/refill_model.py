#!/usr/bin/env python3
"""CPU model of the lane-refill loop of the Connect4(6,7,4) rollout (k_connect_rollout_opened and its grouped form,
docs/EXPERIMENTS.md §29): how many loop iterations a wave runs per step, from the oracle's game lengths alone.

A game enters the loop where the deferred opening (§27) parked it: at block 1 if stage 1 flags it (it ended by ply 12, or a
column was full after 11 plies), at block 3 if stage 2 flags it (not flagged before; it ended by ply 16, or a column was
full after 15 plies), else at block 4.  It then needs (plies - 1) // 4 - start + 1 iterations of one lane.  A wave is 64
lanes over a chunk of consecutive games: every iteration the idle lanes take the chunk's next games in order, then every
live lane plays one block.  With S steps a launch the lanes that find step s handed out go on with the same chunk of step
s + 1 (seed + 1), but only once no game of step s - 1 is playing any more -- at most two steps of a wave are open.

    python tools/refill_model.py [--games 131072] [--seed 0x0123456789ABCDEF]

prints iterations per wave and step for chunks of 512, 1024 and 4096 games and 1, 2, 3 and 8 steps a launch, next to the
ideal (no lane ever idle: the chunk's lane-iterations / 64), and the flag rates.  Nothing here runs on a GPU."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import oracle  # noqa: E402

LANES = 64


def lane_iterations(seed, games, first=0):
    """iterations of one lane that every game needs, and the two flag rates"""
    def capped(cap):
        orc = oracle.ConnectOracle(6, 7, 4, games)
        orc.rollout(seed, first_game=first, max_plies=cap)
        return orc.ended.copy(), (orc.grid != -1).sum(axis=1).max(axis=1)   # ended, the tallest column

    full = oracle.ConnectOracle(6, 7, 4, games)
    full.rollout(seed, first_game=first)
    plies = full.plies.astype(np.int64)
    ended11, tall11 = capped(11)
    ended12, _ = capped(12)
    ended15, tall15 = capped(15)
    ended16, _ = capped(16)
    stage1 = ended12 | (~ended11 & (tall11 == 6))
    stage2 = ~stage1 & (ended16 | (~ended15 & (tall15 == 6)))
    start = np.where(stage1, 1, np.where(stage2, 3, 4))
    need = (plies - 1) // 4 - start + 1
    assert need.min() >= 1
    return need, float(stage1.mean()), float(stage2.mean())


def wave_iterations(chunks):
    """loop iterations of one wave that plays `chunks` -- its chunk of every step of the launch, in order"""
    steps = len(chunks)
    left = np.zeros(LANES, dtype=np.int64)      # blocks the lane's game still needs
    of = np.zeros(LANES, dtype=np.int64)        # the step the lane's game is of
    cur, taken, pending, count = 0, 0, False, 0
    while True:
        idle = np.flatnonzero(left == 0)
        if idle.size and (taken < len(chunks[cur]) or cur + 1 < steps):
            served = min(idle.size, len(chunks[cur]) - taken)
            left[idle[:served]] = chunks[cur][taken:taken + served]
            of[idle[:served]] = cur
            taken += served
            if served < idle.size and cur + 1 < steps and not pending:
                cur, pending = cur + 1, True
                rest = idle[served:]
                taken = min(rest.size, len(chunks[cur]))
                left[rest[:taken]] = chunks[cur][:taken]
                of[rest[:taken]] = cur
        if not left.any() and taken >= len(chunks[cur]) and cur + 1 >= steps:
            return count
        left[left > 0] -= 1
        count += 1
        if pending and not ((left > 0) & (of == cur - 1)).any():
            pending = False


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", type=int, default=1 << 17)
    ap.add_argument("--seed", type=lambda s: int(s, 0), default=0x0123456789ABCDEF)
    args = ap.parse_args()
    group_sizes = (1, 2, 3, 8)
    need, rates = [], None
    for s in range(max(group_sizes)):
        n, r1, r2 = lane_iterations(args.seed + s, args.games)
        need.append(n)
        rates = rates or (r1, r2)
    print(f"{args.games} games, seed 0x{args.seed:016X}: stage 1 flags {100 * rates[0]:.2f} %, stage 2 {100 * rates[1]:.2f} %; "
          f"{need[0].mean():.3f} lane-iterations a game")
    for chunk in (512, 1024, 4096):
        waves = args.games // chunk
        ideal = sum(n[:waves * chunk].sum() for n in need) / (LANES * waves * len(need))
        print(f"chunk {chunk}: ideal {ideal:.2f} iterations a wave and step")
        for steps in group_sizes:
            total = launches = 0
            for first in range(0, max(group_sizes) - steps + 1, steps):   # the launches that fit the steps modelled
                for w in range(waves):
                    total += wave_iterations([need[s][w * chunk:(w + 1) * chunk] for s in range(first, first + steps)])
                launches += 1
            print(f"  {steps} step(s) a launch: {total / (waves * launches * steps):.2f}")


if __name__ == "__main__":
    main()
