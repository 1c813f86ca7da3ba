#!/usr/bin/env python3
"""Sequential halving against the flat allocation: two Monte-Carlo agents play N games of Connect4 at once, at the same
total playouts a position.  Needs one MI355X.

The flat agent values every legal column by `playouts` random games (ConnectBatch.evaluate_actions_tensor) and plays the
best one.  The halving agent spends `playouts * width` games a position by sequential halving
(ConnectBatch.evaluate_actions_halving_tensor) and plays the last surviving column.  Both use the playout policy given.
The halving agent is player 0 in the even games and player 1 in the odd ones.  Every ply is one launch per agent over all
games, an argmax on the device for the flat agent, and one device-side step_actions call (step_actions_observe, which
also returns the next legal mask): nothing crosses to the host until the games are over.

    python board-game-simulator-python_amd/examples/halving_match.py [--games 512] [--playouts 64] [--policy uniform]
"""

import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from simulator.batch import ConnectBatch


def best_columns(counts, legal, playouts):
    """the legal column with the greatest (wins + draws / 2) / playouts of every game; -1 where no column is legal"""
    value = (counts[..., 0].float() + 0.5 * counts[..., 1].float()) / playouts
    value = torch.where(legal.bool(), value, torch.full_like(value, -1.0))
    return torch.where(legal.bool().any(dim=1), value.argmax(dim=1), torch.full_like(value.argmax(dim=1), -1)).to(torch.int32)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", type=int, default=512)
    ap.add_argument("--playouts", type=int, default=64)
    ap.add_argument("--policy", default="uniform", choices=("uniform", "decisive"))
    ap.add_argument("--seed", type=int, default=1)
    args = ap.parse_args()
    n, height, width = args.games, 6, 7
    games = ConnectBatch(height, width, 4, n, use_torch=True)
    halving_player = (torch.arange(n, device="cuda:0") % 2).to(torch.int32)
    legal = games.legal_tensor()
    flat = torch.empty((n, width, 3), dtype=torch.int32, device="cuda:0")
    counts = given = best = None
    for ply in range(height * width):
        games.set_first_game(ply * n)          # fresh game ids every ply
        games.evaluate_actions_tensor(flat, seed=args.seed, playouts=args.playouts, policy=args.policy)
        counts, given, best = games.evaluate_actions_halving_tensor(counts, given, best, seed=args.seed + 1,
                                                                    budget=args.playouts * width, policy=args.policy)
        theirs = best_columns(flat, legal, args.playouts)
        columns = torch.where(halving_player == (ply & 1), best, theirs).contiguous()
        legal = games.step_actions_observe(columns, legal)
    winner = torch.as_tensor(games.winner, device="cuda:0").to(torch.int32)
    won = int((winner == halving_player).sum())
    drawn = int((winner == 2).sum())
    print(f"halving against flat, {args.policy} playouts ({args.playouts} x {width} a position), {n} games of Connect4: "
          f"won {won}, drew {drawn}, lost {n - won - drawn}; score {(won + 0.5 * drawn) / n:.3f}")
    games.close()


if __name__ == "__main__":
    main()
