#!/usr/bin/env python3
"""UCT tree search against sequential halving: two Monte-Carlo agents play N games of Connect4 at once, at the same
playouts a position.  Needs one MI355X.

The tree agent grows a UCT tree a position (ConnectBatch.search_actions_tensor: `iterations` iterations of
`leaf_playouts` playouts) and plays the column with the most visits.  The halving agent spends iterations *
leaf_playouts playouts a position by sequential halving (ConnectBatch.evaluate_actions_halving_tensor) and plays the
last surviving column.  Both use the playout policy given.  The tree agent is player 0 in the even games and player 1 in
the odd ones.  Every ply is one launch per agent over all games and one device-side step_actions call
(step_actions_observe): nothing crosses to the host until the games are over.

    python board-game-simulator-python_amd/examples/tree_match.py [--games 512] [--iterations 64] [--leaf-playouts 16]
        [--explore 65536] [--policy uniform]
"""

import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from simulator.batch import DEFAULT_EXPLORE, ConnectBatch


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", type=int, default=512)
    ap.add_argument("--iterations", type=int, default=64)
    ap.add_argument("--leaf-playouts", type=int, default=16)
    ap.add_argument("--explore", type=int, default=DEFAULT_EXPLORE)
    ap.add_argument("--policy", default="uniform", choices=("uniform", "decisive"))
    ap.add_argument("--seed", type=int, default=1)
    args = ap.parse_args()
    n, height, width = args.games, 6, 7
    budget = args.iterations * args.leaf_playouts
    games = ConnectBatch(height, width, 4, n, use_torch=True)
    tree_player = (torch.arange(n, device="cuda:0") % 2).to(torch.int32)
    legal = games.legal_tensor()
    tree = [None] * 4
    halving = [None] * 3
    for ply in range(height * width):
        games.set_first_game(ply * n)          # fresh game ids every ply
        tree = games.search_actions_tensor(*tree, seed=args.seed, iterations=args.iterations, leaf_playouts=args.leaf_playouts,
                                           explore=args.explore, policy=args.policy)
        halving = games.evaluate_actions_halving_tensor(*halving, seed=args.seed + 1, budget=budget, policy=args.policy)
        columns = torch.where(tree_player == (ply & 1), tree[2], halving[2]).contiguous()
        legal = games.step_actions_observe(columns, legal)
    winner = torch.as_tensor(games.winner, device="cuda:0").to(torch.int32)
    won = int((winner == tree_player).sum())
    drawn = int((winner == 2).sum())
    print(f"tree search ({args.iterations} x {args.leaf_playouts}, explore {args.explore}) against halving (budget {budget}), "
          f"{args.policy} playouts, {n} games of Connect4: won {won}, drew {drawn}, lost {n - won - drawn}; "
          f"score {(won + 0.5 * drawn) / n:.3f}")
    games.close()


if __name__ == "__main__":
    main()
