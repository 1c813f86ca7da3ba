#!/usr/bin/env python3
"""Tree search that keeps its trees against tree search that does not: two UCT agents play N games of Connect4 at once,
at the same iterations a move.  Needs one MI355X.

Both agents run `iterations` iterations of `leaf_playouts` playouts at each of their moves.  The plain agent starts from
an empty root every time (ConnectBatch.search_actions_tensor).  The reuse agent owns a forest (ConnectBatch.search_forest):
after every ply, its own or the opponent's, the forest is advanced by the columns played, so its next search starts from
the subtree under the two stones that came since its last one.  The games are two batches of N / 2: the reuse agent moves
first in one and second in the other, so each ply is one search launch a batch, one advance launch and one device-side
step (step_actions_observe); nothing crosses to the host until the games are over.

    python board-game-simulator-python_amd/examples/tree_reuse_match.py [--games 512] [--iterations 64] [--leaf-playouts 16]
        [--capacity 2 * iterations + 1] [--explore 65536] [--policy uniform] [--json]
"""

import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from simulator.batch import DEFAULT_EXPLORE, ConnectBatch


def play(games: int, iterations: int, leaf_playouts: int, capacity: int, explore: int, policy: str, seed: int) -> dict:
    """the match; {"won", "drawn", "lost", "score"} of the reuse agent and its "mean_carried" nodes a search"""
    half, height, width = games // 2, 6, 7
    kw = dict(iterations=iterations, leaf_playouts=leaf_playouts, explore=explore, policy=policy)
    sides = []      # (batch, forest, the plies' parity at which the reuse agent moves)
    for parity in (0, 1):
        batch = ConnectBatch(height, width, 4, half, use_torch=True)
        sides.append((batch, batch.search_forest(capacity), parity))
    legal = [batch.legal_tensor() for batch, _, _ in sides]
    carried_sum = torch.zeros((), dtype=torch.int64, device="cuda:0")
    searched = torch.zeros((), dtype=torch.int64, device="cuda:0")
    for ply in range(height * width):
        for k, (batch, forest, parity) in enumerate(sides):
            batch.set_first_game((2 * ply + k) * half)          # fresh game ids every ply and batch
            if ply % 2 == parity:
                _, _, best, _, carried = forest.search_tensor(seed=seed + ply, **kw)
                running = best >= 0
                carried_sum += carried[running].sum()
                searched += running.sum()
            else:
                best = batch.search_actions_tensor(seed=seed + 1000 + ply, **kw)[2]
            forest.advance_tensor(best)                         # (an ended board has best = -1: its tree is left alone)
            legal[k] = batch.step_actions_observe(best, legal[k])
    won = drawn = 0
    for batch, forest, parity in sides:
        winner = torch.as_tensor(batch.winner)
        won += int((winner == parity).sum())
        drawn += int((winner == 2).sum())
        forest.close()
        batch.close()
    total = 2 * half
    return {"games": total, "won": won, "drawn": drawn, "lost": total - won - drawn, "score": (won + 0.5 * drawn) / total,
            "mean_carried": float(carried_sum) / max(int(searched), 1), "searches": int(searched)}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", type=int, default=512)
    ap.add_argument("--iterations", type=int, default=64)
    ap.add_argument("--leaf-playouts", type=int, default=16)
    ap.add_argument("--capacity", type=int, default=0, help="nodes a tree; 0: 2 * iterations + 1")
    ap.add_argument("--explore", type=int, default=DEFAULT_EXPLORE)
    ap.add_argument("--policy", default="uniform", choices=("uniform", "decisive"))
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--json", action="store_true", help="print the result as one JSON line")
    args = ap.parse_args()
    capacity = args.capacity or 2 * args.iterations + 1
    res = play(args.games, args.iterations, args.leaf_playouts, capacity, args.explore, args.policy, args.seed)
    if args.json:
        print(json.dumps({**res, "iterations": args.iterations, "leaf_playouts": args.leaf_playouts, "capacity": capacity,
                          "explore": args.explore, "policy": args.policy}))
        return
    print(f"tree search with reuse ({args.iterations} x {args.leaf_playouts}, {capacity} nodes a tree) against the same search "
          f"without, {args.policy} playouts, {res['games']} games of Connect4: won {res['won']}, drew {res['drawn']}, lost "
          f"{res['lost']}; score {res['score']:.3f}; {res['mean_carried']:.1f} nodes carried into a search on average")


if __name__ == "__main__":
    main()
