#!/usr/bin/env python3
"""Tree search that keeps its trees against tree search that does not: two UCT agents play N games of Bounce on the
default 9x6 board at once, at the same iterations a move.  Needs one MI355X.

Both agents run `iterations` iterations of `leaf_playouts` playouts at each of their moves.  The plain agent starts from a
bare root every time (BounceBatch.search_moves_tensor).  The reuse agent owns a forest (BounceBatch.search_moves_forest):
after every ply, its own or the opponent's, the forest is advanced by the slot played, so its next search starts from the
subtree under the two moves that came since its last one.  The games are two batches of N / 2: the reuse agent moves first
in one and second in the other, so each ply is one search launch a batch, one advance launch and one device-side step
(step_actions_observe); nothing crosses to the host until the games are over.  A game that holds `--max-plies` plies is
cut there and counted as a draw.

    python board-game-simulator-python_amd/examples/tree_reuse_match_bounce.py [--games 256] [--iterations 64]
        [--leaf-playouts 16] [--capacity 2 * iterations + 1] [--explore 65536] [--policy uniform] [--max-plies 200] [--json]
"""

import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

from simulator.batch import DEFAULT_EXPLORE, BounceBatch


def play(games: int, iterations: int, leaf_playouts: int, capacity: int, explore: int, policy: str, max_plies: int, seed: int) -> dict:
    """the match; {"won", "drawn", "lost", "score"} of the reuse agent and its "mean_carried" nodes a search"""
    half = games // 2
    grid = np.zeros((9, 6), dtype=np.int8)
    grid[1] = grid[7] = [1, 2, 3, 3, 2, 1]
    kw = dict(iterations=iterations, leaf_playouts=leaf_playouts, explore=explore, policy=policy, max_plies=1024)
    sides = []      # (batch, forest, the plies' parity at which the reuse agent moves)
    for parity in (0, 1):
        batch = BounceBatch(grid, half, use_torch=True)
        sides.append((batch, batch.search_moves_forest(capacity), parity))
    targets = [batch.targets_tensor() for batch, _, _ in sides]
    carried_sum = torch.zeros((), dtype=torch.int64, device="cuda:0")
    searched = torch.zeros((), dtype=torch.int64, device="cuda:0")
    for ply in range(max_plies):
        for k, (batch, forest, parity) in enumerate(sides):
            batch.set_first_game((2 * ply + k) * half)          # fresh game ids every ply and batch
            if ply % 2 == parity:
                _, _, best, _, _, carried = forest.search_tensor(seed=seed + ply, **kw)
                running = best >= 0
                carried_sum += carried[running].sum()
                searched += running.sum()
            else:
                best = batch.search_moves_tensor(seed=seed + 1000 + ply, **kw)[2]
            forest.advance_tensor(best)                         # (an ended board has best = -1: its tree is left alone)
            targets[k] = batch.step_actions_observe(batch.slots_to_moves_tensor(best, targets[k]), targets[k])
    won = drawn = cut = 0
    for batch, forest, parity in sides:
        winner = torch.as_tensor(batch.winner)
        won += int((winner == parity).sum())
        drawn += int((winner == 2).sum()) + int((winner == -1).sum())
        cut += int((winner == -1).sum())
        forest.close()
        batch.close()
    total = 2 * half
    return {"games": total, "won": won, "drawn": drawn, "cut": cut, "lost": total - won - drawn, "score": (won + 0.5 * drawn) / total,
            "mean_carried": float(carried_sum) / max(int(searched), 1), "searches": int(searched)}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", type=int, default=256)
    ap.add_argument("--iterations", type=int, default=64)
    ap.add_argument("--leaf-playouts", type=int, default=16)
    ap.add_argument("--capacity", type=int, default=0, help="nodes a tree; 0: 2 * iterations + 1")
    ap.add_argument("--explore", type=int, default=DEFAULT_EXPLORE)
    ap.add_argument("--policy", default="uniform", choices=("uniform", "decisive"))
    ap.add_argument("--max-plies", type=int, default=200, help="a game that holds this many plies is cut and counted as a draw")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--json", action="store_true", help="print the result as one JSON line")
    args = ap.parse_args()
    capacity = args.capacity or 2 * args.iterations + 1
    res = play(args.games, args.iterations, args.leaf_playouts, capacity, args.explore, args.policy, args.max_plies, args.seed)
    if args.json:
        print(json.dumps({**res, "iterations": args.iterations, "leaf_playouts": args.leaf_playouts, "capacity": capacity,
                          "explore": args.explore, "policy": args.policy, "max_plies": args.max_plies}))
        return
    print(f"tree search with reuse ({args.iterations} x {args.leaf_playouts}, {capacity} nodes a tree) against the same search "
          f"without, {args.policy} playouts, {res['games']} games of Bounce: won {res['won']}, drew {res['drawn']} ({res['cut']} cut "
          f"at {args.max_plies} plies), lost {res['lost']}; score {res['score']:.3f}; {res['mean_carried']:.1f} nodes carried into "
          f"a search on average")


if __name__ == "__main__":
    main()
