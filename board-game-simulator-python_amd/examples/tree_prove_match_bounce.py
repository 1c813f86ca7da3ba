#!/usr/bin/env python3
"""Tree search that proves wins, draws and losses in its tree against tree search that does not: two UCT agents play N
games of Bounce on the default 9x6 board at once, at the same iterations and playouts a move.  Needs one MI355X.

Both agents are given `iterations` iterations of `leaf_playouts` playouts at each of their moves.  The plain agent runs
BounceBatch.search_moves_tensor.  The proving agent runs BounceBatch.search_moves_proving_tensor, the launch of
BounceTreeSearchAgent(prove=True): game-end facts -- a move into the goal row, a blocked side -- stay on the edges of its
tree and are backed up by minimax, a proved edge takes no further iterations, a root whose value is proved stops early,
and `best` is the proved win or the most visited move among those not proved lost.  The games are two batches of N / 2:
the proving agent moves first in one and second in the other, so each ply is one search launch a batch and one
device-side step (step_actions_observe); nothing crosses to the host until the games are over.  A game that holds
`--max-plies` plies is cut there and counted as a draw.

    python board-game-simulator-python_amd/examples/tree_prove_match_bounce.py [--games 512] [--iterations 64]
        [--leaf-playouts 16] [--explore 65536] [--policy uniform] [--max-plies 200] [--json]
"""

import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

from simulator.batch import DEFAULT_EXPLORE, SOLVE_DRAW, SOLVE_LOSS, SOLVE_WIN, BounceBatch


def play(games: int, iterations: int, leaf_playouts: int, explore: int, policy: str, max_plies: int, seed: int) -> dict:
    """the match; {"won", "drawn", "lost", "score"} of the proving agent with the score's standard error, the share of its
    searches that stopped early ("decided_share"), their mean iterations over `iterations` ("mean_done_share") and the
    root moves it proved"""
    half = games // 2
    grid = np.zeros((9, 6), dtype=np.int8)
    grid[1] = grid[7] = [1, 2, 3, 3, 2, 1]
    kw = dict(iterations=iterations, leaf_playouts=leaf_playouts, explore=explore, policy=policy, max_plies=1024)
    sides = [(BounceBatch(grid, half, use_torch=True), parity) for parity in (0, 1)]
    targets = [batch.targets_tensor() for batch, _ in sides]
    tallies = torch.zeros(6, dtype=torch.int64, device="cuda:0")   # searches, stopped early, iterations run, proved W / D / L
    for ply in range(max_plies):
        for k, (batch, parity) in enumerate(sides):
            batch.set_first_game((2 * ply + k) * half)              # fresh game ids every ply and batch
            if ply % 2 == parity:
                _, _, best, _, _, proved, done = batch.search_moves_proving_tensor(seed=seed + ply, **kw)
                running = best >= 0
                tallies += torch.stack([running.sum(), (running & (done < iterations)).sum(), done[running].sum(),
                                        (proved[running] == SOLVE_WIN).sum(), (proved[running] == SOLVE_DRAW).sum(),
                                        (proved[running] == SOLVE_LOSS).sum()])
            else:
                best = batch.search_moves_tensor(seed=seed + 1000 + ply, **kw)[2]
            targets[k] = batch.step_actions_observe(batch.slots_to_moves_tensor(best, targets[k]), targets[k])
    won = drawn = cut = 0
    for batch, parity in sides:
        winner = torch.as_tensor(batch.winner)
        won += int((winner == parity).sum())
        drawn += int((winner == 2).sum()) + int((winner == -1).sum())
        cut += int((winner == -1).sum())
        batch.close()
    total = 2 * half
    lost = total - won - drawn
    score = (won + 0.5 * drawn) / total
    spread = (won * (1.0 - score) ** 2 + drawn * (0.5 - score) ** 2 + lost * score ** 2) / total
    searches, early, ran, wins, draws, losses = (int(x) for x in tallies.cpu())
    return {"games": total, "won": won, "drawn": drawn, "cut": cut, "lost": lost, "score": score,
            "standard_error": (spread / total) ** 0.5, "searches": searches, "decided_share": early / max(searches, 1),
            "mean_done_share": ran / max(searches * iterations, 1), "proved_moves": {"win": wins, "draw": draws, "loss": losses}}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", type=int, default=512)
    ap.add_argument("--iterations", type=int, default=64)
    ap.add_argument("--leaf-playouts", type=int, default=16)
    ap.add_argument("--explore", type=int, default=DEFAULT_EXPLORE)
    ap.add_argument("--policy", default="uniform", choices=("uniform", "decisive"))
    ap.add_argument("--max-plies", type=int, default=200, help="a game that holds this many plies is cut and counted as a draw")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--json", action="store_true", help="print the result as one JSON line")
    args = ap.parse_args()
    res = play(args.games, args.iterations, args.leaf_playouts, args.explore, args.policy, args.max_plies, args.seed)
    if args.json:
        print(json.dumps({**res, "iterations": args.iterations, "leaf_playouts": args.leaf_playouts, "explore": args.explore,
                          "policy": args.policy, "max_plies": args.max_plies}))
        return
    print(f"proving tree search ({args.iterations} x {args.leaf_playouts}) against the same search without the proofs, "
          f"{args.policy} playouts, {res['games']} games of Bounce: won {res['won']}, drew {res['drawn']} ({res['cut']} cut at "
          f"{args.max_plies} plies), lost {res['lost']}; score {res['score']:.3f} +- {res['standard_error']:.3f}; "
          f"{100 * res['decided_share']:.1f} % of its searches stopped early, {100 * res['mean_done_share']:.1f} % of the iterations run")


if __name__ == "__main__":
    main()
