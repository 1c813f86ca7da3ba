#!/usr/bin/env python3
"""Tree search that proves wins, draws and losses in its tree against tree search that does not: two UCT agents play N
games of Connect4 at once, at the same iterations and playouts a move.  Needs one MI355X.

Both agents are given `iterations` iterations of `leaf_playouts` playouts at each of their moves.  The plain agent runs
ConnectBatch.search_actions_tensor.  The proving agent runs ConnectBatch.search_actions_proving_tensor: game-end facts
stay on the edges of its tree and are backed up by minimax, a proved edge takes no further iterations, a root whose
value is proved stops early, and `best` is the proved win or the most visited column among those not proved lost.  The
games are two batches of N / 2: the proving agent moves first in one and second in the other, so each ply is one search
launch a batch and one device-side step (step_actions_observe); nothing crosses to the host until the games are over.

    python board-game-simulator-python_amd/examples/tree_prove_match.py [--games 512] [--iterations 64] [--leaf-playouts 16]
        [--explore 65536] [--policy uniform] [--json]
"""

import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from simulator.batch import DEFAULT_EXPLORE, SOLVE_DRAW, SOLVE_LOSS, SOLVE_WIN, ConnectBatch


def play(games: int, iterations: int, leaf_playouts: int, explore: int, policy: str, seed: int) -> dict:
    """the match; {"won", "drawn", "lost", "score"} of the proving agent, the share of its searches that stopped early
    ("decided_share"), their mean iterations over `iterations` ("mean_done_share") and the root columns it proved"""
    half, height, width = games // 2, 6, 7
    kw = dict(iterations=iterations, leaf_playouts=leaf_playouts, explore=explore, policy=policy)
    sides = [(ConnectBatch(height, width, 4, half, use_torch=True), parity) for parity in (0, 1)]
    legal = [batch.legal_tensor() for batch, _ in sides]
    tallies = torch.zeros(6, dtype=torch.int64, device="cuda:0")   # searches, stopped early, iterations run, proved W / D / L
    for ply in range(height * width):
        for k, (batch, parity) in enumerate(sides):
            batch.set_first_game((2 * ply + k) * half)              # fresh game ids every ply and batch
            if ply % 2 == parity:
                _, _, best, _, proved, done = batch.search_actions_proving_tensor(seed=seed + ply, **kw)
                running = best >= 0
                tallies += torch.stack([running.sum(), (running & (done < iterations)).sum(), done[running].sum(),
                                        (proved[running] == SOLVE_WIN).sum(), (proved[running] == SOLVE_DRAW).sum(),
                                        (proved[running] == SOLVE_LOSS).sum()])
            else:
                best = batch.search_actions_tensor(seed=seed + 1000 + ply, **kw)[2]
            legal[k] = batch.step_actions_observe(best, legal[k])
    won = drawn = 0
    for batch, parity in sides:
        winner = torch.as_tensor(batch.winner)
        won += int((winner == parity).sum())
        drawn += int((winner == 2).sum())
        batch.close()
    total = 2 * half
    searches, early, ran, wins, draws, losses = (int(x) for x in tallies.cpu())
    return {"games": total, "won": won, "drawn": drawn, "lost": total - won - drawn, "score": (won + 0.5 * drawn) / total,
            "searches": searches, "decided_share": early / max(searches, 1), "mean_done_share": ran / max(searches * iterations, 1),
            "proved_columns": {"win": wins, "draw": draws, "loss": losses}}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", type=int, default=512)
    ap.add_argument("--iterations", type=int, default=64)
    ap.add_argument("--leaf-playouts", type=int, default=16)
    ap.add_argument("--explore", type=int, default=DEFAULT_EXPLORE)
    ap.add_argument("--policy", default="uniform", choices=("uniform", "decisive"))
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--json", action="store_true", help="print the result as one JSON line")
    args = ap.parse_args()
    res = play(args.games, args.iterations, args.leaf_playouts, args.explore, args.policy, args.seed)
    if args.json:
        print(json.dumps({**res, "iterations": args.iterations, "leaf_playouts": args.leaf_playouts, "explore": args.explore,
                          "policy": args.policy}))
        return
    print(f"proving tree search ({args.iterations} x {args.leaf_playouts}) against the same search without the proofs, "
          f"{args.policy} playouts, {res['games']} games of Connect4: won {res['won']}, drew {res['drawn']}, lost {res['lost']}; "
          f"score {res['score']:.3f}; {100 * res['decided_share']:.1f} % of its searches stopped early, "
          f"{100 * res['mean_done_share']:.1f} % of the iterations run")


if __name__ == "__main__":
    main()
