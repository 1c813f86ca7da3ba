#!/usr/bin/env python3
"""PUCT tree search for Bounce with an evaluator at the leaves: an API demonstration.  Needs one MI355X.

The "network" is a toy: its logits are a fixed function of the move (further forward is better) and its value counts how
far each side's pieces have come, so the moves it plays say little about Bounce: what the example shows is the loop, and
the one thing a Bounce evaluator has to do that a Connect one has not -- mask its softmax.  Bounce legality cannot be read
off the grid cheaply, so every call hands out `leaf_targets` int64[n, W] beside the leaves: bit ty * W + tx of entry x is
set for every legal move of the piece in column x of the leaf's active row.  BounceBatch.guided_moves_search(nodes, edges,
cpuct, max_plies) makes a GuidedMovesSearch; GuidedMovesSearch.run(evaluate, simulations) calls `evaluate(leaf_grid,
leaf_player, leaf_targets)` once a simulation on the device tensors of the leaves of ALL trees and feeds what it returns
-- priors float32[n, W, H * W], a weight a move slot, and values float32[n], seen from the player to move at the leaf --
into the trees with the next launch.  The boards are then stepped by `best`, and the next search starts anew from them.

    python board-game-simulator-python_amd/examples/guided_search_bounce.py [--roots 4] [--simulations 128] [--moves 4]
"""

import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

from simulator.batch import DEFAULT_CPUCT, BounceBatch


def evaluate(leaf_grid, leaf_player, leaf_targets):
    """a softmax over the legal slots of `leaf_targets`, and a value in [-1, 1] for the player to move"""
    n, h, w = leaf_grid.shape
    cells = torch.arange(h * w, device=leaf_grid.device)
    legal = ((leaf_targets.view(n, w, 1) >> cells.view(1, 1, h * w)) & 1).bool()
    forward = (cells // w).to(torch.float32).view(1, 1, h * w)                   # the target's row
    forward = torch.where(leaf_player.view(n, 1, 1) == 0, forward, (h - 1) - forward)
    logits = torch.where(legal, forward, -torch.inf)
    priors = torch.softmax(logits.view(n, -1), dim=1).view(n, w, h * w)
    priors = torch.nan_to_num(priors, nan=0.0)                                   # (a leaf without a legal move: ignored anyway)
    rows = torch.arange(h, device=leaf_grid.device, dtype=torch.float32).view(1, h, 1)
    pieces = (leaf_grid > 0).to(torch.float32)
    lead = ((rows - (h - 1) / 2) * pieces).sum(dim=(1, 2)) / (h * w)              # > 0: the pieces stand nearer player 0's goal
    values = torch.tanh(lead) * (1 - 2 * leaf_player.to(torch.float32))
    return priors.contiguous(), values.contiguous()


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--roots", type=int, default=4)
    ap.add_argument("--simulations", type=int, default=128)
    ap.add_argument("--moves", type=int, default=4, help="plies played by the search")
    ap.add_argument("--cpuct", type=int, default=DEFAULT_CPUCT, help="c_puct in Q8 (320 = 1.25)")
    ap.add_argument("--seed", type=int, default=1)
    args = ap.parse_args()
    grid = np.zeros((9, 6), dtype=np.int8)
    grid[1] = grid[7] = [1, 2, 3, 3, 2, 1]
    n = args.roots
    games = BounceBatch(grid, n, use_torch=True)
    games.step_random(args.seed, plies=2)               # two random plies, so that the roots differ
    search = games.guided_moves_search(nodes=args.simulations + 1, cpuct=args.cpuct)
    print(f"{n} boards of the default Bounce grid, {args.simulations} simulations a move, cpuct {args.cpuct}, a toy evaluator at the "
          f"leaves (an API demonstration)")
    for ply in range(args.moves):
        with torch.no_grad():
            outs = search.run(evaluate, args.simulations)
        visits, best, nodes, used = outs[4], outs[6], outs[7], outs[8]
        moves = games.slots_to_moves(best.cpu().numpy())            # (before the boards are stepped: a slot holds no source row)
        top = (visits.flatten(1).max(dim=1).values.to(torch.float32) / visits.flatten(1).sum(dim=1).clamp(min=1)).cpu()
        for i in range(n):
            print(f"move {ply}, board {i}: {moves[i, :2].tolist()} -> {moves[i, 2:].tolist()} with {float(top[i]):.2f} of the visits, "
                  f"{int(nodes[i])} nodes, {int(used[i])} edges")
        games.step_actions(moves)                       # the stepped boards restart their trees on their own
    print(f"winners so far: {games.winner.tolist()} (-1: still running)")
    search.close()
    games.close()


if __name__ == "__main__":
    main()
