#!/usr/bin/env python3
"""Guided self-play on the device with trees kept from move to move: an API demonstration.  Needs one MI355X.

n games of Connect4 play against themselves to the end.  The "network" is the small UNTRAINED torch MLP of
examples/guided_search.py, so the games and the rows collected here say nothing about Connect4: what the example shows is
the loop of simulator.batch.GuidedForest --

    outs = forest.run(evaluate, simulations)                  # the first search: begin, simulations evaluations, finish
    while games run:
        columns = pick(outs)                                  # a column a board from the root's visits; -1 where the game is over
        games.step_actions_observe(columns, legal, ended)     # the boards play it
        kept = forest.advance(columns)                        # the trees follow: the subtree under the column becomes the tree
        outs = forest.run(evaluate, simulations, carry=True)  # resume: the search goes on from what was kept

-- in which nothing but the `ended` test comes back to the host.  The evaluations under the move played are kept, so the
next search starts with `kept` nodes that the network has already paid for; the example prints how many that is a move.
The move is the most visited column, or for the first --sample-plies plies a draw from the visits (torch.multinomial under
a seeded generator).  It collects the rows a trainer would want: (grid, visit shares, the game's outcome for the player to
move).

    python board-game-simulator-python_amd/examples/guided_selfplay.py [--games 64] [--simulations 64] [--sample-plies 6]
"""

import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from guided_search import PolicyValueNet
from simulator.batch import DEFAULT_CPUCT, ConnectBatch, GuidedForest


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", type=int, default=64)
    ap.add_argument("--simulations", type=int, default=64)
    ap.add_argument("--cpuct", type=int, default=DEFAULT_CPUCT, help="c_puct in Q8 (320 = 1.25)")
    ap.add_argument("--sample-plies", type=int, default=6, help="plies whose move is drawn from the visits")
    ap.add_argument("--seed", type=int, default=1)
    args = ap.parse_args()
    n, height, width = args.games, 6, 7
    torch.manual_seed(args.seed)
    generator = torch.Generator(device="cuda:0").manual_seed(args.seed)
    net = PolicyValueNet(height, width).to("cuda:0").eval()
    games = ConnectBatch(height, width, 4, n, use_torch=True)
    # room for the nodes one search makes plus as many carried ones: an allowance, not a measurement
    forest = GuidedForest(games, capacity=2 * args.simulations + 1, cpuct=args.cpuct)

    @torch.no_grad()
    def evaluate(leaf_grid, leaf_player):
        priors, values = net(leaf_grid, leaf_player)
        return priors.contiguous(), values.contiguous()

    legal = games.legal_tensor()
    ended = torch.zeros(n, dtype=torch.uint8, device="cuda:0")
    kept = torch.zeros(n, dtype=torch.int32, device="cuda:0")
    grids, movers, shares, running_rows = [], [], [], []
    kept_sum = torch.zeros(2, dtype=torch.int64, device="cuda:0")     # nodes kept, and the moves they were kept over
    outs = forest.run(evaluate, args.simulations)
    for ply in range(height * width):
        root_grid, root_player, _, visits, _, best, _ = outs       # (after finish a tree shows its root)
        running = ended == 0
        if not bool(running.any()):
            break
        weights = visits.to(torch.float32)
        grids.append(root_grid.clone())
        movers.append(root_player.clone())
        shares.append(weights / weights.sum(dim=1, keepdim=True).clamp(min=1))
        running_rows.append(running.clone())
        if ply < args.sample_plies:
            weights = torch.where(weights.sum(dim=1, keepdim=True) > 0, weights, torch.ones_like(weights))
            drawn = torch.multinomial(weights, 1, generator=generator).squeeze(1).to(torch.int32)
        else:
            drawn = best
        columns = torch.where(running, drawn, torch.full_like(best, -1)).contiguous()
        games.step_actions_observe(columns, legal, ended=ended)
        forest.advance(columns, kept)
        kept_sum += torch.stack([(kept * running).sum(), running.sum()])
        outs = forest.run(evaluate, args.simulations, carry=True)

    reward = torch.from_numpy(games.reward).to("cuda:0")           # int8[n, 2]: the outcome for player 0 and for player 1
    rows = []
    for grid, mover, share, running in zip(grids, movers, shares, running_rows):
        outcome = reward.gather(1, mover.to(torch.int64).view(-1, 1)).squeeze(1)
        rows.append((grid[running], share[running], outcome[running]))
    total = sum(int(r[0].shape[0]) for r in rows)
    winners = games.winner
    print(f"{n} games of Connect4 played to the end, {args.simulations} simulations a move, an untrained MLP at the leaves "
          f"(an API demonstration: the games mean nothing)")
    print(f"{total} (grid, visit shares, outcome) rows; player 0 won {int((winners == 0).sum())}, player 1 won {int((winners == 1).sum())}, "
          f"{int((winners == 2).sum())} draws")
    print(f"nodes kept a move: {int(kept_sum[0]) / max(1, int(kept_sum[1])):.1f} of the {args.simulations} a search evaluates")
    forest.close()
    games.close()


if __name__ == "__main__":
    main()
