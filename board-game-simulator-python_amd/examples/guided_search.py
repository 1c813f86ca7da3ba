#!/usr/bin/env python3
"""PUCT tree search with a policy/value network at the leaves: an API demonstration.  Needs one MI355X.

The "network" is a small UNTRAINED torch MLP, so the visit shares it prints say nothing about Connect4: what the example
shows is the loop.  ConnectBatch.guided_search(capacity, cpuct) makes a GuidedSearch; GuidedSearch.run(evaluate,
simulations) calls `evaluate(leaf_grid, leaf_player)` once a simulation on the device tensors of the leaves of ALL trees
(int8[n, 6, 7]: -1 empty, 0 and 1 the players; int8[n] the player to move) and feeds what it returns -- priors
float32[n, 7] and values float32[n], seen from the player to move at the leaf -- into the trees with the next launch.
The trees, the descent and the statistics stay on the device; every call is an enqueue on the batch's stream.  The same
loop by hand: outs = search.begin(); outs = search.step(*evaluate(outs[0], outs[1])) ...; search.finish(...).

    python board-game-simulator-python_amd/examples/guided_search.py [--roots 4] [--simulations 128] [--cpuct 320]
"""

import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from simulator.batch import DEFAULT_CPUCT, ConnectBatch


class PolicyValueNet(torch.nn.Module):
    """two planes (the mover's stones, the other player's) -> a logit a column and a value in [-1, 1]"""

    def __init__(self, height: int, width: int, hidden: int = 64):
        super().__init__()
        self.body = torch.nn.Sequential(torch.nn.Linear(2 * height * width, hidden), torch.nn.ReLU(),
                                        torch.nn.Linear(hidden, hidden), torch.nn.ReLU())
        self.policy = torch.nn.Linear(hidden, width)
        self.value = torch.nn.Linear(hidden, 1)

    def forward(self, grid, player):
        mover = player.view(-1, 1, 1)
        planes = torch.stack([grid == mover, grid == 1 - mover], dim=1).to(torch.float32).flatten(1)
        x = self.body(planes)
        return torch.softmax(self.policy(x), dim=1), torch.tanh(self.value(x)).squeeze(1)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--roots", type=int, default=4)
    ap.add_argument("--simulations", type=int, default=128)
    ap.add_argument("--cpuct", type=int, default=DEFAULT_CPUCT, help="c_puct in Q8 (320 = 1.25)")
    ap.add_argument("--seed", type=int, default=1)
    args = ap.parse_args()
    n, height, width = args.roots, 6, 7
    torch.manual_seed(args.seed)
    net = PolicyValueNet(height, width).to("cuda:0").eval()
    games = ConnectBatch(height, width, 4, n, use_torch=True)
    games.step_random(args.seed, plies=4)               # a few random plies, so that the roots differ
    search = games.guided_search(capacity=args.simulations + 1, cpuct=args.cpuct)

    @torch.no_grad()
    def evaluate(leaf_grid, leaf_player):
        priors, values = net(leaf_grid, leaf_player)
        return priors.contiguous(), values.contiguous()

    leaf_grid, leaf_player, leaf_kind, visits, scores, best, nodes = search.run(evaluate, args.simulations)
    shares = (visits.to(torch.float32) / visits.sum(dim=1, keepdim=True).clamp(min=1)).cpu()
    print(f"{n} roots of Connect4, {args.simulations} simulations a root, cpuct {args.cpuct}, an untrained MLP at the leaves "
          f"(an API demonstration: the shares mean nothing)")
    for i in range(n):
        print(f"root {i}: visit shares {[round(float(x), 3) for x in shares[i]]}, best column {int(best[i])}, {int(nodes[i])} nodes")
    search.close()
    games.close()


if __name__ == "__main__":
    main()
