#!/usr/bin/env python3
"""Sequential halving against the flat allocation: two Monte-Carlo agents play N games of Bounce on the default 9x6 board,
at the same playouts a position.  Needs one MI355X.

The flat agent (MonteCarloAgent) values every legal move of a position by `playouts` random games and plays the best
one: `playouts` x A games for a position with A legal moves.  The halving agent (BounceHalvingAgent) spends the same
`playouts` x A games on that position by sequential halving (BounceBatch.evaluate_moves_halving) and plays the last
surviving move; the positions it moves in are grouped by A, one launch a group.  Both use the playout policy given.  The
halving agent is player 0 in the even games and player 1 in the odd ones.  A game that holds `--max-plies` plies (default
200) is cut there and counted as a draw.

    python board-game-simulator-python_amd/examples/halving_match_bounce.py [--games 256] [--playouts 64] [--policy uniform]
"""

import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np

from simulator.agents import BounceHalvingAgent, MonteCarloAgent
from simulator.game.bounce import Config


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", type=int, default=256)
    ap.add_argument("--playouts", type=int, default=64, help="playouts a legal move of the flat agent (at least 9)")
    ap.add_argument("--policy", default="uniform", choices=("uniform", "decisive"))
    ap.add_argument("--max-plies", type=int, default=200, help="a game that holds this many plies is cut and counted as a draw")
    ap.add_argument("--seed", type=int, default=1)
    args = ap.parse_args()
    n = args.games
    grid = np.zeros((9, 6), dtype=np.int8)
    grid[1] = grid[7] = [1, 2, 3, 3, 2, 1]
    config = Config(grid)
    flat = MonteCarloAgent(playouts=args.playouts, seed=args.seed, policy=args.policy)
    halving = BounceHalvingAgent(seed=args.seed + 1, policy=args.policy)
    states = [config.sample_initial_state() for _ in range(n)]
    for ply in range(args.max_plies):
        if all(s.has_ended for s in states):
            break
        # player ply & 1 moves in every game: the halving agent in the games of that parity, the flat agent in the others
        mine = [k for k in range(ply & 1, n, 2) if not states[k].has_ended]
        theirs = [k for k in range(1 - (ply & 1), n, 2) if not states[k].has_ended]
        chosen = dict(zip(theirs, flat.choose_many([states[k] for k in theirs], first_game=ply * n)))   # fresh ids every ply
        for moves in sorted({len(states[k].actions) for k in mine}):
            group = [k for k in mine if len(states[k].actions) == moves]
            halving.budget = args.playouts * moves       # what the flat agent spends on such a position
            chosen.update(zip(group, halving.choose_many([states[k] for k in group], first_game=ply * n + group[0])))
        for k, action in chosen.items():
            if action is not None:
                states[k] = action.sample_next_state()
    won = drawn = cut = 0
    for k, s in enumerate(states):
        winner = int(s.to_json()["winner"])
        cut += not s.has_ended
        drawn += (not s.has_ended) or winner == 2
        won += s.has_ended and winner == k % 2
    flat.close()
    halving.close()
    print(f"halving against flat, {args.policy} playouts ({args.playouts} x legal moves a position), {n} games of Bounce: "
          f"won {won}, drew {drawn} ({cut} cut at {args.max_plies} plies), lost {n - won - drawn}; score {(won + 0.5 * drawn) / n:.3f}")


if __name__ == "__main__":
    main()
