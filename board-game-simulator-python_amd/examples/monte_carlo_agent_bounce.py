#!/usr/bin/env python3
"""Flat Monte-Carlo against uniform random play on the default 9x6 Bounce board, a few hundred games at once.  Needs one
MI355X.

The games live in one BounceBatch.  Each ply, the side to move of every running game is either the Monte-Carlo agent
(all its games are evaluated in ONE launch: every legal (source, target) move, `playouts` random games each, capped at
`--max-plies` absolute plies) or the random agent (a uniform legal move).  The agent plays first in half of the games and
second in the other half.  Games still running after `--plies` plies are reported as unfinished.

    python board-game-simulator-python_amd/examples/monte_carlo_agent_bounce.py [--games 256] [--playouts 32]
"""

import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np

from simulator.agents import BOUNCE_MAX_PLIES, MonteCarloAgent
from simulator.batch import BounceBatch


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", type=int, default=256)
    ap.add_argument("--playouts", type=int, default=32)
    ap.add_argument("--max-plies", type=int, default=BOUNCE_MAX_PLIES)
    ap.add_argument("--plies", type=int, default=300)
    ap.add_argument("--seed", type=int, default=1)
    args = ap.parse_args()
    n = args.games
    grid = np.zeros((9, 6), dtype=np.int8)
    grid[1] = grid[7] = [1, 2, 3, 3, 2, 1]
    games = BounceBatch(grid, n)
    h, w = games.height, games.width
    agent = MonteCarloAgent(playouts=args.playouts, seed=args.seed, max_plies=args.max_plies)
    rng = np.random.default_rng(args.seed)
    agent_player = (np.arange(n) % 2).astype(np.int8)   # the agent is player 0 in even games, player 1 in odd ones
    cells = np.arange(h * w, dtype=np.uint64)
    for ply in range(args.plies):
        if games.has_ended.all():
            break
        t = games.targets
        legal = ((t[:, :w, None] >> cells) & np.uint64(1)) != 0      # [n, x, c]: the move of column x's piece to cell c
        running = legal.reshape(n, -1).any(axis=1)
        # the agent: the best move of every game (one launch for all of them; game ids move on every ply)
        values = agent.bounce_values(games, first_game=ply * n).reshape(n, -1)
        best = np.where(legal.reshape(n, -1), np.nan_to_num(values, nan=-1.0), -2.0).argmax(axis=1)
        # the random agent: a uniform legal move
        rand = (rng.random((n, w * h * w)) * legal.reshape(n, -1)).argmax(axis=1)
        slot = np.where(games.player == agent_player, best, rand)
        x, c = slot // (h * w), slot % (h * w)
        row = t[:, w].astype(np.int64)
        moves = np.stack([x, row, c % w, c // w], -1).astype(np.int32)
        moves[~running, 0] = -1
        games.step_actions(moves, want_status=False)
    winner = games.winner
    won, drawn, open_ = (winner == agent_player).sum(), (winner == 2).sum(), (winner == -1).sum()
    print(f"MonteCarloAgent ({args.playouts} playouts a move) against uniform random, {n} games of Bounce 9x6: "
          f"won {won} ({won / n:.1%}), drew {drawn}, lost {n - won - drawn - open_}, unfinished {open_}")
    agent.close()


if __name__ == "__main__":
    main()
