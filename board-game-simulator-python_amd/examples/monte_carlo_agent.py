#!/usr/bin/env python3
"""Flat Monte-Carlo against uniform random play on Connect4, a few hundred games at once.  Needs one MI355X.

The games live in one ConnectBatch.  Each ply, the side to move of every running game is either the Monte-Carlo agent
(all its games are evaluated in ONE launch: every legal column, `playouts` random games each) or the random agent (a
uniform legal column).  The agent plays first in half of the games and second in the other half.

    python board-game-simulator-python_amd/examples/monte_carlo_agent.py [--games 400] [--playouts 64] [--policy decisive]
"""

import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np

from simulator.agents import MonteCarloAgent
from simulator.batch import ConnectBatch


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", type=int, default=400)
    ap.add_argument("--playouts", type=int, default=64)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--policy", choices=("uniform", "decisive"), default="uniform", help="the playout policy")
    args = ap.parse_args()
    n = args.games
    games = ConnectBatch(6, 7, 4, n)
    agent = MonteCarloAgent(playouts=args.playouts, seed=args.seed, policy=args.policy)
    rng = np.random.default_rng(args.seed)
    agent_player = (np.arange(n) % 2).astype(np.int8)   # the agent is player 0 in even games, player 1 in odd ones
    ply = 0
    while not games.has_ended.all():
        legal = games.legal.astype(bool)
        running = legal.any(axis=1)
        # the agent: the best column of every game (one launch for all of them; game ids move on every ply)
        values = agent.values(games, first_game=ply * n)
        best = np.where(legal, np.nan_to_num(values, nan=-1.0), -2.0).argmax(axis=1)
        # the random agent: a uniform legal column
        rand = (rng.random(legal.shape) * legal).argmax(axis=1)
        cols = np.where(games.player == agent_player, best, rand)
        games.step_actions(np.where(running, cols, -1).astype(np.int32), want_status=False)
        ply += 1
    winner = games.winner
    won, drawn = (winner == agent_player).sum(), (winner == 2).sum()
    print(f"MonteCarloAgent ({args.playouts} {args.policy} playouts a column) against uniform random, {n} games of Connect4: "
          f"won {won} ({won / n:.1%}), drew {drawn}, lost {n - won - drawn}")
    agent.close()


if __name__ == "__main__":
    main()
