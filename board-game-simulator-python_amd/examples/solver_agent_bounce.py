"""The exact Bounce horizon search in front of flat Monte-Carlo, against flat Monte-Carlo alone, on the default 9x6 board.
Needs one MI355X.

One side is `SolverAgent(depth=3, fallback=MonteCarloAgent(...))`: it plays a forced win within three plies as fast as
it can, never a move that loses by force within three plies while another one exists, and otherwise the move the
Monte-Carlo values like best.  The other side is the same `MonteCarloAgent` alone, which sees a win in one or a loss in
two only as a slightly better or worse average.  The sides alternate from game to game.

    python board-game-simulator-python_amd/examples/solver_agent_bounce.py [--games 32] [--playouts 32]
"""

import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

from simulator.agents import MonteCarloAgent, SolverAgent  # noqa: E402
from simulator.game.bounce import Config  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", type=int, default=32)
    ap.add_argument("--playouts", type=int, default=32)
    ap.add_argument("--depth", type=int, default=3)
    ap.add_argument("--plies", type=int, default=200, help="games still running after this many plies count as unfinished")
    args = ap.parse_args()

    grid = np.zeros((9, 6), dtype=np.int8)
    grid[1] = grid[7] = [1, 2, 3, 3, 2, 1]
    cfg = Config(grid)
    mc = MonteCarloAgent(playouts=args.playouts)
    solver = SolverAgent(depth=args.depth, fallback=mc)
    states = [cfg.sample_initial_state() for _ in range(args.games)]
    solver_side = [g % 2 for g in range(args.games)]   # the solver is player 0 in even games, player 1 in odd ones
    for ply in range(args.plies):
        live = [i for i, s in enumerate(states) if not s.has_ended]
        if not live:
            break
        theirs = [i for i in live if states[i].player != solver_side[i]]
        values = dict(zip(theirs, mc.predict_many([states[i] for i in theirs], first_game=ply * args.games)))
        for i in live:
            s = states[i]
            action = solver.choose(s) if s.player == solver_side[i] else max(values[i], key=values[i].get)
            states[i] = action.sample_next_state()
    winners = np.array([s.to_json()["winner"] for s in states])
    side = np.array(solver_side)
    print(f"{args.games} games: solver (depth {args.depth}) + Monte-Carlo won {int((winners == side).sum())}, Monte-Carlo alone "
          f"won {int((winners == 1 - side).sum())}, draws {int((winners == 2).sum())}, unfinished {int((winners == -1).sum())}")
    solver.close()
    mc.close()


if __name__ == "__main__":
    main()
