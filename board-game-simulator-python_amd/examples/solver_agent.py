"""Monte-Carlo agents playing 6x7 connect-4 against each other, the exact solver taking over for one side once a board
has at most --solve-from empty cells: every game of the batch is played position by position, each side's move chosen
from its agent's values of all positions of the batch in one call.

    python examples/solver_agent.py --games 64 --solve-from 14
"""

import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

from simulator.agents import MonteCarloAgent, SolverAgent  # noqa: E402
from simulator.game.connect import Config  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", type=int, default=64)
    ap.add_argument("--playouts", type=int, default=256)
    ap.add_argument("--solve-from", type=int, default=14, help="empty cells from which the solver plays for player 0")
    args = ap.parse_args()

    cfg = Config(6, 7, 4)
    mc = MonteCarloAgent(playouts=args.playouts)
    solver = SolverAgent(max_nodes=1 << 22, fallback=mc)
    states = [cfg.sample_initial_state() for _ in range(args.games)]
    solved_moves = 0
    while any(not s.has_ended for s in states):
        live = [i for i, s in enumerate(states) if not s.has_ended]
        values = mc.predict_many([states[i] for i in live])
        for j, i in enumerate(live):
            s = states[i]
            if s.player == 0 and int((s.grid < 0).sum()) <= args.solve_from:
                action = solver.choose(s)
                solved_moves += 1
            else:
                action = max(values[j], key=values[j].get)
            states[i] = action.sample_next_state()
    winners = np.array([s.to_json()["winner"] for s in states])
    print(f"{args.games} games: player 0 (Monte-Carlo, then the solver from {args.solve_from} empty cells) won "
          f"{int((winners == 0).sum())}, player 1 (Monte-Carlo) won {int((winners == 1).sum())}, draws "
          f"{int((winners == 2).sum())}; {solved_moves} moves chosen by the solver")
    solver.close()
    mc.close()


if __name__ == "__main__":
    main()
