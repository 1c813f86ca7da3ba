"""Expected flat Monte-Carlo counts from the oracle, shared by the evaluate tests: root i replicated width * playouts
times, stepped by its column (illegal columns leave the board and drop out of the count), then rollout(seed,
first_game * width * playouts, max_plies), the winners counted relative to the root's player."""

import numpy as np

from oracle import oracle


def connect_expected(h, w, k, roots, seed, first_game, playouts, max_plies, per_ply):
    """(counts int32[n, w, 3], env-steps) from the oracle"""
    grid, player, winner, plies = roots
    n = grid.shape[0]
    rep = w * playouts
    orc = oracle.ConnectOracle(h, w, k, n * rep, per_ply=per_ply)
    orc.grid[:] = np.repeat(grid, rep, axis=0)
    orc.player[:] = np.repeat(player, rep)
    orc.winner[:] = np.repeat(winner, rep)
    orc.plies[:] = np.repeat(plies, rep)
    cols = np.tile(np.repeat(np.arange(w, dtype=np.int32), playouts), n)
    legal = orc.step_actions(cols) == 0
    orc.winner[~legal] = 2            # an illegal column: the board leaves the count (and the rollout)
    steps = int(legal.sum()) + orc.rollout(seed, first_game=first_game * rep, max_plies=max_plies)
    win = orc.winner.reshape(n, w, playouts)
    ok = legal.reshape(n, w, playouts)
    mover = player.astype(np.int16)[:, None, None]
    counts = np.stack([(ok & (win == mover)).sum(-1), (ok & (win == 2)).sum(-1), (ok & (win == 1 - mover)).sum(-1)], -1)
    return counts.astype(np.int32), steps
