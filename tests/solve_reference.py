"""CPU answer for the exact Connect solver (bgs_connect_solve_actions), independent of the kernel: retrograde analysis
from a set of root positions.

Forward, layer d holds every distinct position (by grid bytes) reached in d plies from some root, the moves played by
the oracle (game_trees.connect_children).  Backward, from the layer the horizon stops at, every position gets its value
for the side to move: (+1, t) it can force a win that ends t plies from it (the fastest), (-1, t) the other side can
(the slowest), (0, 0) neither.  A move that wins scores (+1, 1), one that fills the board (0, 0), one into a running
child of value (s, t) scores (-s, t + 1), and positions at the horizon score (0, 0).  The root's moves are the answer.
"""

import numpy as np

from tests import game_trees as gt

NONE, LOSS, DRAW, WIN, UNKNOWN, BUDGET = -2, -1, 0, 1, 2, 3


def _keys(grid):
    n = grid.shape[0]
    key = np.ascontiguousarray(np.ascontiguousarray(grid).reshape(n, -1).view(np.uint8))
    return key.view(f"V{key.shape[1]}").ravel()


def _dedup(layer):
    """(distinct positions of `layer` by grid bytes, index of every row's position among them)"""
    if layer[0].shape[0] == 0:
        return layer, np.zeros(0, dtype=np.int64)
    rep = gt._unique_rows(layer[0])
    distinct = gt._take(layer, rep)
    keys = _keys(distinct[0])
    order = np.argsort(keys)
    inverse = order[np.searchsorted(keys[order], _keys(layer[0]))]
    return distinct, inverse


def _best(sign, dist):
    """per row, the best move for the side to move: a win as fast as possible, else a draw / open line, else the
    slowest loss.  sign, dist int[n, w]; illegal moves carry sign -9."""
    key = np.where(sign == 1, 1000 - dist, np.where(sign == 0, 0, np.where(sign == -1, -1000 + dist, -10**6)))
    j = np.argmax(key, axis=1)
    rows = np.arange(sign.shape[0])
    return sign[rows, j], dist[rows, j]


def solve(h, w, k, roots, depth):
    """codes int8[n, w] and plies int16[n, w] of bgs_connect_solve_actions for the positions `roots` (reference layout:
    grid, player, winner, plies) at horizon `depth`"""
    grid = roots[0]
    n = grid.shape[0]
    depth = int(depth)
    # ---- forward: per layer, the running positions and, per (position, column), the move's status and child
    layers, moves = [], []
    layer = tuple(np.asarray(a).copy() for a in roots)
    running = np.flatnonzero(layer[2] == -1)
    layer = gt._take(layer, running)
    for d in range(depth):
        m = layer[0].shape[0]
        if m == 0:
            layers.append(layer)
            moves.append((np.zeros((0, w), dtype=np.int8), np.zeros((0, w), dtype=np.int64)))
            break
        status, kids = gt.connect_children(h, w, k, layer, list(range(w)))
        outcome = np.full(m * w, -9, dtype=np.int8)   # -9 illegal, 1 win, 0 draw, 2 running child
        legal = status == 0
        kw = kids[2]
        outcome[legal & (kw == np.repeat(layer[1], w))] = 1   # the mover won
        outcome[legal & (kw == 2)] = 0
        outcome[legal & (kw == -1)] = 2
        child = np.full(m * w, -1, dtype=np.int64)
        go = np.flatnonzero(outcome == 2)
        nxt, inv = _dedup(gt._take(kids, go))
        child[go] = inv
        if d + 1 == depth:
            child[go] = -1   # beyond the horizon: cut
        layers.append(layer)
        moves.append((outcome.reshape(m, w), child.reshape(m, w)))
        if d + 1 == depth:
            break
        layer = nxt
    # ---- backward
    below_sign = below_dist = None
    root_sign = root_dist = None
    for d in range(len(moves) - 1, -1, -1):
        outcome, child = moves[d]
        sign = np.where(outcome == 1, 1, np.where(outcome == -9, -9, 0)).astype(np.int64)
        dist = np.where(outcome == 1, 1, 0).astype(np.int64)
        deep = (outcome == 2) & (child >= 0)
        if deep.any():
            cs, cd = below_sign[child[deep]], below_dist[child[deep]]
            sign[deep] = -cs
            dist[deep] = np.where(cs != 0, cd + 1, 0)
        if d == 0:
            root_sign, root_dist = sign, dist
        else:
            below_sign, below_dist = _best(sign, dist)
    # ---- the roots' answer
    codes = np.full((n, w), NONE, dtype=np.int8)
    plies = np.zeros((n, w), dtype=np.int16)
    if root_sign is None:
        return codes, plies
    empty = (np.asarray(roots[0])[running] < 0).sum(axis=(1, 2))   # empty cells are -1
    c = np.where(root_sign == 1, WIN, np.where(root_sign == -1, LOSS, np.where(root_sign == -9, NONE, 0)))
    p = np.where(np.abs(root_sign) == 1, root_dist, 0)
    zero = root_sign == 0
    exact = (empty <= depth)[:, None]
    c = np.where(zero & exact, DRAW, np.where(zero, UNKNOWN, c))
    p = np.where(zero & exact, empty[:, None], p)
    codes[running] = c
    plies[running] = p
    return codes, plies
