"""CPU answer for the exact Bounce solver (bgs_bounce_solve_moves), independent of the kernel: retrograde analysis from a
set of root positions, in the style of tests/solve_reference.py.

Forward, layer d holds every distinct position -- keyed by (grid, player): the player is not derivable from a Bounce
grid -- reached in d plies from some root, the moves listed and played by the oracle (game_trees.bounce_actions /
bounce_children).  The winner the oracle reports after a move is the only source of "the game ended".  Backward, from
the layer the horizon stops at, every position gets its value for the side to move: (+1, t) it can force a win that ends
t plies from it (the fastest), (-1, t) the other side can (the slowest), (0, 0) neither.  A move that wins scores (+1, 1),
one that ends the game as a draw (0, 0), one into a running child of value (s, t) scores (-s, t + 1), and a child beyond
the horizon scores (0, 0).  The root's moves are the answer; a root move that itself draws is DRAW with plies 1.
"""

import numpy as np

from tests import game_trees as gt
from tests.solve_reference import BUDGET, DRAW, LOSS, NONE, UNKNOWN, WIN, _best  # noqa: F401  (the codes are re-exported)


def _keys(layer):
    n = layer[0].shape[0]
    key = np.concatenate([np.ascontiguousarray(layer[0]).reshape(n, -1).view(np.uint8),
                          np.ascontiguousarray(layer[1]).reshape(n, -1).view(np.uint8)], axis=1)
    key = np.ascontiguousarray(key)
    return key.view(f"V{key.shape[1]}").ravel()


def _dedup(layer):
    """(distinct positions of `layer` by (grid, player), index of every row's position among them)"""
    if layer[0].shape[0] == 0:
        return layer, np.zeros(0, dtype=np.int64)
    keys = _keys(layer)
    _, first, inverse = np.unique(keys, return_index=True, return_inverse=True)
    return gt._take(layer, first), inverse.ravel()


def _expand(cfg, layer, cut):
    """the moves of every position of `layer` (all running): (pos int[m], move int[m, 4], outcome int8[m]: 1 the mover
    won, 0 a draw, 2 a running child), and the distinct running children with every such move's index among them (-1
    elsewhere; `cut`: the children lie beyond the horizon and are not kept)"""
    acts = gt.bounce_actions(cfg, layer)
    moves = [(i, (sx, sy, tx, ty)) for i, a in enumerate(acts) for (sx, sy), (tx, ty) in a]
    assert all(acts), "a running position has a legal move (the oracle settles blocked games)"
    pos = np.array([i for i, _ in moves], dtype=np.int64)
    mv = np.array([m for _, m in moves], dtype=np.int64).reshape(-1, 4)
    status, kids = gt.bounce_children(cfg, layer, moves)
    assert (status == 0).all()
    mover = layer[1][pos]
    kw = kids[2]
    assert ((kw == -1) | (kw == 2) | (kw == mover)).all(), "a move never wins the game for the other side"
    outcome = np.where(kw == mover, 1, np.where(kw == 2, 0, 2)).astype(np.int8)
    child = np.full(pos.size, -1, dtype=np.int64)
    nxt = None
    if not cut:
        go = np.flatnonzero(outcome == 2)
        nxt, inv = _dedup(gt._take(kids, go))
        child[go] = inv
    return pos, mv, outcome, child, nxt


def solve(cfg, roots, depth, stats=None):
    """codes int8[n, W, H * W] and plies int16[n, W, H * W] of bgs_bounce_solve_moves for the positions `roots`
    (reference layout: grid, player, winner, plies) at horizon `depth`.  stats (a dict, optional) receives the number of
    positions the forward pass expanded ("nodes")."""
    cfg = np.asarray(cfg, dtype=np.int8)
    h, w = cfg.shape
    n = roots[0].shape[0]
    depth = int(depth)
    assert depth >= 1
    codes = np.full((n, w, h * w), NONE, dtype=np.int8)
    plies = np.zeros((n, w, h * w), dtype=np.int16)
    layer = tuple(np.asarray(a).copy() for a in roots)
    running = np.flatnonzero(layer[2] == -1)
    layer = gt._take(layer, running)
    # ---- forward
    levels = []
    nodes = 0
    for d in range(depth):
        if layer[0].shape[0] == 0:
            break
        nodes += layer[0].shape[0]
        pos, mv, outcome, child, nxt = _expand(cfg, layer, cut=d + 1 == depth)
        levels.append((layer[0].shape[0], pos, mv, outcome, child))
        if d + 1 == depth:
            break
        layer = nxt
    if stats is not None:
        stats["nodes"] = nodes
    if not levels:
        return codes, plies
    # ---- backward
    below_sign = below_dist = None
    for d in range(len(levels) - 1, -1, -1):
        npos, pos, mv, outcome, child = levels[d]
        sign = np.where(outcome == 1, 1, 0).astype(np.int64)
        dist = np.where(outcome == 1, 1, 0).astype(np.int64)
        deep = child >= 0
        if deep.any():
            cs, cd = below_sign[child[deep]], below_dist[child[deep]]
            sign[deep] = -cs
            dist[deep] = np.where(cs != 0, cd + 1, 0)
        if d == 0:
            break
        # per position, the best of its moves: a table [position, k-th move], padded with "illegal"
        start = np.searchsorted(pos, np.arange(npos))
        k = np.arange(pos.size) - start[pos]
        width = int(k.max()) + 1
        tab_s = np.full((npos, width), -9, dtype=np.int64)
        tab_d = np.zeros((npos, width), dtype=np.int64)
        tab_s[pos, k] = sign
        tab_d[pos, k] = dist
        below_sign, below_dist = _best(tab_s, tab_d)
    # ---- the roots' answer
    npos, pos, mv, outcome, child = levels[0]
    c = np.where(sign == 1, WIN, np.where(sign == -1, LOSS, np.where(outcome == 0, DRAW, UNKNOWN)))
    p = np.where(sign != 0, dist, np.where(outcome == 0, 1, 0))
    codes[running[pos], mv[:, 0], mv[:, 3] * w + mv[:, 2]] = c
    plies[running[pos], mv[:, 0], mv[:, 3] * w + mv[:, 2]] = p
    return codes, plies
