"""Every reachable position of small games, layer by layer, for the exhaustive tests (CPU; the oracle plays the moves).

A layer is a batch in the reference layout: (grid int8[n, H, W], player int8[n], winner int8[n], plies int32[n]).

* Connect: layer d holds every position reachable in exactly d plies, each once (the grid decides the rest).
* Bounce: the walk is breadth-first over (grid, player), each position once at the depth it is first reached; games
  can cycle, so a later layer never repeats an earlier position.
* `end_games`: positions close to the end of random games, for geometries whose tree is too large to walk.
"""

import numpy as np

from oracle import oracle


def _unique_rows(*arrays):
    """index of the first row of every distinct (arrays...) tuple, in sorted order of the bytes"""
    n = arrays[0].shape[0]
    if n == 0:
        return np.zeros(0, dtype=np.int64)
    key = np.ascontiguousarray(np.concatenate([np.ascontiguousarray(a).reshape(n, -1).view(np.uint8) for a in arrays], axis=1))
    _, idx = np.unique(key.view(f"V{key.shape[1]}").ravel(), return_index=True)
    return np.sort(idx)


def _take(layer, idx):
    return tuple(a[idx].copy() for a in layer)


def connect_children(h, w, k, layer, columns):
    """every board of `layer` with every column of `columns` applied by the oracle: (status, child layer), board-major"""
    grid, player, winner, plies = layer
    m = len(columns)
    orc = oracle.ConnectOracle(h, w, k, grid.shape[0] * m)
    orc.grid[:] = np.repeat(grid, m, axis=0)
    orc.player[:] = np.repeat(player, m)
    orc.winner[:] = np.repeat(winner, m)
    orc.plies[:] = np.repeat(plies, m)
    status = orc.step_actions(np.tile(np.asarray(columns, dtype=np.int32), grid.shape[0]))
    return status, (orc.grid, orc.player, orc.winner, orc.plies)


def connect_layers(h, w, k, max_depth=None):
    """yields (depth, layer) for depth 0 .. the last non-empty layer (or max_depth)"""
    orc = oracle.ConnectOracle(h, w, k, 1)
    layer = (orc.grid.copy(), orc.player.copy(), orc.winner.copy(), orc.plies.copy())
    depth = 0
    while layer[0].shape[0]:
        yield depth, layer
        if max_depth is not None and depth >= max_depth:
            return
        running = layer[2] == -1
        status, kids = connect_children(h, w, k, _take(layer, np.flatnonzero(running)), list(range(w)))
        kids = _take(kids, np.flatnonzero(status == 0))
        layer = _take(kids, _unique_rows(kids[0]))
        depth += 1


def bounce_actions(cfg, layer):
    """the oracle's canonical move list of every board"""
    grid, player, winner, plies = layer
    orc = oracle.BounceOracle(cfg, 1)
    out = []
    for i in range(grid.shape[0]):
        orc.grid[0], orc.player[0], orc.winner[0], orc.plies[0] = grid[i], player[i], winner[i], plies[i]
        out.append(orc.actions(0))
    return out


def bounce_children(cfg, layer, moves):
    """board i of `layer` with moves[j] applied for every (i, move) of the list `moves` = [(i, (sx, sy, tx, ty)), ...]"""
    grid, player, winner, plies = layer
    idx = np.array([i for i, _ in moves], dtype=np.int64)
    mv = np.array([m for _, m in moves], dtype=np.int32).reshape(-1, 4)
    orc = oracle.BounceOracle(cfg, len(moves))
    orc.grid[:], orc.player[:], orc.winner[:], orc.plies[:] = grid[idx], player[idx], winner[idx], plies[idx]
    status = orc.step_actions(mv)
    return status, (orc.grid, orc.player, orc.winner, orc.plies)


def bounce_layers(cfg, max_depth=None):
    """yields (depth, layer, actions) breadth-first; `actions` is the oracle's move list of every board of the layer"""
    orc = oracle.BounceOracle(cfg, 1)
    layer = (orc.grid.copy(), orc.player.copy(), orc.winner.copy(), orc.plies.copy())
    seen = {layer[0][0].tobytes() + layer[1][:1].tobytes()}
    depth = 0
    while layer[0].shape[0]:
        acts = bounce_actions(cfg, layer)
        yield depth, layer, acts
        if max_depth is not None and depth >= max_depth:
            return
        moves = [(i, (sx, sy, tx, ty)) for i, a in enumerate(acts) for (sx, sy), (tx, ty) in a]
        if not moves:
            return
        status, kids = bounce_children(cfg, layer, moves)
        assert (status == 0).all()
        keep = []
        for j in _unique_rows(kids[0], kids[1]):
            key = kids[0][j].tobytes() + kids[1][j : j + 1].tobytes()
            if key not in seen:
                seen.add(key)
                keep.append(j)
        layer = _take(kids, np.array(keep, dtype=np.int64))
        depth += 1


def end_games(h, w, k, n, seed, last=3):
    """the positions `last`, ..., 1 plies before the end of n oracle games played from the start (distinct boards)"""
    orc = oracle.ConnectOracle(h, w, k, n)
    hist = []
    picked = []
    while not orc.ended.all():
        hist = (hist + [(orc.grid.copy(), orc.player.copy(), orc.winner.copy(), orc.plies.copy())])[-last:]
        before = orc.ended.copy()
        orc.step_random(seed)
        done = np.flatnonzero(orc.ended & ~before)
        for snap in hist:
            picked.append(_take(snap, done))
    layer = tuple(np.concatenate([p[j] for p in picked]) for j in range(4))
    layer = _take(layer, np.flatnonzero(layer[2] == -1))
    return _take(layer, _unique_rows(layer[0]))
