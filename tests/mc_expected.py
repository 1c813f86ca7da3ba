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


# ---- Bounce (bgs_bounce_evaluate_moves): root i replicated S * P times (S = W * H * W slots), every copy stepped by its
# slot's move (slot s = x * H * W + c: the piece in column x of the active row to cell c; a refused move drops the copy),
# then rollout(seed, first_game * S * P, max_plies), the winners counted relative to the root's player
def make_roots(grid, n, seed):
    """n positions (grid, player, winner, plies): the start, random mid-game positions at several plies, ended boards"""
    rng = np.random.default_rng(seed)
    orc = oracle.BounceOracle(grid, n)
    kind = np.arange(n) % 4    # 0 start, 1 a few plies, 2 many plies, 3 played to the end
    target = np.where(kind == 1, rng.integers(1, 6, n), np.where(kind == 2, rng.integers(6, 30, n), 0))
    for ply in range(400):
        moves = np.full((n, 4), -1, dtype=np.int32)
        for i in range(n):
            if orc.winner[i] != -1 or kind[i] == 0 or (kind[i] != 3 and ply >= target[i]):
                continue
            acts = orc.actions(i)
            if acts:
                (sx, sy), (tx, ty) = acts[rng.integers(len(acts))]
                moves[i] = (sx, sy, tx, ty)
        if (moves[:, 0] < 0).all():
            break
        orc.step_actions(moves)
    return orc.grid.copy(), orc.player.copy(), orc.winner.copy(), orc.plies.copy()


def slot_moves(h, w, row):
    """int32[S, 4]: the move of every slot for a root whose active row is `row` (a goal row when nothing can move: refused)"""
    s = np.arange(w * h * w)
    x, c = s // (h * w), s % (h * w)
    return np.stack([x, np.full_like(s, row), c % w, c // w], -1).astype(np.int32)


def active_rows(grid, roots):
    """the active row of every root (0, a goal row, when it has no move: every slot is refused)"""
    orc = oracle.BounceOracle(grid, 1)
    rows = np.zeros(roots[0].shape[0], dtype=np.int64)
    for i in range(rows.size):
        orc.grid[:], orc.player[:], orc.winner[:], orc.plies[:] = (a[i] for a in roots)
        acts = orc.actions(0)
        rows[i] = acts[0][0][1] if acts else 0
    return rows


def expected(grid, roots, seed, first_game, playouts, max_plies, rows=None):
    """(counts int32[n, W, H * W, 3], env-steps) from the oracle, literally: one replicated batch, one rollout"""
    g, player, winner, plies = roots
    h, w = grid.shape
    n, S = g.shape[0], w * h * w
    rep = S * playouts
    rows = active_rows(grid, roots) if rows is None else rows
    orc = oracle.BounceOracle(grid, n * rep)
    orc.grid[:] = np.repeat(g, rep, axis=0)
    orc.player[:] = np.repeat(player, rep)
    orc.winner[:] = np.repeat(winner, rep)
    orc.plies[:] = np.repeat(plies, rep)
    moves = np.concatenate([np.repeat(slot_moves(h, w, r), playouts, axis=0) for r in rows])
    legal = orc.step_actions(moves) == 0
    orc.winner[~legal] = 2            # a refused move: the copy leaves the count (and the rollout)
    steps = int(legal.sum()) + orc.rollout(seed, first_game=first_game * rep, max_plies=max_plies)
    win = orc.winner.reshape(n, S, playouts)
    ok = legal.reshape(n, S, playouts)
    mover = player.astype(np.int16)[:, None, None]
    counts = np.stack([(ok & (win == mover)).sum(-1), (ok & (win == 2)).sum(-1), (ok & (win == 1 - mover)).sum(-1)], -1)
    return counts.reshape(n, w, h * w, 3).astype(np.int32), steps


def expected_by_slot(grid, roots, seed, first_game, playouts, max_plies):
    """the same counts for large batches: every LEGAL (root, slot) on its own, as games ((first_game + i) * S + s) * P + p
    -- the ids the replicated batch gives them -- so that the illegal slots are never replicated"""
    g, player, winner, plies = roots
    h, w = grid.shape
    n, S = g.shape[0], w * h * w
    rows = active_rows(grid, roots)
    counts = np.zeros((n, S, 3), dtype=np.int64)
    steps = 0
    orc = oracle.BounceOracle(grid, playouts)
    for i in range(n):
        if winner[i] != -1:
            continue
        probe = oracle.BounceOracle(grid, 1)
        probe.grid[:], probe.player[:], probe.winner[:], probe.plies[:] = g[i], player[i], winner[i], plies[i]
        for (sx, sy), (tx, ty) in probe.actions(0):
            s = sx * h * w + ty * w + tx
            orc.grid[:], orc.player[:], orc.winner[:], orc.plies[:] = g[i], player[i], winner[i], plies[i]
            assert sy == rows[i] and (orc.step_actions(np.tile(np.int32([sx, sy, tx, ty]), (playouts, 1))) == 0).all()
            steps += playouts + orc.rollout(seed, first_game=((first_game + i) * S + s) * playouts, max_plies=max_plies)
            m = int(player[i])
            counts[i, s] = [(orc.winner == m).sum(), (orc.winner == 2).sum(), (orc.winner == 1 - m).sum()]
    return counts.reshape(n, w, h * w, 3).astype(np.int32), steps
