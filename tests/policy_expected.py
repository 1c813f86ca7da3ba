"""The CPU reference of the playout policies of bgs_connect_evaluate_actions_policy (include/bgs.h), built on the
oracle's public API alone, and the case table of tests/test_gpu_evaluate_policy.py.  No GPU import; not a test module.

The decisive policy, per ply of a playout after its forced first column: L = the legal columns (ascending), W = those
whose landing cell completes `count` in a row for the side to move, B = those whose landing cell would complete it for
the opponent; the candidate list S is W, else B, else L; the ply draws the word it draws under the uniform policy and
plays element (draw * |S|) >> 32 of S.

The reference plays the replicated boards of mc_expected.connect_expected in lock step: every ply takes orc.legal(),
builds S with a plain numpy statement of "a stone of `who` in column x makes `count` in a row", picks the index with
oracle.connect_sample_index (oracle.sample_index under the per-ply contract) and calls orc.step_actions."""

from collections import namedtuple

import numpy as np

from oracle import oracle
from tests import fuzz_cases as fc

UNCAPPED = 2**31 - 1
SEED = 0x5EED0F0E7A1A7E00
CLASSES = ("win", "block", "neither", "win_many", "block_many")


def completes(grid, who, k):
    """bool[n, w]: column x of board i is open and a stone of who[i] dropped there makes k in a row.  grid int8[n, h, w]
    (-1 empty, row 0 at the bottom), who int[n].  Whether the board has ended is the caller's business."""
    n, h, w = grid.shape
    height = (grid != -1).sum(axis=1)                 # [n, w]: the row a stone dropped in column x lands in
    mine = grid == np.asarray(who).reshape(n, 1, 1)
    board = np.arange(n)[:, None]
    xs = np.arange(w)[None, :]
    out = np.zeros((n, w), dtype=bool)
    for dx, dy in ((1, 0), (0, 1), (1, 1), (1, -1)):
        run = np.ones((n, w), dtype=np.int64)         # the stone itself
        for sign in (1, -1):
            alive = np.ones((n, w), dtype=bool)
            for s in range(1, k):
                xx, yy = xs + sign * s * dx, height + sign * s * dy
                inside = (xx >= 0) & (xx < w) & (yy >= 0) & (yy < h)
                alive &= inside & mine[board, np.clip(yy, 0, h - 1), np.clip(xx, 0, w - 1)]
                run += alive
        out |= run >= k
    return out & (height < h)


def candidates(orc, rows, uniform=False):
    """(S bool[len(rows), w], has_w, has_b, |W|, |B|) of the boards `rows` of the oracle batch"""
    legal = orc.legal()[rows].astype(bool)
    grid, who = orc.grid[rows], orc.player[rows].astype(np.int64)
    win = completes(grid, who, orc.k) & legal
    block = completes(grid, 1 - who, orc.k) & legal
    has_w, has_b = win.any(axis=1), block.any(axis=1)
    chosen = np.where(has_w[:, None], win, np.where(has_b[:, None], block, legal))
    return (legal if uniform else chosen), has_w, has_b, win.sum(axis=1), block.sum(axis=1)


def connect_policy_expected(h, w, k, roots, seed, first_game, playouts, max_plies, per_ply, uniform=False):
    """(counts int32[n, w, 3], env-steps, {class: plies}) of the decisive policy (uniform=True: S = L forced, the uniform
    policy played by this loop).  The classes count the plies after the first column: "win" (W not empty), "block" (W
    empty, B not), "neither", and the plies of the first two with two or more candidates ("win_many", "block_many")."""
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
    orc.winner[~legal] = 2            # an illegal column: the board leaves the count (and the playouts)
    steps = int(legal.sum())
    sample = oracle.sample_index if per_ply else oracle.connect_sample_index
    base = first_game * rep
    seen = dict.fromkeys(CLASSES, 0)
    while True:
        rows = np.flatnonzero((orc.winner == -1) & (orc.plies < max_plies))
        if rows.size == 0:
            break
        chosen, has_w, has_b, n_w, n_b = candidates(orc, rows, uniform)
        seen["win"] += int(has_w.sum())
        seen["block"] += int((~has_w & has_b).sum())
        seen["neither"] += int((~has_w & ~has_b).sum())
        seen["win_many"] += int((has_w & (n_w >= 2)).sum())
        seen["block_many"] += int((~has_w & (n_b >= 2)).sum())
        size = chosen.sum(axis=1)
        at = orc.plies[rows]
        idx = np.array([sample(seed, (base + int(r)) & (2**64 - 1), int(p), int(s)) for r, p, s in zip(rows, at, size)])
        move = np.full(orc.n, -1, dtype=np.int32)
        move[rows] = (np.cumsum(chosen, axis=1) > idx[:, None]).argmax(axis=1)   # the idx-th candidate, ascending
        assert (orc.step_actions(move)[rows] == 0).all()
        steps += rows.size
    win = orc.winner.reshape(n, w, playouts)
    ok = legal.reshape(n, w, playouts)
    mover = player.astype(np.int16)[:, None, None]
    counts = np.stack([(ok & (win == mover)).sum(-1), (ok & (win == 2)).sum(-1), (ok & (win == 1 - mover)).sum(-1)], -1)
    return counts.astype(np.int32), steps, seen


# ---- the cases of the GPU comparison.  Roots: fuzz_cases.connect_roots -- the start, positions a few plies in, the
# near-full end of the tiled game, positions one to three plies before the end of random games, ended boards.
# cap: None, or plies past the median ply count of the running roots (the later roots start at or beyond it).
Case = namedtuple("Case", "h w k playouts cap first_game")
CASES = (
    Case(6, 7, 4, 64, None, 5),                # Connect4
    Case(6, 7, 4, 37, 3, 1 << 33),             # a cap that cuts playouts, game ids beyond 32 bits
    Case(5, 6, 3, 32, None, 3),                # count 3, one word
    Case(7, 8, 5, 24, None, 0),                # count 5, one word of exactly 64 bits
    Case(2, 5, 3, 16, None, 9),                # more columns than a column field counts: the general bit search
    Case(6, 12, 4, 16, None, 2),               # two words, count 4
    Case(8, 8, 6, 12, 6, 11),                  # two words, a general count, capped
    Case(12, 13, 5, 6, None, 7),               # three words, count 5
    Case(9, 16, 3, 5, None, 4),                # three words, count 3, sixteen columns
)


def nw_of(h, w):
    return (w * (h + 1) + 63) // 64


def case_roots(case):
    rng = np.random.default_rng(31000 + 100 * case.h + case.w + 7 * case.k)
    return fc.connect_roots(case.h, case.w, case.k, rng)


def case_max_plies(case, roots):
    if case.cap is None:
        return UNCAPPED
    return int(np.median(roots[3][roots[2] == -1])) + case.cap
