"""The CPU statement of bgs_connect_evaluate_actions_halving (include/bgs.h), built on the oracle's public API alone, and
the case table of tests/test_gpu_evaluate_halving.py.  No GPU import; not a test module.

For a running root with A legal columns, R = max(1, ceil(log2 A)) rounds: in round r every surviving column plays
q_r = budget // (survivors * R) further playouts, indices [P_r, P_r + q_r); then the ceil(survivors / 2) columns ranked
highest by (2 * wins + draws descending, column ascending) survive.  Playout p of column c of root i is the game
((first_game + i) * width + c) * budget + p.

The reference plays only the playouts the schedule gives: per round, one oracle batch of the (root, surviving column,
playout) boards of every root, stepped by their column and played in the lock step of tests/policy_expected.py -- every
ply takes the candidate list (policy_expected.candidates; the legal columns under the uniform policy), picks the index
with oracle.connect_sample_index (oracle.sample_index under the per-ply contract) under the playout's own game id and
calls orc.step_actions.  Env-steps are the oracle's ply counts past the root's; the selection is numpy's lexsort."""

import functools
from collections import namedtuple

import numpy as np

from oracle import oracle
from tests import fuzz_cases as fc
from tests.policy_expected import candidates

UNCAPPED = 2**31 - 1
SEED = 0x5EED0F0E7A1A7E00
MASK64 = 2**64 - 1


def rounds(x):
    """R(x) = max(1, ceil(log2 x))"""
    return max(1, (int(x) - 1).bit_length())


def min_budget(w):
    return w * rounds(w)


def schedule(a, budget):
    """[(survivors, q_r)] of a root with `a` legal columns"""
    out, m = [], int(a)
    for _ in range(rounds(a) if a else 0):
        out.append((m, budget // (m * rounds(a))))
        m = (m + 1) // 2
    return out


def legal_columns(h, w, k, roots):
    """bool[n, w]: the legal columns of every root (none on an ended board)"""
    grid, player, winner, plies = roots
    orc = oracle.ConnectOracle(h, w, k, grid.shape[0])
    orc.grid[:], orc.player[:], orc.winner[:], orc.plies[:] = grid, player, winner, plies
    return orc.legal().astype(bool) & (winner == -1)[:, None]


def _play(h, w, k, roots, rows, cols, ids, seed, max_plies, per_ply, policy):
    """(winner int8[len(rows)], env-steps): root rows[j] after column cols[j], played on as game ids[j]"""
    grid, player, winner, plies = roots
    orc = oracle.ConnectOracle(h, w, k, rows.size, per_ply=per_ply)
    orc.grid[:], orc.player[:], orc.winner[:], orc.plies[:] = grid[rows], player[rows], winner[rows], plies[rows]
    assert (orc.step_actions(cols.astype(np.int32)) == 0).all()
    sample = oracle.sample_index if per_ply else oracle.connect_sample_index
    while True:
        live = np.flatnonzero((orc.winner == -1) & (orc.plies < max_plies))
        if live.size == 0:
            break
        chosen = candidates(orc, live, policy == "uniform")[0]
        size = chosen.sum(axis=1)
        idx = np.array([sample(seed, ids[r], int(p), int(s)) for r, p, s in zip(live, orc.plies[live], size)])
        move = np.full(orc.n, -1, dtype=np.int32)
        move[live] = (np.cumsum(chosen, axis=1) > idx[:, None]).argmax(axis=1)   # the idx-th candidate, ascending
        assert (orc.step_actions(move)[live] == 0).all()
    return orc.winner.copy(), int((orc.plies.astype(np.int64) - plies[rows]).sum())


def halving_expected(h, w, k, roots, seed, first_game, budget, max_plies, per_ply, policy="uniform"):
    """(counts int32[n, w, 3], given int32[n, w], best int32[n], env-steps, {"cuts", "tied_cuts"}): "cuts" counts the
    selections that dropped a column, "tied_cuts" those where the last column kept and the first one dropped had equal
    scores, so that the column order decided"""
    assert budget >= min_budget(w)
    grid, player, winner, plies = roots
    n = grid.shape[0]
    alive = legal_columns(h, w, k, roots)
    total = np.array([rounds(a) if a else 0 for a in alive.sum(axis=1)])
    counts = np.zeros((n, w, 3), dtype=np.int64)
    given = np.zeros((n, w), dtype=np.int64)
    first_p = np.zeros(n, dtype=np.int64)
    steps, seen = 0, {"cuts": 0, "tied_cuts": 0}
    for r in range(int(total.max(initial=0))):
        active = np.flatnonzero(total > r)
        q = {int(i): budget // (int(alive[i].sum()) * int(total[i])) for i in active}
        rows, cols, ids = [], [], []
        for i in map(int, active):
            for c in map(int, np.flatnonzero(alive[i])):
                for p in range(int(first_p[i]), int(first_p[i]) + q[i]):
                    rows.append(i)
                    cols.append(c)
                    ids.append((((first_game + i) * w + c) * budget + p) & MASK64)
        rows, cols = np.array(rows, dtype=np.int64), np.array(cols, dtype=np.int64)
        won, played = _play(h, w, k, roots, rows, cols, ids, seed, max_plies, per_ply, policy)
        steps += played
        mover = player[rows].astype(np.int64)
        np.add.at(counts, (rows, cols, 0), won == mover)
        np.add.at(counts, (rows, cols, 1), won == 2)
        np.add.at(counts, (rows, cols, 2), won == 1 - mover)
        for i in map(int, active):
            survivors = np.flatnonzero(alive[i])
            given[i, survivors] += q[i]
            first_p[i] += q[i]
            score = 2 * counts[i, survivors, 0] + counts[i, survivors, 1]
            order = np.lexsort((survivors, -score))        # score descending, then column ascending
            keep = (survivors.size + 1) // 2
            if keep < survivors.size:
                seen["cuts"] += 1
                seen["tied_cuts"] += int(score[order[keep - 1]] == score[order[keep]])
            alive[i] = False
            alive[i, survivors[order[:keep]]] = True
    assert (alive.sum(axis=1) == (total > 0)).all() and (given.sum(axis=1) <= budget).all()
    best = np.where(total > 0, alive.argmax(axis=1), -1)
    return counts.astype(np.int32), given.astype(np.int32), best.astype(np.int32), steps, seen


# ---- the cases of the GPU comparison.  Roots: a spread of fuzz_cases.connect_roots (the start, positions a few plies in,
# positions one to three plies before the end of random games, ended boards) and the last positions of its tiled game,
# whose columns fill up one by one: roots with W, ..., 3, 2, 1 legal columns.  At most 32 roots a case.
# cap: None, or plies past the median ply count of the running roots (the later roots start at or beyond it).
Case = namedtuple("Case", "h w k budget cap first_game")
CASES = (
    Case(6, 7, 4, 100, None, 5),               # Connect4: q = 4, 8, 16 for 7 columns
    Case(6, 7, 4, 100, 3, 1 << 33),            # a cap that cuts playouts, game ids beyond 32 bits
    Case(5, 6, 3, 64, None, 3),                # count 3, one word
    Case(2, 5, 3, 40, None, 9),                # more columns than a column field counts: the general bit search
    Case(6, 12, 4, 96, None, 2),               # two words
    Case(12, 13, 5, 60, None, 7),              # three words; q = 1 in the first round
)
DECISIVE = (0, 1, 4, 5)                        # the cases that run under the decisive policy too
RUNNING_ROOTS, ENDED_ROOTS, TILED_ROOTS = 20, 2, 8


def case_id(case):
    return f"{case.h}x{case.w}x{case.k}-B{case.budget}" + ("-capped" if case.cap is not None else "")


@functools.lru_cache(maxsize=None)
def _case_roots(h, w, k):
    rng = np.random.default_rng(41000 + 100 * h + w + 7 * k)
    mixed = fc.connect_roots(h, w, k, rng)
    running, ended = np.flatnonzero(mixed[2] == -1), np.flatnonzero(mixed[2] != -1)
    tiled = fc.tiled_game(h, w, k, last=min(w + 1, TILED_ROOTS))
    roots = fc.concat([fc.take(mixed, running[:RUNNING_ROOTS]), fc.take(mixed, ended[:ENDED_ROOTS]), tiled])
    assert roots[0].shape[0] <= 32
    return roots


def case_roots(case):
    return _case_roots(case.h, case.w, case.k)


def case_max_plies(case, roots=None):
    if case.cap is None:
        return UNCAPPED
    roots = case_roots(case) if roots is None else roots
    return int(np.median(roots[3][roots[2] == -1])) + case.cap


@functools.lru_cache(maxsize=None)
def case_expected(index, per_ply=False, policy="uniform"):
    """halving_expected of CASES[index], computed once a session and shared: treat the arrays as read-only"""
    case = CASES[index]
    roots = case_roots(case)
    return halving_expected(case.h, case.w, case.k, roots, SEED, case.first_game, case.budget, case_max_plies(case, roots), per_ply,
                            policy)
