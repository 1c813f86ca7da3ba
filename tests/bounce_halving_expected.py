"""The CPU statement of bgs_bounce_evaluate_moves_halving (include/bgs.h), built on the oracle's public API alone, and the
case table of tests/test_gpu_evaluate_bounce_halving.py.  No GPU import; not a test module.

The arms of a running root are its A legal moves in the oracle's canonical order (ascending slot x * H * W + ty * W + tx).
R = max(1, ceil(log2 A)) rounds: in round r every surviving arm plays q_r = budget // (survivors * R) further playouts,
indices [P_r, P_r + q_r); then the ceil(survivors / 2) arms ranked highest by (2 * wins + draws descending, slot
ascending) survive.  Playout p of slot s of root i is the game ((first_game + i) * S + s) * budget + p, S = W * H * W.  A
running root with budget < A * R is short: nothing is played, best = SHORT.

The reference plays only the playouts the schedule gives: per round, one oracle batch of the (root, surviving arm,
playout) boards of every root, stepped by their move and played in the lock step of tests/bounce_policy_expected.py --
every ply of a running board below the cap takes the canonical list L, keeps the moves W into the mover's goal row when
the policy is decisive and there are any, and plays element oracle.sample_index(seed, game, plies, size) of that list
under the playout's own game id.  Env-steps are the transitions made, first moves included; the selection is numpy's
lexsort."""

import functools
from collections import namedtuple

import numpy as np

from oracle import oracle
from tests.bounce_policy_expected import GRIDS, MASK64, SEED, root_actions, short_cap
from tests.halving_expected import rounds, schedule
from tests.mc_expected import make_roots

LONG = 1024
SHORT = -2        # BGS_HALVING_SHORT


def min_budget(moves):
    """moves * R(moves): the least budget that gives every arm a playout in every round"""
    return int(moves) * rounds(moves)


def candidates(actions, mover, height, uniform):
    """the candidate list of a ply (the rule of tests/bounce_policy_expected.py): the moves into the mover's goal row when
    the policy is decisive and there are any, else every move"""
    goal_y = 0 if mover else height - 1
    wins = [] if uniform else [a for a in actions if a[1][1] == goal_y]
    return wins or actions


def _play(grid, roots, rows, firsts, ids, seed, max_plies, uniform):
    """(winner int8[len(rows)], env-steps): root rows[j] after the move firsts[j], played on as game ids[j]"""
    g, player, winner, plies = roots
    h = grid.shape[0]
    orc = oracle.BounceOracle(grid, rows.size)
    orc.grid[:], orc.player[:], orc.winner[:], orc.plies[:] = g[rows], player[rows], winner[rows], plies[rows]
    assert (orc.step_actions(firsts) == 0).all()
    steps = int(rows.size)
    lists = {}   # (board, player) -> L: boards repeat among the playouts of a root
    while True:
        active = np.flatnonzero((orc.winner == -1) & (orc.plies < max_plies))
        if active.size == 0:
            break
        moves = np.full((rows.size, 4), -1, dtype=np.int32)
        for k in active:
            mover = int(orc.player[k])
            key = (orc.grid[k].tobytes(), mover)
            if key not in lists:
                lists[key] = orc.actions(int(k))
            cand = candidates(lists[key], mover, h, uniform)
            (sx, sy), (tx, ty) = cand[oracle.sample_index(seed, ids[k], int(orc.plies[k]), len(cand))]
            moves[k] = (sx, sy, tx, ty)
        assert (orc.step_actions(moves)[active] == 0).all()
        steps += int(active.size)
    return orc.winner.copy(), steps


def bounce_halving_expected(grid, roots, seed, first_game, budget, max_plies, policy="uniform"):
    """(counts int32[n, W, H * W, 3], given int32[n, W, H * W], best int32[n], env-steps, {"cuts", "tied_cuts", "short"}):
    "cuts" counts the selections that dropped an arm, "tied_cuts" those where the last arm kept and the first one dropped
    had equal scores, so that the slot order decided, "short" the running roots the budget is too small for"""
    g, player, winner, plies = roots
    h, w = grid.shape
    n, S = g.shape[0], w * h * w
    max_plies = min(int(max_plies), 65535)
    arms = []     # per root: [(slot, (sx, sy, tx, ty))], ascending slot
    for i, acts in enumerate(root_actions(grid, roots)):
        mine = [(sx * h * w + ty * w + tx, (sx, sy, tx, ty)) for (sx, sy), (tx, ty) in acts] if plies[i] < 65535 else []
        assert mine == sorted(mine)
        arms.append(mine)
    total = np.array([rounds(len(a)) if a else 0 for a in arms])
    short = np.array([bool(a) and budget < min_budget(len(a)) for a in arms])
    total[short] = 0
    alive = [list(range(len(a))) for a in arms]
    counts = np.zeros((n, S, 3), dtype=np.int64)
    given = np.zeros((n, S), dtype=np.int64)
    first_p = np.zeros(n, dtype=np.int64)
    steps, seen = 0, {"cuts": 0, "tied_cuts": 0, "short": int(short.sum())}
    for r in range(int(total.max(initial=0))):
        active = np.flatnonzero(total > r)
        q = {int(i): budget // (len(alive[i]) * int(total[i])) for i in active}
        rows, slots, firsts, ids = [], [], [], []
        for i in map(int, active):
            for a in alive[i]:
                slot, move = arms[i][a]
                for p in range(int(first_p[i]), int(first_p[i]) + q[i]):
                    rows.append(i)
                    slots.append(slot)
                    firsts.append(move)
                    ids.append((((first_game + i) * S + slot) * budget + p) & MASK64)
        rows, slots = np.array(rows, dtype=np.int64), np.array(slots, dtype=np.int64)
        won, played = _play(grid, roots, rows, np.array(firsts, dtype=np.int32), ids, seed, max_plies, policy == "uniform")
        steps += played
        mover = player[rows].astype(np.int64)
        np.add.at(counts, (rows, slots, 0), won == mover)
        np.add.at(counts, (rows, slots, 1), won == 2)
        np.add.at(counts, (rows, slots, 2), won == 1 - mover)
        for i in map(int, active):
            at = np.array([arms[i][a][0] for a in alive[i]])
            given[i, at] += q[i]
            first_p[i] += q[i]
            score = 2 * counts[i, at, 0] + counts[i, at, 1]
            order = np.lexsort((at, -score))              # score descending, then slot ascending
            keep = (at.size + 1) // 2
            if keep < at.size:
                seen["cuts"] += 1
                seen["tied_cuts"] += int(score[order[keep - 1]] == score[order[keep]])
            alive[i] = sorted(alive[i][k] for k in order[:keep])
    best = np.full(n, -1, dtype=np.int64)
    for i in range(n):
        if short[i]:
            best[i] = SHORT
        elif total[i]:
            assert len(alive[i]) == 1
            best[i] = arms[i][alive[i][0]][0]
    assert (given.sum(axis=1) <= budget).all()
    shape = (n, w, h * w)
    return counts.reshape(shape + (3,)).astype(np.int32), given.reshape(shape).astype(np.int32), best.astype(np.int32), steps, seen


# ---- the cases of the GPU comparison: roots from make_roots(grid, n, roots_seed) (the start, positions a few and many
# plies in, boards played to the end), at most 8 a case and about 1500 playouts.  cap_past: None (1024 plies), or plies
# past the least ply count of a running root (bounce_policy_expected.short_cap).  The budgets are at least the greatest
# A * R(A) of the case's roots, but for "default" (160 against 204 for its 34-arm root) and "mixed".
Case = namedtuple("Case", "name grid n roots_seed budget cap_past first_game policies")
CASES = (
    Case("default", "default", 8, 5, 160, None, 5, ("uniform", "decisive")),
    Case("small", "small", 8, 6, 96, 6, 2**33, ("uniform", "decisive")),     # a cap that cuts playouts, ids beyond 32 bits
    Case("crowded", "crowded", 6, 8, 256, None, 3, ("uniform",)),             # a root with three arms: 3 -> 2 -> 1
    Case("blocked_start", "blocked_start", 8, 10, 64, None, 5, ("uniform",)),
    Case("narrow", "narrow", 8, 9, 40, None, 7, ("uniform",)),                # one column: roots with a single arm
    Case("wide", "wide", 6, 11, 512, None, 5, ("decisive",)),                 # 12 columns: the three-word move list, 71 arms
    Case("tall_wide", "tall_wide", 6, 12, 352, None, 2**33, ("decisive",)),
    Case("mixed", "default", 8, 5, 100, None, 9, ("uniform",)),               # A * R(A) from 8 to 204: three roots short
)
BY_NAME = {c.name: c for c in CASES}
RUNS = [(c.name, p) for c in CASES for p in c.policies]


@functools.lru_cache(maxsize=None)
def _roots(grid_name, n, roots_seed):
    return make_roots(GRIDS[grid_name], n, roots_seed)


def case_grid(case):
    return GRIDS[case.grid]


def case_roots(case):
    return _roots(case.grid, case.n, case.roots_seed)


def case_max_plies(case, roots=None):
    roots = case_roots(case) if roots is None else roots
    return LONG if case.cap_past is None else short_cap(roots, case.cap_past)


def arm_counts(case):
    """the legal moves of every root of the case (0: an ended root, or one without a move)"""
    return np.array([len(a) for a in root_actions(case_grid(case), case_roots(case))])


@functools.lru_cache(maxsize=None)
def case_expected(name, policy="uniform"):
    """bounce_halving_expected of the case, computed once a session and shared: treat the arrays as read-only"""
    case = BY_NAME[name]
    roots = case_roots(case)
    return bounce_halving_expected(case_grid(case), roots, SEED, case.first_game, case.budget, case_max_plies(case, roots), policy)
