"""The CPU reference of the Bounce playout policy (bgs_bounce_evaluate_moves_policy, include/bgs.h) and the case table of
its tests.  Not a test module.

The reference is built on the oracle's public API alone (BounceOracle.actions, step_actions, oracle.sample_index): one
oracle board for every legal (root, slot, playout), stepped by the slot's move, then all boards played in lock step.  A
running board below the cap takes its canonical action list L, keeps the actions W whose target lies in the mover's goal
row (the top row y = H - 1 for player 0, the bottom row y = 0 for player 1) when there are any, and plays element
sample_index(seed, G, plies, |S|) of that list, G the game id of bgs.h.  With uniform=True the list is always L: the
oracle's own rollout."""

from collections import namedtuple

import numpy as np

from oracle import oracle
from tests.mc_expected import make_roots
from tests.test_gpu_parity import BOUNCE_GRIDS

SEED = 0x5EED0F0E7A1A7E00
CLASSES = ("win", "win_many", "none")   # playout plies with W not empty, with |W| >= 2, with W empty
MASK64 = (1 << 64) - 1

# more than 8 columns (the kernel's three-word move list) on at most 64 cells, tall enough that games last
TALL_WIDE = np.array([[0] * 9, [1, 2, 1, 2, 1, 2, 1, 2, 1], [0] * 9, [0] * 9, [0] * 9, [2, 1, 2, 1, 2, 1, 2, 1, 2], [0] * 9],
                     dtype=np.int8)
GRIDS = dict(BOUNCE_GRIDS, tall_wide=TALL_WIDE)

# name: a grid of GRIDS; n roots from make_roots(grid, n, roots_seed); the CPU checks run `playouts` a move from
# `first_game`, capped at (the least ply count of a running root) + cap_past, or at 1024 plies when cap_past is None
Case = namedtuple("Case", "name n roots_seed playouts cap_past first_game")
CASES = [
    Case("default", 8, 5, 6, None, 5),
    Case("small", 8, 6, 6, 6, 2**33),
    Case("big_values", 8, 7, 4, None, 5),
    Case("crowded", 8, 8, 3, None, 2**33),
    Case("narrow", 8, 9, 6, None, 5),
    Case("blocked_start", 8, 10, 6, None, 5),
    Case("wide", 8, 11, 3, None, 5),
    Case("tall_wide", 8, 12, 3, None, 2**33),
]
LONG = 1024


def case_roots(case):
    return make_roots(GRIDS[case.name], case.n, case.roots_seed)


def short_cap(roots, past):
    """`past` plies beyond the least ply count of a running root (of any root when none runs)"""
    _, _, winner, plies = roots
    running = winner == -1
    return int((plies[running] if running.any() else plies).min()) + past


def case_max_plies(case, roots):
    return LONG if case.cap_past is None else short_cap(roots, case.cap_past)


def root_actions(grid, roots):
    """the oracle's action list of every root (empty for an ended one)"""
    g, player, winner, plies = roots
    probe = oracle.BounceOracle(grid, 1)
    out = []
    for i in range(g.shape[0]):
        probe.grid[:], probe.player[:], probe.winner[:], probe.plies[:] = g[i], player[i], winner[i], plies[i]
        out.append(probe.actions(0) if winner[i] == -1 else [])
    return out


def bounce_policy_expected(grid, roots, seed, first_game, playouts, max_plies, uniform=False):
    """(counts int32[n, W, H * W, 3], env-steps, seen): the counts and transitions of the evaluation under the decisive
    policy (uniform=True: under the uniform policy) and the playout plies of every class of CLASSES"""
    g, player, winner, plies = roots
    h, w = grid.shape
    n, S = g.shape[0], w * h * w
    counts = np.zeros((n, S, 3), dtype=np.int32)
    seen = dict.fromkeys(CLASSES, 0)
    root, slot, first = [], [], []
    for i, acts in enumerate(root_actions(grid, roots)):
        for (sx, sy), (tx, ty) in acts:
            root.append(i)
            slot.append(sx * h * w + ty * w + tx)
            first.append((sx, sy, tx, ty))
    if not root:
        return counts.reshape(n, w, h * w, 3), 0, seen
    root, slot = np.repeat(root, playouts), np.repeat(slot, playouts)
    N = root.size
    game = [(((first_game + int(root[k])) * S + int(slot[k])) * playouts + k % playouts) & MASK64 for k in range(N)]
    orc = oracle.BounceOracle(grid, N)
    orc.grid[:], orc.player[:], orc.winner[:], orc.plies[:] = g[root], player[root], winner[root], plies[root]
    assert (orc.step_actions(np.repeat(np.int32(first), playouts, axis=0)) == 0).all()
    steps = N
    lists = {}   # (board, player) -> (L, W): boards repeat among the playouts of a root
    while True:
        active = np.flatnonzero((orc.winner == -1) & (orc.plies < max_plies))
        if active.size == 0:
            break
        moves = np.full((N, 4), -1, dtype=np.int32)
        for k in active:
            mover = int(orc.player[k])
            key = (orc.grid[k].tobytes(), mover)
            if key not in lists:
                L = orc.actions(int(k))
                goal_y = 0 if mover else h - 1
                lists[key] = (L, [a for a in L if a[1][1] == goal_y])
            L, W = lists[key]
            seen["win" if W else "none"] += 1
            seen["win_many"] += len(W) >= 2
            cand = L if uniform or not W else W
            (sx, sy), (tx, ty) = cand[oracle.sample_index(seed, game[k], int(orc.plies[k]), len(cand))]
            moves[k] = (sx, sy, tx, ty)
        assert (orc.step_actions(moves)[active] == 0).all()
        steps += int(active.size)
    mover = player[root]
    for j, hit in enumerate((orc.winner == mover, orc.winner == 2, orc.winner == 1 - mover)):
        np.add.at(counts[:, :, j], (root[hit], slot[hit]), 1)
    return counts.reshape(n, w, h * w, 3), steps, seen
