"""CPU-only checks of tests/bounce_guided_expected.py, the CPU statement of bgs_bounce_guided_step, against facts derived
by hand: the quantisation on hand-picked rows, the sense of the selection rule (a move into the goal row collects the
visits), the restart of a stepped board, the independence of the trees, the cap -- and the coverage conditions that keep
the sweeps of tests/test_gpu_bounce_guided.py from being vacuous, over the union of those sweeps."""

import os
import re

import numpy as np
import pytest

from oracle import oracle
from tests import bounce_guided_expected as bg
from tests import fuzz_cases as fc
from tests.search_bounce_expected import _actions, _step, min_edges, slot_of

CORNERS = list(fc.BOUNCE_CORNERS)
RUNS = [(key, sweep[0]) for key in CORNERS for sweep in bg.SWEEPS]


def test_the_statement_speaks_the_header_constants():
    from tests.conftest import PKG

    with open(os.path.join(os.path.dirname(PKG), "include", "bgs.h")) as f:
        text = f.read()
    assert int(re.search(r"^#define BGS_BOUNCE_FOREST_MAX_NODES (\d+)$", text, flags=re.M).group(1)) == bg.MAX_NODES
    assert "#define BGS_BOUNCE_FOREST_MAX_EDGES (1 << 29)" in text and bg.MAX_EDGES == 1 << 29
    assert "#define BGS_BOUNCE_SEARCH_MIN_EDGES(h, w) ((h) >= 3 ? (w) * (w) * ((h) - 2) : 1)" in text
    assert (min_edges(9, 6), min_edges(2, 5), bg.default_edges(9, 6, 49)) == (252, 1, 252 + 32 * 48)


def test_the_quantisation():
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    row = np.zeros(40, dtype=np.float32)
    row[[3, 7, 11, 19, 23, 29, 31, 37]] = [0.5, nan, -1.0, inf, 0.0, 2.0 ** -16, 2.0 ** -17, 0.75]
    assert bg.prior_weights(row, [3, 7, 11, 19, 23, 29, 31, 37]) == {3: 32768, 7: 0, 11: 0, 19: 65536, 23: 0, 29: 1, 31: 0, 37: 49152}
    shares = bg.prior_shares(row, [3, 19, 37])          # W = 147456
    assert shares == [14563, 29127, 21845] and 65536 - 3 < sum(shares) <= 65536
    # an all-zero row, and a row with weight on illegal slots only: equal P over the legal slots
    assert bg.prior_shares(np.zeros(40, dtype=np.float32), [1, 2, 5]) == [21845, 21845, 21845]
    assert bg.prior_shares(row, [7, 11, 23, 31]) == [16384, 16384, 16384, 16384]
    # 512 arms of full weight: W = 2^25, the largest there is, and P = 128 each
    assert bg.prior_shares(np.ones(512, dtype=np.float32), list(range(512))) == [128] * 512
    # the target masks are those of bgs_bounce_read_targets: bit ty * w + tx of entry sx
    masks = bg.target_masks([((0, 1), (1, 2)), ((0, 1), (0, 3)), ((2, 1), (2, 0))], 3)
    assert masks.tolist() == [(1 << 7) | (1 << 9), 0, 1 << 2] and bg.legal_slots(masks, 4, 3) == [7, 9, 2 * 12 + 2]


@pytest.mark.parametrize("run", RUNS, ids=lambda r: f"{r[0]}-{r[1]}")
def test_the_invariants_of_a_run(run):
    key, sweep = run
    grid, roots, nodes, edges, cpuct, max_plies = bg.sweep_arguments(key, sweep)
    model, calls = bg.sweep_expected(key, sweep)
    h, w = grid.shape
    assert len(calls) == bg.SIMULATIONS + 1 and (calls[-1][2] == bg.IDLE).all()
    for i, root in enumerate(model.root):
        position = (roots[0][i], int(roots[1][i]), int(roots[3][i]))
        arms = len(_actions(grid, position)) if roots[2][i] == -1 else 0
        if not arms:
            assert root is None and calls[0][2][i] == bg.IDLE and calls[-1][6][i] == -1 and not calls[-1][4][i].any()
            assert calls[-1][8][i] == 0 and not calls[0][3][i].any()
            continue
        assert calls[0][2][i] == bg.EVALUATE and model.restarts[i] == 1
        assert [slot_of(a, h, w) for a in _actions(grid, position)] == bg.legal_slots(calls[0][3][i], h, w)
        # the first evaluation is the root's: every later one went down an edge of the root
        assert sum(root.n) == bg.SIMULATIONS - 1 == int(calls[-1][4][i].sum())
        assert model.count[i] == 1 + bg.count_nodes(root) <= nodes and calls[-1][7][i] == model.count[i] - 1
        assert model.used[i] == sum(len(node.actions) for node in bg.walk(root)) <= edges and calls[-1][8][i] == model.used[i]
        for node in bg.walk(root):
            arms = len(node.actions)
            assert 1 <= arms <= min_edges(h, w)
            assert all(0 <= node.s[a] <= 2048 * node.n[a] for a in range(arms))
            assert 65536 - arms < sum(node.P) <= 65536
            for a, child in enumerate(node.child):
                if child is not None:                   # a child's visits are the edge's, but for the one that made it
                    assert sum(child.n) == node.n[a] - 1 and child.position[2] < model.cap
    assert model.seen["made"] == sum(c - 1 for c in model.count if c)


def test_the_sweeps_are_not_vacuous():
    """the coverage conditions, over the union of the runs the GPU comparison makes"""
    total, served = bg.new_seen(), dict.fromkeys(bg.SPECIALS, 0)
    for key, sweep in RUNS:
        model = bg.sweep_expected(key, sweep)[0]
        for name, x in model.seen.items():
            total[name] = max(total[name], x) if name.startswith("max_") else total[name] + x
        for name in bg.SPECIALS:
            served[name] += model.served[name]
    assert all(served[name] > 0 for name in bg.SPECIALS), served            # every special row was served to an EVALUATE leaf
    assert total["goal"] > 0 and total["blocked"] > 0 and total["cap"] > 0, total   # (a draw is rare: not asked for)
    assert total["refused_nodes"] > 0 and total["refused_edges"] > 0, total
    assert total["max_depth"] >= 3, total
    assert total["max_leaf_arms"] > 64, total                               # a lane holds more than one arm
    assert total["made"] > 0


def test_a_move_into_the_goal_row_collects_the_visits():
    """the constant evaluator (uniform priors, value 0), cpuct = 256, more simulations than a root has arms: a root with a
    move into the goal row ends with `best` on a move that wins at once -- a move into the goal row, that is, unless the
    root also has a move that wins by leaving the opponent without one: both are worth sigma = 0, and where the root has none
    of the second kind `best` is a goal move"""
    roots_with_a_goal_move = goal_moves_chosen = 0
    for key in ("default", "8x8", "16x4"):
        grid = fc.BOUNCE_CORNERS[key]()
        h, w = grid.shape
        roots = fc.bounce_end_games(grid, 12, 77, last=2)
        n = roots[0].shape[0]
        goal, wins = [], []
        for i in range(n):
            position = (roots[0][i], int(roots[1][i]), int(roots[3][i]))
            acts = _actions(grid, position)
            assert len(acts) < 128
            goal.append([slot_of(a, h, w) for a in acts if a[1][1] in (0, h - 1)])
            wins.append([slot_of(a, h, w) for a in acts if _step(grid, position, a)[0] == position[1]])
            assert set(goal[i]) <= set(wins[i])
        best = bg.GuidedMoves(grid, n, 129, cpuct=256).run(roots, bg.constant_network_moves, 128)[-1][6]
        for i in range(n):
            if goal[i]:
                roots_with_a_goal_move += 1
                goal_moves_chosen += int(best[i] in goal[i])
                assert best[i] in wins[i], (key, i, wins[i], best[i])
                assert best[i] in goal[i] or goal[i] != wins[i], (key, i, goal[i], best[i])
    assert roots_with_a_goal_move >= 12 and goal_moves_chosen >= 8


def stepped(grid, roots, moves):
    """`roots` after `moves` int32[n, 4] (a negative row: the board stays), by the oracle"""
    orc = oracle.BounceOracle(grid, roots[0].shape[0])
    orc.grid[:], orc.player[:], orc.winner[:], orc.plies[:] = roots
    assert (orc.step_actions(moves)[moves[:, 0] >= 0] == 0).all()
    return orc.grid.copy(), orc.player.copy(), orc.winner.copy(), orc.plies.copy()


def first_moves(grid, roots, which):
    """int32[n, 4]: the first legal move of every running board of `which` (a bool mask), -1 elsewhere"""
    n = roots[0].shape[0]
    moves = np.full((n, 4), -1, dtype=np.int32)
    for i in np.flatnonzero(which & (roots[2] == -1)):
        (sx, sy), (tx, ty) = _actions(grid, (roots[0][i], int(roots[1][i]), int(roots[3][i])))[0]
        moves[i] = (sx, sy, tx, ty)
    return moves


def test_a_stepped_board_restarts_its_tree():
    case = fc.bounce_case("default")
    roots, n = case.roots, case.roots[0].shape[0]
    model = bg.GuidedMoves(case.grid, n, 33)
    call = model.step(roots, flags=bg.RESTART)
    for _ in range(12):
        call = model.step(roots, *bg.fake_network_moves(call[0], call[1], call[3]))
    moves = first_moves(case.grid, roots, np.arange(n) % 2 == 0)
    moved = moves[:, 0] >= 0
    assert moved.sum() >= 4 and (~moved & (roots[2] == -1)).sum() >= 4
    after = stepped(case.grid, roots, moves)
    before_restarts = list(model.restarts)
    last, call = call, model.step(after, *bg.fake_network_moves(call[0], call[1], call[3]))
    running = after[2] == -1
    assert [model.restarts[i] - before_restarts[i] for i in range(n)] == [int(moved[i] or not running[i]) for i in range(n)]
    assert (call[7][moved] == 0).all() and not call[4][moved].any() and (call[6][moved] == -1).all()
    assert (call[2][moved & running] == bg.EVALUATE).all() and (call[2][moved & ~running] == bg.IDLE).all()
    np.testing.assert_array_equal(call[0][moved], after[0][moved])
    carried = ~moved & running                  # the others carry on: a visit more than a call ago, and no node fewer
    assert (call[4][carried].sum(axis=(1, 2)) == 12).all() and (last[4][carried].sum(axis=(1, 2)) == 11).all()
    assert (call[7][carried] >= last[7][carried]).all() and call[7][carried].sum() > 0


def test_two_halves_of_a_batch_give_the_whole():
    case = fc.bounce_case("8x8")
    n = case.roots[0].shape[0]
    cut = n // 2 + 1
    parts = (slice(None), slice(0, cut), slice(cut, None))
    runs = [bg.GuidedMoves(case.grid, len(range(n)[part]), 17).run(tuple(a[part] for a in case.roots), bg.fake_network_moves, 24)
            for part in parts]
    for t, (whole, first, second) in enumerate(zip(*runs)):
        for name, x, a, b in zip(bg.NAMES, whole, first, second):
            np.testing.assert_array_equal(x, np.concatenate([a, b]), err_msg=f"{name} call {t}")


def test_a_cap_one_ply_past_the_root_makes_every_leaf_terminal():
    """max_plies = the root's ply count + 1: whatever arm is taken, the position behind it holds the cap, so every leaf after
    the root's own evaluation is TERMINAL with sigma 1024 -- 2048 - 1024 for the root's mover -- and no node is ever made"""
    grid = fc.BOUNCE_CORNERS["default"]()
    orc = oracle.BounceOracle(grid, 1)
    roots = (orc.grid.copy(), orc.player.copy(), orc.winner.copy(), orc.plies.copy())
    assert roots[3][0] == 0 and roots[2][0] == -1
    model = bg.GuidedMoves(grid, 1, 33, max_plies=1)
    calls = model.run(roots, bg.fake_network_moves, 32)
    assert calls[0][2][0] == bg.EVALUATE and calls[-1][2][0] == bg.IDLE
    assert all(call[2][0] == bg.TERMINAL and call[1][0] == 1 for call in calls[1:-1])
    assert all(call[7][0] == 0 and not call[3].any() for call in calls[1:])
    assert model.seen["made"] == 0 and model.seen["cap"] == 31 and model.seen["evaluated"] == 1
    visits, scores = calls[-1][4][0], calls[-1][5][0]
    assert visits.sum() == 31 and (scores == 1024 * visits).all()
    # the same root under the default cap does make nodes
    assert bg.GuidedMoves(grid, 1, 33).run(roots, bg.fake_network_moves, 32)[-1][7][0] > 0
