"""What the CPU statement of sequential halving (tests/halving_expected.py) and its case table hold: the schedule
arithmetic of include/bgs.h, the kinds of root the GPU comparison must see, and the agreement of the helper's playouts
with the flat evaluation's reference where the two must coincide.  No GPU."""

import numpy as np
import pytest

from tests import halving_expected as he
from tests import mc_expected as mc
from tests.policy_expected import completes


def test_rounds_is_the_ceiling_of_log2_and_at_least_one():
    assert [he.rounds(x) for x in range(1, 18)] == [1, 1, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 4, 4, 4, 4, 5]
    assert [he.min_budget(w) for w in (1, 2, 5, 6, 7, 12, 13, 16)] == [1, 2, 15, 18, 21, 48, 52, 64]


@pytest.mark.parametrize("w", range(1, 17))
def test_schedule_arithmetic(w):
    for a in range(1, w + 1):
        for budget in (he.min_budget(w), he.min_budget(w) + 1, 100, 448, 1000, 2**31 - 1):
            if budget < he.min_budget(w):
                continue
            plan = he.schedule(a, budget)
            assert len(plan) == he.rounds(a)
            assert all(q >= 1 for _, q in plan), (a, budget, plan)
            assert sum(m * q for m, q in plan) <= budget, (a, budget, plan)
            assert plan[0][0] == a and (plan[-1][0] + 1) // 2 == 1
            for (m, _), (m_next, _) in zip(plan, plan[1:]):
                assert m_next == (m + 1) // 2
    assert he.schedule(0, 100) == []


def test_seven_columns_survive_as_7_4_2_1():
    plan = he.schedule(7, 100)
    assert [m for m, _ in plan] == [7, 4, 2] and (plan[-1][0] + 1) // 2 == 1
    assert [q for _, q in plan] == [4, 8, 16]
    assert [q for _, q in he.schedule(13, 60)] == [1, 2, 3, 7]


def test_the_table_is_the_one_the_gpu_comparison_needs():
    assert [(c.h, c.w, c.k, c.budget) for c in he.CASES] == [
        (6, 7, 4, 100), (6, 7, 4, 100), (5, 6, 3, 64), (2, 5, 3, 40), (6, 12, 4, 96), (12, 13, 5, 60)]
    assert he.CASES[1].cap is not None and he.CASES[1].first_game == 1 << 33
    assert [(he.CASES[j].h, he.CASES[j].w) for j in he.DECISIVE] == [(6, 7), (6, 7), (6, 12), (12, 13)]
    for case in he.CASES:
        assert case.budget >= he.min_budget(case.w)
        assert case_roots_count(case) <= 32


def case_roots_count(case):
    return he.case_roots(case)[0].shape[0]


def test_the_roots_hold_every_kind_of_root():
    legal_counts, ended = set(), 0
    for case in he.CASES:
        roots = he.case_roots(case)
        legal = he.legal_columns(case.h, case.w, case.k, roots)
        legal_counts |= {(case.w, int(a)) for a in legal.sum(axis=1)}
        ended += int((roots[2] != -1).sum())
        assert not legal[roots[2] != -1].any()
    # Connect4: roots with 1, 2, 3 and all 7 columns legal (so 1, 2 and 3 rounds), and the wide boards have 4 rounds
    assert {(7, 1), (7, 2), (7, 3), (7, 7)} <= legal_counts
    assert (12, 12) in legal_counts and (13, 13) in legal_counts
    assert ended >= len(he.CASES)
    # a column that wins at once: all its playouts are wins, whatever the draws
    counts, given, best, _, seen = he.case_expected(0)
    at_once = (given > 0) & (counts[..., 0] == given) & (given == given.max(axis=1, keepdims=True))
    roots = he.case_roots(he.CASES[0])
    sure = 0
    for i, c in zip(*np.nonzero(at_once)):
        sure += int(completes(roots[0][i:i + 1], roots[1][i:i + 1].astype(np.int64), 4)[0, c])
    assert sure >= 1
    # at least one cut that the column order decided
    assert seen["cuts"] > 0 and seen["tied_cuts"] >= 1, seen


def test_results_are_consistent_with_the_schedule():
    for index, case in enumerate(he.CASES):
        counts, given, best, steps, _ = he.case_expected(index)
        roots = he.case_roots(case)
        legal = he.legal_columns(case.h, case.w, case.k, roots)
        a = legal.sum(axis=1)
        assert (given[~legal] == 0).all() and (counts[~legal] == 0).all()
        assert (given[legal] >= 1).all()
        assert (counts.sum(axis=-1) <= given).all()
        if case.cap is None:
            assert (counts.sum(axis=-1) == given).all()
        assert (given.sum(axis=1) <= case.budget).all()
        assert ((best == -1) == (a == 0)).all()
        for i in np.flatnonzero(a):
            plan = he.schedule(a[i], case.budget)
            assert legal[i, best[i]] and given[i, best[i]] == sum(q for _, q in plan)
            assert sorted(given[i][legal[i]]) == sorted(
                sum(q for _, q in plan[:r + 1]) for r, (m, _) in enumerate(plan)
                for _ in range(m - ((m + 1) // 2 if r + 1 < len(plan) else 0)))
        assert steps >= int(given.sum())


@pytest.mark.parametrize("per_ply", [False, True], ids=["per-block", "per-ply"])
def test_a_single_legal_column_is_the_flat_evaluation_of_that_column(per_ply):
    """one legal column: one round of `budget` playouts, the games of the flat evaluation with playouts = budget"""
    case = he.CASES[0]
    roots = he.case_roots(case)
    legal = he.legal_columns(case.h, case.w, case.k, roots)
    rows = np.flatnonzero(legal.sum(axis=1) == 1)
    assert rows.size
    single = tuple(a[rows] for a in roots)
    counts, given, best, steps, _ = he.halving_expected(case.h, case.w, case.k, single, he.SEED, 11, case.budget, he.UNCAPPED, per_ply)
    flat, flat_steps = mc.connect_expected(case.h, case.w, case.k, single, he.SEED, 11, case.budget, he.UNCAPPED, per_ply)
    np.testing.assert_array_equal(counts, flat)
    assert steps == flat_steps
    assert (given.sum(axis=1) == case.budget).all()
    np.testing.assert_array_equal(best, legal[rows].argmax(axis=1))
