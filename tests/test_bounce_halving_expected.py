"""What the CPU statement of Bounce sequential halving (tests/bounce_halving_expected.py) and its case table hold: the
schedule arithmetic of include/bgs.h, the kinds of root the GPU comparison must see, and the agreement of the helper's
playouts with the flat evaluation's reference where the two must coincide.  No GPU."""

import numpy as np
import pytest

from tests import bounce_halving_expected as bh
from tests import bounce_policy_expected as be


def test_rounds_and_the_schedule_for_1_2_3_5_and_33_arms():
    assert [bh.rounds(a) for a in (1, 2, 3, 5, 33, 512)] == [1, 1, 2, 3, 6, 9]
    assert [bh.min_budget(a) for a in (1, 2, 3, 5, 33, 512)] == [1, 2, 6, 15, 198, 4608]
    assert bh.schedule(1, 40) == [(1, 40)]
    assert bh.schedule(2, 40) == [(2, 20)]
    assert bh.schedule(3, 40) == [(3, 6), (2, 10)]
    assert bh.schedule(5, 160) == [(5, 10), (3, 17), (2, 26)]
    assert bh.schedule(33, 198) == [(33, 1), (17, 1), (9, 3), (5, 6), (3, 11), (2, 16)]
    for a in (1, 2, 3, 5, 33):
        for budget in (bh.min_budget(a), bh.min_budget(a) + 1, 1024, 2**31 - 1):
            plan = bh.schedule(a, budget)
            assert len(plan) == bh.rounds(a) and all(q >= 1 for _, q in plan)
            assert sum(m * q for m, q in plan) <= budget
            assert plan[0][0] == a and (plan[-1][0] + 1) // 2 == 1
            assert all(m_next == (m + 1) // 2 for (m, _), (m_next, _) in zip(plan, plan[1:]))
        assert bh.schedule(a, bh.min_budget(a) - 1)[0][1] == 0 or a == 1   # one less: the first round has no playout


def test_the_table_is_the_one_the_gpu_comparison_needs():
    by = bh.BY_NAME
    assert by["default"].budget == 160 and by["default"].policies == ("uniform", "decisive")
    assert by["small"].cap_past is not None and by["small"].first_game == 2**33
    assert by["wide"].policies == by["tall_wide"].policies == ("decisive",)
    assert bh.case_grid(by["wide"]).shape[1] > 8 and bh.case_grid(by["tall_wide"]).shape[1] > 8     # the three-word move list
    assert {"crowded", "blocked_start", "mixed"} <= set(by)
    for case in bh.CASES:
        arms = bh.arm_counts(case)
        assert arms.size <= 8
        playouts = case.budget * int((arms > 0).sum())
        assert playouts <= 1800, (case.name, playouts)
    arms = bh.arm_counts(by["mixed"])
    need = [bh.min_budget(a) for a in arms if a]
    assert min(need) < by["mixed"].budget < max(need)


def test_the_roots_hold_every_kind_of_root():
    arms, ended, unmoved = set(), 0, 0
    for case in bh.CASES:
        roots = bh.case_roots(case)
        a = bh.arm_counts(case)
        arms |= set(a.tolist())
        ended += int((roots[2] != -1).sum())
        assert not a[roots[2] != -1].any()
        unmoved += int(((a == 0) & (roots[3] == 0)).sum())      # a start position nobody can move in
    assert 1 in arms and any(a >= 3 and a % 2 for a in arms) and any(a > 32 for a in arms)
    assert ended >= len(bh.CASES) and unmoved >= 1


def test_results_are_consistent_with_the_schedule():
    cuts = tied = 0
    for name, policy in bh.RUNS:
        case = bh.BY_NAME[name]
        counts, given, best, steps, seen = bh.case_expected(name, policy)
        n = best.size
        counts, given = counts.reshape(n, -1, 3), given.reshape(n, -1)
        arms = bh.arm_counts(case)
        cuts += seen["cuts"]
        tied += seen["tied_cuts"]
        assert (given.sum(axis=1) <= case.budget).all()
        assert (counts.sum(axis=-1) <= given).all()
        assert steps >= int(given.sum())
        for i, a in enumerate(arms):
            if a == 0:
                assert best[i] == -1 and not given[i].any()
            elif case.budget < bh.min_budget(a):
                assert best[i] == bh.SHORT and not given[i].any() and not counts[i].any()
            else:
                plan = bh.schedule(a, case.budget)
                assert given[i, best[i]] == sum(q for _, q in plan) and int((given[i] > 0).sum()) == a
                assert sorted(given[i][given[i] > 0]) == sorted(
                    sum(q for _, q in plan[:r + 1]) for r, (m, _) in enumerate(plan)
                    for _ in range(m - ((m + 1) // 2 if r + 1 < len(plan) else 0)))
    assert cuts > 0 and tied > 0


def test_the_mixed_case_has_short_roots_and_evaluated_ones():
    _, given, best, _, seen = bh.case_expected("mixed")
    assert seen["short"] == int((best == bh.SHORT).sum()) >= 1
    assert int((best >= 0).sum()) >= 1
    assert not given[best == bh.SHORT].any() and given[best >= 0].any()


def test_the_capped_case_has_playouts_counted_nowhere():
    counts, given, _, _, _ = bh.case_expected("small")
    assert int(given.sum()) > int(counts.sum()) > 0


def test_a_single_legal_move_is_the_flat_evaluation_of_that_slot():
    """one legal move: one round of `budget` playouts, the games of the flat evaluation with playouts = budget"""
    case = bh.BY_NAME["narrow"]
    grid, roots = bh.case_grid(case), bh.case_roots(case)
    rows = np.flatnonzero(bh.arm_counts(case) == 1)
    assert rows.size
    single = tuple(a[rows] for a in roots)
    for policy in ("uniform", "decisive"):
        counts, given, best, steps, _ = bh.bounce_halving_expected(grid, single, bh.SEED, 11, 40, bh.LONG, policy)
        flat, flat_steps, _ = be.bounce_policy_expected(grid, single, bh.SEED, 11, 40, bh.LONG, uniform=policy == "uniform")
        np.testing.assert_array_equal(counts, flat)
        assert steps == flat_steps and (given.reshape(rows.size, -1).sum(axis=1) == 40).all() and (best >= 0).all()


@pytest.mark.parametrize("policy", ["uniform", "decisive"])
def test_an_arms_counts_are_a_prefix_of_the_flat_evaluation(policy):
    """an arm's games are the first `given` of the flat evaluation with playouts = budget: slot by slot its counts are
    at most the flat counts"""
    case = bh.BY_NAME["small"]
    grid, roots = bh.case_grid(case), bh.case_roots(case)
    cap = bh.case_max_plies(case, roots)
    counts, given, _, _, _ = bh.case_expected("small", policy)
    flat, _, _ = be.bounce_policy_expected(grid, roots, bh.SEED, case.first_game, case.budget, cap, uniform=policy == "uniform")
    assert (counts <= flat).all() and (counts[given == 0] == 0).all() and counts.any()
