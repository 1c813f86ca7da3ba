"""What the case table of the policy, halving and tree-search sweeps (tests/policy_fuzz_cases.py) must contain, stated on
the CPU references alone -- tests/policy_expected.py, halving_expected.py, search_expected.py, search_prove_expected.py
and their Bounce twins -- so that it runs anywhere: the GPU comparison of tests/test_gpu_fuzz_policy.py is only as good
as its cases.  These are conditions on the table, not measurements: where a draw of the table misses one, the recipe
changes (more budget, another corner), never the condition.

Cost of the references.  A decisive playout ply costs the lock-step reference about 26 us, and a search iteration pays
numpy's fixed cost a ply on top, so the decisive searches are the expensive side: over the 16 + 16 Connect keys the
decisive evaluation takes 5 s, the halving 12 s a policy, the uniform searches 4 s and the decisive ones 60 s (worst: key
10, 8x16x6 uncapped at T = 36, 11 s on 4 roots), the proving searches on the corners 3 s and 42 s; every Bounce reference
together 20 s.  A sum or a maximum that holds over some runs holds over all of them, so the search conditions below are
stated on the uniform runs, the halving ones on the decisive runs, and this module never plays a decisive search."""

import numpy as np
import pytest

from tests import bounce_policy_expected as bp
from tests import fuzz_cases as fc
from tests import halving_expected as he
from tests import policy_expected as pe
from tests import policy_fuzz_cases as pf

CELLS = {(nw, four) for nw in (1, 2, 3) for four in (True, False)}


def test_the_keys_are_the_corner_tables_and_the_random_keys_asked_for():
    assert pf.connect_keys()[: pf.CONNECT_CASES] == list(range(16)) and set(fc.CONNECT_CORNERS) <= set(pf.connect_keys())
    assert pf.bounce_keys()[: pf.BOUNCE_CASES] == list(range(12)) and set(fc.BOUNCE_CORNERS) <= set(pf.bounce_keys())
    assert len(fc.CONNECT_CORNERS) == 16 and len(fc.BOUNCE_CORNERS) == 6
    for key in pf.connect_keys():
        c, base = pf.connect_key(key), fc.connect_case(key)
        assert (c.h, c.w, c.k, c.nw) == (base.h, base.w, base.k, base.nw)
        least = he.min_budget(c.w)
        assert c.budget in (least, 2 * least + 1, 5 * least) and 0 <= c.first_game < 1 << 40, pf.describe(c)
        assert 8 <= c.iterations <= 40 and c.leaf_playouts in (1, 3, 8) and c.explore in (0, 20000, 65536), pf.describe(c)
        assert c.playouts == (4 if isinstance(key, str) else c.playouts) and c.playouts in (1, 3, 4, 8), pf.describe(c)
    for key in pf.bounce_keys():
        c, base = pf.bounce_key(key), fc.bounce_case(key)
        np.testing.assert_array_equal(c.grid, base.grid)
        assert c.playouts in (1, 3, 6) and c.max_plies == (base.max_plies[0], fc.LONG) and c.roots[0].shape[0] <= 4
    assert {pf.connect_key(key).per_ply for key in pf.connect_keys()} == {False, True}
    assert {pf.connect_key(key).max_plies == pf.UNCAPPED for key in pf.connect_keys()} == {False, True}
    assert {pf.bounce_key(key).min_pool for key in pf.bounce_corner_keys()} == {False, True}


def test_connect_ply_classes():
    """each of (NW in 1, 2, 3) x (k == 4, k != 4): the decisive playouts of its keys together hold plies that win, that only
    block, that do neither, and plies with two or more winning / blocking cells (where the draw picks among them)"""
    total = {cell: dict.fromkeys(pe.CLASSES, 0) for cell in CELLS}
    for key in pf.connect_keys():
        c = pf.connect_key(key)
        for name, plies in pf.connect_eval_expected(key)[2].items():
            total[(c.nw, c.k == 4)][name] += plies
    for cell, seen in total.items():
        assert all(seen[name] > 0 for name in pe.CLASSES), f"(NW, k == 4) = {cell}: {seen}"


def test_connect_cell_choice_on_one_word():
    """both ways draw_from_cells picks a cell on one word -- the column-field search (h <= 15 and w <= 2^h) and the general
    bit search -- are taken with several W or B cells to choose from"""
    have = set()
    for key in pf.connect_keys():
        c = pf.connect_key(key)
        seen = pf.connect_eval_expected(key)[2]
        if c.nw == 1 and seen["win_many"] + seen["block_many"] > 0:
            have.add(c.w > (1 << c.h))
    assert have == {False, True}, have


def test_connect_halving_roots_cuts_and_teams():
    """every count of legal columns from 1 to w among the halving roots of some key of every NW; over the table, cuts that
    the score decided and cuts that the column order decided; the wide budgets reach the 256-lane team, the others not"""
    ladders = set()
    cuts = tied = 0
    for key in pf.connect_keys():
        c = pf.connect_key(key)
        legal = he.legal_columns(c.h, c.w, c.k, c.halving_roots).sum(axis=1)
        if set(range(1, c.w + 1)) <= set(legal.tolist()):
            ladders.add(c.nw)
        seen = pf.connect_halving_expected(key, "decisive")[4]
        cuts, tied = cuts + seen["cuts"], tied + seen["tied_cuts"]
        assert c.budget // he.rounds(c.w) <= 512, pf.describe(c)
        assert c.halving_roots[0].shape[0] <= pf.EVAL_ROOTS and c.roots[0].shape[0] <= pf.EVAL_ROOTS
    assert ladders == {1, 2, 3}, ladders
    assert cuts > 0 and 0 < tied < cuts, (cuts, tied)
    wide = {pf.connect_key(key).nw: pf.connect_key(key) for key in pf.WIDE}
    assert set(wide) == {1, 2, 3} and wide[3].w * (wide[3].h + 1) == 192
    for c in wide.values():
        budget, roots = c.wide
        assert budget // he.rounds(c.w) > 512 and roots[0].shape[0] == 2 and (roots[2] == -1).all()
        assert pf.connect_halving_expected(c.key, "uniform", True)[4]["cuts"] > 0


def test_connect_search_branches():
    """over the uniform searches of the table (the decisive ones add to every sum): selections the column order decided,
    leaves that end the game, leaves at the cap, roots whose best column the tie-break chose; a path of three edges or
    more for every NW; and, for every NW, a corner whose proving search proves a root column"""
    total = dict.fromkeys(("tied_selections", "terminal_leaves", "capped_leaves", "best_ties"), 0)
    depth = dict.fromkeys((1, 2, 3), 0)
    for key in pf.connect_keys():
        c = pf.connect_key(key)
        assert c.search_roots[0].shape[0] <= pf.SEARCH_ROOTS
        assert pf.connect_search_roots(c, "decisive")[0].shape[0] <= (pf.WIDE_SEARCH_ROOTS if c.nw == 3 else pf.SEARCH_ROOTS)
        seen = pf.connect_search_expected(key, "uniform")[5]
        for name in total:
            total[name] += seen[name]
        depth[c.nw] = max(depth[c.nw], seen["max_depth"])
    assert all(value > 0 for value in total.values()), total
    assert all(value >= 3 for value in depth.values()), depth
    proved = set()
    for key in pf.connect_corner_keys():
        codes = pf.connect_prove_expected(key, "uniform")[4]
        if ((codes != pf.sp.SOLVE_UNKNOWN) & (codes != pf.sp.SOLVE_NONE)).any():
            proved.add(pf.connect_key(key).nw)
    assert proved == {1, 2, 3}, proved


def test_bounce_classes_and_halving_roots():
    """grids of at most 8 and of more than 8 columns: decisive playout plies with a move into the goal row, with two or
    more, and with none; a halving root with three arms or more and one with exactly one"""
    total = {wide: dict.fromkeys(bp.CLASSES, 0) for wide in (False, True)}
    arms = set()
    for key in pf.bounce_keys():
        c = pf.bounce_key(key)
        for cap in (0, 1):
            for name, plies in pf.bounce_eval_expected(key, cap)[2].items():
                total[c.grid.shape[1] > 8][name] += plies
        counts = [len(a) for a in bp.root_actions(c.grid, c.roots)]
        arms |= set(counts)
        assert c.budgets == (pf.bh.min_budget(max(counts + [1])), 4 * max(counts + [1])), pf.describe(c)
    for wide, seen in total.items():
        assert all(seen[name] > 0 for name in bp.CLASSES), f"more than 8 columns {wide}: {seen}"
    assert 1 in arms and max(arms) >= 3, arms


def test_every_key_has_running_roots_and_few_ended_ones():
    for c in [pf.connect_key(key) for key in pf.connect_keys()]:
        for roots in (c.roots, c.halving_roots, c.search_roots, pf.connect_search_roots(c, "decisive")):
            ended = int((roots[2] != -1).sum())
            assert 0 < roots[0].shape[0] - ended and 2 * ended <= roots[0].shape[0], pf.describe(c)
    for c in [pf.bounce_key(key) for key in pf.bounce_keys()]:
        ended = int((c.roots[2] != -1).sum())
        assert 0 < c.roots[0].shape[0] - ended and 2 * ended <= c.roots[0].shape[0], pf.describe(c)


def flat(case):
    out = []
    for field in case:
        if isinstance(field, tuple) and field and isinstance(field[-1], tuple):     # wide: (budget, roots)
            field = (field[0],) + field[1]
        for a in field if isinstance(field, tuple) else (field,):
            out.append(np.asarray(a))
    return out


def test_the_table_is_deterministic():
    for build, keys in ((pf.connect_key, pf.connect_keys()), (pf.bounce_key, pf.bounce_keys())):
        for key in keys:
            a, b = flat(build.__wrapped__(key)), flat(build.__wrapped__(key))
            assert len(a) == len(b)
            for x, y in zip(a, b):
                assert x.dtype == y.dtype and x.shape == y.shape and (x == y).all(), key


def test_the_draws_of_fuzz_cases_are_untouched():
    """this table draws from bases of its own: the first cases of tests/fuzz_cases.py are what they were"""
    assert [(c.h, c.w, c.k, c.roots[0].shape[0]) for c in (fc.connect_case(key) for key in range(3))] == [
        (9, 8, 2, 42), (2, 9, 6, 38), (4, 4, 3, 42)]
    assert [fc.bounce_case(key).grid.shape for key in range(3)] == [(5, 8), (5, 12), (6, 6)]
    bases = (fc.CONNECT_BASE, fc.BOUNCE_BASE, fc.CONNECT_BASE + 500_000, fc.BOUNCE_BASE + 500_000)
    assert all(abs(mine - base) >= 1000 for mine in (pf.CONNECT_BASE, pf.BOUNCE_BASE) for base in bases)
