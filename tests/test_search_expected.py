"""What tests/search_expected.py -- the CPU statement of bgs_connect_search_actions and the case table of
tests/test_gpu_search.py -- holds: the arithmetic of the contract, the invariants of every tree it grows, and that the
table as a whole reaches the branches the GPU comparison is there for.  No GPU."""

import numpy as np
import pytest

from tests import search_expected as se
from tests.policy_expected import completes


def test_lg_is_the_piecewise_linear_log2():
    for e in range(31):
        assert se.lg(1 << e) == 256 * e
    last = -1
    for total in range(1, (1 << 16) + 1):
        e = total.bit_length() - 1
        got = se.lg(total)
        assert got == 256 * e + ((total * 256) >> e) - 256
        assert got >= last
        last = got
    top = 2**31 - 1
    assert se.lg(top) == 256 * 30 + ((top * 256) >> 30) - 256 == 256 * 31 - 1
    assert se.lg(top) >= se.lg(top - 1) >= se.lg(1 << 30)


def test_the_terms_fit_32_bits_at_the_ceilings():
    top = 2**31 - 1
    assert se.MAX_EXPLORE * se.lg(top) < 2**32
    assert se.e_term(se.MAX_EXPLORE, top, 1) == se.isqrt(se.MAX_EXPLORE * se.lg(top)) < 2**16
    assert se.q_term(2 * se.MAX_PLAYOUTS, se.MAX_PLAYOUTS) == 4096 and 2 * se.MAX_PLAYOUTS < 2**31
    assert ((4096 + 2**16) << 4) + 16 < 2**32           # U with a column packed under it
    for x in (0, 1, 2, 3, 4, 15, 16, 17, 2**24 - 1, 2**24, 2**32 - 1):
        r = se.isqrt(x)
        assert r * r <= x < (r + 1) * (r + 1)


def _walk(root):
    """(node, playouts through the edge into it or None for the root) of every node of a tree"""
    stack = [(root, None)]
    while stack:
        node, came = stack.pop()
        yield node, came
        for c, child in enumerate(node.child):
            if child is not None:
                stack.append((child, node.n[c]))


@pytest.mark.parametrize("run", se.RUNS, ids=se.run_id)
def test_every_tree_keeps_the_books(run):
    index, policy, per_ply = run
    case = se.CASES[index]
    T, P = case.iterations, case.playouts
    roots = se.case_roots(case)
    trees = se.case_trees(index, per_ply, policy)[0]
    counts, visits, best, nodes, steps, seen = se.case_expected(index, per_ply, policy)
    running = roots[2] == -1
    assert roots[0].shape[0] <= 24 and T * P <= 1024
    assert (visits[running].sum(axis=1) == T * P).all()
    assert (visits % P == 0).all() and (nodes <= T).all()
    assert (counts[~running] == 0).all() and (visits[~running] == 0).all() and (best[~running] == -1).all() and (nodes[~running] == 0).all()
    # every playout through a root column is a win, a draw, a loss or was capped: exactly
    capped = seen["capped"]
    assert (counts >= 0).all() and (capped >= 0).all()
    np.testing.assert_array_equal(counts.sum(axis=2), visits - capped)
    if case.cap is None:
        assert (capped == 0).all()
    else:
        assert capped.sum() >= seen["capped_leaves"] * P > 0 and counts.sum() > 0
    for i, root in enumerate(trees):
        if root is None:
            continue
        legal = root.legal
        assert best[i] in legal and visits[i, best[i]] == visits[i].max()
        assert all(visits[i, c] == 0 for c in range(case.w) if c not in legal)
        if T <= len(legal):                              # expansion only: the first T legal columns, P visits each
            assert [c for c in range(case.w) if visits[i, c]] == legal[:T] and set(visits[i, legal[:T]]) == {P}
        for node, came in _walk(root):
            assert all(node.n[c] == 0 and node.s[c] == 0 for c in range(case.w) if c not in node.legal)
            assert all(0 <= node.s[c] <= 2 * node.n[c] for c in node.legal)
            if came is not None:
                assert sum(node.n) == came - P           # every visit of the edge but the one that made the node
    assert steps > 0 and seen["max_depth"] >= 1


def test_capped_playouts_are_those_the_cap_cut():
    """the capped case under both policies: some leaves are capped at once (P playouts each), some games are cut in
    mid-play, and the rest finish; test_every_tree_keeps_the_books holds counts to visits - capped exactly"""
    index = next(j for j, case in enumerate(se.CASES) if case.cap is not None)
    P = se.CASES[index].playouts
    for policy in ("uniform", "decisive"):
        assert (index, policy, False) in se.RUNS
        counts, visits, *_, seen = se.case_expected(index, False, policy)
        at_once = seen["capped_leaves"] * P
        assert at_once >= P
        assert seen["capped"].sum() > at_once                   # games cut in mid-play as well
        assert counts.sum() > 0 and (seen["capped"] <= visits).all()


def test_pure_exploitation_never_leaves_the_best_mean():
    """explore = 0: every UCB selection the search made, at the moment it made it, took the lowest column among those with
    the largest Q (the model records Q of the legal columns at each selection)"""
    index = next(j for j, case in enumerate(se.CASES) if case.explore == 0)
    seen = se.case_trees(index)[3]
    assert len(seen["greedy"]) == seen["selections"] >= 100
    left = 0
    for q, legal, taken in seen["greedy"]:
        assert taken == legal[q.index(max(q))]
        left += int(q.count(max(q)) > 1)
    assert left >= 1                                            # ties among the best means occurred and went to the lowest column
    assert se.e_term(0, 2**31 - 1, 1) == 0
    # ... and a search that explores records nothing there
    assert se.case_trees(0)[3]["greedy"] == []


def test_the_table_reaches_every_branch():
    total = dict.fromkeys(("selections", "tied_selections", "terminal_leaves", "capped_leaves", "max_depth", "best_ties"), 0)
    one_column = ended = False
    for index, policy, per_ply in se.RUNS:
        seen = se.case_expected(index, per_ply, policy)[5]
        for key in total:
            total[key] = max(total[key], seen[key]) if key == "max_depth" else total[key] + seen[key]
        trees = se.case_trees(index, per_ply, policy)[0]
        one_column |= any(t is not None and len(t.legal) == 1 for t in trees)
        ended |= any(t is None for t in trees)
    print(total)
    assert total["selections"] >= 1 and total["tied_selections"] >= 1 and total["terminal_leaves"] >= 1
    assert total["capped_leaves"] >= 1 and total["max_depth"] >= 3
    assert one_column and ended
    assert {se.CASES[j].playouts for j, _, _ in se.RUNS} >= {1, 70}
    assert {(se.CASES[j].w * (se.CASES[j].h + 1) + 63) // 64 for j, _, _ in se.RUNS} == {1, 2, 3}


def test_a_win_in_one_is_the_best_column():
    """case 1 (48 x 16): on a root with a winning column the search's best column wins at once"""
    case = se.CASES[0]
    roots = se.case_roots(case)
    wins = completes(roots[0], roots[1].astype(np.int64), case.k) & (roots[2] == -1)[:, None]
    best = se.case_expected(0)[2]
    rows = np.flatnonzero(wins.any(axis=1))
    assert rows.size >= 1
    for i in rows:
        assert wins[i, best[i]], (i, best[i], wins[i])


def test_two_shards_equal_the_whole():
    case = se.CASES[4]
    roots = se.case_roots(case)
    cut = roots[0].shape[0] // 2
    tail = (case.iterations, case.playouts, case.explore, se.UNCAPPED, False, "decisive")
    whole = se.search_expected(case.h, case.w, case.k, roots, se.SEED, 100, *tail)
    lo = se.search_expected(case.h, case.w, case.k, tuple(a[:cut] for a in roots), se.SEED, 100, *tail)
    hi = se.search_expected(case.h, case.w, case.k, tuple(a[cut:] for a in roots), se.SEED, 100 + cut, *tail)
    for x, y, z in zip(lo[:4], hi[:4], whole[:4]):
        np.testing.assert_array_equal(np.concatenate([x, y]), z)
    assert lo[4] + hi[4] == whole[4]
