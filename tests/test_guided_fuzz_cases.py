"""CPU-only: what the case table of tests/guided_fuzz_cases.py must hold, so that the fuzz of the guided searches
(tests/test_gpu_guided_fuzz.py) cannot turn vacuous.  The CPU statements run over the whole table once (cached in
guided_fuzz_cases: the GPU tests of the same session share them).  The conditions are on the union of the default keys:
they are conditions, not measurements -- a table that misses one gets other bases, not other conditions."""

import numpy as np

from tests import bounce_guided_expected as bg
from tests import guided_expected as ge
from tests import guided_fuzz_cases as gf
from tests import guided_shares as gs

CONNECT = list(range(gf.CONNECT_CASES))
BOUNCE = list(range(gf.BOUNCE_CASES))


def test_the_table_is_reproducible_and_within_the_header_ranges():
    assert gf.connect_keys()[: gf.CONNECT_CASES] == CONNECT and gf.bounce_keys()[: gf.BOUNCE_CASES] == BOUNCE
    for key in CONNECT:
        case = gf.connect_key(key)
        again = gf.connect_key.__wrapped__(key)
        assert case[1:5] + case[6:8] == again[1:5] + again[6:8]
        for x, y in zip(case.roots + case.roots_after + (case.columns,), again.roots + again.roots_after + (again.columns,)):
            np.testing.assert_array_equal(x, y)
        n = case.roots[0].shape[0]
        assert 1 <= n <= gf.CONNECT_ROOTS and case.capacity in gf.CAPACITIES and case.cpuct in gf.CPUCTS
        assert 1 <= case.h <= 15 and 1 <= case.w <= 16 and 1 <= case.k <= 7 and case.nw == (case.w * (case.h + 1) + 63) // 64
        assert (case.columns >= 0).any() == (key % 2 == 0 and bool(((case.roots[2] == -1) & (np.arange(n) % 2 == 0)).any()))
        moved = case.columns >= 0
        np.testing.assert_array_equal(case.roots_after[3][moved], case.roots[3][moved] + 1)
        np.testing.assert_array_equal(case.roots_after[0][~moved], case.roots[0][~moved])
    for key in BOUNCE:
        case = gf.bounce_key(key)
        again = gf.bounce_key.__wrapped__(key)
        assert case[3:] == again[3:]
        for x, y in zip((case.grid,) + case.roots, (again.grid,) + again.roots):
            np.testing.assert_array_equal(x, y)
        h, w = case.grid.shape
        assert 1 <= case.roots[0].shape[0] <= gf.BOUNCE_ROOTS and case.nodes in gf.NODES and case.cpuct in gf.CPUCTS
        assert case.edges in (bg.min_edges(h, w), bg.default_edges(h, w, case.nodes)) and case.grid.max() <= 15
        assert case.max_plies == 65535 or case.max_plies == gf.fc.bounce_case(key).max_plies[0]


def test_the_connect_keys_are_not_vacuous():
    facts = [gf.connect_expected(key)[0].facts for key in CONNECT]
    assert {gf.connect_key(key).nw for key in CONNECT} == {1, 2, 3}
    assert {gf.connect_key(key).capacity for key in CONNECT} == set(gf.CAPACITIES)
    assert sum(f["refused"] for f in facts) > 0                                # a node that did not fit
    assert sum(f["won"] for f in facts) > 0 and sum(f["full"] for f in facts) > 0   # TERMINAL by a win and by a full board
    assert max(f["max_depth"] for f in facts) >= 3
    for name in ge.SPECIALS:
        assert sum(f["served"][name] for f in facts) > 0, name                 # served to an EVALUATE leaf
    assert sum(f["restarted"] for f in facts) > 0
    assert all(f["running"] > 0 for f in facts)
    for key in CONNECT:                                                        # every run ends idle, with its visits in
        model, calls = gf.connect_expected(key)
        assert len(calls) == gf.SIMULATIONS + 1 and (calls[-1][2] == ge.IDLE).all()
        assert (calls[0][2] == ge.EVALUATE).sum() == model.facts["running"]


def test_the_bounce_keys_are_not_vacuous():
    facts = [gf.bounce_expected(key)[0].facts for key in BOUNCE]
    widths = [gf.bounce_key(key).grid.shape[1] for key in BOUNCE]
    assert min(widths) <= 8 < max(widths)                                      # NC = 1 and NC = 3
    assert sum(f["refused_nodes"] for f in facts) > 0 and sum(f["refused_edges"] for f in facts) > 0
    assert sum(f["goal"] + f["blocked"] for f in facts) > 0                    # TERMINAL by a win ...
    assert sum(f["draw"] for f in facts) > 0 and sum(f["cap"] for f in facts) > 0   # ... by a draw and by the cap
    assert max(f["max_depth"] for f in facts) >= 3
    for name in bg.SPECIALS:
        assert sum(f["served"][name] for f in facts) > 0, name
    assert all(f["running"] > 0 for f in facts)
    for key in BOUNCE:
        _, calls = gf.bounce_expected(key)
        assert len(calls) == gf.SIMULATIONS + 1 and (calls[-1][2] == bg.IDLE).all()


def test_the_trees_of_the_table_reach_depth_three():
    """the whole-tree comparison has inner nodes to look at: edges with visits three levels down, in each game"""
    def deepest(model):
        best = 0
        for i in range(model.n):
            nodes = gs.model_nodes(model, i)
            level = {id(nodes[0]): 1} if nodes else {}
            for node in nodes:
                for a, child in enumerate(node.child):
                    if child is not None:
                        level[id(child)] = level[id(node)] + 1
                if sum(node.n) > 0:
                    best = max(best, level[id(node)])
        return best

    assert max(deepest(gf.connect_expected(key)[0]) for key in CONNECT) >= 3
    assert max(deepest(gf.bounce_expected(key)[0]) for key in BOUNCE) >= 3
