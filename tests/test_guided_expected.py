"""CPU-only checks of tests/guided_expected.py, the CPU statement of bgs_connect_guided_step: the invariants of the
trees it grows over the corner boards of tests/fuzz_cases.py under `fake_network`, a hand-worked example with its numbers
written out, and the sense of the selection rule -- an immediately winning column collects the visits."""

import functools

import numpy as np
import pytest

from tests import fuzz_cases as fc
from tests import guided_expected as ge

SIMULATIONS = 48
CORNERS = list(fc.CONNECT_CORNERS)


@functools.lru_cache(maxsize=None)
def corner_run(key, capacity, cpuct=320):
    """(the Guided, every call's outputs) of SIMULATIONS simulations over the corner's roots under fake_network"""
    case = fc.connect_case(key)
    guided = ge.Guided(case.h, case.w, case.k, case.roots[0].shape[0], capacity, cpuct)
    return guided, guided.run(case.roots, ge.fake_network, SIMULATIONS)


def test_the_statement_speaks_the_header_constants():
    import os
    import re

    from tests.conftest import PKG

    with open(os.path.join(os.path.dirname(PKG), "include", "bgs.h")) as f:
        text = f.read()
    defined = {name: eval(value.rstrip("u"), {}) for name, value in
               re.findall(r"^#define BGS_GUIDED_(\w+)\s+(\(?[\d <]+\)?u?)\s", text, flags=re.M)}
    assert defined == {"RESTART": ge.RESTART, "FINISH": ge.FINISH, "EVALUATE": ge.EVALUATE, "TERMINAL": ge.TERMINAL, "IDLE": ge.IDLE,
                       "MAX_CAPACITY": ge.MAX_CAPACITY, "MAX_VISITS": ge.MAX_VISITS}


def walk(root):
    if root is not None:
        yield root
        for child in root.child:
            yield from walk(child)


@pytest.mark.parametrize("key", CORNERS)
def test_the_invariants_of_a_run(key):
    case = fc.connect_case(key)
    guided, calls = corner_run(key, SIMULATIONS + 1)
    running = case.roots[2] == -1
    assert len(calls) == SIMULATIONS + 1
    assert (calls[0][2][running] == ge.EVALUATE).all() and (calls[0][2][~running] == ge.IDLE).all()
    assert (calls[-1][2] == ge.IDLE).all()
    for i, root in enumerate(guided.root):
        if not running[i]:
            assert root is None and calls[-1][5][i] == -1 and not calls[-1][3][i].any()
            continue
        # the first evaluation is the root's: every later one went down an edge of the root
        assert sum(root.n) == guided.applied[i] == SIMULATIONS - 1
        assert guided.count[i] == 1 + ge.count_nodes(root) <= SIMULATIONS + 1
        for node in walk(root):
            assert all(0 <= node.s[c] <= 2048 * node.n[c] for c in range(case.w))
            assert all(node.n[c] == 0 and node.P[c] == 0 for c in range(case.w) if c not in node.legal)
            assert 65536 - case.w < sum(node.P) <= 65536
            for c, child in enumerate(node.child):
                if child is not None:                   # a child's visits are the edge's, but for the one that made it
                    assert sum(child.n) == node.n[c] - 1
    assert len(guided.made) == sum(c - 1 for c in guided.count if c)


def test_every_special_row_was_fed():
    for key in CORNERS:
        corner_run(key, SIMULATIONS + 1)
    assert all(ge.SEEN[name] > 0 for name in ge.SPECIALS), ge.SEEN


def test_the_quantisation():
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    row = np.array([0.5, nan, -1.0, inf, 0.0, 2.0 ** -16, 2.0 ** -17, 0.75], dtype=np.float32)
    assert ge.prior_weights(row, list(range(8))) == {0: 32768, 1: 0, 2: 0, 3: 65536, 4: 0, 5: 1, 6: 0, 7: 49152}
    shares = ge.prior_shares(row, [0, 3, 7], 8)         # W = 147456
    assert shares == [14563, 0, 0, 29127, 0, 0, 0, 21845] and 65536 - 8 < sum(shares) <= 65536
    # an all-zero row, and a row with weight on illegal columns only: equal P over the legal columns
    assert ge.prior_shares(np.zeros(8, dtype=np.float32), [1, 2, 5], 8) == [0, 21845, 21845, 0, 0, 21845, 0, 0]
    assert ge.prior_shares(row, [1, 2, 4, 6], 8) == [0, 16384, 16384, 0, 16384, 0, 16384, 0]
    for x, sigma in ((0.0, 1024), (1.0, 2048), (-1.0, 0), (1.5, 2048), (-3.0, 0), (nan, 1024), (inf, 2048), (0.5, 1536),
                     (-0.00048828125, 1024), (-0.0009765625, 1023), (0.00146484375, 1025), (-0.99951171875, 1)):
        assert ge.value_sigma(np.float32(x)) == sigma, x


@pytest.mark.parametrize("capacity", (2, 3))
def test_a_small_tree_never_exceeds_its_capacity(capacity):
    for key in ("6x7x7", "2x7x4", "1x16x2"):
        case = fc.connect_case(key)
        guided, calls = corner_run(key, capacity)
        assert guided.refused > 0
        for i, root in enumerate(guided.root):
            if root is not None:
                assert 1 + ge.count_nodes(root) == guided.count[i] <= capacity
                assert sum(root.n) == SIMULATIONS - 1             # an edge whose node did not fit is evaluated all the same
        assert max(int(call[6].max()) for call in calls) == capacity - 1


def test_a_hand_worked_example():
    """1 x 3 board, k = 2, cpuct = 256 (c_puct = 1), priors (1/2, 1/4, 1/4) for every leaf and a value a leaf."""
    roots = (np.full((1, 1, 3), -1, dtype=np.int8), np.zeros(1, dtype=np.int8), np.full(1, -1, dtype=np.int8), np.zeros(1, dtype=np.int32))
    value_of = {(-1, -1, -1): 0.0, (0, -1, -1): 0.5, (-1, 0, -1): -1.0, (1, 0, -1): 0.25}

    def evaluate(grid, player):
        return np.array([[0.5, 0.25, 0.25]], dtype=np.float32), np.array([value_of[tuple(grid[0, 0])]], dtype=np.float32)

    guided = ge.Guided(1, 3, 2, 1, 8, 256)
    calls = guided.run(roots, evaluate, 4)

    def row(call):
        return [x[0].tolist() for x in call]

    # begin: the unexpanded root is the leaf
    assert row(calls[0]) == [[[-1, -1, -1]], 0, ge.EVALUATE, [0, 0, 0], [0, 0, 0], -1, 0]
    # step 1: the root gets P = (32768, 16384, 16384) and nothing else.  N = 0: isqrt(1 << 12) = 64, E = (256 * P * 64) >> 19
    # = P / 32 = (1024, 512, 512), Q = 2048 everywhere: column 0.  One stone does not win and the edge has no child.
    assert row(calls[1]) == [[[0, -1, -1]], 1, ge.EVALUATE, [0, 0, 0], [0, 0, 0], -1, 0]
    assert guided.root[0].P == [32768, 16384, 16384]
    # step 2: the leaf's value 0.5 is sigma = 1536 for player 1, so 2048 - 1536 = 512 for the root's mover; columns 1 and 2 of
    # the new node get P = 32768 each.  N = 1: isqrt(2 << 12) = 90.  U(0) = 2 * 512 / 1 + ((2^23 * 90) >> 19) / 2 = 1024 + 720,
    # U(1) = U(2) = 2048 + ((2^22 * 90) >> 19) / 1 = 2048 + 720: column 1, the lower of the two
    assert row(calls[2]) == [[[-1, 0, -1]], 1, ge.EVALUATE, [1, 0, 0], [512, 0, 0], 0, 1]
    assert guided.root[0].child[0].P == [0, 32768, 32768]
    # step 3: value -1 is sigma = 0 for player 1, 2048 for the root's mover.  best: one visit each, the larger s: column 1.
    # N = 2: isqrt(3 << 12) = 110.  U = (1024 + 1760 / 2, 4096 + 880 / 2, 2048 + 880 / 1) = (1904, 4536, 2928): column 1 and
    # down.  The child has P = floor((32768, -, 16384) * 65536 / 49152) = (43690, 0, 21845) and N = 0: U = 2048 + (1365, -,
    # 682): column 0, player 1's stone beside player 0's: no win, two stones of three, no child
    assert row(calls[3]) == [[[1, 0, -1]], 0, ge.EVALUATE, [1, 1, 0], [512, 2048, 0], 1, 2]
    assert guided.root[0].child[1].P == [43690, 0, 21845]
    # finish: value 0.25 is sigma = 1280 for player 0: the root's edge 1 gets 1280, the child's edge 0 gets 768
    assert row(calls[4]) == [[[-1, -1, -1]], 0, ge.IDLE, [1, 2, 0], [512, 3328, 0], 1, 3]
    child = guided.root[0].child[1]
    assert (child.n, child.s) == ([1, 0, 0], [768, 0, 0]) and child.child[0].P == [0, 0, 65536]


def winning_columns(case, i):
    """the columns that win board i of the case's roots at once"""
    position = (case.roots[0][i], int(case.roots[1][i]), int(case.roots[3][i]))
    legal = ge._legal(case.h, case.w, case.k, position)
    return [c for c in range(case.w) if legal[c] and ge._step(case.h, case.w, case.k, position, c)[0] == int(case.roots[1][i])]


def test_an_immediate_win_collects_the_visits():
    """the constant evaluator (uniform priors, value 0), cpuct = 256, 64 simulations: a root with an immediately winning
    column ends with `best` on such a column"""
    roots_with_a_win = 0
    for key in CORNERS:
        case = fc.connect_case(key)
        n = case.roots[0].shape[0]
        guided = ge.Guided(case.h, case.w, case.k, n, 65, 256)
        best = guided.run(case.roots, ge.constant_network, 64)[-1][5]
        for i in np.flatnonzero(case.roots[2] == -1):
            wins = winning_columns(case, i)
            if wins:
                roots_with_a_win += 1
                assert best[i] in wins, (key, i, wins, best[i], guided.root[i].n, guided.root[i].s)
    assert roots_with_a_win >= 16
