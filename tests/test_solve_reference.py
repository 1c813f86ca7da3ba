"""The CPU reference of the exact Connect solver (tests/solve_reference.py: retrograde analysis over the oracle's moves)
against an independent memoized negamax written here from the rules, on every reachable position of four small
geometries, at full depth and at depths 1-4.  No GPU."""

import functools

import numpy as np
import pytest

from tests import game_trees as gt
from tests import solve_reference as ref

GEOMS = [(2, 3, 2), (3, 3, 3), (3, 4, 3), (4, 3, 3)]


def _won(cells, h, w, k, y, x, who):
    for dy, dx in ((0, 1), (1, 0), (1, 1), (1, -1)):
        run = 1
        for s in (1, -1):
            yy, xx = y + s * dy, x + s * dx
            while 0 <= yy < h and 0 <= xx < w and cells[yy * w + xx] == who:
                run += 1
                yy, xx = yy + s * dy, xx + s * dx
        if run >= k:
            return True
    return False


def negamax_columns(h, w, k, grid, player, depth):
    """(code, plies) of every column of one running position, by plain recursion over tuples of cells"""

    @functools.lru_cache(maxsize=None)
    def move(cells, who, x, left):
        """value (sign, plies) for `who` of playing column x with `left` plies of horizon (>= 1), or None if illegal"""
        if cells[(h - 1) * w + x] >= 0:   # row 0 is the bottom: a full column
            return None
        y = _landing(cells, x)
        nxt = list(cells)
        nxt[y * w + x] = who
        nxt = tuple(nxt)
        if _won(nxt, h, w, k, y, x, who):
            return (1, 1)
        if all(c >= 0 for c in nxt) or left == 1:
            return (0, 0)
        s, t = node(nxt, 1 - who, left - 1)
        return (-s, t + 1) if s else (0, 0)

    def _landing(cells, x):
        # the reference layout's row 0 is the bottom: a stone falls to the lowest empty row
        return min(y for y in range(h) if cells[y * w + x] < 0)

    @functools.lru_cache(maxsize=None)
    def node(cells, who, left):
        best = None
        for x in range(w):
            v = move(cells, who, x, left)
            if v is None:
                continue
            key = {1: 1000 - v[1], 0: 0, -1: -1000 + v[1]}[v[0]]
            if best is None or key > best[0]:
                best = (key, v)
        return best[1]

    cells = tuple(int(c) for c in np.asarray(grid).ravel())
    empty = sum(c < 0 for c in cells)
    out = []
    for x in range(w):
        v = move(cells, int(player), x, depth)
        if v is None:
            out.append((ref.NONE, 0))
        elif v[0] == 1:
            out.append((ref.WIN, v[1]))
        elif v[0] == -1:
            out.append((ref.LOSS, v[1]))
        elif empty <= depth:
            out.append((ref.DRAW, empty))
        else:
            out.append((ref.UNKNOWN, 0))
    return out


def all_positions(h, w, k):
    layers = [layer for _, layer in gt.connect_layers(h, w, k)]
    return tuple(np.concatenate([l[j] for l in layers]) for j in range(4))


@pytest.mark.parametrize("geom", GEOMS, ids=lambda g: "x".join(map(str, g)))
def test_reference_equals_recursive_negamax(geom):
    h, w, k = geom
    pos = all_positions(h, w, k)
    for depth in (h * w, 1, 2, 3, 4):
        codes, plies = ref.solve(h, w, k, pos, depth)
        for i in range(pos[0].shape[0]):
            if pos[2][i] != -1:
                assert (codes[i] == ref.NONE).all() and (plies[i] == 0).all()
                continue
            want = negamax_columns(h, w, k, pos[0][i], pos[1][i], depth)
            got = list(zip(codes[i].tolist(), plies[i].tolist()))
            assert got == want, (geom, depth, i, pos[0][i], got, want)


def test_reference_known_values():
    """the start of 2x3 connect-2: the first player wins on the second of its stones whatever it plays (3 plies)"""
    pos = all_positions(2, 3, 2)
    codes, plies = ref.solve(2, 3, 2, gt._take(pos, np.array([0])), 6)
    assert codes.tolist() == [[ref.WIN] * 3] and plies.tolist() == [[3] * 3]
