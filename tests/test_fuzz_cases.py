"""What the fuzz case table (tests/fuzz_cases.py) must contain, stated on the CPU references alone -- the oracle,
tests/solve_reference.py, tests/solve_reference_bounce.py, tests/mc_expected.py -- so that it runs anywhere: the GPU
comparison of tests/test_gpu_fuzz.py is only as good as its cases.  These are conditions on the table, not
measurements: where a draw of the table misses one, the recipe or the corner table changes, never the condition.

Cost of the references.  With the naive recipe (48 oracle games a case stepped a random number of plies) 24 Connect
cases at depths 1-4 took 3.9 s (worst: 3x13x4, 1.6 s) and 16 Bounce cases at depths 1-3 took 6.1 s (worst: a 9x6 grid
with 26 pieces, 10 612 positions, 3.6 s).  The table as it stands -- 24 + 16 Connect cases of up to 42 roots (18 on
16 columns) at depths 1-4, 5 and the full solve on the late roots; 16 + 6 Bounce cases of up to 20 roots at depths 1-3,
and 4 on the small trees -- takes 10.9 s for the Connect references (worst: 11x16x5, 2.1 s), 8.2 s for the Bounce ones
(worst: a 9x7 grid with 20 pieces, 9 884 positions at depth 3, 3.3 s), 1 s for the oracle's expected counts and 3.2 s
for building the table twice, on the same host; the whole module runs in 25 s.
"""

import numpy as np
import pytest

from tests import fuzz_cases as fc
from tests import game_trees as gt
from tests import solve_reference as ref
from tests import solve_reference_bounce as refb

# the cases that cannot have a running root next to their ended ones.  None today: every Connect start position runs
# (the k = 1 boards keep it as their only running root, and the recipe never keeps more ended roots than running ones),
# and a random Bounce grid whose start position is settled at reset is drawn again.
NO_RUNNING_ROOT = ()


@pytest.fixture(scope="module")
def connect_answers():
    """key -> [(depth, rows, codes, plies)] from the reference"""
    out = {}
    for key in fc.connect_keys():
        c = fc.connect_case(key)
        out[key] = [(d, rows) + ref.solve(c.h, c.w, c.k, fc.take(c.roots, rows), d) for d, rows in fc.connect_solves(c)]
    return out


@pytest.fixture(scope="module")
def bounce_answers():
    """key -> [(depth, codes, plies)] from the reference"""
    return {key: [(d,) + fc.bounce_reference(key, d)[:2] for d in fc.bounce_depths(key)] for key in fc.bounce_keys()}


def decided(codes):
    return (codes == ref.WIN) | (codes == ref.LOSS)


def test_connect_solver_cells(connect_answers):
    """each of (NW in 1, 2, 3) x (k == 4, k != 4): a case whose answer holds WIN and LOSS with some plies >= 3, and a case
    that holds DRAW"""
    deep, drawn = set(), set()
    for key, answers in connect_answers.items():
        c = fc.connect_case(key)
        cell = (c.nw, c.k == 4)
        codes = np.concatenate([a[2].ravel() for a in answers])
        plies = np.concatenate([a[3].ravel() for a in answers])
        if (codes == ref.WIN).any() and (codes == ref.LOSS).any() and (plies[decided(codes)] >= 3).any():
            deep.add(cell)
        if (codes == ref.DRAW).any():
            drawn.add(cell)
    cells = {(nw, four) for nw in (1, 2, 3) for four in (True, False)}
    assert deep == cells, f"no WIN + LOSS with plies >= 3 in (NW, k == 4) = {sorted(cells - deep)}"
    assert drawn == cells, f"no DRAW in (NW, k == 4) = {sorted(cells - drawn)}"


def test_connect_values_and_sides():
    """every k from 1 to 7, w in {1, 2, 16}, h in {1, 15} and a board of exactly 192 bits, each with a running root"""
    ks, ws, hs, bits = set(), set(), set(), set()
    for key in fc.connect_keys():
        c = fc.connect_case(key)
        assert 1 <= c.h <= 15 and 1 <= c.w <= 16 and c.w * (c.h + 1) <= 192 and 1 <= c.k <= 7, fc.describe(c)
        if (c.roots[2] == -1).any():
            ks.add(c.k)
            ws.add(c.w)
            hs.add(c.h)
            bits.add(c.w * (c.h + 1))
    assert set(range(1, 8)) <= ks, ks
    assert {1, 2, 16} <= ws, ws
    assert {1, 15} <= hs, hs
    assert 192 in bits, bits


def test_bounce_solver_classes(bounce_answers):
    """grids of at most 8 and of more than 8 columns: a case with WIN, LOSS and UNKNOWN and plies 1, 2 and 3; a legal move
    whose target is cell 63; a DRAW at ply 1"""
    full = set()
    last_cell = draw_at_one = False
    for key, answers in bounce_answers.items():
        c = fc.bounce_case(key)
        h, w = c.grid.shape
        assert h * w <= 64 and c.grid.max() <= 15 and not c.grid[0].any() and not c.grid[-1].any(), fc.describe(c)
        codes = np.concatenate([a[1].ravel() for a in answers])
        plies = np.concatenate([a[2].ravel() for a in answers])
        if {ref.WIN, ref.LOSS, ref.UNKNOWN} <= set(np.unique(codes).tolist()) and {1, 2, 3} <= set(np.unique(plies[decided(codes)]).tolist()):
            full.add(w > 8)
        draw_at_one |= bool(((codes == ref.DRAW) & (plies == 1)).any())
        last_cell |= any(ty * w + tx == 63 for acts in gt.bounce_actions(c.grid, c.roots) for _, (tx, ty) in acts)
    assert full == {False, True}, f"WIN, LOSS, UNKNOWN with plies 1, 2, 3 only for (w > 8) in {full}"
    assert last_cell, "no legal move into cell 63"
    assert draw_at_one, "no DRAW at ply 1"
    assert refb.DRAW == ref.DRAW


def test_connect_evaluation_totals():
    """every NW: a case whose expected counts hold wins, draws and losses"""
    have = set()
    for key in fc.connect_keys():
        c = fc.connect_case(key)
        for j, p in enumerate(c.playouts):
            roots = c.eval_rows[j].size
            assert roots * c.w * p <= fc.EVAL_BOARDS or roots == 1, fc.describe(c)
            if c.nw not in have and (fc.connect_eval_expected(c, j)[1].sum(axis=(0, 1)) > 0).all():
                have.add(c.nw)
    assert have == {1, 2, 3}, have


def test_bounce_evaluation_totals():
    """NC = 1 (at most 8 columns) and NC = 3: a case whose expected counts hold wins, draws and losses"""
    have = set()
    for key in fc.bounce_keys():
        c = fc.bounce_case(key)
        for cap in c.max_plies:
            if c.nc not in have and (fc.bounce_eval_expected(c, cap)[1].sum(axis=(0, 1, 2)) > 0).all():
                have.add(c.nc)
    assert have == {1, 3}, have


def test_every_case_has_running_roots_and_few_ended_ones():
    for case in [fc.connect_case(k) for k in fc.connect_keys()] + [fc.bounce_case(k) for k in fc.bounce_keys()]:
        ended = int((case.roots[2] != -1).sum())
        n = case.roots[0].shape[0]
        assert 2 * ended <= n, fc.describe(case)
        assert n > ended or case.key in NO_RUNNING_ROOT, fc.describe(case)
        unique = gt._unique_rows(case.roots[0]) if isinstance(case, fc.ConnectCase) else gt._unique_rows(case.roots[0], case.roots[1])
        assert unique.size == n, fc.describe(case)
    assert not NO_RUNNING_ROOT or set(NO_RUNNING_ROOT) <= set(fc.CONNECT_CORNERS) | set(fc.BOUNCE_CORNERS)


def flat(case):
    out = []
    for field in case:
        for a in field if isinstance(field, tuple) else (field,):
            out.append(np.asarray(a))
    return out


def test_the_table_is_deterministic():
    for build, keys in ((fc.connect_case, fc.connect_keys()), (fc.bounce_case, fc.bounce_keys())):
        for key in keys:
            a, b = flat(build.__wrapped__(key)), flat(build.__wrapped__(key))
            assert len(a) == len(b)
            for x, y in zip(a, b):
                assert x.dtype == y.dtype and x.shape == y.shape and (x == y).all(), key


def test_the_old_fuzz_draws_are_pinned():
    """the generators moved here from test_gpu_fuzz.py: the first cases of its three sweeps draw what they drew there"""
    assert [fc.random_connect_geometries(np.random.default_rng(1000 + c), 1)[0] for c in range(5)] == [
        (4, 9, 6), (14, 10, 6), (10, 7, 6), (5, 4, 5), (11, 1, 1)]
    assert [(g.shape, int(g.sum())) for g in (fc.random_bounce_grid(np.random.default_rng(5000 + c)) for c in range(5))] == [
        ((7, 1), 6), ((4, 3), 6), ((9, 6), 26), ((5, 5), 3), ((3, 2), 1)]
    assert [(g.shape, int(g.sum())) for g in (fc.random_piece_list_grid(np.random.default_rng(9000 + c)) for c in range(5))] == [
        ((8, 2), 6), ((5, 6), 58), ((7, 8), 25), ((11, 2), 38), ((10, 6), 11)]
