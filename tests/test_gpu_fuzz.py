"""Differential fuzzing of the HIP path against the CPU oracle: random geometries, random start grids, random mixes of
sampled plies, caller-chosen moves, loads and rollouts; and the evaluation and solver launches (evaluate_actions,
evaluate_moves, solve_actions, solve_moves) over the random and hand-picked cases of tests/fuzz_cases.py against the
oracle's expected counts and the retrograde references.  Seeds are fixed; everything is bit-exact or it fails."""

import numpy as np
import pytest

from tests import fuzz_cases as fc
from tests import game_trees as gt
from tests import solve_reference as ref
from tests.fuzz_cases import EXTRA, random_bounce_grid, random_connect_geometries, random_piece_list_grid
from tests.knobs import knobs

from oracle import oracle

pytestmark = pytest.mark.gpu

SEED = 0x0123456789ABCDEF
# BGS_FUZZ_CASES=N widens the sweeps (default: 24 Connect + 32 Bounce + 24 piece-list cases of steps and rollouts; 24
# Connect + 16 Bounce cases, and the corner tables, of every evaluation and solver launch)
SOLVE_NODES = 1 << 22    # the depths of fuzz_cases keep every search far below it: no BUDGET code may appear


def same(dev, orc, what):
    np.testing.assert_array_equal(dev.grid, orc.grid, err_msg=f"grid {what}")
    np.testing.assert_array_equal(dev.winner, orc.winner, err_msg=f"winner {what}")
    np.testing.assert_array_equal(dev.plies, orc.plies, err_msg=f"plies {what}")
    np.testing.assert_array_equal(dev.reward, orc.reward, err_msg=f"reward {what}")


@pytest.mark.parametrize("case", range(max(24, EXTRA)))
def test_connect_random_geometry(case):
    from simulator.batch import ConnectBatch

    rng = np.random.default_rng(1000 + case)
    (h, w, k), = random_connect_geometries(rng, 1)
    n = int(rng.integers(1, 3000))
    first = int(rng.integers(0, 1 << 40))
    seed = SEED ^ case
    dev = ConnectBatch(h, w, k, n)
    orc = oracle.ConnectOracle(h, w, k, n)
    dev.set_first_game(first)
    what = f"connect {h}x{w}x{k} n={n}"
    # a few sampled plies, a few caller-chosen ones (some illegal), then a capped and a full rollout
    for _ in range(int(rng.integers(0, 4))):
        dev.step_random(seed)
        orc.step_random(seed, first_game=first)
    for _ in range(int(rng.integers(0, 4))):
        cols = rng.integers(-1, w + 1, size=n).astype(np.int32)
        np.testing.assert_array_equal(dev.step_actions(cols), orc.step_actions(cols), err_msg=what)
    same(dev, orc, what + " after steps")
    np.testing.assert_array_equal(dev.legal, orc.legal(), err_msg=what)
    cap = int(rng.integers(0, h * w + 2))
    dev.rollout(seed, max_plies=cap)
    orc.rollout(seed, first_game=first, max_plies=cap)
    same(dev, orc, what + f" capped at {cap}")
    dev.rollout(seed)
    orc.rollout(seed, first_game=first)
    same(dev, orc, what + " finished")
    assert dev.has_ended.all()
    # from the initial state, with a fresh seed, into the same handle
    dev.rollout(seed + 1, from_initial=True)
    orc.reset()
    orc.rollout(seed + 1, first_game=first)
    same(dev, orc, what + " from initial")
    # reload the final boards and check that the device derives the same verdicts from the grids alone
    again = ConnectBatch(h, w, k, n)
    assert (again.write_state(orc.grid) == 0).all()
    same(again, orc, what + " reloaded")


@pytest.mark.parametrize("case", range(max(32, EXTRA)))
def test_bounce_random_grid(case):
    from simulator.batch import BounceBatch

    rng = np.random.default_rng(5000 + case)
    grid = random_bounce_grid(rng)
    n = int(rng.integers(1, 600))
    first = int(rng.integers(0, 1 << 40))
    seed = SEED ^ (case << 8)
    dev = BounceBatch(grid, n)
    orc = oracle.BounceOracle(grid, n)
    dev.set_first_game(first)
    what = f"bounce {grid.shape} case {case}"
    same(dev, orc, what + " after reset")
    np.testing.assert_array_equal(dev.action_count, orc.count_actions(), err_msg=what)
    for ply in range(int(rng.integers(0, 6))):
        dev.step_random(seed)
        orc.step_random(seed, first_game=first)
        same(dev, orc, what + f" step {ply}")
    np.testing.assert_array_equal(dev.action_count, orc.count_actions(), err_msg=what)
    # exhaustive target sets of a few boards
    masks = dev.targets
    width = dev.width
    for i in range(0, n, max(1, n // 7)):
        got = []
        row = int(masks[i, width])
        for x in range(width):
            m = int(masks[i, x])
            got += [((x, row), (c % width, c // width)) for c in range(64) if (m >> c) & 1]
        assert got == orc.actions(i), f"{what} board {i}"
    # caller-chosen moves: the oracle's own legal moves, some garbage, some skips
    moves = np.full((n, 4), -1, dtype=np.int32)
    for i in range(n):
        acts = orc.actions(i)
        r = rng.random()
        if acts and r < 0.6:
            (sx, sy), (tx, ty) = acts[rng.integers(len(acts))]
            moves[i] = [sx, sy, tx, ty]
        elif r < 0.8:
            moves[i] = rng.integers(0, 12, size=4)
    np.testing.assert_array_equal(dev.step_actions(moves), orc.step_actions(moves), err_msg=what)
    same(dev, orc, what + " after chosen moves")
    cap = int(rng.integers(0, 40))
    dev.rollout(seed, max_plies=cap)
    orc.rollout(seed, first_game=first, max_plies=cap)
    same(dev, orc, what + f" capped at {cap}")
    dev.rollout(seed, max_plies=600)
    orc.rollout(seed, first_game=first, max_plies=600)
    same(dev, orc, what + " rolled out")
    dev.rollout(seed + 3, max_plies=600, from_initial=True)
    orc.reset()
    orc.rollout(seed + 3, first_game=first, max_plies=600)
    same(dev, orc, what + " from initial")
    again = BounceBatch(grid, n)
    assert (again.write_state(orc.grid, orc.player, orc.winner, orc.plies) == 0).all()
    same(again, orc, what + " reloaded")


@pytest.mark.parametrize("case", range(max(24, EXTRA)))
def test_bounce_piece_list_random_grid(case):
    """K3p (one lane per board on the piece list; the 8-, 12- and 16-piece instantiations, the bulk + tail plan for caps
    beyond 768 plies, parked boards) against the oracle on random start grids, batch sizes around the wave / workgroup
    boundaries, random first-game offsets."""
    from simulator.batch import BounceBatch

    rng = np.random.default_rng(9000 + case)
    grid = random_piece_list_grid(rng)
    n = int(rng.choice([1, 63, 64, 65, 255, 257, 1000, 2500, 6000]))
    first = int(rng.integers(0, 1 << 40))
    cap = int(rng.choice([0, 1, 7, 60, 500, 769, 2000]))
    old = knobs.get("bounce_group")
    knobs["bounce_group"] = "1"
    try:
        dev = BounceBatch(grid, n)
        orc = oracle.BounceOracle(grid, n)
        dev.set_first_game(first)
        what = f"piece-list bounce {grid.shape} {int((grid > 0).sum())} pieces n={n} cap={cap} case {case}"
        dev.rollout(SEED ^ case, max_plies=cap, from_initial=True)
        total = orc.rollout(SEED ^ case, first_game=first, max_plies=cap)
        same(dev, orc, what)
        assert dev.steps == total, what
        dev.close()
    finally:
        if old is None:
            del knobs["bounce_group"]
        else:
            knobs["bounce_group"] = old


# ---- the evaluation and solver launches over the case table of tests/fuzz_cases.py
def snapshot(b):
    return b.grid.tobytes(), b.player.tobytes(), b.winner.tobytes(), b.plies.tobytes()


def load_connect(case, roots, evaluate=False):
    from simulator.batch import ConnectBatch

    b = ConnectBatch(case.h, case.w, case.k, roots[0].shape[0])
    assert (b.write_state(*roots) == 0).all(), fc.describe(case)
    if evaluate:
        if case.per_ply:
            b.set_rng_contract("per-ply")
        b.set_first_game(case.first_game)
    b.reset_steps()
    return b


def load_bounce(case, roots):
    from simulator.batch import BounceBatch

    b = BounceBatch(case.grid, roots[0].shape[0])
    assert (b.write_state(*roots) == 0).all(), fc.describe(case)
    b.set_first_game(case.first_game)
    b.reset_steps()
    return b


def assert_rows_equal(got, want, rows, what, names):
    """got, want: tuples of arrays [n, ...]; names the first differing root (its row in the case's roots) and entries"""
    n = got[0].shape[0]
    bad = np.zeros(n, dtype=bool)
    for g, w in zip(got, want):
        assert g.shape == w.shape, (what, g.shape, w.shape)
        bad |= (g != w).reshape(n, -1).any(axis=1)
    if bad.any():
        i = int(np.flatnonzero(bad)[0])
        at = np.argwhere(np.logical_or.reduce([g[i] != w[i] for g, w in zip(got, want)]))[:6]
        detail = [(tuple(int(v) for v in a),) + tuple(x for g, w in zip(got, want) for x in (g[i][tuple(a)].tolist(), w[i][tuple(a)].tolist()))
                  for a in at]
        raise AssertionError(f"{what}: {int(bad.sum())} of {n} roots differ, first root {int(rows[i])} of the case "
                             f"(entry, {', '.join(f'{m}, want' for m in names)}) {detail}")


@pytest.mark.parametrize("key", fc.connect_keys(), ids=str)
def test_connect_solve_random_geometry(key):
    case = fc.connect_case(key)
    for depth, rows in fc.connect_solves(case):
        roots = fc.take(case.roots, rows)
        what = f"{fc.describe(case)} solve_actions depth {depth}"
        b = load_connect(case, roots)
        before = snapshot(b)
        codes, plies = b.solve_actions(depth=depth, max_nodes=SOLVE_NODES)
        assert not (codes == ref.BUDGET).any(), what
        assert_rows_equal((codes, plies), ref.solve(case.h, case.w, case.k, roots, depth), rows, what, ("code", "plies"))
        assert snapshot(b) == before and b.steps == 0, what
        b.close()


@pytest.mark.parametrize("key", fc.bounce_keys(), ids=str)
def test_bounce_solve_random_grid(key):
    case = fc.bounce_case(key)
    h, w = case.grid.shape
    rows = np.arange(case.roots[0].shape[0])
    legal = np.zeros((rows.size, w, h * w), dtype=bool)
    for i, acts in enumerate(gt.bounce_actions(case.grid, case.roots)):
        for (sx, _), (tx, ty) in acts:
            legal[i, sx, ty * w + tx] = True
    b = load_bounce(case, case.roots)
    before = snapshot(b)
    for depth in fc.bounce_depths(key):
        what = f"{fc.describe(case)} solve_moves depth {depth}"
        codes, plies = b.solve_moves(depth=depth, max_nodes=SOLVE_NODES)
        assert not (codes == ref.BUDGET).any(), what
        assert_rows_equal((codes, plies), fc.bounce_reference(key, depth)[:2], rows, what, ("code", "plies"))
        assert_rows_equal((codes != ref.NONE,), (legal,), rows, what + " legal slots", ("legal",))
        assert snapshot(b) == before and b.steps == 0, what
    b.close()


@pytest.mark.parametrize("key", fc.connect_keys(), ids=str)
def test_connect_evaluate_random_geometry(key):
    case = fc.connect_case(key)
    for j, playouts in enumerate(case.playouts):
        roots, want, steps = fc.connect_eval_expected(case, j)
        what = (f"{fc.describe(case)} evaluate_actions playouts {playouts} max_plies {case.max_plies} per_ply {case.per_ply} "
                f"first_game {case.first_game}")
        b = load_connect(case, roots, evaluate=True)
        before = snapshot(b)
        got = b.evaluate_actions(seed=fc.EVAL_SEED, playouts=playouts, max_plies=case.max_plies)
        assert_rows_equal((got,), (want,), case.eval_rows[j], what, ("count",))
        assert b.steps == steps, what
        assert snapshot(b) == before, what
        b.close()


@pytest.mark.parametrize("key", fc.bounce_keys(), ids=str)
def test_bounce_evaluate_random_grid(key):
    case = fc.bounce_case(key)
    for max_plies in case.max_plies:
        roots, want, steps = fc.bounce_eval_expected(case, max_plies)
        what = f"{fc.describe(case)} evaluate_moves playouts {case.playouts} max_plies {max_plies} first_game {case.first_game}"
        b = load_bounce(case, roots)
        before = snapshot(b)
        got = b.evaluate_moves(seed=fc.EVAL_SEED, playouts=case.playouts, max_plies=max_plies)
        assert_rows_equal((got,), (want,), case.eval_rows, what, ("count",))
        assert b.steps == steps, what
        assert snapshot(b) == before, what
        b.close()


def test_default_board_static_and_run_time_geometry_agree_in_evaluate_and_solve(monkeypatch):
    """the 9x6 default grid through the compile-time geometry (the product's choice) and, under the test-build knob
    bounce_static_geom=0, through the run-time record every other grid takes: the same counts, codes and plies, the
    references' ones.  The knob is read when a batch is created."""
    case = fc.bounce_case("default")
    max_plies = case.max_plies[0]
    roots, want, steps = fc.bounce_eval_expected(case, max_plies)
    results = []
    for static in (True, False):
        if not static:
            monkeypatch.setitem(knobs, "bounce_static_geom", "0")
        else:
            assert "bounce_static_geom" not in knobs
        what = f"{fc.describe(case)} static geometry {static}"
        b = load_bounce(case, roots)            # created after the knob is set
        counts = b.evaluate_moves(seed=fc.EVAL_SEED, playouts=case.playouts, max_plies=max_plies)
        assert_rows_equal((counts,), (want,), case.eval_rows, what + f" evaluate_moves playouts {case.playouts} max_plies {max_plies}", ("count",))
        assert b.steps == steps, what
        b.close()
        b = load_bounce(case, case.roots)
        solved = []
        for depth in fc.bounce_depths("default"):
            codes, plies = b.solve_moves(depth=depth, max_nodes=SOLVE_NODES)
            assert_rows_equal((codes, plies), fc.bounce_reference("default", depth)[:2], np.arange(codes.shape[0]),
                              what + f" solve_moves depth {depth}", ("code", "plies"))
            solved += [codes, plies]
        b.close()
        results.append([counts] + solved)
    for a, c in zip(*results):
        np.testing.assert_array_equal(a, c)
