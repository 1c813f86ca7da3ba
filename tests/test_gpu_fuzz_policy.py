"""The launches that play the decisive policy, halve or search -- evaluate_actions / evaluate_moves with
policy="decisive", evaluate_actions_halving / evaluate_moves_halving, search_actions / search_moves, their proving
variants and the forest's restart -- over the corner geometries and random cases of tests/policy_fuzz_cases.py, against
the CPU statements of tests/policy_expected.py, halving_expected.py, search_expected.py, search_prove_expected.py and
their Bounce twins: every output and the bgs_steps delta bit for bit, the boards untouched.
tests/test_policy_fuzz_cases.py states what the table holds; BGS_FUZZ_CASES=N widens the random keys of every sweep here.

The kernels finish in milliseconds at these sizes; the CPU references, cached per key, are the slower side.

Everything here needs a real MI355X: `pytest -m gpu`.
"""

import numpy as np
import pytest

from tests import policy_fuzz_cases as pf
from tests.knobs import knobs
from tests.test_gpu_fuzz import snapshot

pytestmark = pytest.mark.gpu

SEED = pf.SEED


def load_connect(case, roots):
    from simulator.batch import ConnectBatch

    b = ConnectBatch(case.h, case.w, case.k, roots[0].shape[0])
    assert (b.write_state(*roots) == 0).all(), pf.describe(case)
    if case.per_ply:
        b.set_rng_contract("per-ply")
    b.set_first_game(case.first_game)
    b.reset_steps()
    return b


def load_bounce(case):
    from simulator.batch import BounceBatch

    b = BounceBatch(case.grid, case.roots[0].shape[0])
    assert (b.write_state(*case.roots) == 0).all(), pf.describe(case)
    b.set_first_game(case.first_game)
    b.reset_steps()
    return b


def check(b, before, got, want, steps, what, names):
    """every output equal (the first differing root and its entries named), the env-steps the reference's, the boards as
    they were"""
    got, want = tuple(got), tuple(want)
    assert len(got) == len(want) == len(names), what
    n = got[0].shape[0]
    bad = np.zeros(n, dtype=bool)
    for name, g, w in zip(names, got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, w.dtype, g.shape, w.shape)
        bad |= (g != w).reshape(n, -1).any(axis=1)
    if bad.any():
        i = int(np.flatnonzero(bad)[0])
        detail = []
        for name, g, w in zip(names, got, want):
            gi, wi = np.atleast_1d(g[i]), np.atleast_1d(w[i])
            detail += [f"{name}{[int(v) for v in at]}: {gi[tuple(at)].tolist()}, want {wi[tuple(at)].tolist()}" for at in np.argwhere(gi != wi)[:6]]
        raise AssertionError(f"{what}: {int(bad.sum())} of {n} roots differ, first root {i}: " + "; ".join(detail))
    assert b.steps == steps, f"{what}: {b.steps} env-steps, the reference makes {steps}"
    assert snapshot(b) == before, f"{what}: grid, player, winner or plies changed"


def search_kw(case, policy):
    return dict(seed=SEED, iterations=case.iterations, leaf_playouts=case.leaf_playouts, explore=case.explore, max_plies=case.max_plies,
                policy=policy)


# ------------------------------------------------------------------------------------------------ Connect
@pytest.mark.parametrize("key", pf.connect_keys(), ids=str)
def test_connect_decisive_evaluate(key):
    case = pf.connect_key(key)
    want, steps, seen = pf.connect_eval_expected(key)
    what = f"{pf.describe(case)} evaluate_actions decisive playouts {case.playouts}"
    b = load_connect(case, case.roots)
    before = snapshot(b)
    got = b.evaluate_actions(seed=SEED, playouts=case.playouts, max_plies=case.max_plies, policy="decisive")
    print(f"{what}: steps {b.steps} / {steps}, plies {seen}")
    check(b, before, (got,), (want,), steps, what, ("count",))
    b.close()


@pytest.mark.parametrize("policy", pf.POLICIES)
@pytest.mark.parametrize("key", pf.connect_keys(), ids=str)
def test_connect_halving(key, policy):
    case = pf.connect_key(key)
    *want, steps, seen = pf.connect_halving_expected(key, policy)
    what = f"{pf.describe(case)} evaluate_actions_halving {policy} budget {case.budget}"
    b = load_connect(case, case.halving_roots)
    before = snapshot(b)
    got = b.evaluate_actions_halving(seed=SEED, budget=case.budget, max_plies=case.max_plies, policy=policy)
    print(f"{what}: steps {b.steps} / {steps}, selections {seen}")
    check(b, before, got, want, steps, what, ("counts", "given", "best"))
    b.close()


@pytest.mark.parametrize("policy", pf.POLICIES)
@pytest.mark.parametrize("key", list(pf.WIDE))
def test_connect_halving_on_the_workgroup_team(key, policy):
    """a round of more than 512 playouts goes to the 256-lane team: two roots of one corner a board width in words"""
    case = pf.connect_key(key)
    budget, roots = case.wide
    *want, steps, seen = pf.connect_halving_expected(key, policy, True)
    what = f"{pf.describe(case)} evaluate_actions_halving {policy} budget {budget} (the 256-lane team)"
    b = load_connect(case, roots)
    before = snapshot(b)
    got = b.evaluate_actions_halving(seed=SEED, budget=budget, max_plies=case.max_plies, policy=policy)
    print(f"{what}: steps {b.steps} / {steps}, selections {seen}")
    check(b, before, got, want, steps, what, ("counts", "given", "best"))
    b.close()


@pytest.mark.parametrize("policy", pf.POLICIES)
@pytest.mark.parametrize("key", pf.connect_keys(), ids=str)
def test_connect_search(key, policy):
    case = pf.connect_key(key)
    roots = pf.connect_search_roots(case, policy)
    *want, steps, seen = pf.connect_search_expected(key, policy)
    what = f"{pf.describe(case)} search_actions {policy} T {case.iterations} P {case.leaf_playouts} explore {case.explore}"
    b = load_connect(case, roots)
    before = snapshot(b)
    got = b.search_actions(**search_kw(case, policy))
    print(f"{what}: steps {b.steps} / {steps}, { {k: v for k, v in seen.items() if isinstance(v, int)} }")
    check(b, before, got, want, steps, what, ("counts", "visits", "best", "nodes"))
    b.close()


@pytest.mark.parametrize("policy", pf.POLICIES)
@pytest.mark.parametrize("key", pf.connect_keys(), ids=str)
def test_connect_forest_restart_equals_the_plain_search(key, policy):
    """a forest with room for every node (T + 1), restarted twice -- the second time over the first one's trees: the
    plain search's outputs and steps, nothing carried"""
    case = pf.connect_key(key)
    roots = pf.connect_search_roots(case, policy)
    *want, steps, _ = pf.connect_search_expected(key, policy)
    want = tuple(want) + (np.zeros_like(want[3]),)
    b = load_connect(case, roots)
    before = snapshot(b)
    forest = b.search_forest(case.iterations + 1)
    for again in (False, True):
        what = f"{pf.describe(case)} search_forest restart {policy} T {case.iterations} P {case.leaf_playouts} (second {again})"
        b.reset_steps()
        got = forest.search(restart=True, **search_kw(case, policy))
        check(b, before, got, want, steps, what, ("counts", "visits", "best", "nodes", "carried"))
    forest.close()
    b.close()


@pytest.mark.parametrize("policy", pf.POLICIES)
@pytest.mark.parametrize("key", pf.connect_corner_keys())
def test_connect_proving_search_on_the_corners(key, policy):
    case = pf.connect_key(key)
    roots = pf.connect_search_roots(case, policy)
    *want, steps, seen = pf.connect_prove_expected(key, policy)
    what = f"{pf.describe(case)} search_actions_proving {policy} T {case.iterations} P {case.leaf_playouts} explore {case.explore}"
    b = load_connect(case, roots)
    before = snapshot(b)
    got = b.search_actions_proving(**search_kw(case, policy))
    print(f"{what}: steps {b.steps} / {steps}, { {k: v for k, v in seen.items() if isinstance(v, int) and v} }")
    check(b, before, got, want, steps, what, ("counts", "visits", "best", "nodes", "proved", "done"))
    b.close()


# ------------------------------------------------------------------------------------------------ Bounce
def bounce_evaluate(case, key):
    for cap, max_plies in enumerate(case.max_plies):
        want, steps, seen = pf.bounce_eval_expected(key, cap)
        what = f"{pf.describe(case)} evaluate_moves decisive playouts {case.playouts} max_plies {max_plies}"
        b = load_bounce(case)               # (created here: the test-build knobs are read when a batch is created)
        before = snapshot(b)
        got = b.evaluate_moves(seed=SEED, playouts=case.playouts, max_plies=max_plies, policy="decisive")
        print(f"{what}: steps {b.steps} / {steps}, plies {seen}")
        check(b, before, (got,), (want,), steps, what, ("count",))
        b.close()


def bounce_halving(case, key, policy):
    for j, (budget, max_plies) in enumerate(zip(case.budgets, case.max_plies)):
        *want, steps, seen = pf.bounce_halving_expected(key, j, policy)
        what = f"{pf.describe(case)} evaluate_moves_halving {policy} budget {budget} max_plies {max_plies}"
        b = load_bounce(case)
        before = snapshot(b)
        got = b.evaluate_moves_halving(seed=SEED, budget=budget, max_plies=max_plies, policy=policy)
        print(f"{what}: steps {b.steps} / {steps}, selections {seen}")
        check(b, before, got, want, steps, what, ("counts", "given", "best"))
        b.close()


@pytest.mark.parametrize("key", pf.bounce_keys(), ids=str)
def test_bounce_decisive_evaluate(key):
    bounce_evaluate(pf.bounce_key(key), key)


@pytest.mark.parametrize("policy", pf.POLICIES)
@pytest.mark.parametrize("key", pf.bounce_keys(), ids=str)
def test_bounce_halving(key, policy):
    bounce_halving(pf.bounce_key(key), key, policy)


def test_default_board_run_time_geometry_gives_the_decisive_evaluation_and_the_halving(monkeypatch):
    """the 9x6 default grid once more under the test-build knob bounce_static_geom=0: the run-time geometry record every
    other grid takes gives the references' counts too.  The knob is read when a batch is created."""
    assert "bounce_static_geom" not in knobs
    monkeypatch.setitem(knobs, "bounce_static_geom", "0")
    case = pf.bounce_key("default")
    bounce_evaluate(case, "default")
    for policy in pf.POLICIES:
        bounce_halving(case, "default", policy)


def bounce_search_kw(case, policy):
    return dict(seed=SEED, iterations=case.iterations, leaf_playouts=case.leaf_playouts, explore=case.explore,
                max_plies=pf.bounce_search_cap(case), policy=policy, edges=pf.bounce_edges(case))


@pytest.mark.parametrize("policy", pf.POLICIES)
@pytest.mark.parametrize("key", pf.bounce_corner_keys())
def test_bounce_search_on_the_corners(key, policy):
    case = pf.bounce_key(key)
    kw = bounce_search_kw(case, policy)
    *want, steps, seen = pf.bounce_search_expected(key, policy)
    what = f"{pf.describe(case)} search_moves {kw}"
    b = load_bounce(case)
    assert kw["edges"] == (b.search_min_edges() if case.min_pool else b.search_default_edges(case.iterations)), what
    before = snapshot(b)
    got = b.search_moves(**kw)
    print(f"{what}: steps {b.steps} / {steps}, { {k: v for k, v in seen.items() if isinstance(v, int) and v} }")
    check(b, before, got, want, steps, what, ("counts", "visits", "best", "nodes", "used"))
    b.close()


@pytest.mark.parametrize("policy", pf.POLICIES)
@pytest.mark.parametrize("key", pf.bounce_corner_keys())
def test_bounce_proving_search_on_the_corners(key, policy):
    case = pf.bounce_key(key)
    kw = bounce_search_kw(case, policy)
    *want, steps, seen = pf.bounce_prove_expected(key, policy)
    what = f"{pf.describe(case)} search_moves_proving {kw}"
    b = load_bounce(case)
    before = snapshot(b)
    got = b.search_moves_proving(**kw)
    print(f"{what}: steps {b.steps} / {steps}, { {k: v for k, v in seen.items() if isinstance(v, int) and v} }")
    check(b, before, got, want, steps, what, ("counts", "visits", "best", "nodes", "used", "proved", "done"))
    b.close()
