"""The CPU side of the playout policy (bgs_connect_evaluate_actions_policy): the reference of tests/policy_expected.py
checked against the oracle, what the case table of the GPU comparison must hold, and the plumbing that needs no device.
The conditions on the table are conditions, not measurements: where the table misses one, the table changes."""

import fnmatch
import inspect
import os
import re

import numpy as np
import pytest

from oracle import oracle
from tests import policy_expected as pe
from tests.conftest import PKG, ROOT
from tests.mc_expected import connect_expected


@pytest.mark.parametrize("geom", [(6, 7, 4), (5, 6, 3), (7, 8, 5), (2, 5, 3), (8, 8, 6), (12, 13, 5), (4, 4, 1), (3, 3, 2)],
                         ids=lambda g: "x".join(map(str, g)))
def test_completion_agrees_with_the_oracles_winner(geom):
    """on every column of a few hundred random positions: `completes` for the mover is "step_actions makes the mover
    the winner"; for the other side it is the same statement on the board with the sides exchanged"""
    h, w, k = geom
    n = 600
    orc = oracle.ConnectOracle(h, w, k, n)
    rng = np.random.default_rng(h * 1000 + w * 10 + k)
    stop = rng.integers(0, max(1, h * w // 2), n)
    for ply in range(h * w):                 # board i: up to stop[i] uniformly random plies
        legal = orc.legal().astype(bool)
        pick = (rng.random((n, w)) * legal).argmax(axis=1)
        orc.step_actions(np.where((stop > ply) & legal.any(axis=1), pick, -1).astype(np.int32))
    running = orc.winner == -1
    assert running.sum() >= 100 or k <= 2, geom
    for side in (0, 1):                      # 0: the mover; 1: the opponent, "if the opponent dropped there now"
        who = (orc.player ^ side).astype(np.int64)
        got = pe.completes(orc.grid, who, k)
        for x in range(w):
            probe = oracle.ConnectOracle(h, w, k, n)
            probe.grid[:], probe.winner[:], probe.plies[:] = orc.grid, orc.winner, orc.plies
            probe.player[:] = who
            ok = probe.step_actions(np.full(n, x, dtype=np.int32)) == 0
            np.testing.assert_array_equal(ok, running & orc.legal()[:, x].astype(bool))
            np.testing.assert_array_equal(got[running, x], (ok & (probe.winner == who))[running], err_msg=f"{geom} column {x} side {side}")


@pytest.mark.parametrize("case", pe.CASES[:3] + pe.CASES[5:6], ids=lambda c: f"{c.h}x{c.w}x{c.k}")
@pytest.mark.parametrize("per_ply", [False, True])
def test_uniform_candidates_reproduce_the_oracles_rollout(case, per_ply):
    """with S = L forced the lock-step loop is the oracle's own rollout: counts and steps of mc_expected"""
    roots = pe.case_roots(case)
    cap = pe.case_max_plies(case, roots)
    got, steps, seen = pe.connect_policy_expected(case.h, case.w, case.k, roots, pe.SEED, case.first_game, case.playouts, cap,
                                                  per_ply, uniform=True)
    want, want_steps = connect_expected(case.h, case.w, case.k, roots, pe.SEED, case.first_game, case.playouts, cap, per_ply)
    np.testing.assert_array_equal(got, want)
    assert steps == want_steps
    assert sum(seen[c] for c in ("win", "block", "neither")) == steps - _first_moves(case, roots)


def _first_moves(case, roots):
    """the first columns played: one a (running root, open column, playout)"""
    grid, _, winner, _ = roots
    open_ = (grid[:, -1, :] == -1) & (winner == -1)[:, None]
    return int(open_.sum()) * case.playouts


@pytest.fixture(scope="module")
def classes():
    """case -> the plies of every class in the decisive reference (default RNG contract)"""
    out = {}
    for case in pe.CASES:
        roots = pe.case_roots(case)
        out[case] = pe.connect_policy_expected(case.h, case.w, case.k, roots, pe.SEED, case.first_game, case.playouts,
                                               pe.case_max_plies(case, roots), False)[2]
    return out


def test_the_cases_reach_every_class_of_ply(classes):
    """for NW = 1, 2, 3 and for count != 4: plies that win, plies that only block, plies that do neither, and plies with
    two or more winning / blocking columns (where the draw picks among them)"""
    for label, member in [("NW = 1", lambda c: pe.nw_of(c.h, c.w) == 1), ("NW = 2", lambda c: pe.nw_of(c.h, c.w) == 2),
                          ("NW = 3", lambda c: pe.nw_of(c.h, c.w) == 3), ("count != 4", lambda c: c.k != 4),
                          ("count == 4", lambda c: c.k == 4)]:
        total = {name: sum(seen[name] for c, seen in classes.items() if member(c)) for name in pe.CLASSES}
        assert all(total[name] > 0 for name in pe.CLASSES), f"{label}: {total}"


def test_the_cases_cover_the_geometries_and_roots_asked_for():
    geoms = {(c.h, c.w, c.k) for c in pe.CASES}
    assert (6, 7, 4) in geoms and (12, 13, 5) in geoms and len(geoms) >= 5
    assert {3, 5} <= {c.k for c in pe.CASES}
    assert {1, 2, 3} <= {pe.nw_of(c.h, c.w) for c in pe.CASES}
    assert any(c.cap is not None for c in pe.CASES) and any(c.first_game != 0 for c in pe.CASES)
    for case in pe.CASES:
        grid, _, winner, plies = pe.case_roots(case)
        running = winner == -1
        empty = (grid == -1).sum(axis=(1, 2))
        assert (plies == 0).any(), case                                  # the start
        assert (running & (plies > 0)).any(), case                       # mid-game
        assert (~running).any() or case.k > min(case.h, case.w), case    # ended boards
        if case.cap is not None:                                         # the cap cuts some roots' playouts and lets others run
            cap = pe.case_max_plies(case, (grid, None, winner, plies))
            assert (plies[running] < cap).any() and cap < case.h * case.w, case
    assert any(((pe.case_roots(c)[0] == -1).sum(axis=(1, 2)) <= 4).any() for c in pe.CASES)   # a near-full board


def test_the_header_and_the_map_hold_the_symbol():
    header = open(os.path.join(ROOT, "include", "bgs.h")).read()
    assert re.search(r"BGS_API\s+int\s+bgs_connect_evaluate_actions_policy\s*\(", header)
    assert re.search(r"#define\s+BGS_POLICY_UNIFORM\s+0\b", header) and re.search(r"#define\s+BGS_POLICY_DECISIVE\s+1\b", header)
    text = open(os.path.join(PKG, "csrc", "bgs.map")).read()
    exported = re.search(r"global:\s*([^;]+);", text).group(1).split()
    assert any(fnmatch.fnmatchcase("bgs_connect_evaluate_actions_policy", pattern) for pattern in exported), exported
    from simulator.game import _abi

    assert "bgs_connect_evaluate_actions_policy" in _abi.SIGNATURES
    assert (_abi.POLICY_UNIFORM, _abi.POLICY_DECISIVE) == (0, 1)


def test_python_argument_checks_that_need_no_device():
    from simulator.agents import MonteCarloAgent
    from simulator.batch import ConnectBatch, playout_policy

    assert (playout_policy("uniform"), playout_policy("decisive")) == (0, 1)
    for bad in ("Decisive", "", None, 1):
        with pytest.raises(ValueError, match="policy"):
            playout_policy(bad)
    for method in (ConnectBatch.evaluate_actions, ConnectBatch.evaluate_actions_tensor):
        assert inspect.signature(method).parameters["policy"].default == "uniform"
    assert inspect.signature(MonteCarloAgent).parameters["policy"].default == "uniform"
    with pytest.raises(ValueError, match="policy"):
        MonteCarloAgent(policy="greedy")
