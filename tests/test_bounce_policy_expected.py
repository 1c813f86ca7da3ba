"""The CPU side of the Bounce playout policy (bgs_bounce_evaluate_moves_policy): the reference of
tests/bounce_policy_expected.py checked against the oracle's own rollout, what the case table of the GPU comparison must
hold, and the plumbing that needs no device.  The conditions on the table are conditions, not measurements: where the
table misses one, the table changes."""

import fnmatch
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from tests import bounce_policy_expected as be
from tests import kernel_units
from tests.conftest import PKG, PRODUCT_LIB, ROOT, TEST_LIB
from tests.mc_expected import expected

SYMBOL = "bgs_bounce_evaluate_moves_policy"


@pytest.fixture(scope="module")
def runs():
    """case name -> (roots, cap, uniform (counts, steps, seen), decisive (counts, steps, seen))"""
    out = {}
    for case in be.CASES:
        grid, roots = be.GRIDS[case.name], be.case_roots(case)
        cap = be.case_max_plies(case, roots)
        args = (grid, roots, be.SEED, case.first_game, case.playouts, cap)
        out[case.name] = (roots, cap, be.bounce_policy_expected(*args, uniform=True), be.bounce_policy_expected(*args))
    return out


@pytest.mark.parametrize("case", be.CASES, ids=lambda c: c.name)
def test_uniform_candidates_reproduce_the_oracles_rollout(case, runs):
    """with S = L forced the lock-step loop is the oracle's own rollout: counts and steps of mc_expected"""
    roots, cap, (got, steps, seen), _ = runs[case.name]
    want, want_steps = expected(be.GRIDS[case.name], roots, be.SEED, case.first_game, case.playouts, cap)
    np.testing.assert_array_equal(got, want)
    assert steps == want_steps
    first_moves = sum(len(a) for a in be.root_actions(be.GRIDS[case.name], roots)) * case.playouts
    assert seen["win"] + seen["none"] == steps - first_moves and seen["win_many"] <= seen["win"]


def test_the_cases_reach_every_class_of_ply(runs):
    """over the grids of at most 8 columns (one word of move counts) and, separately, over the wider ones (three words):
    plies with a winning move, with two or more (where the draw picks among them), and with none"""
    for label, member in [("NC = 1", lambda g: g.shape[1] <= 8), ("NC = 3", lambda g: g.shape[1] > 8)]:
        names = [c.name for c in be.CASES if member(be.GRIDS[c.name])]
        total = {k: sum(runs[name][3][2][k] for name in names) for k in be.CLASSES}
        assert names and all(total[k] > 0 for k in be.CLASSES), f"{label}: {total}"
    # a wide grid on which a playout ply can fail to win, tall enough that games last
    assert runs["tall_wide"][3][2]["none"] > 0 and be.TALL_WIDE.shape[1] > 8 and be.TALL_WIDE.size <= 64


def test_the_cases_cover_the_grids_caps_and_roots_asked_for(runs):
    assert {"default", "small", "big_values", "crowded", "narrow", "blocked_start", "wide", "tall_wide"} == {c.name for c in be.CASES}
    assert any(c.first_game > 2**32 for c in be.CASES)
    cut = False
    for case in be.CASES:
        (grid, _, winner, plies), cap, _, (counts, _, _) = runs[case.name]
        running = winner == -1
        assert (plies == 0).any(), case                                   # the start
        if case.name == "blocked_start":                                  # the start has no move: it is an ended root itself
            assert not running.any()
            continue
        assert (~running).any(), case                                     # ended roots
        assert (plies > 0).any(), case                                    # roots past the start ...
        assert (running & (plies > 0)).any() or case.name == "narrow", case   # ... running ones (narrow: the first move ends the game)
        legal = np.zeros(counts.shape[:3], dtype=bool)
        for i, acts in enumerate(be.root_actions(be.GRIDS[case.name], runs[case.name][0])):
            for (sx, _), (tx, ty) in acts:
                legal[i, sx, ty * grid.shape[2] + tx] = True
        assert not counts[~legal].any()
        cut = cut or bool((counts.sum(-1)[legal] < case.playouts).any())
    assert cut, "no case has a cap that cuts playouts"


def test_decisive_playouts_differ_and_are_shorter_on_the_default_board(runs):
    _, _, (uniform, uniform_steps, _), (decisive, decisive_steps, _) = runs["default"]
    assert not np.array_equal(uniform, decisive)
    assert decisive_steps < uniform_steps


def test_the_header_the_map_and_the_binding_hold_the_symbol():
    header = open(os.path.join(ROOT, "include", "bgs.h")).read()
    assert re.search(r"BGS_API\s+int\s+" + SYMBOL + r"\s*\(", header)
    text = open(os.path.join(PKG, "csrc", "bgs.map")).read()
    exported = re.search(r"global:\s*([^;]+);", text).group(1).split()
    assert any(fnmatch.fnmatchcase(SYMBOL, pattern) for pattern in exported), exported
    from simulator.game import _abi

    assert SYMBOL in _abi.SIGNATURES
    assert _abi.SIGNATURES[SYMBOL] == _abi.SIGNATURES["bgs_connect_evaluate_actions_policy"]


def test_python_signatures_show_the_policy():
    from simulator.agents import MonteCarloAgent
    from simulator.batch import BounceBatch, playout_policy

    for method in (BounceBatch.evaluate_moves, BounceBatch.evaluate_moves_tensor):
        assert inspect.signature(method).parameters["policy"].default == "uniform"
    assert inspect.signature(MonteCarloAgent).parameters["policy"].default == "uniform"
    with pytest.raises(ValueError, match="policy"):
        playout_policy("greedy")


def test_both_libraries_export_it_from_six_kernel_units():
    for path in (PRODUCT_LIB, TEST_LIB):
        out = subprocess.check_output(["nm", "-D", "--defined-only", path], text=True)
        assert SYMBOL in {line.split()[-1] for line in out.splitlines() if line.strip()}, path
    kernel_units.check_six_distinct_ids()
