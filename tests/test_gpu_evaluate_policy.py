"""Playout policies of the flat Monte-Carlo evaluation (bgs_connect_evaluate_actions_policy,
ConnectBatch.evaluate_actions(policy=...), MonteCarloAgent(policy=...)) against the CPU reference of
tests/policy_expected.py: counts and bgs_steps bit for bit.  tests/test_policy_expected.py states what the case table
holds (every class of ply for NW = 1, 2, 3 and count != 4).

Everything here needs a real MI355X: `pytest -m gpu`.
"""

import ctypes

import numpy as np
import pytest

from tests import policy_expected as pe

pytestmark = pytest.mark.gpu

SEED = pe.SEED


def load(h, w, k, roots, per_ply=False, first_game=0, use_torch=None):
    from simulator.batch import ConnectBatch

    grid, player, winner, plies = roots
    b = ConnectBatch(h, w, k, grid.shape[0], use_torch=use_torch)
    assert (b.write_state(grid, player, winner, plies) == 0).all()
    if per_ply:
        b.set_rng_contract("per-ply")
    b.set_first_game(first_game)
    b.reset_steps()
    return b


def snapshot(b):
    return b.grid.tobytes(), b.player.tobytes(), b.winner.tobytes(), b.plies.tobytes()


@pytest.mark.parametrize("case", pe.CASES, ids=lambda c: f"{c.h}x{c.w}x{c.k}-P{c.playouts}")
@pytest.mark.parametrize("per_ply", [False, True], ids=["per-block", "per-ply"])
def test_decisive_counts_and_steps_equal_the_reference(case, per_ply):
    h, w, k = case.h, case.w, case.k
    roots = pe.case_roots(case)
    max_plies = pe.case_max_plies(case, roots)
    b = load(h, w, k, roots, per_ply, case.first_game)
    before = snapshot(b)
    got = b.evaluate_actions(seed=SEED, playouts=case.playouts, max_plies=max_plies, policy="decisive")
    want, steps, seen = pe.connect_policy_expected(h, w, k, roots, SEED, case.first_game, case.playouts, max_plies, per_ply)
    print(f"{case} per_ply={per_ply}: steps {b.steps} / {steps}, plies by class {seen}, "
          f"entries that differ {int((got != want).any(-1).sum())} of {want.shape[0] * want.shape[1]}")
    np.testing.assert_array_equal(got, want, err_msg=str(case))
    assert b.steps == steps, case
    assert snapshot(b) == before, case
    b.close()


def test_playouts_spanning_waves_equal_the_reference():
    """more playouts than a wave takes: a (root, column) is split over waves"""
    case = pe.CASES[0]
    roots = tuple(a[:5] for a in pe.case_roots(case))
    b = load(case.h, case.w, case.k, roots, first_game=3)
    got = b.evaluate_actions(seed=SEED, playouts=700, policy="decisive")
    want, steps, _ = pe.connect_policy_expected(case.h, case.w, case.k, roots, SEED, 3, 700, pe.UNCAPPED, False)
    np.testing.assert_array_equal(got, want)
    assert b.steps == steps


@pytest.mark.parametrize("case", [pe.CASES[0], pe.CASES[7]], ids=lambda c: f"{c.h}x{c.w}x{c.k}")
def test_two_shards_equal_the_whole_batch(case):
    h, w, k = case.h, case.w, case.k
    roots = pe.case_roots(case)
    n = roots[0].shape[0]
    cut = n // 2
    kw = dict(seed=SEED, playouts=case.playouts, policy="decisive")
    whole = load(h, w, k, roots, first_game=100).evaluate_actions(**kw)
    lo = load(h, w, k, tuple(a[:cut] for a in roots), first_game=100).evaluate_actions(**kw)
    hi = load(h, w, k, tuple(a[cut:] for a in roots), first_game=100 + cut).evaluate_actions(**kw)
    np.testing.assert_array_equal(np.concatenate([lo, hi]), whole)


@pytest.mark.parametrize("policy", ["uniform", "decisive"])
def test_device_output_equals_host_output(policy):
    import torch

    case = pe.CASES[0]
    roots = pe.case_roots(case)
    n = roots[0].shape[0]
    b = load(case.h, case.w, case.k, roots, use_torch=True, first_game=9)
    host = b.evaluate_actions(seed=SEED, playouts=48, policy=policy)
    steps = b.steps
    b.reset_steps()
    out = torch.full((n, case.w, 3), -1, dtype=torch.int32, device="cuda:0")
    assert b.evaluate_actions_tensor(out, seed=SEED, playouts=48, policy=policy) is out
    torch.cuda.synchronize()
    np.testing.assert_array_equal(out.cpu().numpy(), host)
    assert b.steps == steps
    if policy == "decisive":
        want, want_steps, _ = pe.connect_policy_expected(case.h, case.w, case.k, roots, SEED, 9, 48, pe.UNCAPPED, False)
        np.testing.assert_array_equal(host, want)
        assert steps == want_steps


@pytest.mark.parametrize("case", [pe.CASES[0], pe.CASES[1], pe.CASES[6], pe.CASES[7]], ids=lambda c: f"{c.h}x{c.w}x{c.k}")
@pytest.mark.parametrize("per_ply", [False, True], ids=["per-block", "per-ply"])
def test_uniform_policy_is_the_old_entry_point_byte_for_byte(case, per_ply):
    from simulator.game import _abi

    roots = pe.case_roots(case)
    max_plies = pe.case_max_plies(case, roots)
    n = roots[0].shape[0]
    b = load(case.h, case.w, case.k, roots, per_ply, case.first_game)
    old = np.full((n, case.w, 3), -1, dtype=np.int32)
    new = np.full((n, case.w, 3), -2, dtype=np.int32)
    _abi.check(_abi.lib().bgs_connect_evaluate_actions(b._handle, SEED, 300, max_plies, ctypes.c_void_p(old.ctypes.data), 0))
    old_steps = b.steps
    b.reset_steps()
    _abi.check(_abi.lib().bgs_connect_evaluate_actions_policy(b._handle, SEED, 300, max_plies, _abi.POLICY_UNIFORM,
                                                              ctypes.c_void_p(new.ctypes.data), 0))
    assert old.tobytes() == new.tobytes()
    assert b.steps == old_steps
    np.testing.assert_array_equal(b.evaluate_actions(seed=SEED, playouts=300, max_plies=max_plies, policy="uniform"), old)


# ---- properties that need no reference: hand-built Connect4 roots
def _root(columns, h=6, w=7):
    """(grid, player, winner, plies) rows of the board after `columns`, played from the start by alternating sides"""
    from oracle import oracle

    orc = oracle.ConnectOracle(h, w, 4, 1)
    for c in columns:
        assert (orc.step_actions(np.int32([c])) == 0).all()
    assert orc.winner[0] == -1
    return orc.grid.copy(), orc.player.copy(), orc.winner.copy(), orc.plies.copy()


def _stack(rows):
    return tuple(np.concatenate([r[j] for r in rows]) for j in range(4))


# player 0 to move everywhere.  Player 1 holds three stacked stones in column 3 and player 0 has no winning cell:
SINGLE_THREAT = [0, 3, 0, 3, 1, 3]
# player 1 holds columns 2-4 of the bottom row with both ends open: two winning cells, and player 0 has none
TWO_THREATS = [0, 2, 6, 3, 0, 4]
# player 0 wins at once in column 0; player 1 threatens column 1
WIN_NOW = [0, 1, 0, 1, 0, 1]
# player 0 holds columns 2-4 of the bottom row with both ends open: columns 1 and 5 win at once
TWO_WINS = [3, 0, 4, 0, 2, 6]


def evaluate_hand_built(playouts=64, per_ply=False):
    roots = _stack([_root(c) for c in (SINGLE_THREAT, TWO_THREATS, WIN_NOW, TWO_WINS)])
    assert (roots[1] == 0).all()
    return load(6, 7, 4, roots, per_ply).evaluate_actions(seed=SEED, playouts=playouts, policy="decisive")


@pytest.mark.parametrize("per_ply", [False, True], ids=["per-block", "per-ply"])
def test_threats_are_taken_and_blocked_whatever_the_draws(per_ply):
    playouts = 64
    won, lost = (playouts, 0, 0), (0, 0, playouts)
    single, double, win_now, two_wins = evaluate_hand_built(playouts, per_ply)
    # the opponent has exactly one winning cell: every column that neither wins nor blocks loses every playout (the
    # opponent's first ply takes the cell); the block keeps the game open
    for c in range(7):
        if c != 3:
            assert tuple(single[c]) == lost, (c, single)
    assert single[3].sum() == playouts and single[3, 2] < playouts
    # the opponent has two winning cells: every column that does not win at once loses all its playouts
    for c in range(7):
        assert tuple(double[c]) == lost, (c, double)
    # a column that wins at once wins every playout; the columns that leave the opponent's single threat open lose
    assert tuple(win_now[0]) == won
    for c in range(2, 7):
        assert tuple(win_now[c]) == lost, (c, win_now)
    assert win_now[1].sum() == playouts
    # two winning cells of the mover: both win at once, and after any other column the opponent blocks one and the
    # mover takes the other
    for c in range(7):
        assert tuple(two_wins[c]) == won, (c, two_wins)


# ---- refusals
def test_refusals():
    import torch

    from simulator.batch import BounceBatch, ConnectBatch
    from simulator.game import _abi

    call = _abi.lib().bgs_connect_evaluate_actions_policy
    b = ConnectBatch(6, 7, 4, 4)
    out = np.zeros(4 * 7 * 3, dtype=np.int32)
    for policy in (2, -1, 99):
        assert call(b._handle, 1, 8, 100, policy, ctypes.c_void_p(out.ctypes.data), 0) == _abi.BGS_ERR_ARG
        assert "policy" in _abi.last_error()
    with pytest.raises(ValueError, match="policy"):
        b.evaluate_actions(policy="greedy")
    with pytest.raises(ValueError, match="policy"):
        b.evaluate_actions_tensor(policy="greedy")
    with pytest.raises(ValueError, match="playouts"):
        b.evaluate_actions(playouts=0, policy="decisive")
    with pytest.raises(ValueError, match="max_plies"):
        b.evaluate_actions(max_plies=0, policy="decisive")
    grid = np.zeros((9, 6), dtype=np.int8)
    grid[1] = grid[7] = [1, 2, 3, 3, 2, 1]
    bounce = BounceBatch(grid, 64)
    big = np.zeros(64 * 6 * 3, dtype=np.int32)
    for policy in (_abi.POLICY_UNIFORM, _abi.POLICY_DECISIVE):
        assert call(bounce._handle, 1, 8, 100, policy, ctypes.c_void_p(big.ctypes.data), 0) == _abi.BGS_ERR_ARG
        assert "Connect" in _abi.last_error()
    with pytest.raises(ValueError, match="Connect"):
        bounce.evaluate_actions(policy="decisive")
    with pytest.raises(ValueError, match="bit-packed"):
        ConnectBatch(20, 20, 5, 4).evaluate_actions(policy="decisive")
    t = torch.zeros(4 * 7 * 3 + 1, dtype=torch.int32, device="cuda:0")
    rc = call(b._handle, 1, 8, 100, _abi.POLICY_DECISIVE, ctypes.c_void_p(t.data_ptr() + 4), 1)
    assert rc == _abi.BGS_ERR_ARG and "aligned" in _abi.last_error()


# ---- the agent
def _state_after(columns, config=(6, 7, 4)):
    from simulator.game.connect import Config

    s = Config(*config).sample_initial_state()
    for c in columns:
        s = s.action_at(c).sample_next_state()
    return s


def test_decisive_agent_equals_the_batch_call():
    from simulator.agents import MonteCarloAgent, SolverAgent
    from simulator.batch import ConnectBatch
    from simulator.game import bounce

    agent = MonteCarloAgent(playouts=96, seed=SEED, policy="decisive")
    states = [_state_after(cs) for cs in ([], [3], [3, 3, 2], [0, 1, 0, 1, 0, 1], [3, 3, 3, 3, 3, 3, 2], [0, 3, 0, 3, 1, 3])]
    many = agent.predict_many(states, first_game=4)
    b = ConnectBatch(6, 7, 4, len(states))
    grid = np.stack([s.grid for s in states])
    player = np.array([s.player for s in states], dtype=np.int8)
    assert (b.write_state(grid, player, np.full(len(states), -1, dtype=np.int8)) == 0).all()
    b.set_first_game(4)
    counts = b.evaluate_actions(seed=SEED, playouts=96, policy="decisive").astype(np.float64)
    value = (counts[..., 0] + 0.5 * counts[..., 1]) / 96
    for g, (s, m) in enumerate(zip(states, many)):
        assert list(m) == s.actions
        assert m == {a: float(value[g, a.column]) for a in s.actions}
        assert agent.predict(s, game=4 + g) == m
    assert many[3][states[3].action_at(0)] == 1.0
    assert max(many[5], key=many[5].get).column == 3        # the only column that does not lose at once
    uniform = MonteCarloAgent(playouts=96, seed=SEED).predict_many(states, first_game=4)
    assert uniform != many
    # ... and it serves as the solver's fallback
    solver = SolverAgent(depth=2, fallback=agent)
    assert set(solver.predict(states[1])) == set(states[1].actions)
    solver.close()

    grid = np.zeros((9, 6), dtype=np.int8)
    grid[1] = grid[7] = [1, 2, 3, 3, 2, 1]
    with pytest.raises(ValueError, match="Bounce"):
        agent.predict(bounce.Config(grid).sample_initial_state())
    agent.close()
