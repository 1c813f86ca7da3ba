"""The decisive playout policy of the Bounce flat Monte-Carlo evaluation (bgs_bounce_evaluate_moves_policy,
BounceBatch.evaluate_moves(policy=...), MonteCarloAgent(policy="decisive") on Bounce states) against the CPU reference of
tests/bounce_policy_expected.py, which plays the policy's definition (include/bgs.h) on the oracle's public API.

Everything here needs a real MI355X: `pytest -m gpu`.
"""

import ctypes

import numpy as np
import pytest

from oracle import oracle
from tests import bounce_policy_expected as be

pytestmark = pytest.mark.gpu

SEED = be.SEED
BY_NAME = {c.name: c for c in be.CASES}


def load(grid, roots, first_game=0, use_torch=None):
    from simulator.batch import BounceBatch

    b = BounceBatch(grid, roots[0].shape[0], use_torch=use_torch)
    assert (b.write_state(*roots) == 0).all()
    b.set_first_game(first_game)
    b.reset_steps()
    return b


def snapshot(b):
    return b.grid.tobytes(), b.player.tobytes(), b.winner.tobytes(), b.plies.tobytes()


def legal_slots(grid, roots):
    """bool[n, W, H * W]: the legal (root, slot) pairs per the oracle"""
    h, w = grid.shape
    out = np.zeros((roots[0].shape[0], w, h * w), dtype=bool)
    for i, acts in enumerate(be.root_actions(grid, roots)):
        for (sx, _), (tx, ty) in acts:
            out[i, sx, ty * w + tx] = True
    return out


@pytest.mark.parametrize("first_game", [5, 2**33])
@pytest.mark.parametrize("playouts", [1, 7, 48])
@pytest.mark.parametrize("name", list(BY_NAME))
def test_counts_and_steps_equal_the_reference(name, playouts, first_game):
    grid, roots = be.GRIDS[name], be.case_roots(BY_NAME[name])
    legal = legal_slots(grid, roots)
    for max_plies in (be.short_cap(roots, 6), be.LONG):
        b = load(grid, roots, first_game)
        before = snapshot(b)
        got = b.evaluate_moves(seed=SEED, playouts=playouts, max_plies=max_plies, policy="decisive")
        want, steps, _ = be.bounce_policy_expected(grid, roots, SEED, first_game, playouts, max_plies)
        what = f"{name} P={playouts} max_plies={max_plies} first_game={first_game}"
        np.testing.assert_array_equal(got, want, err_msg=what)
        assert b.steps == steps, what
        assert snapshot(b) == before, what
        assert not got[roots[2] != -1].any() and not got[~legal].any(), what   # ended roots, illegal slots: 0, 0, 0
        if name == "blocked_start":
            assert not got.any() and b.steps == 0
        b.close()


def test_a_segment_split_over_chunks():
    """more playouts than a chunk (512): a (root, slot) is handed out in pieces, to several waves"""
    grid = be.GRIDS["small"]
    roots = be.case_roots(BY_NAME["small"])
    running = np.flatnonzero(roots[2] == -1)[:2]
    roots = tuple(a[running] for a in roots)
    b = load(grid, roots, first_game=3)
    got = b.evaluate_moves(seed=SEED, playouts=600, max_plies=be.LONG, policy="decisive")
    want, steps, _ = be.bounce_policy_expected(grid, roots, SEED, 3, 600, be.LONG)
    np.testing.assert_array_equal(got, want)
    assert b.steps == steps


def test_uniform_through_the_new_entry_is_the_old_entry():
    from simulator.batch import BounceBatch
    from simulator.game import _abi

    n, playouts = 256, 32
    b = BounceBatch(be.GRIDS["default"], n)
    b.step_random(seed=SEED ^ 1, plies=5)
    b.reset_steps()
    old = b.evaluate_moves(seed=SEED, playouts=playouts, max_plies=be.LONG)
    old_steps = b.steps
    b.reset_steps()
    new = np.full_like(old, -1)
    _abi.check(_abi.lib().bgs_bounce_evaluate_moves_policy(b._handle, ctypes.c_uint64(SEED), playouts, be.LONG, _abi.POLICY_UNIFORM,
                                                           ctypes.c_void_p(new.ctypes.data), 0))
    assert new.tobytes() == old.tobytes() and b.steps == old_steps and old.any()
    b.reset_steps()
    decisive = b.evaluate_moves(seed=SEED, playouts=playouts, max_plies=be.LONG, policy="decisive")
    assert decisive.tobytes() != old.tobytes() and b.steps < old_steps


@pytest.mark.parametrize("name", ["default", "big_values", "tall_wide"])
def test_wins_in_one_are_taken(name):
    """not through the reference loop: a first move into the goal row wins every playout; a first move after which the
    other side can land in ITS goal row loses every playout (the cap lies at least two plies past every root)"""
    grid, roots = be.GRIDS[name], be.case_roots(BY_NAME[name])
    h, w = grid.shape
    playouts = 5
    b = load(grid, roots)
    got = b.evaluate_moves(seed=SEED, playouts=playouts, max_plies=int(roots[3].max()) + 2, policy="decisive")
    probe = oracle.BounceOracle(grid, 1)
    seen = {"win": 0, "loss": 0}
    for i, acts in enumerate(be.root_actions(grid, roots)):
        mover = int(roots[1][i])
        for (sx, sy), (tx, ty) in acts:
            slot = got[i, sx, ty * w + tx]
            if ty in (0, h - 1):
                assert slot.tolist() == [playouts, 0, 0], (name, i, sx, tx, ty)
                seen["win"] += 1
                continue
            probe.grid[:], probe.player[:], probe.winner[:], probe.plies[:] = (a[i] for a in roots)
            assert probe.step_actions(np.int32([[sx, sy, tx, ty]]))[0] == 0
            if probe.winner[0] == -1 and any(t[1] == (h - 1 if mover else 0) for _, t in probe.actions(0)):
                assert slot.tolist() == [0, 0, playouts], (name, i, sx, tx, ty)
                seen["loss"] += 1
    assert seen["win"] and seen["loss"], seen


def test_sharded_batches_give_the_whole_batch():
    from tests.mc_expected import make_roots

    grid = be.GRIDS["default"]
    roots = make_roots(grid, 48, seed=11)
    kw = dict(seed=SEED, playouts=16, max_plies=be.LONG, policy="decisive")
    whole = load(grid, roots, first_game=100).evaluate_moves(**kw)
    half = [tuple(a[s] for a in roots) for s in (slice(0, 20), slice(20, 48))]
    lo = load(grid, half[0], first_game=100).evaluate_moves(**kw)
    hi = load(grid, half[1], first_game=120).evaluate_moves(**kw)
    np.testing.assert_array_equal(np.concatenate([lo, hi]), whole)
    assert whole.any()


def test_device_path_writes_everything_in_stream_order():
    import torch

    from tests.mc_expected import make_roots

    grid = be.GRIDS["small"]
    n, playouts = 64, 8
    roots = make_roots(grid, n, seed=13)
    b = load(grid, roots, use_torch=True)
    ref = load(grid, roots)
    stream = torch.cuda.Stream(device=0)
    b.set_stream(stream.cuda_stream)
    with torch.cuda.stream(stream):
        out = torch.full((n, 3, 18, 3), -1, dtype=torch.int32, device="cuda:0")
        b.step_random(seed=SEED ^ 5, plies=2)      # enqueued before the evaluation on the same stream
        b.evaluate_moves_tensor(out, seed=SEED, playouts=playouts, max_plies=512, policy="decisive")
    stream.synchronize()
    got = out.cpu().numpy()
    assert (got >= 0).all()
    ref.step_random(seed=SEED ^ 5, plies=2)
    assert snapshot(ref) == snapshot(b)
    np.testing.assert_array_equal(got, ref.evaluate_moves(seed=SEED, playouts=playouts, max_plies=512, policy="decisive"))
    want, _, _ = be.bounce_policy_expected(grid, (ref.grid, ref.player, ref.winner, ref.plies), SEED, 0, playouts, 512)
    np.testing.assert_array_equal(got, want)
    assert want.any()


def test_a_larger_launch_keeps_its_invariants():
    from simulator.batch import BounceBatch

    grid = be.GRIDS["default"]
    n, playouts = 4096, 16
    b = BounceBatch(grid, n)
    b.step_random(seed=SEED ^ 1, plies=3)
    b.step_random(seed=SEED ^ 2, plies=4)
    roots = (b.grid, b.player, b.winner, b.plies)
    b.reset_steps()
    got = b.evaluate_moves(seed=SEED, playouts=playouts, max_plies=be.LONG, policy="decisive")
    steps = b.steps
    t = b.targets[:, :6]
    legal = ((t[..., None] >> np.arange(54, dtype=np.uint64)) & np.uint64(1)) != 0
    legal &= (roots[2] == -1)[:, None, None]
    per_slot = got.sum(-1)
    assert (got >= 0).all() and (per_slot <= playouts).all()
    assert (per_slot[~legal] == 0).all() and per_slot[legal].any()
    assert steps >= int(legal.sum()) * playouts
    cut = 1500
    parts, part_steps = [], 0
    for sl, first in ((slice(0, cut), 0), (slice(cut, n), cut)):
        s = load(grid, tuple(a[sl] for a in roots), first_game=first)
        parts.append(s.evaluate_moves(seed=SEED, playouts=playouts, max_plies=be.LONG, policy="decisive"))
        part_steps += s.steps
        s.close()
    np.testing.assert_array_equal(np.concatenate(parts), got)
    assert part_steps == steps


def uniform_takes_both_games(bounce_state):
    from simulator.agents import MonteCarloAgent
    from simulator.game.connect import Config

    agent = MonteCarloAgent(playouts=8, seed=SEED)
    start = Config(6, 7, 4).sample_initial_state()
    ok = list(agent.predict(start)) == start.actions and list(agent.predict(bounce_state)) == bounce_state.actions
    agent.close()
    return ok


def test_decisive_agent_on_bounce_states():
    from simulator.agents import BOUNCE_MAX_PLIES, MonteCarloAgent, SolverAgent
    from simulator.game.bounce import Config

    config = Config(be.GRIDS["default"])
    states = [config.sample_initial_state()]
    rng = np.random.default_rng(3)
    for _ in range(5):
        s = states[-1]
        for _ in range(int(rng.integers(1, 4))):
            if s.has_ended:
                break
            acts = s.actions
            s = acts[int(rng.integers(len(acts)))].sample_next_state()
        if not s.has_ended:
            states.append(s)
    agent = MonteCarloAgent(playouts=32, seed=SEED, policy="decisive")
    many = agent.predict_many(states)
    g = np.stack([s.grid for s in states])
    roots = (g, np.array([s.player for s in states], np.int8), np.full(len(states), -1, np.int8),
             np.array([s._plies for s in states], np.int32))
    want, _, _ = be.bounce_policy_expected(config.grid, roots, SEED, 0, 32, BOUNCE_MAX_PLIES)
    for k, (s, m) in enumerate(zip(states, many)):
        assert list(m) == s.actions
        assert m == agent.predict(s, game=k)
        for a in s.actions:
            (sx, _), (tx, ty) = a._source, a._target
            wdl = want[k, sx, ty * 6 + tx]
            assert m[a] == (wdl[0] + 0.5 * wdl[1]) / 32
    chosen = agent.choose_many(states)
    assert all(c in s.actions for c, s in zip(chosen, states)) and chosen[-1] == agent.choose(states[-1], game=len(states) - 1)
    uniform = MonteCarloAgent(playouts=32, seed=SEED)
    assert uniform.predict_many(states) != many
    uniform.close()
    # ... it serves as the solver's fallback, and halving stays refused for Bounce states
    solver = SolverAgent(depth=2, fallback=agent)
    assert set(solver.predict(states[1])) == set(states[1].actions)
    solver.close()
    # Connect's "decisive" is another policy: this agent has played Bounce's and keeps to it
    from simulator.game.connect import Config as ConnectConfig

    with pytest.raises(ValueError, match="Connect"):
        agent.predict(ConnectConfig(6, 7, 4).sample_initial_state())
    assert uniform_takes_both_games(states[0])
    agent.close()
    halving = MonteCarloAgent(playouts=32, seed=SEED, policy="decisive", allocation="halving")
    with pytest.raises(ValueError, match="halving"):
        halving.predict(states[0])
    halving.close()


def test_refusals():
    import torch

    from simulator.batch import BounceBatch, ConnectBatch
    from simulator.game import _abi

    call = _abi.lib().bgs_bounce_evaluate_moves_policy
    b = BounceBatch(be.GRIDS["default"], 4)
    out = np.zeros(4 * 6 * 54 * 3, dtype=np.int32)
    for policy in (2, -1):
        assert call(b._handle, 1, 8, 100, policy, ctypes.c_void_p(out.ctypes.data), 0) == _abi.BGS_ERR_ARG
        assert "policy" in _abi.last_error()
    with pytest.raises(ValueError, match="policy"):
        b.evaluate_moves(policy="greedy")
    with pytest.raises(ValueError, match="policy"):
        b.evaluate_moves_tensor(policy="greedy")
    with pytest.raises(ValueError, match="playouts"):
        b.evaluate_moves(playouts=0, policy="decisive")
    with pytest.raises(ValueError, match="max_plies"):
        b.evaluate_moves(max_plies=0, policy="decisive")
    t = torch.zeros(4 * 6 * 54 * 3 + 4, dtype=torch.int32, device="cuda:0")
    rc = call(b._handle, 1, 8, 100, _abi.POLICY_DECISIVE, ctypes.c_void_p(t.data_ptr() + 4), 1)
    assert rc == _abi.BGS_ERR_ARG and "aligned" in _abi.last_error()
    c = ConnectBatch(6, 7, 4, 4)
    big = np.zeros(4 * 7 * 42 * 3, dtype=np.int32)
    for policy in (_abi.POLICY_UNIFORM, _abi.POLICY_DECISIVE):
        assert call(c._handle, 1, 8, 100, policy, ctypes.c_void_p(big.ctypes.data), 0) == _abi.BGS_ERR_ARG
        assert "Bounce" in _abi.last_error()
    wide = np.zeros((9, 8), dtype=np.int8)   # 72 cells: a generic board
    wide[1] = wide[7] = 1
    with pytest.raises(ValueError, match="bit-packed"):
        BounceBatch(wide, 4).evaluate_moves(policy="decisive")
    # the Connect entry keeps refusing Bounce batches
    assert _abi.lib().bgs_connect_evaluate_actions_policy(b._handle, 1, 8, 100, _abi.POLICY_DECISIVE, ctypes.c_void_p(out.ctypes.data),
                                                          0) == _abi.BGS_ERR_ARG
    assert "Connect" in _abi.last_error()
