"""Sequential-halving Monte-Carlo evaluation of Bounce boards (bgs_bounce_evaluate_moves_halving,
BounceBatch.evaluate_moves_halving, simulator.agents.BounceHalvingAgent) against the CPU statement of
tests/bounce_halving_expected.py: counts, given, best and the bgs_steps delta bit for bit.
tests/test_bounce_halving_expected.py states what the case table holds.

The launcher has one team size (a 256-lane workgroup a root), so there is no threshold between team sizes to test.

Everything here needs a real MI355X: `pytest -m gpu`.
"""

import ctypes

import numpy as np
import pytest

from tests import bounce_halving_expected as bh

pytestmark = pytest.mark.gpu

SEED = bh.SEED


def load(grid, roots, first_game=0, use_torch=None):
    from simulator.batch import BounceBatch

    b = BounceBatch(grid, roots[0].shape[0], use_torch=use_torch)
    assert (b.write_state(*roots) == 0).all()
    b.set_first_game(first_game)
    b.reset_steps()
    return b


def snapshot(b):
    return b.grid.tobytes(), b.player.tobytes(), b.winner.tobytes(), b.plies.tobytes()


def assert_equal(got, want, what=""):
    for name, g, w in zip(("counts", "given", "best"), got, want):
        np.testing.assert_array_equal(g, w, err_msg=f"{name} {what}")


@pytest.mark.parametrize("name,policy", bh.RUNS, ids=[f"{n}-{p}" for n, p in bh.RUNS])
def test_counts_given_best_and_steps_equal_the_reference(name, policy):
    case = bh.BY_NAME[name]
    grid, roots = bh.case_grid(case), bh.case_roots(case)
    b = load(grid, roots, case.first_game)
    before = snapshot(b)
    kw = dict(seed=SEED, budget=case.budget, max_plies=bh.case_max_plies(case, roots), policy=policy)
    got = b.evaluate_moves_halving(**kw)
    got_steps = b.steps
    counts, given, best, steps, seen = bh.case_expected(name, policy)
    print(f"{name} {policy}: steps {got_steps} / {steps}, selections {seen}, "
          f"roots whose best differs {int((got[2] != best).sum())} of {best.size}")
    assert_equal(got, (counts, given, best), name)
    assert got_steps == steps, name
    assert snapshot(b) == before, name        # boards, plies and status are unchanged
    b.reset_steps()
    assert_equal(b.evaluate_moves_halving(**kw), got, f"{name}, the second call")
    assert b.steps == steps
    b.close()


@pytest.mark.parametrize("name", ["default", "tall_wide"])
def test_a_cap_one_ply_past_the_roots_leaves_the_slot_order_to_decide(name):
    """max_plies = root plies + 1: every playout is capped after its first move and scores 0"""
    case = bh.BY_NAME[name]
    grid, roots = bh.case_grid(case), bh.case_roots(case)
    h, w = grid.shape
    # the running roots of one ply count whose first moves end nothing: no move into a goal row (a move that leaves
    # the other side without a move would end the game too: checked below through counts == 0)
    acts = bh.root_actions(grid, roots)
    quiet = np.array([bool(a) and all(t[1] not in (0, h - 1) for _, t in a) for a in acts])
    at = np.bincount(roots[3][quiet]).argmax()
    rows = np.flatnonzero(quiet & (roots[3] == at))
    assert rows.size >= 1
    picked = tuple(a[rows] for a in roots)
    b = load(grid, picked)
    budget = max(bh.min_budget(len(acts[i])) for i in rows) + 3
    counts, given, best = b.evaluate_moves_halving(seed=SEED, budget=budget, max_plies=int(at) + 1)
    assert (counts == 0).all()
    given = given.reshape(rows.size, -1)
    for k, i in enumerate(rows):
        slots = np.array([sx * h * w + ty * w + tx for (sx, _), (tx, ty) in acts[i]])
        want = np.zeros(w * h * w, dtype=np.int32)
        for m, q in bh.schedule(slots.size, budget):
            want[slots[:m]] += q               # all scores are 0: the m lowest slots survive
        np.testing.assert_array_equal(given[k], want)
        assert best[k] == slots[0]
    assert b.steps == int(given.sum())         # the first moves alone
    b.close()


@pytest.mark.parametrize("name", ["default", "tall_wide"])
def test_two_shards_equal_the_whole_batch(name):
    case = bh.BY_NAME[name]
    grid, roots = bh.case_grid(case), bh.case_roots(case)
    cut = roots[0].shape[0] // 2
    kw = dict(seed=SEED, budget=case.budget, max_plies=bh.LONG, policy="decisive")
    whole = load(grid, roots, first_game=100).evaluate_moves_halving(**kw)
    lo = load(grid, tuple(a[:cut] for a in roots), first_game=100).evaluate_moves_halving(**kw)
    hi = load(grid, tuple(a[cut:] for a in roots), first_game=100 + cut).evaluate_moves_halving(**kw)
    assert_equal(tuple(np.concatenate([x, y]) for x, y in zip(lo, hi)), whole)
    assert whole[0].any()


def test_one_legal_move_is_the_flat_evaluation_of_that_slot():
    """a root with one legal move (the narrow board has them): one round of `budget` playouts, the games of
    evaluate_moves(playouts=budget)"""
    case = bh.BY_NAME["narrow"]
    grid, mixed = bh.case_grid(case), bh.case_roots(case)
    rows = np.flatnonzero(bh.arm_counts(case) == 1)
    roots = tuple(a[rows] for a in mixed)
    acts = bh.root_actions(grid, roots)
    assert acts and all(len(a) == 1 for a in acts)
    budget = 40
    b = load(grid, roots, first_game=17)
    counts, given, best = b.evaluate_moves_halving(seed=SEED, budget=budget, max_plies=bh.LONG)
    steps = b.steps
    b.reset_steps()
    flat = b.evaluate_moves(seed=SEED, playouts=budget, max_plies=bh.LONG)
    np.testing.assert_array_equal(counts, flat)
    assert b.steps == steps and steps >= budget * len(acts)
    h, w = grid.shape
    slots = np.array([sx * h * w + ty * w + tx for ((sx, _), (tx, ty)), in acts])
    np.testing.assert_array_equal(best, slots)
    want = np.zeros((len(acts), w * h * w), dtype=np.int32)
    want[np.arange(len(acts)), slots] = budget
    np.testing.assert_array_equal(given.reshape(len(acts), -1), want)
    b.close()


@pytest.mark.parametrize("policy", ["uniform", "decisive"])
def test_device_outputs_equal_host_outputs(policy):
    import torch

    from simulator.batch import playout_policy
    from simulator.game import _abi

    case = bh.BY_NAME["default"]
    grid, roots = bh.case_grid(case), bh.case_roots(case)
    h, w = grid.shape
    n, S = roots[0].shape[0], w * h * w
    b = load(grid, roots, use_torch=True, first_game=case.first_game)
    kw = dict(seed=SEED, budget=case.budget, max_plies=bh.LONG, policy=policy)
    host = b.evaluate_moves_halving(**kw)
    steps = b.steps
    assert_equal(host, bh.case_expected("default", policy)[:3])
    b.reset_steps()
    # every output sits in the middle of a buffer of sentinels: nothing outside its extent is touched (the offsets keep
    # the 16-byte alignment)
    sizes = (n * S * 3, n * S, n)
    pads = [torch.full((size + 8,), -7, dtype=torch.int32, device="cuda:0") for size in sizes]
    shapes = ((n, w, h * w, 3), (n, w, h * w), (n,))
    outs = [p[4:4 + size].view(shape) for p, size, shape in zip(pads, sizes, shapes)]
    got = b.evaluate_moves_halving_tensor(*outs, **kw)
    assert all(g is o for g, o in zip(got, outs))
    torch.cuda.synchronize()
    assert_equal(tuple(g.cpu().numpy() for g in got), host)
    assert b.steps == steps
    for p, size in zip(pads, sizes):
        assert bool((p[:4] == -7).all()) and bool((p[4 + size:] == -7).all())
    fresh = b.evaluate_moves_halving_tensor(**kw)
    torch.cuda.synchronize()
    assert_equal(tuple(g.cpu().numpy() for g in fresh), host)
    # given and best may be NULL
    code = playout_policy(policy)
    call = _abi.lib().bgs_bounce_evaluate_moves_halving
    counts = np.full((n, w, h * w, 3), -1, dtype=np.int32)
    _abi.check(call(b._handle, SEED, case.budget, bh.LONG, code, ctypes.c_void_p(counts.ctypes.data), None, None, 0))
    np.testing.assert_array_equal(counts, host[0])
    only = torch.full((n, w, h * w, 3), -7, dtype=torch.int32, device="cuda:0")
    _abi.check(call(b._handle, SEED, case.budget, bh.LONG, code, ctypes.c_void_p(only.data_ptr()), None, None, 1))
    torch.cuda.synchronize()
    np.testing.assert_array_equal(only.cpu().numpy(), host[0])
    b.close()


def test_refusals_return_err_arg_and_leave_the_outputs_untouched():
    import torch

    from simulator.batch import HALVING_SHORT, BounceBatch, ConnectBatch
    from simulator.game import _abi

    call = _abi.lib().bgs_bounce_evaluate_moves_halving
    U = _abi.POLICY_UNIFORM
    grid = bh.GRIDS["default"]
    n, S = 4, 6 * 9 * 6
    b = BounceBatch(grid, n)
    outs = [np.full(n * S * 3, -5, dtype=np.int32), np.full(n * S, -5, dtype=np.int32), np.full(n, -5, dtype=np.int32)]
    ptr = [ctypes.c_void_p(o.ctypes.data) for o in outs]

    def refused(word, *args):
        assert call(*args) == _abi.BGS_ERR_ARG
        assert word in _abi.last_error(), _abi.last_error()
        assert all((o == -5).all() for o in outs)

    refused("budget", b._handle, 1, 0, 100, U, *ptr, 0)
    refused("budget", b._handle, 1, -3, 100, U, *ptr, 0)
    refused("max_plies", b._handle, 1, 200, 0, U, *ptr, 0)
    for policy in (2, -1, 99):
        refused("policy", b._handle, 1, 200, 100, policy, *ptr, 0)
    refused("counts", b._handle, 1, 200, 100, U, None, ptr[1], ptr[2], 0)
    # a budget of 1 is taken by the call: every root of the start position (22 moves) is short
    assert call(b._handle, 1, 1, 1, U, *ptr, 0) == _abi.BGS_OK
    assert not outs[0].any() and not outs[1].any() and (outs[2] == HALVING_SHORT).all() and HALVING_SHORT == -2
    assert BounceBatch.halving_min_budget(22) == 110 and BounceBatch.halving_min_budget(1) == 1
    for o in outs:
        o[:] = -5
    # Connect and generic batches
    connect = ConnectBatch(6, 7, 4, n)
    refused("Bounce", connect._handle, 1, 200, 100, U, *ptr, 0)
    for method in (connect.evaluate_moves_halving, connect.evaluate_moves_halving_tensor):
        with pytest.raises(ValueError, match="Bounce"):
            method(budget=200)
    wide = np.zeros((9, 8), dtype=np.int8)    # 72 cells: a generic board
    wide[1] = wide[7] = 1
    generic = BounceBatch(wide, n)
    big = [np.full(n * 8 * 72 * 3, -5, dtype=np.int32), np.full(n * 8 * 72, -5, dtype=np.int32), np.full(n, -5, dtype=np.int32)]
    assert call(generic._handle, 1, 200, 100, U, *[ctypes.c_void_p(o.ctypes.data) for o in big], 0) == _abi.BGS_ERR_ARG
    assert "bit-packed" in _abi.last_error() and all((o == -5).all() for o in big)
    # n * S * budget beyond int64
    flat = np.zeros((3, 21), dtype=np.int8)                        # S = 21 * 3 * 21 = 1323
    flat[1, 0] = 1
    huge = BounceBatch(flat, 1 << 22)                              # 2^22 x 1323 x (2^31 - 1) > 2^63
    assert call(huge._handle, 1, 2**31 - 1, 100, U, *ptr, 0) == _abi.BGS_ERR_ARG
    assert "overflows" in _abi.last_error() and all((o == -5).all() for o in outs)
    huge.close()
    # misaligned device pointers, each in turn
    dev = [torch.full((o.size + 4,), -5, dtype=torch.int32, device="cuda:0") for o in outs]
    for bad in range(3):
        at = [ctypes.c_void_p(d.data_ptr() + (4 if j == bad else 0)) for j, d in enumerate(dev)]
        assert call(b._handle, 1, 200, 100, U, *at, 1) == _abi.BGS_ERR_ARG
        assert "aligned" in _abi.last_error()
    torch.cuda.synchronize()
    assert all(bool((d == -5).all()) for d in dev)
    # the Python layer
    with pytest.raises(ValueError, match="policy"):
        b.evaluate_moves_halving(policy="greedy")
    with pytest.raises(ValueError, match="policy"):
        b.evaluate_moves_halving_tensor(policy="greedy")
    with pytest.raises(ValueError, match="budget"):
        b.evaluate_moves_halving(budget=0)
    with pytest.raises(ValueError, match="max_plies"):
        b.evaluate_moves_halving(budget=200, max_plies=0)


# ---- the agent
def _states(config, count, seed):
    states = [config.sample_initial_state()]
    rng = np.random.default_rng(seed)
    while len(states) < count:
        s = states[-1]
        for _ in range(int(rng.integers(1, 4))):
            if s.has_ended:
                break
            acts = s.actions
            s = acts[int(rng.integers(len(acts)))].sample_next_state()
        states.append(config.sample_initial_state() if s.has_ended else s)
    return states


@pytest.mark.parametrize("policy", ["uniform", "decisive"])
def test_halving_agent_equals_the_batch_call(policy):
    from simulator.agents import BOUNCE_MAX_PLIES, BounceHalvingAgent
    from simulator.game.bounce import Config
    from simulator.game.connect import Config as ConnectConfig

    grid = bh.GRIDS["default"]
    states = _states(Config(grid), 6, seed=3)
    budget = 512
    agent = BounceHalvingAgent(budget=budget, seed=SEED, policy=policy)
    many = agent.predict_many(states, first_game=4)
    chosen = agent.choose_many(states, first_game=4)
    roots = (np.stack([s.grid for s in states]), np.array([s.player for s in states], np.int8),
             np.full(len(states), -1, np.int8), np.array([s._plies for s in states], np.int32))
    b = load(grid, roots, first_game=4)
    counts, given, best = b.evaluate_moves_halving(seed=SEED, budget=budget, max_plies=BOUNCE_MAX_PLIES, policy=policy)
    for k, (s, m) in enumerate(zip(states, many)):
        assert list(m) == s.actions
        for a in s.actions:
            (sx, _), (tx, ty) = a._source, a._target
            wdl, g = counts[k, sx, ty * 6 + tx], given[k, sx, ty * 6 + tx]
            assert g > 0 and m[a] == (wdl[0] + 0.5 * wdl[1]) / g
        assert agent.predict(s, game=4 + k) == m
        (sx, _), (tx, ty) = chosen[k]._source, chosen[k]._target
        assert sx * 54 + ty * 6 + tx == best[k] and chosen[k] in s.actions
        assert agent.choose(s, game=4 + k) == chosen[k]
    agent.close()
    b.close()
    # a budget too small for a state: the error names the budget it needs
    small = BounceHalvingAgent(budget=20, seed=SEED, policy=policy)
    need = b.halving_min_budget(len(states[0].actions))
    for method in (small.predict, small.choose):
        with pytest.raises(ValueError, match=str(need)):
            method(states[0])
    with pytest.raises(ValueError, match="allocation"):
        small.predict(ConnectConfig(6, 7, 4).sample_initial_state())
    small.close()
