"""Sequential-halving Monte-Carlo evaluation (bgs_connect_evaluate_actions_halving,
ConnectBatch.evaluate_actions_halving, MonteCarloAgent(allocation="halving")) against the CPU statement of
tests/halving_expected.py: counts, given, best and the bgs_steps delta bit for bit.  tests/test_halving_expected.py states
what the case table holds.

Everything here needs a real MI355X: `pytest -m gpu`.
"""

import ctypes

import numpy as np
import pytest

from tests import halving_expected as he

pytestmark = pytest.mark.gpu

SEED = he.SEED
RUNS = [(j, "uniform") for j in range(len(he.CASES))] + [(j, "decisive") for j in he.DECISIVE]


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


def assert_equal(got, want, what=""):
    for name, g, w in zip(("counts", "given", "best"), got, want):
        np.testing.assert_array_equal(g, w, err_msg=f"{name} {what}")


@pytest.mark.parametrize("index,policy", RUNS, ids=[f"{he.case_id(he.CASES[j])}-{p}" for j, p in RUNS])
@pytest.mark.parametrize("per_ply", [False, True], ids=["per-block", "per-ply"])
def test_counts_given_best_and_steps_equal_the_reference(index, policy, per_ply):
    case = he.CASES[index]
    roots = he.case_roots(case)
    max_plies = he.case_max_plies(case, roots)
    b = load(case.h, case.w, case.k, roots, per_ply, case.first_game)
    before = snapshot(b)
    got = b.evaluate_actions_halving(seed=SEED, budget=case.budget, max_plies=max_plies, policy=policy)
    counts, given, best, steps, seen = he.case_expected(index, per_ply, policy)
    print(f"{case} {policy} per_ply={per_ply}: steps {b.steps} / {steps}, selections {seen}, "
          f"roots whose best differs {int((got[2] != best).sum())} of {best.size}")
    assert_equal(got, (counts, given, best), str(case))
    assert b.steps == steps, case
    assert snapshot(b) == before, case     # planes, status and plies are unchanged
    b.close()


@pytest.mark.parametrize("index", [0, 4], ids=lambda j: he.case_id(he.CASES[j]))
def test_a_cap_one_ply_past_the_root_leaves_the_column_order_to_decide(index):
    """max_plies = root plies + 1: every playout that its first move does not end is capped at once and scores 0"""
    from tests.policy_expected import completes

    case = he.CASES[index]
    roots = he.case_roots(case)
    # the running roots of one ply count whose first moves end nothing: no winning column, more than one empty cell
    quiet = (roots[2] == -1) & ~completes(roots[0], roots[1].astype(np.int64), case.k).any(axis=1)
    quiet &= (roots[0] < 0).sum(axis=(1, 2)) > 1
    at = np.bincount(roots[3][quiet]).argmax()
    rows = np.flatnonzero(quiet & (roots[3] == at))
    assert rows.size >= 1
    picked = tuple(a[rows] for a in roots)
    b = load(case.h, case.w, case.k, picked)
    counts, given, best = b.evaluate_actions_halving(seed=SEED, budget=case.budget, max_plies=int(at) + 1)
    legal = he.legal_columns(case.h, case.w, case.k, picked)
    assert (counts == 0).all()
    for i in range(rows.size):
        cols = np.flatnonzero(legal[i])
        want = np.zeros(case.w, dtype=np.int32)
        for m, q in he.schedule(cols.size, case.budget):
            want[cols[:m]] += q             # all scores are 0: the m lowest columns survive
        np.testing.assert_array_equal(given[i], want)
        assert best[i] == cols[0]
    assert b.steps == int(given.sum())     # the first moves alone


@pytest.mark.parametrize("h,w,k,budget,roots_kept", [(6, 7, 4, 1600, 4), (6, 12, 4, 2100, 2)], ids=["6x7x4", "6x12x4"])
def test_the_workgroup_team_and_the_wave_team_give_the_reference(h, w, k, budget, roots_kept):
    """a round of more than 512 playouts goes to a 256-lane team, fewer to one wave: both are the helper's answer"""
    assert budget // he.rounds(w) > 512 >= he.min_budget(w) * 2 // he.rounds(w)
    mixed = he._case_roots(h, w, k)
    legal = he.legal_columns(h, w, k, mixed)
    rows = np.flatnonzero(legal.sum(axis=1) == w)[1:roots_kept].tolist() + [int(np.flatnonzero(legal.sum(axis=1) == 3)[0])]
    roots = tuple(a[rows] for a in mixed)
    for b_ in (budget, he.min_budget(w) * 2):
        b = load(h, w, k, roots, first_game=3)
        got = b.evaluate_actions_halving(seed=SEED, budget=b_)
        counts, given, best, steps, _ = he.halving_expected(h, w, k, roots, SEED, 3, b_, he.UNCAPPED, False)
        assert_equal(got, (counts, given, best), f"budget {b_}")
        assert b.steps == steps
        b.close()


@pytest.mark.parametrize("index", [0, 5], ids=lambda j: he.case_id(he.CASES[j]))
def test_two_shards_equal_the_whole_batch(index):
    case = he.CASES[index]
    h, w, k = case.h, case.w, case.k
    roots = he.case_roots(case)
    cut = roots[0].shape[0] // 2
    kw = dict(seed=SEED, budget=case.budget, policy="decisive")
    whole = load(h, w, k, roots, first_game=100).evaluate_actions_halving(**kw)
    lo = load(h, w, k, tuple(a[:cut] for a in roots), first_game=100).evaluate_actions_halving(**kw)
    hi = load(h, w, k, tuple(a[cut:] for a in roots), first_game=100 + cut).evaluate_actions_halving(**kw)
    assert_equal(tuple(np.concatenate([x, y]) for x, y in zip(lo, hi)), whole)


@pytest.mark.parametrize("policy", ["uniform", "decisive"])
def test_device_outputs_equal_host_outputs(policy):
    import torch

    case = he.CASES[0]
    roots = he.case_roots(case)
    n = roots[0].shape[0]
    b = load(case.h, case.w, case.k, roots, use_torch=True, first_game=case.first_game)
    host = b.evaluate_actions_halving(seed=SEED, budget=case.budget, policy=policy)
    steps = b.steps
    b.reset_steps()
    outs = [torch.full(shape, -7, dtype=torch.int32, device="cuda:0") for shape in ((n, case.w, 3), (n, case.w), (n,))]
    got = b.evaluate_actions_halving_tensor(*outs, seed=SEED, budget=case.budget, policy=policy)
    assert all(g is o for g, o in zip(got, outs))
    torch.cuda.synchronize()
    assert_equal(tuple(g.cpu().numpy() for g in got), host)
    assert b.steps == steps
    assert_equal(host, he.case_expected(0, False, policy)[:3])
    fresh = b.evaluate_actions_halving_tensor(seed=SEED, budget=case.budget, policy=policy)
    torch.cuda.synchronize()
    assert_equal(tuple(g.cpu().numpy() for g in fresh), host)
    # given and best may be NULL
    from simulator.batch import playout_policy
    from simulator.game import _abi

    code = playout_policy(policy)
    counts = np.full((n, case.w, 3), -1, dtype=np.int32)
    _abi.check(_abi.lib().bgs_connect_evaluate_actions_halving(
        b._handle, SEED, case.budget, he.UNCAPPED, code, ctypes.c_void_p(counts.ctypes.data), None, None, 0))
    np.testing.assert_array_equal(counts, host[0])
    only = torch.full((n, case.w, 3), -7, dtype=torch.int32, device="cuda:0")
    _abi.check(_abi.lib().bgs_connect_evaluate_actions_halving(
        b._handle, SEED, case.budget, he.UNCAPPED, code, ctypes.c_void_p(only.data_ptr()), None, None, 1))
    torch.cuda.synchronize()
    np.testing.assert_array_equal(only.cpu().numpy(), host[0])


@pytest.mark.parametrize("per_ply", [False, True], ids=["per-block", "per-ply"])
def test_one_legal_column_is_the_flat_evaluation_of_that_column(per_ply):
    case = he.CASES[0]
    mixed = he.case_roots(case)
    legal = he.legal_columns(case.h, case.w, case.k, mixed)
    rows = np.flatnonzero(legal.sum(axis=1) == 1)
    assert rows.size
    roots = tuple(a[rows] for a in mixed)
    b = load(case.h, case.w, case.k, roots, per_ply, first_game=17)
    counts, given, best = b.evaluate_actions_halving(seed=SEED, budget=case.budget)
    steps = b.steps
    b.reset_steps()
    flat = b.evaluate_actions(seed=SEED, playouts=case.budget)
    np.testing.assert_array_equal(counts, flat)
    assert b.steps == steps
    np.testing.assert_array_equal(best, legal[rows].argmax(axis=1))
    np.testing.assert_array_equal(given, legal[rows] * case.budget)


# ---- refusals
def test_refusals_return_err_arg_and_leave_the_outputs_untouched():
    import torch

    from simulator.batch import BounceBatch, ConnectBatch
    from simulator.game import _abi

    call = _abi.lib().bgs_connect_evaluate_actions_halving
    U = _abi.POLICY_UNIFORM
    n, w = 4, 7
    b = ConnectBatch(6, w, 4, n)
    outs = [np.full(n * w * 3, -5, dtype=np.int32), np.full(n * w, -5, dtype=np.int32), np.full(n, -5, dtype=np.int32)]
    ptr = [ctypes.c_void_p(o.ctypes.data) for o in outs]

    def refused(word, *args):
        assert call(*args) == _abi.BGS_ERR_ARG
        assert word in _abi.last_error(), _abi.last_error()
        assert all((o == -5).all() for o in outs)

    assert he.min_budget(w) == 21 == b.halving_min_budget()
    refused("budget", b._handle, 1, 20, 100, U, *ptr, 0)
    refused("budget", b._handle, 1, 0, 100, U, *ptr, 0)
    refused("budget", b._handle, 1, -3, 100, U, *ptr, 0)
    refused("max_plies", b._handle, 1, 21, 0, U, *ptr, 0)
    for policy in (2, -1, 99):
        refused("policy", b._handle, 1, 100, 100, policy, *ptr, 0)
    refused("counts", b._handle, 1, 100, 100, U, None, ptr[1], ptr[2], 0)
    assert call(b._handle, 1, 21, 1, U, *ptr, 0) == _abi.BGS_OK       # the least budget and the least cap are taken
    for o in outs:
        o[:] = -5
    # Bounce and generic batches
    grid = np.zeros((9, 6), dtype=np.int8)
    grid[1] = grid[7] = [1, 2, 3, 3, 2, 1]
    bounce = BounceBatch(grid, 4)
    refused("Connect", bounce._handle, 1, 100, 100, U, *ptr, 0)
    for method in (bounce.evaluate_actions_halving, bounce.evaluate_actions_halving_tensor):
        with pytest.raises(ValueError, match="Connect"):
            method(budget=100)
    generic = ConnectBatch(20, 20, 5, 4)
    big = [np.full(4 * 20 * 3, -5, dtype=np.int32), np.full(4 * 20, -5, dtype=np.int32), np.full(4, -5, dtype=np.int32)]
    assert call(generic._handle, 1, 200, 100, U, *[ctypes.c_void_p(o.ctypes.data) for o in big], 0) == _abi.BGS_ERR_ARG
    assert "bit-packed" in _abi.last_error() and all((o == -5).all() for o in big)
    # n * width * budget beyond int64
    huge = ConnectBatch(1, 16, 2, (1 << 28) + 1)       # (2^28 + 1) boards x 16 columns x (2^31 - 1) playouts > 2^63
    assert call(huge._handle, 1, 2**31 - 1, 100, U, *ptr, 0) == _abi.BGS_ERR_ARG
    assert "overflows" in _abi.last_error() and all((o == -5).all() for o in outs)
    huge.close()
    # misaligned device pointers, each in turn
    dev = [torch.full((o.size + 4,), -5, dtype=torch.int32, device="cuda:0") for o in outs]
    for bad in range(3):
        at = [ctypes.c_void_p(d.data_ptr() + (4 if j == bad else 0)) for j, d in enumerate(dev)]
        assert call(b._handle, 1, 100, 100, U, *at, 1) == _abi.BGS_ERR_ARG
        assert "aligned" in _abi.last_error()
    torch.cuda.synchronize()
    assert all(bool((d == -5).all()) for d in dev)
    # the Python layer
    with pytest.raises(ValueError, match="policy"):
        b.evaluate_actions_halving(policy="greedy")
    with pytest.raises(ValueError, match="policy"):
        b.evaluate_actions_halving_tensor(policy="greedy")
    with pytest.raises(ValueError, match="budget"):
        b.evaluate_actions_halving(budget=20)
    with pytest.raises(ValueError, match="max_plies"):
        b.evaluate_actions_halving(budget=100, max_plies=0)


# ---- the agent
def _state_after(columns, config=(6, 7, 4)):
    from simulator.game.connect import Config

    s = Config(*config).sample_initial_state()
    for c in columns:
        s = s.action_at(c).sample_next_state()
    return s


@pytest.mark.parametrize("policy", ["uniform", "decisive"])
def test_halving_agent_equals_the_batch_call(policy):
    from simulator.agents import MonteCarloAgent
    from simulator.batch import ConnectBatch
    from simulator.game import bounce

    agent = MonteCarloAgent(playouts=64, seed=SEED, policy=policy, allocation="halving")
    states = [_state_after(cs) for cs in ([], [3], [3, 3, 2], [0, 1, 0, 1, 0, 1], [3, 3, 3, 3, 3, 3, 2], [0, 3, 0, 3, 1, 3])]
    many = agent.predict_many(states, first_game=4)
    chosen = agent.choose_many(states, first_game=4)
    b = ConnectBatch(6, 7, 4, len(states))
    grid = np.stack([s.grid for s in states])
    player = np.array([s.player for s in states], dtype=np.int8)
    assert (b.write_state(grid, player, np.full(len(states), -1, dtype=np.int8)) == 0).all()
    b.set_first_game(4)
    counts, given, best = b.evaluate_actions_halving(seed=SEED, budget=64 * 7, policy=policy)
    for g, (s, m) in enumerate(zip(states, many)):
        assert list(m) == s.actions
        assert m == {a: float((counts[g, a.column, 0] + 0.5 * counts[g, a.column, 1]) / given[g, a.column]) for a in s.actions}
        assert agent.predict(s, game=4 + g) == m
        assert chosen[g].column == best[g]
        assert agent.choose(s, game=4 + g).column == best[g]
    assert chosen[3].column == 0                                  # the column that wins at once
    # budget= overrides playouts * width
    small = MonteCarloAgent(playouts=64, seed=SEED, policy=policy, allocation="halving", budget=100)
    b.set_first_game(0)
    c2, g2, best2 = b.evaluate_actions_halving(seed=SEED, budget=100, policy=policy)
    assert [a.column for a in small.choose_many(states)] == best2.tolist()
    small.close()
    # the flat agent chooses its best-valued action, the first on ties
    flat = MonteCarloAgent(playouts=64, seed=SEED, policy=policy)
    values = flat.predict_many(states, first_game=4)
    for s, v, a in zip(states, values, flat.choose_many(states, first_game=4)):
        top = max(v.values())
        assert a == next(x for x in s.actions if v[x] == top)
    assert flat.choose(states[3], game=7).column == 0
    flat.close()

    grid = np.zeros((9, 6), dtype=np.int8)
    grid[1] = grid[7] = [1, 2, 3, 3, 2, 1]
    start = bounce.Config(grid).sample_initial_state()
    for method in (agent.predict, agent.choose):
        with pytest.raises(ValueError, match="Bounce"):
            method(start)
    agent.close()
    with pytest.raises(ValueError, match="allocation"):
        MonteCarloAgent(allocation="thirds")
    with pytest.raises(ValueError, match="budget"):
        MonteCarloAgent(budget=100)
