"""The batched UCT tree search (bgs_connect_search_actions, ConnectBatch.search_actions, TreeSearchAgent) against the CPU
statement of tests/search_expected.py: counts, visits, best, nodes and the bgs_steps delta bit for bit.
tests/test_search_expected.py states what the case table holds.

Everything here needs a real MI355X: `pytest -m gpu`.
"""

import ctypes

import numpy as np
import pytest

from tests import search_expected as se

pytestmark = pytest.mark.gpu

SEED = se.SEED
NAMES = ("counts", "visits", "best", "nodes")


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
    for name, g, w in zip(NAMES, got, want):
        np.testing.assert_array_equal(g, w, err_msg=f"{name} {what}")


def arguments(case, roots, policy="uniform"):
    return dict(seed=SEED, iterations=case.iterations, leaf_playouts=case.playouts, explore=case.explore,
                max_plies=se.case_max_plies(case, roots), policy=policy)


@pytest.mark.parametrize("run", se.RUNS, ids=se.run_id)
def test_counts_visits_best_nodes_and_steps_equal_the_reference(run):
    index, policy, per_ply = run
    case = se.CASES[index]
    roots = se.case_roots(case)
    b = load(case.h, case.w, case.k, roots, per_ply, case.first_game)
    before = snapshot(b)
    got = b.search_actions(**arguments(case, roots, policy))
    counts, visits, best, nodes, steps, seen = se.case_expected(index, per_ply, policy)
    tallies = {key: value for key, value in seen.items() if isinstance(value, int)}
    print(f"{case} {policy} per_ply={per_ply}: steps {b.steps} / {steps}, {tallies}, capped playouts {int(seen['capped'].sum())}, "
          f"roots whose best differs {int((got[2] != best).sum())} of {best.size}")
    assert_equal(got, (counts, visits, best, nodes), str(case))
    assert b.steps == steps, case
    assert snapshot(b) == before, case     # planes, status and plies are unchanged
    b.close()


@pytest.mark.parametrize("index", [0, 10], ids=lambda j: se.case_id(se.CASES[j]))
def test_two_shards_equal_the_whole_batch(index):
    case = se.CASES[index]
    h, w, k = case.h, case.w, case.k
    roots = se.case_roots(case)
    cut = roots[0].shape[0] // 2
    kw = arguments(case, roots, "decisive")
    whole = load(h, w, k, roots, first_game=100).search_actions(**kw)
    lo = load(h, w, k, tuple(a[:cut] for a in roots), first_game=100).search_actions(**kw)
    hi = load(h, w, k, tuple(a[cut:] for a in roots), first_game=100 + cut).search_actions(**kw)
    assert_equal(tuple(np.concatenate([x, y]) for x, y in zip(lo, hi)), whole)


@pytest.mark.parametrize("policy", ["uniform", "decisive"])
def test_device_outputs_a_reused_workspace_and_null_outputs(policy):
    import torch

    from simulator.batch import playout_policy
    from simulator.game import _abi

    case = se.CASES[0]
    roots = se.case_roots(case)
    n, w = roots[0].shape[0], case.w
    kw = arguments(case, roots, policy)
    want = se.case_expected(0, False, policy)
    b = load(case.h, case.w, case.k, roots, use_torch=True, first_game=case.first_game)
    host = b.search_actions(**kw)                  # workspace = NULL: the library's own
    assert_equal(host, want[:4])
    steps = b.steps
    assert steps == want[4]
    # the device variant with a caller's workspace, filled with rubbish: the kernel resets its tree
    need = b.search_workspace_bytes(case.iterations)
    assert need % 256 == 0 and need >= n * (case.iterations + 1) * w * 12
    workspace = torch.full((need,), 0xA5, dtype=torch.uint8, device="cuda:0")
    outs = [torch.full(shape, -7, dtype=torch.int32, device="cuda:0") for shape in ((n, w, 3), (n, w), (n,), (n,))]
    b.reset_steps()
    got = b.search_actions_tensor(*outs, workspace=workspace, **kw)
    assert all(g is o for g, o in zip(got, outs))
    torch.cuda.synchronize()
    assert_equal(tuple(g.cpu().numpy() for g in got), host)
    assert b.steps == steps
    # a second call on the same batch and workspace gives the same outputs
    again = b.search_actions_tensor(workspace=workspace, **kw)
    torch.cuda.synchronize()
    assert_equal(tuple(g.cpu().numpy() for g in again), host)
    # the batch's own cached workspace
    fresh = b.search_actions_tensor(**kw)
    assert list(b._search_workspaces) == [case.iterations]
    torch.cuda.synchronize()
    assert_equal(tuple(g.cpu().numpy() for g in fresh), host)
    # a stream other than the null stream
    stream = torch.cuda.Stream()
    b.set_stream(stream.cuda_stream)
    streamed = b.search_actions_tensor(workspace=workspace, **kw)
    stream.synchronize()
    assert_equal(tuple(g.cpu().numpy() for g in streamed), host)
    b.set_stream(0)
    # visits, best and nodes may be NULL, on the host and on the device; the host variant takes a caller's workspace too
    call = _abi.lib().bgs_connect_search_actions
    head = (b._handle, SEED, case.iterations, case.playouts, case.explore, kw["max_plies"], playout_policy(policy))
    counts = np.full((n, w, 3), -1, dtype=np.int32)
    _abi.check(call(*head, ctypes.c_void_p(counts.ctypes.data), None, None, None, None, 0, 0))
    np.testing.assert_array_equal(counts, host[0])
    counts[:] = -1
    _abi.check(call(*head, ctypes.c_void_p(counts.ctypes.data), None, None, None, ctypes.c_void_p(workspace.data_ptr()), need, 0))
    np.testing.assert_array_equal(counts, host[0])
    only = torch.full((n, w, 3), -7, dtype=torch.int32, device="cuda:0")
    _abi.check(call(*head, ctypes.c_void_p(only.data_ptr()), None, None, None, ctypes.c_void_p(workspace.data_ptr()), need, 1))
    torch.cuda.synchronize()
    np.testing.assert_array_equal(only.cpu().numpy(), host[0])
    # a workspace one byte short is refused
    assert call(*head, ctypes.c_void_p(only.data_ptr()), None, None, None, ctypes.c_void_p(workspace.data_ptr()), need - 1, 1) == _abi.BGS_ERR_ARG
    assert "workspace" in _abi.last_error()
    with pytest.raises(ValueError, match="workspace"):
        b.search_actions_tensor(workspace=workspace[:-1], **kw)
    b.close()


def test_refusals_return_err_arg_and_leave_the_outputs_untouched():
    import torch

    from simulator.batch import BounceBatch, ConnectBatch
    from simulator.game import _abi

    call = _abi.lib().bgs_connect_search_actions
    U = _abi.POLICY_UNIFORM
    n, w = 4, 7
    b = ConnectBatch(6, w, 4, n)
    outs = [np.full(n * w * 3, -5, dtype=np.int32), np.full(n * w, -5, dtype=np.int32), np.full(n, -5, dtype=np.int32),
            np.full(n, -5, dtype=np.int32)]
    ptr = [ctypes.c_void_p(o.ctypes.data) for o in outs]
    tail = (None, 0, 0)

    def refused(word, *args):
        assert call(*args) == _abi.BGS_ERR_ARG
        assert word in _abi.last_error(), _abi.last_error()
        assert all((o == -5).all() for o in outs)

    # (handle, seed, iterations, leaf_playouts, explore, max_plies, policy, ...)
    refused("iterations", b._handle, 1, 0, 8, 65536, 100, U, *ptr, *tail)
    refused("iterations", b._handle, 1, -2, 8, 65536, 100, U, *ptr, *tail)
    refused("leaf_playouts", b._handle, 1, 8, 0, 65536, 100, U, *ptr, *tail)
    refused("2^29", b._handle, 1, 1 << 15, (1 << 14) + 1, 65536, 100, U, *ptr, *tail)
    refused("explore", b._handle, 1, 8, 8, -1, 100, U, *ptr, *tail)
    refused("explore", b._handle, 1, 8, 8, (1 << 18) + 1, 100, U, *ptr, *tail)
    refused("max_plies", b._handle, 1, 8, 8, 65536, 0, U, *ptr, *tail)
    for policy in (2, -1, 99):
        refused("policy", b._handle, 1, 8, 8, 65536, 100, policy, *ptr, *tail)
    refused("counts", b._handle, 1, 8, 8, 65536, 100, U, None, *ptr[1:], *tail)
    size = ctypes.c_size_t(77)
    assert _abi.lib().bgs_connect_search_workspace_bytes(b._handle, 0, ctypes.byref(size)) == _abi.BGS_ERR_ARG
    assert "iterations" in _abi.last_error() and size.value == 77
    assert call(b._handle, 1, 1, 1, 0, 1, U, *ptr, *tail) == _abi.BGS_OK       # the least of everything is taken
    assert call(b._handle, 1, 2, 2, 1 << 18, 1, U, *ptr, *tail) == _abi.BGS_OK
    for o in outs:
        o[:] = -5
    # Bounce and generic batches
    grid = np.zeros((9, 6), dtype=np.int8)
    grid[1] = grid[7] = [1, 2, 3, 3, 2, 1]
    bounce = BounceBatch(grid, 4)
    refused("Connect", bounce._handle, 1, 8, 8, 65536, 100, U, *ptr, *tail)
    assert _abi.lib().bgs_connect_search_workspace_bytes(bounce._handle, 8, ctypes.byref(size)) == _abi.BGS_ERR_ARG
    for method in (bounce.search_actions, bounce.search_actions_tensor, bounce.search_workspace_bytes):
        with pytest.raises(ValueError, match="Connect"):
            method(iterations=8)
    generic = ConnectBatch(20, 20, 5, 4)
    big = [np.full(4 * 20 * 3, -5, dtype=np.int32), np.full(4 * 20, -5, dtype=np.int32), np.full(4, -5, dtype=np.int32),
           np.full(4, -5, dtype=np.int32)]
    assert call(generic._handle, 1, 8, 8, 65536, 100, U, *[ctypes.c_void_p(o.ctypes.data) for o in big], *tail) == _abi.BGS_ERR_ARG
    assert "bit-packed" in _abi.last_error() and all((o == -5).all() for o in big)
    # (n * T * P beyond int64 takes 2^34 boards at T * P <= 2^29, more than a device holds: that refusal is not reached here)
    # misaligned device pointers, each in turn; a NULL, misaligned or short workspace
    need = b.search_workspace_bytes(8)
    workspace = torch.zeros(need + 256, dtype=torch.uint8, device="cuda:0")
    dev = [torch.full((o.size + 4,), -5, dtype=torch.int32, device="cuda:0") for o in outs]
    for bad in range(4):
        at = [ctypes.c_void_p(d.data_ptr() + (4 if j == bad else 0)) for j, d in enumerate(dev)]
        assert call(b._handle, 1, 8, 8, 65536, 100, U, *at, ctypes.c_void_p(workspace.data_ptr()), need, 1) == _abi.BGS_ERR_ARG
        assert "aligned" in _abi.last_error()
    at = [ctypes.c_void_p(d.data_ptr()) for d in dev]
    assert call(b._handle, 1, 8, 8, 65536, 100, U, *at, None, 0, 1) == _abi.BGS_ERR_ARG
    assert "workspace" in _abi.last_error()
    assert call(b._handle, 1, 8, 8, 65536, 100, U, *at, ctypes.c_void_p(workspace.data_ptr() + 64), need, 1) == _abi.BGS_ERR_ARG
    assert "256-byte" in _abi.last_error()
    assert call(b._handle, 1, 8, 8, 65536, 100, U, *at, ctypes.c_void_p(workspace.data_ptr()), need - 1, 1) == _abi.BGS_ERR_ARG
    assert "too small" in _abi.last_error()
    assert call(b._handle, 1, 9, 8, 65536, 100, U, *at, ctypes.c_void_p(workspace.data_ptr()), need, 1) == _abi.BGS_ERR_ARG
    assert "too small" in _abi.last_error()          # (sized for 8 iterations, asked for 9)
    torch.cuda.synchronize()
    assert all(bool((d == -5).all()) for d in dev)
    # the Python layer
    with pytest.raises(ValueError, match="policy"):
        b.search_actions(policy="greedy")
    with pytest.raises(ValueError, match="policy"):
        b.search_actions_tensor(policy="greedy")
    with pytest.raises(ValueError, match="iterations"):
        b.search_actions(iterations=0)
    with pytest.raises(ValueError, match="iterations"):
        b.search_actions_tensor(iterations=0)
    with pytest.raises(ValueError, match="explore"):
        b.search_actions(explore=1 << 19)
    for batch in (b, bounce, generic):
        batch.close()


# ---- the agent
def _state_after(columns, config=(6, 7, 4)):
    from simulator.game.connect import Config

    s = Config(*config).sample_initial_state()
    for c in columns:
        s = s.action_at(c).sample_next_state()
    return s


@pytest.mark.parametrize("policy", ["uniform", "decisive"])
def test_tree_search_agent_equals_the_batch_call(policy):
    from simulator.agents import TreeSearchAgent
    from simulator.batch import ConnectBatch
    from simulator.game import bounce

    agent = TreeSearchAgent(iterations=32, leaf_playouts=16, explore=40000, policy=policy, seed=SEED)
    states = [_state_after(cs) for cs in ([], [3], [3, 3, 2], [0, 1, 0, 1, 0, 1], [3, 3, 3, 3, 3, 3, 2], [0, 3, 0, 3, 1, 3])]
    many = agent.predict_many(states, first_game=4)
    chosen = agent.choose_many(states, first_game=4)
    b = ConnectBatch(6, 7, 4, len(states))
    grid = np.stack([s.grid for s in states])
    player = np.array([s.player for s in states], dtype=np.int8)
    assert (b.write_state(grid, player, np.full(len(states), -1, dtype=np.int8)) == 0).all()
    b.set_first_game(4)
    counts, visits, best, nodes = b.search_actions(seed=SEED, iterations=32, leaf_playouts=16, explore=40000, policy=policy)
    for g, (s, m) in enumerate(zip(states, many)):
        assert list(m) == s.actions
        assert m == {a: float(visits[g, a.column]) / 512 for a in s.actions}
        assert abs(sum(m.values()) - 1.0) < 1e-12
        assert agent.predict(s, game=4 + g) == m
        assert chosen[g].column == best[g]
        assert agent.choose(s, game=4 + g).column == best[g]
    assert chosen[3].column == 0                                  # the column that wins at once
    grid = np.zeros((9, 6), dtype=np.int8)
    grid[1] = grid[7] = [1, 2, 3, 3, 2, 1]
    start = bounce.Config(grid).sample_initial_state()
    for method in (agent.predict, agent.choose):
        with pytest.raises(ValueError, match="Bounce"):
            method(start)
    agent.close()
    with pytest.raises(ValueError, match="explore"):
        TreeSearchAgent(explore=-1)
    with pytest.raises(ValueError, match="iterations"):
        TreeSearchAgent(iterations=0)
