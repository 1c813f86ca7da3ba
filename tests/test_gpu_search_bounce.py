"""The batched UCT tree search for Bounce (bgs_bounce_search_moves, BounceBatch.search_moves, BounceTreeSearchAgent)
against the CPU statement of tests/search_bounce_expected.py: counts, visits, best, nodes, used and the bgs_steps delta bit
for bit.  tests/test_search_bounce_expected.py states what the case table holds.

Every launch here is one workgroup a root over at most 24 roots; the CPU model, cached per case, is the slower side.

Everything here needs a real MI355X: `pytest -m gpu`.
"""

import ctypes
import functools

import numpy as np
import pytest

from tests import fuzz_cases as fc
from tests import search_bounce_expected as sb

pytestmark = pytest.mark.gpu

SEED = sb.SEED
NAMES = ("counts", "visits", "best", "nodes", "used")


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
    for name, g, w in zip(NAMES, got, want):
        np.testing.assert_array_equal(g, w, err_msg=f"{name} {what}")


def arguments(case, roots, policy="uniform"):
    return dict(seed=SEED, iterations=case.iterations, leaf_playouts=case.playouts, explore=case.explore,
                max_plies=sb.case_max_plies(case, roots), policy=policy, edges=sb.case_edges(case))


@pytest.mark.parametrize("name,policy", sb.RUNS, ids=[f"{n}-{p}" for n, p in sb.RUNS])
def test_outputs_and_steps_equal_the_reference(name, policy):
    case = sb.BY_NAME[name]
    grid, roots = sb.case_grid(case), sb.case_roots(case)
    b = load(grid, roots, case.first_game)
    before = snapshot(b)
    kw = arguments(case, roots, policy)
    got = b.search_moves(**kw)
    got_steps = b.steps
    *want, steps, seen = sb.case_expected(name, policy)
    tallies = {key: value for key, value in seen.items() if isinstance(value, int)}
    print(f"{name} {policy}: steps {got_steps} / {steps}, {tallies}, capped playouts {int(seen['capped'].sum())}, "
          f"roots whose best differs {int((got[2] != want[2]).sum())} of {want[2].size}")
    assert_equal(got, want, name)
    assert got_steps == steps, name
    assert snapshot(b) == before, name        # planes, status and plies are unchanged
    if case.edges is None:                    # edges=None is the default pool
        b.reset_steps()
        del kw["edges"]
        assert_equal(b.search_moves(**kw), want, f"{name}, edges=None")
        assert b.steps == steps
    b.close()


@pytest.mark.parametrize("name", ["default", "tall_wide"])
def test_two_shards_equal_the_whole_batch(name):
    case = sb.BY_NAME[name]
    grid, roots = sb.case_grid(case), sb.case_roots(case)
    cut = roots[0].shape[0] // 2
    kw = arguments(case, roots, "decisive")
    whole = load(grid, roots, first_game=100).search_moves(**kw)
    lo = load(grid, tuple(a[:cut] for a in roots), first_game=100).search_moves(**kw)
    hi = load(grid, tuple(a[cut:] for a in roots), first_game=100 + cut).search_moves(**kw)
    assert_equal(tuple(np.concatenate([x, y]) for x, y in zip(lo, hi)), whole)
    assert whole[0].any()


@pytest.mark.parametrize("policy", ["uniform", "decisive"])
def test_device_outputs_a_reused_workspace_and_null_outputs(policy):
    import torch

    from simulator.batch import playout_policy
    from simulator.game import _abi

    case = sb.BY_NAME["default"]
    grid, roots = sb.case_grid(case), sb.case_roots(case)
    h, w = grid.shape
    n, S = roots[0].shape[0], w * h * w
    kw = arguments(case, roots, policy)
    edges = kw["edges"]
    *want, want_steps, _ = sb.case_expected("default", policy)
    b = load(grid, roots, use_torch=True, first_game=case.first_game)
    host = b.search_moves(**kw)                    # workspace = NULL: the library's own
    assert_equal(host, want)
    steps = b.steps
    assert steps == want_steps
    # the device variant with a caller's workspace, filled with rubbish: the kernel resets its tree
    need = b.search_moves_workspace_bytes(case.iterations, edges)
    share = 16 * edges + 12 * (case.iterations + 1)
    assert need % 256 == 0 and need == n * ((share + 255) // 256 * 256)
    assert b.search_moves_workspace_bytes(case.iterations) == need         # edges=None: the default pool
    workspace = torch.full((need,), 0xA5, dtype=torch.uint8, device="cuda:0")
    shapes = ((n, w, h * w, 3), (n, w, h * w), (n,), (n,), (n,))
    outs = [torch.full(shape, -7, dtype=torch.int32, device="cuda:0") for shape in shapes]
    b.reset_steps()
    got = b.search_moves_tensor(*outs, workspace=workspace, **kw)
    assert all(g is o for g, o in zip(got, outs))
    torch.cuda.synchronize()
    assert_equal(tuple(g.cpu().numpy() for g in got), host)
    assert b.steps == steps
    # a second call on the same batch and workspace gives the same outputs
    again = b.search_moves_tensor(workspace=workspace, **kw)
    torch.cuda.synchronize()
    assert_equal(tuple(g.cpu().numpy() for g in again), host)
    # the batch's own cached workspace
    fresh = b.search_moves_tensor(**kw)
    assert list(b._search_workspaces) == [(case.iterations, edges)]
    torch.cuda.synchronize()
    assert_equal(tuple(g.cpu().numpy() for g in fresh), host)
    # a stream other than the null stream
    stream = torch.cuda.Stream()
    b.set_stream(stream.cuda_stream)
    streamed = b.search_moves_tensor(workspace=workspace, **kw)
    stream.synchronize()
    assert_equal(tuple(g.cpu().numpy() for g in streamed), host)
    b.set_stream(0)
    # visits, best, nodes and used may be NULL, on the host and on the device; the host variant takes a caller's workspace too
    call = _abi.lib().bgs_bounce_search_moves
    head = (b._handle, SEED, case.iterations, case.playouts, case.explore, kw["max_plies"], playout_policy(policy), edges)
    counts = np.full((n, w, h * w, 3), -1, dtype=np.int32)
    _abi.check(call(*head, ctypes.c_void_p(counts.ctypes.data), None, None, None, None, None, 0, 0))
    np.testing.assert_array_equal(counts, host[0])
    counts[:] = -1
    _abi.check(call(*head, ctypes.c_void_p(counts.ctypes.data), None, None, None, None, ctypes.c_void_p(workspace.data_ptr()), need, 0))
    np.testing.assert_array_equal(counts, host[0])
    only = torch.full((n, w, h * w, 3), -7, dtype=torch.int32, device="cuda:0")
    _abi.check(call(*head, ctypes.c_void_p(only.data_ptr()), None, None, None, None, ctypes.c_void_p(workspace.data_ptr()), need, 1))
    torch.cuda.synchronize()
    np.testing.assert_array_equal(only.cpu().numpy(), host[0])
    # a workspace one byte short is refused
    assert call(*head, ctypes.c_void_p(only.data_ptr()), None, None, None, None, ctypes.c_void_p(workspace.data_ptr()), need - 1,
                1) == _abi.BGS_ERR_ARG
    assert "workspace" in _abi.last_error()
    with pytest.raises(ValueError, match="workspace"):
        b.search_moves_tensor(workspace=workspace[:-1], **kw)
    b.close()


def test_refusals_return_err_arg_and_leave_the_outputs_untouched():
    import torch

    from simulator.batch import BounceBatch, ConnectBatch
    from simulator.game import _abi

    call = _abi.lib().bgs_bounce_search_moves
    U = _abi.POLICY_UNIFORM
    grid = sb.GRIDS["default"]
    h, w = grid.shape
    n, S, E = 4, w * h * w, sb.min_edges(h, w)
    assert E == 252
    b = BounceBatch(grid, n)
    outs = [np.full(n * S * 3, -5, dtype=np.int32), np.full(n * S, -5, dtype=np.int32)] + [np.full(n, -5, dtype=np.int32) for _ in range(3)]
    ptr = [ctypes.c_void_p(o.ctypes.data) for o in outs]
    tail = (None, 0, 0)

    def refused(word, *args):
        assert call(*args) == _abi.BGS_ERR_ARG
        assert word in _abi.last_error(), _abi.last_error()
        assert all((o == -5).all() for o in outs)

    # (handle, seed, iterations, leaf_playouts, explore, max_plies, policy, edges, ...)
    refused("iterations", b._handle, 1, 0, 8, 65536, 100, U, E, *ptr, *tail)
    refused("iterations", b._handle, 1, -2, 8, 65536, 100, U, E, *ptr, *tail)
    refused("leaf_playouts", b._handle, 1, 8, 0, 65536, 100, U, E, *ptr, *tail)
    refused("2^29", b._handle, 1, 1 << 15, (1 << 14) + 1, 65536, 100, U, E, *ptr, *tail)
    refused("explore", b._handle, 1, 8, 8, -1, 100, U, E, *ptr, *tail)
    refused("explore", b._handle, 1, 8, 8, (1 << 18) + 1, 100, U, E, *ptr, *tail)
    refused("max_plies", b._handle, 1, 8, 8, 65536, 0, U, E, *ptr, *tail)
    for policy in (2, -1, 99):
        refused("policy", b._handle, 1, 8, 8, 65536, 100, policy, E, *ptr, *tail)
    refused("edges", b._handle, 1, 8, 8, 65536, 100, U, E - 1, *ptr, *tail)
    refused("edges", b._handle, 1, 8, 8, 65536, 100, U, 0, *ptr, *tail)
    refused("edges", b._handle, 1, 8, 8, 65536, 100, U, -4, *ptr, *tail)
    refused("counts", b._handle, 1, 8, 8, 65536, 100, U, E, None, *ptr[1:], *tail)
    size = ctypes.c_size_t(77)
    sizes = _abi.lib().bgs_bounce_search_workspace_bytes
    assert sizes(b._handle, 0, E, ctypes.byref(size)) == _abi.BGS_ERR_ARG
    assert "iterations" in _abi.last_error() and size.value == 77
    assert sizes(b._handle, 8, E - 1, ctypes.byref(size)) == _abi.BGS_ERR_ARG
    assert "edges" in _abi.last_error() and size.value == 77
    assert call(b._handle, 1, 1, 1, 0, 1, U, E, *ptr, *tail) == _abi.BGS_OK       # the least of everything is taken
    assert call(b._handle, 1, 2, 2, 1 << 18, 1, U, E, *ptr, *tail) == _abi.BGS_OK
    for o in outs:
        o[:] = -5
    # Connect and generic batches
    connect = ConnectBatch(6, 7, 4, n)
    refused("Bounce", connect._handle, 1, 8, 8, 65536, 100, U, E, *ptr, *tail)
    assert sizes(connect._handle, 8, E, ctypes.byref(size)) == _abi.BGS_ERR_ARG and size.value == 77
    for method in (connect.search_moves, connect.search_moves_tensor, connect.search_moves_workspace_bytes):
        with pytest.raises(ValueError, match="Bounce"):
            method(iterations=8)
    wide = np.zeros((9, 8), dtype=np.int8)    # 72 cells: a generic board
    wide[1] = wide[7] = 1
    generic = BounceBatch(wide, n)
    big = [np.full(n * 8 * 72 * 3, -5, dtype=np.int32), np.full(n * 8 * 72, -5, dtype=np.int32)] + [np.full(n, -5, dtype=np.int32) for _ in range(3)]
    assert call(generic._handle, 1, 8, 8, 65536, 100, U, 8 * 8 * 7, *[ctypes.c_void_p(o.ctypes.data) for o in big], *tail) == _abi.BGS_ERR_ARG
    assert "bit-packed" in _abi.last_error() and all((o == -5).all() for o in big)
    # (n * T * P beyond int64 takes 2^34 boards at T * P <= 2^29, more than a device holds: that refusal is not reached here)
    # misaligned device pointers, each in turn; a NULL, misaligned or short workspace
    need = b.search_moves_workspace_bytes(8, E)
    workspace = torch.zeros(need + 256, dtype=torch.uint8, device="cuda:0")
    dev = [torch.full((o.size + 4,), -5, dtype=torch.int32, device="cuda:0") for o in outs]
    for bad in range(5):
        at = [ctypes.c_void_p(d.data_ptr() + (4 if j == bad else 0)) for j, d in enumerate(dev)]
        assert call(b._handle, 1, 8, 8, 65536, 100, U, E, *at, ctypes.c_void_p(workspace.data_ptr()), need, 1) == _abi.BGS_ERR_ARG
        assert "aligned" in _abi.last_error() and NAMES[bad] in _abi.last_error()
    at = [ctypes.c_void_p(d.data_ptr()) for d in dev]
    assert call(b._handle, 1, 8, 8, 65536, 100, U, E, *at, None, 0, 1) == _abi.BGS_ERR_ARG
    assert "workspace" in _abi.last_error()
    assert call(b._handle, 1, 8, 8, 65536, 100, U, E, *at, ctypes.c_void_p(workspace.data_ptr() + 64), need, 1) == _abi.BGS_ERR_ARG
    assert "256-byte" in _abi.last_error()
    assert call(b._handle, 1, 8, 8, 65536, 100, U, E, *at, ctypes.c_void_p(workspace.data_ptr()), need - 1, 1) == _abi.BGS_ERR_ARG
    assert "too small" in _abi.last_error()
    assert b.search_moves_workspace_bytes(40, E) > need     # (a root's share is rounded up to 256 bytes: 9 iterations would still fit)
    assert call(b._handle, 1, 40, 8, 65536, 100, U, E, *at, ctypes.c_void_p(workspace.data_ptr()), need, 1) == _abi.BGS_ERR_ARG
    assert "too small" in _abi.last_error()          # (sized for 8 iterations, asked for 40)
    assert b.search_moves_workspace_bytes(8, E + 16) > need
    assert call(b._handle, 1, 8, 8, 65536, 100, U, E + 16, *at, ctypes.c_void_p(workspace.data_ptr()), need, 1) == _abi.BGS_ERR_ARG
    assert "too small" in _abi.last_error()          # (sized for E edges, asked for E + 16)
    # ... and the host call with a caller's workspace that is misaligned or short
    refused("256-byte", b._handle, 1, 8, 8, 65536, 100, U, E, *ptr, ctypes.c_void_p(workspace.data_ptr() + 64), need, 0)
    refused("too small", b._handle, 1, 8, 8, 65536, 100, U, E, *ptr, ctypes.c_void_p(workspace.data_ptr()), need - 1, 0)
    torch.cuda.synchronize()
    assert all(bool((d == -5).all()) for d in dev)
    # the Python layer
    with pytest.raises(ValueError, match="policy"):
        b.search_moves(policy="greedy")
    with pytest.raises(ValueError, match="policy"):
        b.search_moves_tensor(policy="greedy")
    with pytest.raises(ValueError, match="iterations"):
        b.search_moves(iterations=0)
    with pytest.raises(ValueError, match="iterations"):
        b.search_moves_tensor(iterations=0)
    with pytest.raises(ValueError, match="explore"):
        b.search_moves(explore=1 << 19)
    with pytest.raises(ValueError, match="edges"):
        b.search_moves(edges=E - 1)
    with pytest.raises(ValueError, match="edges"):
        b.search_moves_workspace_bytes(8, edges=E - 1)
    for batch in (b, connect, generic):
        batch.close()


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
def test_tree_search_agent_equals_the_batch_call(policy):
    from simulator.agents import BOUNCE_MAX_PLIES, BounceTreeSearchAgent
    from simulator.game.bounce import Config
    from simulator.game.connect import Config as ConnectConfig

    grid = sb.GRIDS["default"]
    config = Config(grid)
    states = _states(config, 6, seed=3)
    T, P = 32, 16
    agent = BounceTreeSearchAgent(iterations=T, leaf_playouts=P, explore=40000, policy=policy, seed=SEED)
    many = agent.predict_many(states, first_game=4)
    chosen = agent.choose_many(states, first_game=4)
    roots = (np.stack([s.grid for s in states]), np.array([s.player for s in states], np.int8),
             np.full(len(states), -1, np.int8), np.array([s._plies for s in states], np.int32))
    b = load(grid, roots, first_game=4)
    counts, visits, best, nodes, used = b.search_moves(seed=SEED, iterations=T, leaf_playouts=P, explore=40000,
                                                       max_plies=BOUNCE_MAX_PLIES, policy=policy)
    for k, (s, m) in enumerate(zip(states, many)):
        assert list(m) == s.actions
        assert m == {a: float(visits[k, a._source[0], a._target[1] * 6 + a._target[0]]) / (T * P) for a in s.actions}
        assert abs(sum(m.values()) - 1.0) < 1e-12
        assert agent.predict(s, game=4 + k) == m
        (sx, _), (tx, ty) = chosen[k]._source, chosen[k]._target
        assert sx * 54 + ty * 6 + tx == best[k] and chosen[k] in s.actions
        assert agent.choose(s, game=4 + k) == chosen[k]
    b.close()
    # a position with a win in one, the search of tests/test_search_bounce_expected.py::test_a_move_into_the_goal_row_is_best
    from simulator.game.bounce import State
    from tests.test_search_bounce_expected import tactical_root

    _, (tg, tplayer, _, tplies), wins = tactical_root()
    tactical = State._fresh(config, *config._engine().load(tg[0], int(tplayer[0]), -1, int(tplies[0])))
    sharp = BounceTreeSearchAgent(iterations=64, leaf_playouts=8, policy=policy, seed=SEED)
    move = sharp.choose(tactical, game=0)
    assert move._source[0] * 54 + move._target[1] * 6 + move._target[0] in wins and int(move._target[1]) in (0, 8)
    sharp.close()
    for method in (agent.predict, agent.choose):
        with pytest.raises(ValueError, match="Connect"):
            method(ConnectConfig(6, 7, 4).sample_initial_state())
    agent.close()
    # a pool of the caller's: the agent passes `edges` on
    tight = BounceTreeSearchAgent(iterations=T, leaf_playouts=P, explore=40000, policy=policy, seed=SEED, edges=252)
    b = load(grid, roots, first_game=4)
    want = b.search_moves(seed=SEED, iterations=T, leaf_playouts=P, explore=40000, max_plies=BOUNCE_MAX_PLIES, policy=policy, edges=252)
    assert (want[4] <= 252).all()
    assert [a for a in tight.choose_many(states, first_game=4)] == [
        {x._source[0] * 54 + x._target[1] * 6 + x._target[0]: x for x in s.actions}[int(slot)] for s, slot in zip(states, want[2])]
    tight.close()
    b.close()


# ---- a small fuzz: random geometries and start grids from the generators of tests/fuzz_cases.py, 4 roots each, T * P <= 256,
# both policies, the pool alternating between the minimum and the default.  BGS_FUZZ_CASES widens it as elsewhere.
FUZZ_KEYS = list(range(max(8, fc.EXTRA)))
FUZZ_SHAPES = ((32, 8), (64, 4), (16, 16), (256, 1), (5, 51))


def _fuzz_arguments(key):
    case = fc.bounce_case(key)
    h, w = case.grid.shape
    rows = case.eval_rows[:4]
    roots = fc.take(case.roots, rows)
    T, P = FUZZ_SHAPES[key % len(FUZZ_SHAPES)]
    edges = sb.min_edges(h, w) if key % 2 == 0 else sb.default_edges(h, w, T)
    max_plies = case.max_plies[0] if key % 3 == 0 else sb.LONG
    return case, roots, dict(iterations=T, leaf_playouts=P, explore=sb.DEFAULT_EXPLORE, max_plies=int(max_plies), edges=edges)


@functools.lru_cache(maxsize=None)
def _fuzz_expected(key, policy):
    case, roots, kw = _fuzz_arguments(key)
    return sb.search_bounce_expected(case.grid, roots, SEED, case.first_game, kw["iterations"], kw["leaf_playouts"], kw["explore"],
                                     kw["max_plies"], policy, kw["edges"])


@pytest.mark.parametrize("policy", ["uniform", "decisive"])
@pytest.mark.parametrize("key", FUZZ_KEYS)
def test_fuzz_random_geometries_equal_the_reference(key, policy):
    case, roots, kw = _fuzz_arguments(key)
    b = load(case.grid, roots, case.first_game)
    before = snapshot(b)
    got = b.search_moves(seed=SEED, policy=policy, **kw)
    *want, steps, seen = _fuzz_expected(key, policy)
    print(f"{fc.describe(case)} {policy} {kw}: steps {b.steps} / {steps}, "
          f"{ {k: v for k, v in seen.items() if isinstance(v, int)} }")
    assert_equal(got, want, fc.describe(case))
    assert b.steps == steps
    assert snapshot(b) == before
    b.close()
