"""The proving tree search for Bounce (bgs_bounce_search_moves_proving, BounceBatch.search_moves_proving,
BounceTreeSearchAgent(prove=True)) against the CPU statement of tests/search_bounce_prove_expected.py: counts, visits,
best, nodes, used, proved, done and the bgs_steps delta bit for bit, over the case table of the plain Bounce search and the
hand-made cases; and the root's tags against the exact horizon solver on the same roots.
tests/test_search_bounce_prove_expected.py states what the cases hold.

Every launch here is one workgroup a root over at most 8 roots; the CPU model, cached per case, is the slower side.

Everything here needs a real MI355X: `pytest -m gpu`.
"""

import ctypes
import functools

import numpy as np
import pytest

from tests import fuzz_cases as fc
from tests import search_bounce_expected as sb
from tests import search_bounce_prove_expected as sp
from tests.test_gpu_search_bounce import FUZZ_KEYS, _fuzz_arguments, _states, load, snapshot

pytestmark = pytest.mark.gpu

SEED = sb.SEED
NAMES = ("counts", "visits", "best", "nodes", "used", "proved", "done")
RUNS = [("table", n, p) for n, p in sp.RUNS] + [("hand", n, p) for n, p in sp.hand_runs()]


def assert_equal(got, want, what=""):
    assert len(got) == len(NAMES)
    for name, g, w in zip(NAMES, got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, name
        np.testing.assert_array_equal(g, w, err_msg=f"{name} {what}")


def run_of(kind, name, policy):
    """(grid, roots, first_game, the keyword arguments of the launch, the model's answer)"""
    if kind == "table":
        case = sb.BY_NAME[name]
        grid, roots = sb.case_grid(case), sb.case_roots(case)
        kw = dict(seed=SEED, iterations=case.iterations, leaf_playouts=case.playouts, explore=case.explore,
                  max_plies=sb.case_max_plies(case, roots), policy=policy, edges=sb.case_edges(case))
        return grid, roots, case.first_game, kw, sp.case_expected(name, policy)
    case = sp.HAND_BY_NAME[name]
    h, w = case.grid.shape
    kw = dict(seed=SEED, iterations=case.iterations, leaf_playouts=case.playouts, explore=case.explore, max_plies=case.max_plies,
              policy=policy, edges=sb.default_edges(h, w, case.iterations) if case.edges is None else case.edges)
    return case.grid, case.roots, case.first_game, kw, sp.hand_expected(name, policy)


@pytest.mark.parametrize("kind,name,policy", RUNS, ids=[f"{k}-{n}-{p}" for k, n, p in RUNS])
def test_outputs_and_steps_equal_the_reference(kind, name, policy):
    grid, roots, first_game, kw, (*want, steps, seen) = run_of(kind, name, policy)
    b = load(grid, roots, first_game)
    before = snapshot(b)
    got = b.search_moves_proving(**kw)
    got_steps = b.steps
    tallies = {key: value for key, value in seen.items() if isinstance(value, int)}
    print(f"{name} {policy}: steps {got_steps} / {steps}, {tallies}, done {got[6].tolist()} / {want[6].tolist()}")
    assert_equal(got, want, name)
    assert got_steps == steps, name
    assert snapshot(b) == before, name        # planes, status and plies are unchanged
    b.close()


@pytest.mark.parametrize("name", ["default", "crowded"])
def test_two_shards_equal_the_whole_batch(name):
    case = sb.BY_NAME[name]
    grid, roots, _, kw, _ = run_of("table", name, "uniform")
    cut = roots[0].shape[0] // 2
    whole = load(grid, roots, first_game=100).search_moves_proving(**kw)
    lo = load(grid, tuple(a[:cut] for a in roots), first_game=100).search_moves_proving(**kw)
    hi = load(grid, tuple(a[cut:] for a in roots), first_game=100 + cut).search_moves_proving(**kw)
    assert_equal(tuple(np.concatenate([x, y]) for x, y in zip(lo, hi)), whole)
    assert whole[0].any() and (whole[6] < case.iterations).any() and (whole[5] != sp.SOLVE_NONE).any()


@pytest.mark.parametrize("policy", ["uniform", "decisive"])
def test_device_outputs_a_reused_workspace_and_null_outputs(policy):
    import torch

    from simulator.batch import playout_policy
    from simulator.game import _abi

    case = sb.BY_NAME["default"]
    grid, roots, first_game, kw, (*want, want_steps, _) = run_of("table", "default", policy)
    h, w = grid.shape
    n, edges = roots[0].shape[0], kw["edges"]
    b = load(grid, roots, use_torch=True, first_game=first_game)
    host = b.search_moves_proving(**kw)            # workspace = NULL: the library's own
    assert_equal(host, want)
    steps = b.steps
    assert steps == want_steps
    # the device variant with a caller's workspace, filled with rubbish, and outputs filled with a sentinel: every entry of
    # every output is written, proved and done included
    need = b.search_moves_workspace_bytes(case.iterations, edges)     # the plain search's workspace serves both
    workspace = torch.full((need,), 0xA5, dtype=torch.uint8, device="cuda:0")
    slots = (n, w, h * w)
    shapes = (slots + (3,), slots, (n,), (n,), (n,), slots, (n,))
    outs = [torch.full(shape, 77 if name == "proved" else -7, dtype=torch.int8 if name == "proved" else torch.int32, device="cuda:0")
            for name, shape in zip(NAMES, shapes)]
    b.reset_steps()
    got = b.search_moves_proving_tensor(*outs, workspace=workspace, **kw)
    assert all(g is o for g, o in zip(got, outs))
    torch.cuda.synchronize()
    assert_equal(tuple(g.cpu().numpy() for g in got), host)
    assert b.steps == steps
    # a second call on the same batch and workspace gives the same outputs: the tags of the first do not leak
    again = b.search_moves_proving_tensor(workspace=workspace, **kw)
    torch.cuda.synchronize()
    assert_equal(tuple(g.cpu().numpy() for g in again), host)
    # the plain search on the workspace the proving search has used, and the proving search after it
    plain = b.search_moves_tensor(workspace=workspace, **kw)
    torch.cuda.synchronize()
    for g, x in zip(plain, sb.case_expected("default", policy)[:5]):
        np.testing.assert_array_equal(g.cpu().numpy(), x)
    again = b.search_moves_proving_tensor(workspace=workspace, **kw)
    torch.cuda.synchronize()
    assert_equal(tuple(g.cpu().numpy() for g in again), host)
    # the batch's own cached workspace is the plain search's
    fresh = b.search_moves_proving_tensor(**kw)
    assert list(b._search_workspaces) == [(case.iterations, edges)]
    torch.cuda.synchronize()
    assert_equal(tuple(g.cpu().numpy() for g in fresh), host)
    # visits, best, nodes, used, proved and done may be NULL, on the host and on the device
    call = _abi.lib().bgs_bounce_search_moves_proving
    head = (b._handle, SEED, case.iterations, case.playouts, case.explore, kw["max_plies"], playout_policy(policy), edges)
    nulls = (None,) * 6
    counts = np.full(slots + (3,), -1, dtype=np.int32)
    _abi.check(call(*head, ctypes.c_void_p(counts.ctypes.data), *nulls, None, 0, 0))
    np.testing.assert_array_equal(counts, host[0])
    only = torch.full(slots + (3,), -7, dtype=torch.int32, device="cuda:0")
    _abi.check(call(*head, ctypes.c_void_p(only.data_ptr()), *nulls, ctypes.c_void_p(workspace.data_ptr()), need, 1))
    torch.cuda.synchronize()
    np.testing.assert_array_equal(only.cpu().numpy(), host[0])
    # proved and done alone beside counts, on the host with a caller's workspace
    proved, done = np.full(slots, 77, dtype=np.int8), np.full(n, -7, dtype=np.int32)
    counts[:] = -1
    _abi.check(call(*head, ctypes.c_void_p(counts.ctypes.data), None, None, None, None, ctypes.c_void_p(proved.ctypes.data),
                    ctypes.c_void_p(done.ctypes.data), ctypes.c_void_p(workspace.data_ptr()), need, 0))
    np.testing.assert_array_equal(counts, host[0])
    np.testing.assert_array_equal(proved, host[5])
    np.testing.assert_array_equal(done, host[6])
    # a workspace one byte short is refused
    assert call(*head, ctypes.c_void_p(only.data_ptr()), *nulls, ctypes.c_void_p(workspace.data_ptr()), need - 1, 1) == _abi.BGS_ERR_ARG
    assert "workspace" in _abi.last_error()
    with pytest.raises(ValueError, match="workspace"):
        b.search_moves_proving_tensor(workspace=workspace[:-1], **kw)
    b.close()


def test_refusals_return_err_arg_and_leave_the_outputs_untouched():
    import torch

    from simulator.batch import BounceBatch, ConnectBatch
    from simulator.game import _abi

    call = _abi.lib().bgs_bounce_search_moves_proving
    U = _abi.POLICY_UNIFORM
    grid = sb.GRIDS["default"]
    h, w = grid.shape
    n, S, E = 4, w * h * w, sb.min_edges(h, w)
    b = BounceBatch(grid, n)
    sizes = (n * S * 3, n * S, n, n, n, n * S, n)
    outs = [np.full(size, -5, dtype=np.int8 if name == "proved" else np.int32) for name, size in zip(NAMES, sizes)]
    ptr = [ctypes.c_void_p(o.ctypes.data) for o in outs]
    tail = (None, 0, 0)

    def refused(word, *args):
        assert call(*args) == _abi.BGS_ERR_ARG
        assert word in _abi.last_error(), _abi.last_error()
        assert all((o == -5).all() for o in outs)

    # (handle, seed, iterations, leaf_playouts, explore, max_plies, policy, edges, ...): what bgs_bounce_search_moves refuses
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
    assert call(b._handle, 1, 1, 1, 0, 1, U, E, *ptr, *tail) == _abi.BGS_OK       # the least of everything is taken
    assert call(b._handle, 1, 2, 2, 1 << 18, 1, U, E, *ptr, *tail) == _abi.BGS_OK
    for o in outs:
        o[:] = -5
    # Connect and generic batches
    connect = ConnectBatch(6, 7, 4, n)
    refused("Bounce", connect._handle, 1, 8, 8, 65536, 100, U, E, *ptr, *tail)
    for method in (connect.search_moves_proving, connect.search_moves_proving_tensor):
        with pytest.raises(ValueError, match="Bounce"):
            method(iterations=8)
    wide = np.zeros((9, 8), dtype=np.int8)    # 72 cells: a generic board
    wide[1] = wide[7] = 1
    generic = BounceBatch(wide, n)
    big_sizes = (n * 8 * 72 * 3, n * 8 * 72, n, n, n, n * 8 * 72, n)
    big = [np.full(size, -5, dtype=np.int8 if name == "proved" else np.int32) for name, size in zip(NAMES, big_sizes)]
    assert call(generic._handle, 1, 8, 8, 65536, 100, U, 8 * 8 * 7, *[ctypes.c_void_p(o.ctypes.data) for o in big], *tail) == _abi.BGS_ERR_ARG
    assert "bit-packed" in _abi.last_error() and all((o == -5).all() for o in big)
    # misaligned device pointers, each in turn, proved and done among them; a NULL, misaligned or short workspace
    need = b.search_moves_workspace_bytes(8, E)
    workspace = torch.zeros(need + 256, dtype=torch.uint8, device="cuda:0")
    dev = [torch.full((o.size + 16,), -5, dtype=torch.int8 if o.dtype == np.int8 else torch.int32, device="cuda:0") for o in outs]
    for bad in range(len(NAMES)):
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
    assert call(b._handle, 1, 40, 8, 65536, 100, U, E, *at, ctypes.c_void_p(workspace.data_ptr()), need, 1) == _abi.BGS_ERR_ARG
    assert "too small" in _abi.last_error()          # (sized for 8 iterations, asked for 40)
    assert call(b._handle, 1, 8, 8, 65536, 100, U, E + 16, *at, ctypes.c_void_p(workspace.data_ptr()), need, 1) == _abi.BGS_ERR_ARG
    assert "too small" in _abi.last_error()          # (sized for E edges, asked for E + 16)
    # ... and the host call with a caller's workspace that is misaligned or short
    refused("256-byte", b._handle, 1, 8, 8, 65536, 100, U, E, *ptr, ctypes.c_void_p(workspace.data_ptr() + 64), need, 0)
    refused("too small", b._handle, 1, 8, 8, 65536, 100, U, E, *ptr, ctypes.c_void_p(workspace.data_ptr()), need - 1, 0)
    torch.cuda.synchronize()
    assert all(bool((d == -5).all()) for d in dev)
    # the Python layer
    with pytest.raises(ValueError, match="policy"):
        b.search_moves_proving(policy="greedy")
    with pytest.raises(ValueError, match="policy"):
        b.search_moves_proving_tensor(policy="greedy")
    with pytest.raises(ValueError, match="iterations"):
        b.search_moves_proving(iterations=0)
    with pytest.raises(ValueError, match="iterations"):
        b.search_moves_proving_tensor(iterations=0)
    with pytest.raises(ValueError, match="explore"):
        b.search_moves_proving(explore=1 << 19)
    with pytest.raises(ValueError, match="edges"):
        b.search_moves_proving(edges=E - 1)
    for batch in (b, connect, generic):
        batch.close()


# ---- the root's tags against the exact horizon solver, on the same roots
MAX_SOLVER_DEPTH = 16


@pytest.mark.parametrize("kind,name,policy", RUNS, ids=[f"{k}-{n}-{p}" for k, n, p in RUNS])
def test_proved_root_moves_agree_with_the_horizon_solver(kind, name, policy):
    grid, roots, first_game, kw, (*want, _, seen) = run_of(kind, name, policy)
    b = load(grid, roots, first_game)
    proved = b.search_moves_proving(**kw)[5]
    np.testing.assert_array_equal(proved, want[5])
    height = seen["height"]
    tagged = (proved == sp.SOLVE_WIN) | (proved == sp.SOLVE_LOSS) | (proved == sp.SOLVE_DRAW)
    assert ((height > 0) == tagged).all()
    left_out = int((height[tagged] > MAX_SOLVER_DEPTH).sum())
    checked = 0
    for depth in sorted(set(height[tagged].tolist())):
        if depth > MAX_SOLVER_DEPTH:
            continue
        codes, _ = b.solve_moves(depth=depth, with_plies=False)
        at = tagged & (height == depth)
        decisive = at & (proved != sp.SOLVE_DRAW)
        np.testing.assert_array_equal(codes[decisive], proved[decisive], err_msg=f"{name}: proofs of {depth} plies")
        drawn = at & (proved == sp.SOLVE_DRAW)
        # the solver's DRAW is "the move itself ends the game drawn"; a draw backed up from below is open to it
        np.testing.assert_array_equal(codes[drawn], np.where(height[drawn] == 1, sp.SOLVE_DRAW, sp.SOLVE_UNKNOWN),
                                      err_msg=f"{name}: draws of {depth} plies")
        checked += int(at.sum())
    print(f"{name} {policy}: {checked} tagged root slots checked, proofs of {sorted(set(height[tagged].tolist()))} plies, {left_out} left out")
    assert left_out == 0 and checked == int(tagged.sum())
    b.close()


# ---- the agent
@pytest.mark.parametrize("policy", ["uniform", "decisive"])
def test_tree_search_agent_equals_the_batch_call(policy):
    from simulator.agents import BOUNCE_MAX_PLIES, BounceTreeSearchAgent
    from simulator.game.bounce import Config, State
    from tests.test_search_bounce_expected import tactical_root

    grid = sb.GRIDS["default"]
    config = Config(grid)
    _, (tg, tplayer, _, tplies), wins = tactical_root()
    tactical = State._fresh(config, *config._engine().load(tg[0], int(tplayer[0]), -1, int(tplies[0])))
    states = _states(config, 5, seed=3) + [tactical]          # the last has a win in one
    T, P = 64, 8
    agent = BounceTreeSearchAgent(iterations=T, leaf_playouts=P, explore=40000, policy=policy, seed=SEED, prove=True)
    out = agent.search(states, first_game=4)
    many = agent.predict_many(states, first_game=4)
    chosen = agent.choose_many(states, first_game=4)
    roots = (np.stack([s.grid for s in states]), np.array([s.player for s in states], np.int8),
             np.full(len(states), -1, np.int8), np.array([s._plies for s in states], np.int32))
    b = load(grid, roots, first_game=4)
    want = b.search_moves_proving(seed=SEED, iterations=T, leaf_playouts=P, explore=40000, max_plies=BOUNCE_MAX_PLIES, policy=policy)
    assert_equal(out, want)
    counts, visits, best, nodes, used, proved, done = want
    assert done[-1] < T and best[-1] in wins
    for k, (s, m) in enumerate(zip(states, many)):
        at = {a: (a._source[0], a._target[1] * 6 + a._target[0]) for a in s.actions}
        share = {a: float(visits[k][at[a]]) for a in s.actions}
        if any(proved[k][at[a]] == sp.SOLVE_WIN for a in s.actions):
            share = {a: 1.0 if proved[k][at[a]] == sp.SOLVE_WIN else 0.0 for a in s.actions}
        elif any(proved[k][at[a]] != sp.SOLVE_LOSS for a in s.actions):
            share = {a: 0.0 if proved[k][at[a]] == sp.SOLVE_LOSS else share[a] for a in s.actions}
        total = sum(share.values())
        assert list(m) == s.actions
        assert m == {a: share[a] / total for a in s.actions}
        assert abs(sum(m.values()) - 1.0) < 1e-12
        assert agent.predict(s, game=4 + k) == m
        (sx, _), (tx, ty) = chosen[k]._source, chosen[k]._target
        assert sx * 54 + ty * 6 + tx == best[k] and chosen[k] in s.actions
        assert agent.choose(s, game=4 + k) == chosen[k]
    assert sorted(many[-1].values())[-2:] == [0.0, 1.0]
    agent.close()
    b.close()
    with pytest.raises(ValueError, match="forest does not prove"):
        BounceTreeSearchAgent(prove=True, reuse=True)


# ---- a small fuzz: the random geometries and shapes of tests/test_gpu_search_bounce.py's fuzz, both policies
@functools.lru_cache(maxsize=None)
def _fuzz_expected(key, policy):
    case, roots, kw = _fuzz_arguments(key)
    return sp.search_bounce_prove_expected(case.grid, roots, SEED, case.first_game, kw["iterations"], kw["leaf_playouts"], kw["explore"],
                                           kw["max_plies"], policy, kw["edges"])


@pytest.mark.parametrize("policy", ["uniform", "decisive"])
@pytest.mark.parametrize("key", FUZZ_KEYS)
def test_fuzz_random_geometries_equal_the_reference(key, policy):
    case, roots, kw = _fuzz_arguments(key)
    b = load(case.grid, roots, case.first_game)
    before = snapshot(b)
    got = b.search_moves_proving(seed=SEED, policy=policy, **kw)
    *want, steps, seen = _fuzz_expected(key, policy)
    print(f"{fc.describe(case)} {policy} {kw}: steps {b.steps} / {steps}, "
          f"{ {k: v for k, v in seen.items() if isinstance(v, int)} }")
    assert_equal(got, want, fc.describe(case))
    assert b.steps == steps
    assert snapshot(b) == before
    b.close()
