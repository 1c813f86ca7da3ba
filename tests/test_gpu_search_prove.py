"""The proving tree search (bgs_connect_search_actions_proving, ConnectBatch.search_actions_proving,
TreeSearchAgent(prove=True)) against the CPU statement of tests/search_prove_expected.py: counts, visits, best, nodes,
proved, done and the bgs_steps delta bit for bit.  tests/test_search_prove_expected.py states what the case table holds.

Everything here needs a real MI355X: `pytest -m gpu`.
"""

import ctypes

import numpy as np
import pytest

from tests import search_expected as se
from tests import search_prove_expected as sp

pytestmark = pytest.mark.gpu

SEED = se.SEED
NAMES = ("counts", "visits", "best", "nodes", "proved", "done")


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
    assert len(got) == len(want) == 6
    for name, g, w in zip(NAMES, got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, name
        np.testing.assert_array_equal(g, w, err_msg=f"{name} {what}")


def arguments(case, roots, policy="uniform"):
    return dict(seed=SEED, iterations=case.iterations, leaf_playouts=case.playouts, explore=case.explore,
                max_plies=sp.case_max_plies(case, roots), policy=policy)


@pytest.mark.parametrize("run", sp.RUNS, ids=sp.run_id)
def test_the_six_outputs_and_steps_equal_the_reference(run):
    index, policy, per_ply = run
    case = sp.CASES[index]
    roots = sp.case_roots(case)
    b = load(case.h, case.w, case.k, roots, per_ply, case.first_game)
    before = snapshot(b)
    got = b.search_actions_proving(**arguments(case, roots, policy))
    *want, steps, seen = sp.case_expected(index, per_ply, policy)
    tallies = {key: value for key, value in seen.items() if isinstance(value, int)}
    print(f"{case.name} {policy} per_ply={per_ply}: steps {b.steps} / {steps}, {tallies}, done {got[5].tolist()}")
    assert_equal(got, want, case.name)
    assert b.steps == steps, case.name
    assert snapshot(b) == before, case.name     # planes, status and plies are unchanged
    b.close()


@pytest.mark.parametrize("index", [1, 5], ids=lambda j: sp.CASES[j].name)
def test_two_shards_equal_the_whole_batch(index):
    case = sp.CASES[index]
    h, w, k = case.h, case.w, case.k
    roots = sp.case_roots(case)
    cut = roots[0].shape[0] // 2
    kw = arguments(case, roots, "decisive")
    whole = load(h, w, k, roots, first_game=100).search_actions_proving(**kw)
    lo = load(h, w, k, tuple(a[:cut] for a in roots), first_game=100).search_actions_proving(**kw)
    hi = load(h, w, k, tuple(a[cut:] for a in roots), first_game=100 + cut).search_actions_proving(**kw)
    assert_equal(tuple(np.concatenate([x, y]) for x, y in zip(lo, hi)), whole)
    assert (whole[5] < case.iterations).any()      # (roots that stopped early among them)


def _device_outputs(torch, n, w, fill=-7):
    shapes = ((n, w, 3), (n, w), (n,), (n,), (n, w), (n,))
    return [torch.full(shape, fill, dtype=torch.int8 if j == 4 else torch.int32, device="cuda:0") for j, shape in enumerate(shapes)]


@pytest.mark.parametrize("policy", ["uniform", "decisive"])
def test_device_outputs_a_reused_workspace_and_null_outputs(policy):
    import torch

    from simulator.batch import playout_policy
    from simulator.game import _abi

    index = 1                                       # 5x6x3: roots that stop early beside roots that do not
    case = sp.CASES[index]
    roots = sp.case_roots(case)
    n, w = roots[0].shape[0], case.w
    kw = arguments(case, roots, policy)
    want = sp.case_expected(index, False, policy)
    b = load(case.h, case.w, case.k, roots, use_torch=True, first_game=case.first_game)
    host = b.search_actions_proving(**kw)          # workspace = NULL: the library's own
    assert_equal(host, want[:6])
    steps = b.steps
    assert steps == want[6]
    # the device variant with a caller's workspace, filled with rubbish: the kernel resets its tree
    need = b.search_workspace_bytes(case.iterations)
    workspace = torch.full((need,), 0xA5, dtype=torch.uint8, device="cuda:0")
    outs = _device_outputs(torch, n, w)
    b.reset_steps()
    got = b.search_actions_proving_tensor(*outs, workspace=workspace, **kw)
    assert all(g is o for g, o in zip(got, outs))
    torch.cuda.synchronize()
    assert_equal(tuple(g.cpu().numpy() for g in got), host)
    assert b.steps == steps
    # a second call on the same batch and workspace -- which now holds a tagged tree -- gives the same outputs
    again = b.search_actions_proving_tensor(workspace=workspace, **kw)
    torch.cuda.synchronize()
    assert_equal(tuple(g.cpu().numpy() for g in again), host)
    # the plain search shares the workspace, the cached one too, and is not disturbed by the tags left there
    plain = b.search_actions_tensor(workspace=workspace, **kw)
    torch.cuda.synchronize()
    for g, x in zip(plain, se.search_expected(case.h, case.w, case.k, roots, SEED, case.first_game, case.iterations, case.playouts,
                                              case.explore, kw["max_plies"], False, policy)[:4]):
        np.testing.assert_array_equal(g.cpu().numpy(), x)
    fresh = b.search_actions_proving_tensor(**kw)
    assert list(b._search_workspaces) == [case.iterations]
    b.search_actions_tensor(**kw)
    assert list(b._search_workspaces) == [case.iterations]
    torch.cuda.synchronize()
    assert_equal(tuple(g.cpu().numpy() for g in fresh), host)
    # visits, best, nodes, proved and done may be NULL, on the host and on the device, each alone too
    call = _abi.lib().bgs_connect_search_actions_proving
    head = (b._handle, SEED, case.iterations, case.playouts, case.explore, kw["max_plies"], playout_policy(policy))
    counts = np.full((n, w, 3), -1, dtype=np.int32)
    _abi.check(call(*head, ctypes.c_void_p(counts.ctypes.data), None, None, None, None, None, None, 0, 0))
    np.testing.assert_array_equal(counts, host[0])
    counts[:] = -1
    proved = np.full((n, w), 9, dtype=np.int8)
    _abi.check(call(*head, ctypes.c_void_p(counts.ctypes.data), None, None, None, ctypes.c_void_p(proved.ctypes.data), None,
                    ctypes.c_void_p(workspace.data_ptr()), need, 0))
    np.testing.assert_array_equal(counts, host[0])
    np.testing.assert_array_equal(proved, host[4])
    done = np.full(n, -1, dtype=np.int32)
    best = np.full(n, -9, dtype=np.int32)
    _abi.check(call(*head, ctypes.c_void_p(counts.ctypes.data), None, ctypes.c_void_p(best.ctypes.data), None, None,
                    ctypes.c_void_p(done.ctypes.data), None, 0, 0))
    np.testing.assert_array_equal(done, host[5])
    np.testing.assert_array_equal(best, host[2])
    only = torch.full((n, w, 3), -7, dtype=torch.int32, device="cuda:0")
    _abi.check(call(*head, ctypes.c_void_p(only.data_ptr()), None, None, None, None, None, ctypes.c_void_p(workspace.data_ptr()), need, 1))
    torch.cuda.synchronize()
    np.testing.assert_array_equal(only.cpu().numpy(), host[0])
    # a workspace one byte short is refused
    assert call(*head, ctypes.c_void_p(only.data_ptr()), None, None, None, None, None, ctypes.c_void_p(workspace.data_ptr()), need - 1,
                1) == _abi.BGS_ERR_ARG
    assert "workspace" in _abi.last_error()
    with pytest.raises(ValueError, match="workspace"):
        b.search_actions_proving_tensor(workspace=workspace[:-1], **kw)
    b.close()


def test_refusals_return_err_arg_and_leave_the_outputs_untouched():
    import torch

    from simulator.batch import BounceBatch, ConnectBatch
    from simulator.game import _abi

    call = _abi.lib().bgs_connect_search_actions_proving
    U = _abi.POLICY_UNIFORM
    n, w = 4, 7
    b = ConnectBatch(6, w, 4, n)
    outs = [np.full(n * w * 3, -5, dtype=np.int32), np.full(n * w, -5, dtype=np.int32), np.full(n, -5, dtype=np.int32),
            np.full(n, -5, dtype=np.int32), np.full(n * w, -5, dtype=np.int8), np.full(n, -5, dtype=np.int32)]
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
        refused("search_actions_proving: unknown policy", b._handle, 1, 8, 8, 65536, 100, policy, *ptr, *tail)
    refused("counts", b._handle, 1, 8, 8, 65536, 100, U, None, *ptr[1:], *tail)
    assert call(b._handle, 1, 1, 1, 0, 1, U, *ptr, *tail) == _abi.BGS_OK       # the least of everything is taken
    assert call(b._handle, 1, 2, 2, 1 << 18, 1, U, *ptr, *tail) == _abi.BGS_OK
    for o in outs:
        o[:] = -5
    # Bounce and generic batches
    grid = np.zeros((9, 6), dtype=np.int8)
    grid[1] = grid[7] = [1, 2, 3, 3, 2, 1]
    bounce = BounceBatch(grid, 4)
    refused("search_actions_proving: Connect", bounce._handle, 1, 8, 8, 65536, 100, U, *ptr, *tail)
    for method in (bounce.search_actions_proving, bounce.search_actions_proving_tensor):
        with pytest.raises(ValueError, match="Connect batches only"):
            method(iterations=8)
    generic = ConnectBatch(20, 20, 5, 4)
    big = [np.full(4 * 20 * 3, -5, dtype=np.int32), np.full(4 * 20, -5, dtype=np.int32), np.full(4, -5, dtype=np.int32),
           np.full(4, -5, dtype=np.int32), np.full(4 * 20, -5, dtype=np.int8), np.full(4, -5, dtype=np.int32)]
    assert call(generic._handle, 1, 8, 8, 65536, 100, U, *[ctypes.c_void_p(o.ctypes.data) for o in big], *tail) == _abi.BGS_ERR_ARG
    assert "search_actions_proving: bit-packed" in _abi.last_error() and all((o == -5).all() for o in big)
    # misaligned device pointers, each in turn; a NULL, misaligned or short workspace
    need = b.search_workspace_bytes(8)
    workspace = torch.zeros(need + 256, dtype=torch.uint8, device="cuda:0")
    dev = [torch.full((o.size + 16,), -5, dtype=torch.int8 if o.dtype == np.int8 else torch.int32, device="cuda:0") for o in outs]
    for bad in range(6):
        at = [ctypes.c_void_p(d.data_ptr() + (4 if j == bad else 0)) for j, d in enumerate(dev)]
        assert call(b._handle, 1, 8, 8, 65536, 100, U, *at, ctypes.c_void_p(workspace.data_ptr()), need, 1) == _abi.BGS_ERR_ARG
        assert "aligned" in _abi.last_error() and NAMES[bad] in _abi.last_error()
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
        b.search_actions_proving(policy="greedy")
    with pytest.raises(ValueError, match="policy"):
        b.search_actions_proving_tensor(policy="greedy")
    with pytest.raises(ValueError, match="iterations"):
        b.search_actions_proving(iterations=0)
    with pytest.raises(ValueError, match="iterations"):
        b.search_actions_proving_tensor(iterations=0)
    with pytest.raises(ValueError, match="explore"):
        b.search_actions_proving(explore=1 << 19)
    for batch in (b, bounce, generic):
        batch.close()


SOLVED = [j for j, case in enumerate(sp.CASES) if (case.h, case.w, case.k) in ((6, 7, 4), (5, 6, 3))]


@pytest.mark.parametrize("index", SOLVED, ids=lambda j: sp.CASES[j].name)
def test_tagged_columns_equal_the_exact_solver(index):
    """every root of the 6x7x4 and 5x6x3 cases with at most 12 empty cells: its tagged columns carry the code of
    solve_actions(depth=None) on the same batch; the solver reports BUDGET for none of these roots"""
    from simulator.batch import SOLVE_BUDGET, SOLVE_NONE, SOLVE_UNKNOWN

    case = sp.CASES[index]
    roots = sp.case_roots(case)
    empty = (roots[0] < 0).sum(axis=(1, 2))
    rows = np.flatnonzero((roots[2] == -1) & (empty <= sp.SOLVED_EMPTY))
    b = load(case.h, case.w, case.k, roots, first_game=case.first_game)
    proved = b.search_actions_proving(**arguments(case, roots))[4]
    codes, _ = b.solve_actions(depth=None, with_plies=False)
    assert not (codes[rows] == SOLVE_BUDGET).any()
    tags = 0
    for i in rows:
        tagged = np.flatnonzero((proved[i] != SOLVE_UNKNOWN) & (proved[i] != SOLVE_NONE))
        np.testing.assert_array_equal(proved[i, tagged], codes[i, tagged], err_msg=f"root {i}")
        tags += tagged.size
    print(f"{case.name}: {rows.size} roots with at most {sp.SOLVED_EMPTY} empty cells, {tags} tagged columns")
    if rows.size:
        np.testing.assert_array_equal(proved[rows] == SOLVE_NONE, codes[rows] == SOLVE_NONE)
    b.close()


# ---- the agent
def _state_after(columns, config=(6, 7, 4)):
    from simulator.game.connect import Config

    s = Config(*config).sample_initial_state()
    for c in columns:
        s = s.action_at(c).sample_next_state()
    return s


@pytest.mark.parametrize("policy", ["uniform", "decisive"])
def test_tree_search_agent_proving_equals_the_batch_call(policy):
    from simulator.agents import TreeSearchAgent
    from simulator.batch import SOLVE_LOSS, SOLVE_WIN, ConnectBatch

    agent = TreeSearchAgent(iterations=48, leaf_playouts=8, explore=40000, policy=policy, seed=SEED, prove=True)
    lines = ([], [3], [3, 3, 2], [0, 1, 0, 1, 0, 1], [3, 3, 3, 3, 3, 3, 2], [2, 2, 3, 3, 4], [0, 3, 0, 3, 1, 3])
    states = [_state_after(cs) for cs in lines]
    many = agent.predict_many(states, first_game=4)
    chosen = agent.choose_many(states, first_game=4)
    b = ConnectBatch(6, 7, 4, len(states))
    grid = np.stack([s.grid for s in states])
    player = np.array([s.player for s in states], dtype=np.int8)
    assert (b.write_state(grid, player, np.full(len(states), -1, dtype=np.int8)) == 0).all()
    b.set_first_game(4)
    out = b.search_actions_proving(seed=SEED, iterations=48, leaf_playouts=8, explore=40000, policy=policy)
    assert_equal(agent.search(states, first_game=4), out)
    counts, visits, best, nodes, proved, done = out
    for g, (s, m) in enumerate(zip(states, many)):
        columns = [a.column for a in s.actions]
        assert list(m) == s.actions
        assert abs(sum(m.values()) - 1.0) < 1e-12
        won = [c for c in columns if proved[g, c] == SOLVE_WIN]
        lost = [c for c in columns if proved[g, c] == SOLVE_LOSS]
        if won:
            assert {a.column: v for a, v in m.items()} == {c: float(c == won[0]) for c in columns}
        elif len(lost) < len(columns):
            alive = sum(int(visits[g, c]) for c in columns if c not in lost)
            assert {a.column: v for a, v in m.items()} == {c: 0.0 if c in lost else float(visits[g, c]) / alive for c in columns}
        else:
            assert {a.column: v for a, v in m.items()} == {c: float(visits[g, c]) / int(visits[g].sum()) for c in columns}
        assert agent.predict(s, game=4 + g) == m
        assert chosen[g].column == best[g]
        assert agent.choose(s, game=4 + g).column == best[g]
    assert chosen[3].column == 0 and proved[3, 0] == SOLVE_WIN and done[3] == 1     # the column that wins at once
    assert (proved[5] == SOLVE_LOSS).all() and done[5] < 48      # three in a row with both ends open: every column loses in two
    assert done[0] == 48                                         # the start position is not decided
    agent.close()
    b.close()


# ---- the sweep: random geometries and root sets of tests/fuzz_cases.py's generators (BGS_FUZZ_CASES widens it)
@pytest.mark.parametrize("key", sp.fuzz_keys())
def test_random_geometries_and_roots_equal_the_reference(key):
    case = sp.fuzz_case(key)
    *want, steps, seen = sp.fuzz_expected(case)
    b = load(case.h, case.w, case.k, case.roots, case.per_ply, case.first_game)
    got = b.search_actions_proving(seed=SEED, iterations=case.iterations, leaf_playouts=case.playouts, explore=case.explore,
                                   max_plies=case.max_plies, policy=case.policy)
    tallies = {name: value for name, value in seen.items() if isinstance(value, int) and value}
    print(f"{case.h}x{case.w}x{case.k} T{case.iterations} P{case.playouts} {case.policy} per_ply={case.per_ply} "
          f"cap={case.max_plies} roots {case.roots[0].shape[0]}: {tallies}")
    assert_equal(got, want, str(case.key))
    assert b.steps == steps
    b.close()
