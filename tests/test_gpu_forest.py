"""Search trees that persist between launches (bgs_connect_forest_search / bgs_connect_forest_advance,
ConnectBatch.search_forest, TreeSearchAgent(reuse=True)) against the CPU statement of tests/forest_expected.py: counts,
visits, best, nodes, carried, kept and the bgs_steps delta bit for bit, at every move of every chain.
tests/test_forest_expected.py states what the chains hold.

Everything here needs a real MI355X: `pytest -m gpu`.
"""

import ctypes

import numpy as np
import pytest

from tests import forest_expected as fe
from tests import search_expected as se

pytestmark = pytest.mark.gpu

SEED = se.SEED
NAMES = ("counts", "visits", "best", "nodes", "carried")


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


def arguments(chain, move, roots):
    return dict(seed=move.seed, iterations=move.iterations, leaf_playouts=move.playouts, explore=chain.explore,
                max_plies=fe.chain_max_plies(chain, roots), policy=chain.policy)


@pytest.mark.parametrize("index", range(len(fe.CHAINS)), ids=lambda j: fe.chain_id(fe.CHAINS[j]))
def test_every_move_of_a_chain_equals_the_reference(index):
    chain = fe.CHAINS[index]
    roots = fe.chain_roots(chain)
    records, _ = fe.chain_expected(index)
    b = load(chain.h, chain.w, chain.k, roots, chain.per_ply, chain.first_game)
    forest = b.search_forest(chain.capacity)
    assert forest.capacity == chain.capacity
    for m, (move, record) in enumerate(zip(chain.moves, records)):
        what = f"{fe.chain_id(chain)} move {m}"
        np.testing.assert_array_equal(b.grid, record.roots[0], err_msg=what)
        np.testing.assert_array_equal(b.winner, record.roots[2], err_msg=what)
        before, steps = snapshot(b), b.steps
        got = forest.search(**arguments(chain, move, roots))
        print(f"{what}: steps {b.steps - steps} / {record.steps}, carried {got[4].tolist()}, nodes {got[3].tolist()}")
        assert_equal(got, record[1:6], what)
        assert b.steps - steps == record.steps, what
        assert snapshot(b) == before, what                    # the search leaves planes, status and plies alone
        for tree, board, kept in record.plies:
            np.testing.assert_array_equal(forest.advance(tree), kept, err_msg=f"kept {what}")
            assert snapshot(b) == before, what                # ... and so does the advance
            assert (b.step_actions(board)[board >= 0] == 0).all()
            before = snapshot(b)
    forest.close()
    b.close()


ANCHOR_RUNS = [(j, "uniform", False) for j in fe.ANCHORS] + [(11, "uniform", False), (0, "decisive", False), (8, "uniform", True)]


@pytest.mark.parametrize("run", ANCHOR_RUNS, ids=se.run_id)
def test_a_restart_with_room_for_every_node_equals_the_plain_search(run):
    index, policy, per_ply = run
    case = se.CASES[index]
    roots = se.case_roots(case)
    counts, visits, best, nodes, steps, _ = se.case_expected(index, per_ply, policy)
    kw = dict(seed=SEED, iterations=case.iterations, leaf_playouts=case.playouts, explore=case.explore,
              max_plies=se.case_max_plies(case, roots), policy=policy)
    b = load(case.h, case.w, case.k, roots, per_ply, case.first_game)
    for capacity in (case.iterations + 1, 2 * case.iterations + 7):
        forest = b.search_forest(capacity)
        for _ in range(2):                                     # the second restart runs over the first one's trees
            b.reset_steps()
            got = forest.search(restart=True, **kw)
            assert_equal(got, (counts, visits, best, nodes, np.zeros_like(nodes)), f"{case} C = {capacity}")
            assert b.steps == steps
        forest.close()
    np.testing.assert_array_equal(b.search_actions(**kw)[1], visits)
    b.close()


@pytest.mark.parametrize("index", [0, 5], ids=lambda j: fe.chain_id(fe.CHAINS[j]))
def test_two_shards_equal_the_whole_batch_along_a_chain(index):
    chain = fe.CHAINS[index]
    roots = fe.chain_roots(chain)
    records, _ = fe.chain_expected(index)
    cut = roots[0].shape[0] // 2
    parts = (slice(None), slice(0, cut), slice(cut, None))
    batches = [load(chain.h, chain.w, chain.k, tuple(a[part] for a in roots), chain.per_ply, 100 + (part.start or 0)) for part in parts]
    forests = [b.search_forest(chain.capacity) for b in batches]
    for move, record in zip(chain.moves, records):
        whole, lo, hi = (f.search(**arguments(chain, move, roots)) for f in forests)
        assert_equal(tuple(np.concatenate([x, y]) for x, y in zip(lo, hi)), whole)
        for tree, board, _ in record.plies:
            kept = [f.advance(tree[part]) for f, part in zip(forests, parts)]
            np.testing.assert_array_equal(np.concatenate(kept[1:]), kept[0])
            for b, part in zip(batches, parts):
                b.step_actions(board[part])
    assert batches[0].steps == batches[1].steps + batches[2].steps
    for x in forests + batches:
        x.close()


def test_device_outputs_null_outputs_a_second_stream_and_a_forest_of_rubbish():
    import torch

    from simulator.batch import playout_policy
    from simulator.game import _abi

    chain = fe.CHAINS[0]
    roots = fe.chain_roots(chain)
    records, _ = fe.chain_expected(0)
    n, w = roots[0].shape[0], chain.w
    kw = [arguments(chain, move, roots) for move in chain.moves[:2]]
    tree, board, kept = records[0].plies[0]
    b = load(chain.h, chain.w, chain.k, roots, use_torch=True, first_game=chain.first_game)
    need = b.forest_bytes(chain.capacity)
    assert need % 256 == 0 and need >= n * chain.capacity * w * 12
    forest = b.search_forest(chain.capacity)
    forest._buffer.fill_(0xA5)                                 # rubbish: the first search restarts every tree
    outs = [torch.full(shape, -7, dtype=torch.int32, device="cuda:0") for shape in ((n, w, 3), (n, w), (n,), (n,), (n,))]
    got = forest.search_tensor(*outs, **kw[0])
    assert all(g is o for g, o in zip(got, outs))
    torch.cuda.synchronize()
    assert_equal(tuple(g.cpu().numpy() for g in got), records[0][1:6])
    assert b.steps == records[0].steps
    before = snapshot(b)
    held = torch.full((n,), -7, dtype=torch.int32, device="cuda:0")
    assert forest.advance_tensor(torch.from_numpy(tree).to("cuda:0"), held) is held
    torch.cuda.synchronize()
    np.testing.assert_array_equal(held.cpu().numpy(), kept)
    assert snapshot(b) == before
    b.step_actions(board)
    # the next search on a stream other than the null stream
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    b.set_stream(stream.cuda_stream)
    with torch.cuda.stream(stream):
        streamed = forest.search_tensor(**kw[1])
    stream.synchronize()
    assert_equal(tuple(g.cpu().numpy() for g in streamed), records[1][1:6])
    b.set_stream(0)
    torch.cuda.synchronize()
    # visits, best, nodes, carried and kept may be NULL, on the host and on the device
    fresh = load(chain.h, chain.w, chain.k, roots, use_torch=True, first_game=chain.first_game)
    other = fresh.search_forest(chain.capacity)
    lib = _abi.lib()
    move = chain.moves[0]
    head = (fresh._handle, move.seed, move.iterations, move.playouts, chain.explore, kw[0]["max_plies"], playout_policy(chain.policy),
            chain.capacity, 1)
    tail = (ctypes.c_void_p(other._buffer.data_ptr()), need)
    counts = np.full((n, w, 3), -1, dtype=np.int32)
    _abi.check(lib.bgs_connect_forest_search(*head, ctypes.c_void_p(counts.ctypes.data), None, None, None, None, *tail, 0))
    np.testing.assert_array_equal(counts, records[0].counts)
    only = torch.full((n, w, 3), -7, dtype=torch.int32, device="cuda:0")
    _abi.check(lib.bgs_connect_forest_search(*head, ctypes.c_void_p(only.data_ptr()), None, None, None, None, *tail, 1))
    torch.cuda.synchronize()
    np.testing.assert_array_equal(only.cpu().numpy(), records[0].counts)
    _abi.check(lib.bgs_connect_forest_advance(fresh._handle, ctypes.c_void_p(tree.ctypes.data), chain.capacity, None, *tail, 0))
    assert (fresh.step_actions(board)[board >= 0] == 0).all()
    other._fresh = False                                       # (the raw calls above have searched it)
    assert_equal(other.search(**kw[1]), records[1][1:6])       # ... and the trees went over all the same
    for x in (forest, other, b, fresh):
        x.close()


def test_refusals_return_err_arg_and_leave_the_outputs_and_the_forest_untouched():
    import torch

    from simulator.batch import BounceBatch, ConnectBatch
    from simulator.game import _abi

    lib = _abi.lib()
    search, advance = lib.bgs_connect_forest_search, lib.bgs_connect_forest_advance
    U = _abi.POLICY_UNIFORM
    n, w, C = 4, 7, 9
    b = ConnectBatch(6, w, 4, n, use_torch=True)
    need = b.forest_bytes(C)
    forest = torch.full((need + 256,), 0x5A, dtype=torch.uint8, device="cuda:0")
    at = ctypes.c_void_p(forest.data_ptr())
    outs = [np.full(n * w * 3, -5, dtype=np.int32), np.full(n * w, -5, dtype=np.int32)] + [np.full(n, -5, dtype=np.int32) for _ in range(3)]
    ptr = [ctypes.c_void_p(o.ctypes.data) for o in outs]
    columns = np.zeros(n, dtype=np.int32)
    cols, kept = ctypes.c_void_p(columns.ctypes.data), ptr[4]

    def refused(word, call, *args):
        assert call(*args) == _abi.BGS_ERR_ARG
        assert word in _abi.last_error(), _abi.last_error()
        assert all((o == -5).all() for o in outs)

    # (handle, seed, iterations, leaf_playouts, explore, max_plies, policy, capacity, restart, outputs, forest, bytes, on_device)
    good = (at, need, 0)
    refused("iterations", search, b._handle, 1, 0, 8, 65536, 100, U, C, 1, *ptr, *good)
    refused("leaf_playouts", search, b._handle, 1, 8, 0, 65536, 100, U, C, 1, *ptr, *good)
    refused("2^29", search, b._handle, 1, 1 << 15, (1 << 14) + 1, 65536, 100, U, C, 1, *ptr, *good)
    refused("explore", search, b._handle, 1, 8, 8, -1, 100, U, C, 1, *ptr, *good)
    refused("explore", search, b._handle, 1, 8, 8, (1 << 18) + 1, 100, U, C, 1, *ptr, *good)
    refused("max_plies", search, b._handle, 1, 8, 8, 65536, 0, U, C, 1, *ptr, *good)
    for policy in (2, -1, 99):
        refused("policy", search, b._handle, 1, 8, 8, 65536, 100, policy, C, 1, *ptr, *good)
    refused("counts", search, b._handle, 1, 8, 8, 65536, 100, U, C, 1, None, *ptr[1:], *good)
    for capacity in (1, 0, -3, _abi.CONNECT_FOREST_MAX_CAPACITY + 1):
        refused("capacity", search, b._handle, 1, 8, 8, 65536, 100, U, capacity, 1, *ptr, *good)
        refused("capacity", advance, b._handle, cols, capacity, kept, *good)
        size = ctypes.c_size_t(77)
        assert lib.bgs_connect_forest_bytes(b._handle, capacity, ctypes.byref(size)) == _abi.BGS_ERR_ARG and size.value == 77
    assert b.forest_bytes(_abi.CONNECT_FOREST_MAX_CAPACITY) > 0 and b.forest_bytes(2) == n * 256
    refused("forest is NULL", search, b._handle, 1, 8, 8, 65536, 100, U, C, 1, *ptr, None, need, 0)
    refused("256-byte", search, b._handle, 1, 8, 8, 65536, 100, U, C, 1, *ptr, ctypes.c_void_p(forest.data_ptr() + 64), need, 0)
    refused("too small", search, b._handle, 1, 8, 8, 65536, 100, U, C, 1, *ptr, at, need - 1, 0)
    refused("too small", search, b._handle, 1, 8, 8, 65536, 100, U, C + 4, 1, *ptr, *good)     # (sized for 9 nodes, asked for 13)
    refused("forest is NULL", advance, b._handle, cols, C, kept, None, need, 0)
    refused("256-byte", advance, b._handle, cols, C, kept, ctypes.c_void_p(forest.data_ptr() + 64), need, 0)
    refused("too small", advance, b._handle, cols, C, kept, at, need - 1, 0)
    refused("columns", advance, b._handle, None, C, kept, *good)
    # Bounce and generic batches
    grid = np.zeros((9, 6), dtype=np.int8)
    grid[1] = grid[7] = [1, 2, 3, 3, 2, 1]
    bounce = BounceBatch(grid, 4)
    generic = ConnectBatch(20, 20, 5, 4)
    for word, other in (("Connect", bounce), ("bit-packed", generic)):
        refused(word, search, other._handle, 1, 8, 8, 65536, 100, U, C, 1, *ptr, *good)
        refused(word, advance, other._handle, cols, C, kept, *good)
        assert lib.bgs_connect_forest_bytes(other._handle, C, ctypes.byref(size)) == _abi.BGS_ERR_ARG and size.value == 77
    for method in (bounce.search_forest, bounce.forest_bytes):
        with pytest.raises(ValueError, match="Connect"):
            method(C)
    # misaligned device outputs, each in turn
    dev = [torch.full((o.size + 4,), -5, dtype=torch.int32, device="cuda:0") for o in outs]
    for bad in range(5):
        where = [ctypes.c_void_p(d.data_ptr() + (4 if j == bad else 0)) for j, d in enumerate(dev)]
        assert search(b._handle, 1, 8, 8, 65536, 100, U, C, 1, *where, at, need, 1) == _abi.BGS_ERR_ARG
        assert "aligned" in _abi.last_error()
    torch.cuda.synchronize()
    assert all(bool((d == -5).all()) for d in dev)
    assert bool((forest == 0x5A).all())                        # no refusal wrote a byte of the forest
    # the least of everything is taken
    assert search(b._handle, 1, 1, 1, 0, 1, U, 2, 1, *ptr, at, need, 0) == _abi.BGS_OK
    assert advance(b._handle, cols, 2, kept, at, need, 0) == _abi.BGS_OK
    # the Python layer
    with pytest.raises(ValueError, match="capacity"):
        b.search_forest(1)
    own = b.search_forest(C)
    with pytest.raises(ValueError, match="policy"):
        own.search(policy="greedy")
    with pytest.raises(ValueError, match="iterations"):
        own.search(iterations=0)
    with pytest.raises(TypeError, match="columns"):
        own.advance(np.zeros(n + 1, dtype=np.int32))
    own.close()
    with pytest.raises(RuntimeError, match="closed"):
        own.search()
    for batch in (b, bounce, generic):
        batch.close()


# ---- the agent
def _start(config=(6, 7, 4)):
    from simulator.game.connect import Config

    return Config(*config).sample_initial_state()


def test_the_reuse_agent_plays_the_reference_game():
    from simulator.agents import TreeSearchAgent

    chain = fe.AGENT_CHAINS[0]
    records, _ = fe.chain_expected(0, agent=True)
    move = chain.moves[0]
    agent = TreeSearchAgent(iterations=move.iterations, leaf_playouts=move.playouts, explore=chain.explore, policy=chain.policy,
                            seed=move.seed, reuse=True)
    assert agent.capacity == chain.capacity == 2 * move.iterations + 1
    states = [_start((chain.h, chain.w, chain.k)) for _ in range(fe.AGENT_STATES)]
    for m, record in enumerate(records):
        got = agent.search(states, first_game=chain.first_game)
        assert len(got) == 5
        assert_equal(got, record[1:6], f"move {m}")
        for _, board, _ in record.plies:                       # the agent's column, then (a two-ply move) the reply
            states = [s.action_at(int(c)).sample_next_state() for s, c in zip(states, board)]
    chosen = agent.choose_many(states, first_game=chain.first_game)       # equal grids: searched on, no advance
    assert all(a is not None for a in chosen)
    agent.close()


def test_the_plain_agent_still_equals_the_batch_call():
    from simulator.agents import TreeSearchAgent
    from simulator.batch import ConnectBatch

    agent = TreeSearchAgent(iterations=16, leaf_playouts=8, seed=SEED)
    assert agent.reuse is False
    states = [_start()]
    for c in (3, 3, 2):
        states.append(states[-1].action_at(c).sample_next_state())
    assert len(agent.search(states, first_game=4)) == 4 and not agent._forests
    b = ConnectBatch(6, 7, 4, len(states))
    assert (b.write_state(np.stack([s.grid for s in states]), np.array([s.player for s in states], dtype=np.int8),
                          np.full(len(states), -1, dtype=np.int8)) == 0).all()
    b.set_first_game(4)
    best = b.search_actions(seed=SEED, iterations=16, leaf_playouts=8)[2]
    assert [a.column for a in agent.choose_many(states, first_game=4)] == best.tolist()
    assert [a.column for a in agent.choose_many(states, first_game=4)] == best.tolist()      # no state between the calls
    agent.close()
    b.close()
