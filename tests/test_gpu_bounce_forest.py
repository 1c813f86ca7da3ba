"""The Bounce forest (bgs_bounce_forest_search / bgs_bounce_forest_advance, BounceBatch.search_moves_forest,
BounceTreeSearchAgent(reuse=True)) against the CPU statement of tests/bounce_forest_expected.py: counts, visits, best,
nodes, used, carried, kept and the bgs_steps delta bit for bit at every move of every chain.
tests/test_bounce_forest_expected.py states what the chains hold.

Every launch here is one workgroup a root over at most 8 roots; the CPU model, cached per chain, is the slower side.

Everything here needs a real MI355X: `pytest -m gpu`.
"""

import ctypes

import numpy as np
import pytest

from tests import bounce_forest_expected as bf
from tests import search_bounce_expected as sb

pytestmark = pytest.mark.gpu

SEED = bf.SEED
NAMES = ("counts", "visits", "best", "nodes", "used", "carried")


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


def part(roots, rows):
    return tuple(a[rows] for a in roots)


def replay(chain, records, rows=slice(None), first_game=None):
    """the chain on the GPU over the boards `rows` of its roots: every output of every move against the records"""
    grid = bf.chain_grid(chain)
    first_game = chain.first_game if first_game is None else first_game
    b = load(grid, part(records[0].roots, rows), first_game)
    forest = b.search_moves_forest(chain.nodes, bf.chain_edges(chain))
    whole = rows == slice(None)
    for m, (move, record) in enumerate(zip(chain.moves, records)):
        what = f"{chain.name}, move {m}"
        want_grid, want_player, want_winner, want_plies = part(record.roots, rows)
        np.testing.assert_array_equal(b.grid, want_grid, err_msg=what)          # the boards the model searched
        np.testing.assert_array_equal(b.plies, want_plies, err_msg=what)
        np.testing.assert_array_equal(b.winner, want_winner, err_msg=what)
        before = snapshot(b)
        b.reset_steps()
        got = forest.search(seed=move.seed, iterations=move.iterations, leaf_playouts=move.playouts, explore=chain.explore,
                            max_plies=record.max_plies, policy=chain.policy)
        print(f"{what}: steps {b.steps} / {record.steps}, carried {got[5].tolist()}, nodes {got[3].tolist()}, used {got[4].tolist()}")
        assert_equal(got, [x[rows] for x in record[2:8]], what)
        if whole:
            assert b.steps == record.steps, what
        assert snapshot(b) == before, what                                      # the search leaves the boards alone
        for tree, board, kept in record.plies:
            moves = b.slots_to_moves(tree[rows])
            same = np.ones(moves.shape[0], dtype=bool)
            if record.desynced >= 0 and whole:
                same[record.desynced] = False
            if whole:
                np.testing.assert_array_equal(moves[same], board[same], err_msg=what)     # the helper decodes the slots
            np.testing.assert_array_equal(forest.advance(tree[rows]), kept[rows], err_msg=what)
            assert snapshot(b) == before, what                                  # ... and so does the advance
            status = b.step_actions(board[rows])
            assert (status[board[rows][:, 0] >= 0] == 0).all()
            before = snapshot(b)
    forest.close()
    b.close()


@pytest.mark.parametrize("name", [c.name for c in bf.CHAINS])
def test_every_move_of_the_chain_equals_the_model(name):
    replay(bf.BY_NAME[name], bf.chain_expected(name)[0])


@pytest.mark.parametrize("name", ["default", "crowded"])
def test_two_shards_equal_the_whole_batch_along_a_chain(name):
    chain = bf.BY_NAME[name]
    records, _ = bf.chain_expected(name)
    cut = chain.n // 2
    replay(chain, records, slice(0, cut))
    replay(chain, records, slice(cut, chain.n), first_game=chain.first_game + cut)


@pytest.mark.parametrize("name", bf.ANCHORS)
def test_a_restart_with_room_for_every_node_is_the_plain_search(name):
    case = sb.BY_NAME[name]
    policy = case.policies[0]
    grid, roots = sb.case_grid(case), sb.case_roots(case)
    *want, steps, _ = sb.case_expected(name, policy)
    want.append(np.zeros_like(want[3]))
    kw = dict(seed=SEED, iterations=case.iterations, leaf_playouts=case.playouts, explore=case.explore,
              max_plies=sb.case_max_plies(case, roots), policy=policy, restart=True)
    b = load(grid, roots, case.first_game)
    for spare in (0, 7):
        forest = b.search_moves_forest(case.iterations + 1 + spare, sb.case_edges(case))
        for again in range(2):                  # the second restart runs over the first one's trees
            b.reset_steps()
            assert_equal(forest.search(**kw), want, f"{name}, C = T + 1 + {spare}, launch {again}")
            assert b.steps == steps
        forest.close()
    b.close()


def test_device_tensors_null_outputs_and_a_forest_of_rubbish():
    import torch

    from simulator.batch import playout_policy
    from simulator.game import _abi

    chain = bf.BY_NAME["default"]
    records, _ = bf.chain_expected("default")
    grid = bf.chain_grid(chain)
    h, w = grid.shape
    n, C, E = chain.n, chain.nodes, bf.chain_edges(chain)
    b = load(grid, records[0].roots, chain.first_game, use_torch=True)
    forest = b.search_moves_forest(C, E)
    share = 64 + 16 * E + 12 * C
    assert b.moves_forest_bytes(C, E) == n * ((share + 255) // 256 * 256) == forest._buffer.numel()
    assert b.moves_forest_bytes(C) == b.moves_forest_bytes(C, b.search_default_edges(C - 1))
    forest._buffer.fill_(0xA5)                  # rubbish: the advance empties such trees, a restart searches them anew
    np.testing.assert_array_equal(forest.advance(np.zeros(n, dtype=np.int32)), np.zeros(n, dtype=np.int32))
    forest._buffer.fill_(0xA5)
    move, record = chain.moves[0], records[0]
    kw = dict(seed=move.seed, iterations=move.iterations, leaf_playouts=move.playouts, explore=chain.explore,
              max_plies=record.max_plies, policy=chain.policy)
    shapes = ((n, w, h * w, 3), (n, w, h * w), (n,), (n,), (n,), (n,))
    outs = [torch.full(shape, -7, dtype=torch.int32, device="cuda:0") for shape in shapes]
    got = forest.search_tensor(*outs, restart=True, **kw)
    assert all(g is o for g, o in zip(got, outs))
    torch.cuda.synchronize()
    assert_equal([g.cpu().numpy() for g in got], record[2:8], "device tensors over rubbish")
    tree, board, kept = record.plies[0]
    slots = torch.as_tensor(tree, device="cuda:0")
    np.testing.assert_array_equal(b.slots_to_moves_tensor(slots).cpu().numpy(), board)      # the device twin of slots_to_moves
    np.testing.assert_array_equal(b.slots_to_moves_tensor(slots, b.targets_tensor()).cpu().numpy(), b.slots_to_moves(tree))
    got_kept = forest.advance_tensor(slots)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(got_kept.cpu().numpy(), kept)
    b.step_actions(board)
    # the second move on the device, then once more from the host with NULL optional outputs on a forest of its own
    move, record = chain.moves[1], records[1]
    kw = dict(seed=move.seed, iterations=move.iterations, leaf_playouts=move.playouts, explore=chain.explore,
              max_plies=record.max_plies, policy=chain.policy)
    got = forest.search_tensor(**kw)
    torch.cuda.synchronize()
    assert_equal([g.cpu().numpy() for g in got], record[2:8], "device tensors, the second move")
    assert (record.carried > 0).any()
    own = b.search_moves_forest(C, E)
    head = (b._handle, move.seed, move.iterations, move.playouts, chain.explore, record.max_plies, playout_policy(chain.policy), C, E, 1)
    tail = (ctypes.c_void_p(own._buffer.data_ptr()), own._buffer.numel())
    fresh = own.search(restart=True, **kw)
    counts = np.full(shapes[0], -1, dtype=np.int32)
    _abi.check(_abi.lib().bgs_bounce_forest_search(*head, ctypes.c_void_p(counts.ctypes.data), None, None, None, None, None, *tail, 0))
    np.testing.assert_array_equal(counts, fresh[0])
    only = torch.full(shapes[0], -7, dtype=torch.int32, device="cuda:0")
    _abi.check(_abi.lib().bgs_bounce_forest_search(*head, ctypes.c_void_p(only.data_ptr()), None, None, None, None, None, *tail, 1))
    torch.cuda.synchronize()
    np.testing.assert_array_equal(only.cpu().numpy(), fresh[0])
    slots = np.ascontiguousarray(fresh[2])
    _abi.check(_abi.lib().bgs_bounce_forest_advance(b._handle, ctypes.c_void_p(slots.ctypes.data), C, E, None, *tail, 0))     # kept = NULL
    assert (own.advance(np.full(n, -1, dtype=np.int32)) <= fresh[3]).all()
    for f in (forest, own):
        f.close()
    with pytest.raises(RuntimeError, match="closed"):
        forest.search(**kw)
    b.close()


def test_refusals_return_err_arg_and_leave_the_outputs_and_the_forest_untouched():
    import torch

    from simulator.batch import BounceBatch, ConnectBatch
    from simulator.game import _abi

    lib = _abi.lib()
    search, advance, sizes = lib.bgs_bounce_forest_search, lib.bgs_bounce_forest_advance, lib.bgs_bounce_forest_bytes
    U = _abi.POLICY_UNIFORM
    grid = sb.GRIDS["default"]
    h, w = grid.shape
    n, S, E, C = 4, w * h * w, sb.min_edges(h, w), 9
    b = BounceBatch(grid, n)
    need = b.moves_forest_bytes(C, E)
    memory = torch.full((need + 256,), 0x5A, dtype=torch.uint8, device="cuda:0")
    forest = ctypes.c_void_p(memory.data_ptr())
    outs = [np.full(n * S * 3, -5, dtype=np.int32), np.full(n * S, -5, dtype=np.int32)] + [np.full(n, -5, dtype=np.int32) for _ in range(4)]
    ptr = [ctypes.c_void_p(o.ctypes.data) for o in outs]
    tail = (forest, need, 0)

    def untouched():
        torch.cuda.synchronize()
        assert all((o == -5).all() for o in outs) and bool((memory == 0x5A).all())

    def refused(word, *args):
        assert search(*args) == _abi.BGS_ERR_ARG
        assert word in _abi.last_error(), _abi.last_error()
        untouched()

    # (handle, seed, iterations, leaf_playouts, explore, max_plies, policy, nodes_cap, edges, restart, ...)
    refused("iterations", b._handle, 1, 0, 8, 65536, 100, U, C, E, 1, *ptr, *tail)
    refused("leaf_playouts", b._handle, 1, 8, 0, 65536, 100, U, C, E, 1, *ptr, *tail)
    refused("2^29", b._handle, 1, 1 << 15, (1 << 14) + 1, 65536, 100, U, C, E, 1, *ptr, *tail)
    refused("explore", b._handle, 1, 8, 8, -1, 100, U, C, E, 1, *ptr, *tail)
    refused("explore", b._handle, 1, 8, 8, (1 << 18) + 1, 100, U, C, E, 1, *ptr, *tail)
    refused("max_plies", b._handle, 1, 8, 8, 65536, 0, U, C, E, 1, *ptr, *tail)
    for policy in (2, -1):
        refused("policy", b._handle, 1, 8, 8, 65536, 100, policy, C, E, 1, *ptr, *tail)
    for bad in (1, 0, -3, 65537):
        refused("nodes_cap", b._handle, 1, 8, 8, 65536, 100, U, bad, E, 1, *ptr, *tail)
    for bad in (E - 1, 0, -4, (1 << 29) + 1):
        refused("edges", b._handle, 1, 8, 8, 65536, 100, U, C, bad, 1, *ptr, *tail)
    refused("counts", b._handle, 1, 8, 8, 65536, 100, U, C, E, 1, None, *ptr[1:], *tail)
    refused("forest is NULL", b._handle, 1, 8, 8, 65536, 100, U, C, E, 1, *ptr, None, need, 0)
    refused("256-byte", b._handle, 1, 8, 8, 65536, 100, U, C, E, 1, *ptr, ctypes.c_void_p(memory.data_ptr() + 64), need, 0)
    refused("too small", b._handle, 1, 8, 8, 65536, 100, U, C, E, 1, *ptr, forest, need - 1, 0)
    refused("too small", b._handle, 1, 8, 8, 65536, 100, U, C + 30, E, 1, *ptr, forest, need, 0)      # sized for C nodes
    refused("too small", b._handle, 1, 8, 8, 65536, 100, U, C, E + 16, 1, *ptr, forest, need, 0)      # sized for E edges
    size = ctypes.c_size_t(77)
    for bad_nodes, bad_edges, word in ((1, E, "nodes_cap"), (65537, E, "nodes_cap"), (C, E - 1, "edges"), (C, (1 << 29) + 1, "edges")):
        assert sizes(b._handle, bad_nodes, bad_edges, ctypes.byref(size)) == _abi.BGS_ERR_ARG
        assert word in _abi.last_error() and size.value == 77
    assert sizes(b._handle, C, E, None) == _abi.BGS_ERR_ARG and "bytes" in _abi.last_error()
    # the advance
    slots, kept = np.zeros(n, dtype=np.int32), np.full(n, -5, dtype=np.int32)
    at, kept_at = ctypes.c_void_p(slots.ctypes.data), ctypes.c_void_p(kept.ctypes.data)

    def advance_refused(word, *args):
        assert advance(*args) == _abi.BGS_ERR_ARG
        assert word in _abi.last_error(), _abi.last_error()
        assert (kept == -5).all()
        untouched()

    advance_refused("slots", b._handle, None, C, E, kept_at, *tail)
    advance_refused("nodes_cap", b._handle, at, 1, E, kept_at, *tail)
    advance_refused("edges", b._handle, at, C, E - 1, kept_at, *tail)
    advance_refused("forest is NULL", b._handle, at, C, E, kept_at, None, need, 0)
    advance_refused("256-byte", b._handle, at, C, E, kept_at, ctypes.c_void_p(memory.data_ptr() + 64), need, 0)
    advance_refused("too small", b._handle, at, C, E, kept_at, forest, need - 1, 0)
    # misaligned device outputs, each in turn
    dev = [torch.full((o.size + 4,), -5, dtype=torch.int32, device="cuda:0") for o in outs]
    for bad in range(6):
        where = [ctypes.c_void_p(d.data_ptr() + (4 if j == bad else 0)) for j, d in enumerate(dev)]
        assert search(b._handle, 1, 8, 8, 65536, 100, U, C, E, 1, *where, forest, need, 1) == _abi.BGS_ERR_ARG
        assert "aligned" in _abi.last_error() and NAMES[bad] in _abi.last_error()
    dev_slots = torch.zeros(n + 1, dtype=torch.int32, device="cuda:0")
    assert advance(b._handle, ctypes.c_void_p(dev_slots.data_ptr() + 2), C, E, None, forest, need, 1) == _abi.BGS_ERR_ARG
    assert "slots" in _abi.last_error()
    torch.cuda.synchronize()
    assert all(bool((d == -5).all()) for d in dev)
    untouched()
    # Connect and generic batches; the Connect forest keeps refusing Bounce
    connect = ConnectBatch(6, 7, 4, n)
    refused("Bounce", connect._handle, 1, 8, 8, 65536, 100, U, C, E, 1, *ptr, *tail)
    advance_refused("Bounce", connect._handle, at, C, E, kept_at, *tail)
    assert sizes(connect._handle, C, E, ctypes.byref(size)) == _abi.BGS_ERR_ARG and "Bounce" in _abi.last_error() and size.value == 77
    assert lib.bgs_connect_forest_bytes(b._handle, C, ctypes.byref(size)) == _abi.BGS_ERR_ARG and "Connect" in _abi.last_error()
    with pytest.raises(ValueError, match="Connect batches only"):
        b.search_forest(C)
    tall = np.zeros((9, 8), dtype=np.int8)      # 72 cells: a generic board
    tall[1] = tall[7] = 1
    generic = BounceBatch(tall, n)
    big = [np.full(n * 8 * 72 * 3, -5, dtype=np.int32), np.full(n * 8 * 72, -5, dtype=np.int32)] + [np.full(n, -5, dtype=np.int32) for _ in range(4)]
    assert search(generic._handle, 1, 8, 8, 65536, 100, U, C, 8 * 8 * 7, 1, *[ctypes.c_void_p(o.ctypes.data) for o in big], *tail) == _abi.BGS_ERR_ARG
    assert "bit-packed" in _abi.last_error() and all((o == -5).all() for o in big)
    advance_refused("bit-packed", generic._handle, at, C, 8 * 8 * 7, kept_at, *tail)
    # the least of everything is taken
    assert search(b._handle, 1, 1, 1, 0, 1, U, 2, E, 1, *ptr, *tail) == _abi.BGS_OK
    # the Python layer
    with pytest.raises(ValueError, match="nodes_cap"):
        b.search_moves_forest(1)
    with pytest.raises(ValueError, match="edges"):
        b.moves_forest_bytes(C, E - 1)
    f = b.search_moves_forest(C, E)
    with pytest.raises(ValueError, match="policy"):
        f.search(policy="greedy")
    with pytest.raises(ValueError, match="iterations"):
        f.search(iterations=0)
    with pytest.raises(TypeError, match="slots"):
        f.advance(np.zeros(n + 1, dtype=np.int32))
    f.close()
    for batch in (b, connect, generic):
        batch.close()


def test_the_reuse_agent_plays_the_models_game():
    """BounceTreeSearchAgent(reuse=True) from the start of the default grid: its own move, then the scripted reply (the move
    the model's chain recorded), and every search equals the model's -- carried nodes included, so the agent read both moves
    off the grids and advanced by them"""
    from simulator.agents import BounceTreeSearchAgent
    from simulator.game.bounce import Config, State

    chain = bf.AGENT_CHAINS[0]
    records, _ = bf.chain_expected("agent", True)
    grid = bf.chain_grid(chain)
    h, w = grid.shape
    config = Config(grid)
    move = chain.moves[0]
    agent = BounceTreeSearchAgent(iterations=move.iterations, leaf_playouts=move.playouts, explore=chain.explore, policy=chain.policy,
                                  seed=SEED, reuse=True)
    assert agent.capacity == chain.nodes == 2 * move.iterations + 1 and agent.edges is None
    plain = BounceTreeSearchAgent(iterations=move.iterations, leaf_playouts=move.playouts, explore=chain.explore, policy=chain.policy,
                                  seed=SEED)
    for m, record in enumerate(records):
        g, player, winner, plies = record.roots
        states = [State._fresh(config, *config._engine().load(g[k], int(player[k]), -1, int(plies[k]))) for k in range(bf.AGENT_STATES)]
        if m == 0:
            want = plain.search(states, first_game=chain.first_game)
            assert len(want) == 5
        if m == len(records) - 1:               # the last move through predict_many: the shares of the root's visits
            many = agent.predict_many(states, first_game=chain.first_game)
            for k, (s, shares) in enumerate(zip(states, many)):
                total = int(record.visits[k].sum())
                assert total > move.iterations * move.playouts or record.carried[k] == 0
                assert shares == {a: float(record.visits[k, a._source[0], a._target[1] * w + a._target[0]]) / total for a in s.actions}
                assert abs(sum(shares.values()) - 1.0) < 1e-12
            break
        got = agent.search(states, first_game=chain.first_game)
        assert_equal(got, record[2:8], f"agent, move {m}")
        if m == 0:
            assert_equal(got[:5], want, "the first search is the plain agent's")
    assert any((r.carried > 0).any() for r in records[1:-1]) or (records[-1].carried > 0).any()
    agent.close()
    plain.close()
