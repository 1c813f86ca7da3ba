"""bgs_connect_guided_advance (GuidedForest, GuidedReuseAgent) against the CPU statement of
tests/guided_advance_expected.py, everything bit for bit: every call's seven outputs and `kept`, and the whole trees, read
back and decoded (tests/guided_shares.py), after every `finish` and after every `advance`.  Trees start on memory that holds
0xA5 in every byte.

* scripted games through the corner geometries at capacities 3, simulations + 1 and 2 * simulations + 1, with advance
  columns of every kind (tests/guided_advance_expected.KINDS), chosen on the CPU;
* Connect4 trees of 300 nodes whose advances cross the chunks of 64 nodes the kernel works in;
* a pending leaf at the ABI level, boards that were not stepped or stepped elsewhere, run(carry=False), two halves of a
  batch, every refusal, an advance replayed from a graph, and the agent.

tests/test_guided_advance_expected.py states what the CPU statement holds.  Everything here needs a real MI355X:
`pytest -m gpu`.
"""

import ctypes

import numpy as np
import pytest

from tests import guided_advance_expected as ga
from tests import guided_expected as ge
from tests import guided_shares as gs
from tests import test_gpu_guided as tc
from tests.guided_torch import torch_evaluator

pytestmark = pytest.mark.gpu


def forest(b, capacity, cpuct=320):
    """a GuidedForest whose memory holds 0xA5 in every byte"""
    from simulator.batch import GuidedForest

    guided = GuidedForest(b, capacity, cpuct)
    guided._buffer.fill_(0xA5)
    return guided


def device(array):
    import torch

    return torch.from_numpy(np.ascontiguousarray(array)).cuda()


def search_against(guided, want, evaluate, carry, what):
    """GuidedForest.run, call by call: `want` is every call's outputs (guided_advance_expected.search)"""
    got = tc.host(guided.resume() if carry else guided.begin())
    tc.assert_equal(got, want[0], f"{what} {'resume' if carry else 'begin'}")
    for t in range(1, len(want)):
        call = guided.finish if t == len(want) - 1 else guided.step
        got = tc.host(call(*tc.rows(got, evaluate)))
        tc.assert_equal(got, want[t], f"{what} call {t}")
    return got


def replay(b, guided, script, evaluate, what):
    """a scripted game on the device: every output, `kept` and every tree equal the statement's"""
    for m, move in enumerate(script):
        search_against(guided, move.calls, evaluate, m > 0, f"{what} move {m}")
        tc.assert_same_trees(guided, move.finished, f"{what} move {m} finished")
        before = tc.snapshot(b), b.steps
        kept = guided.advance(device(move.columns)).cpu().numpy()
        assert (tc.snapshot(b), b.steps) == before                      # the boards and bgs_steps are untouched
        assert kept.dtype == np.int32
        np.testing.assert_array_equal(kept, move.kept, err_msg=f"{what} move {m} kept, columns {move.columns.tolist()} {move.kinds}")
        tc.assert_same_trees(guided, move.advanced, f"{what} move {m} advanced")
        assert (b.step_actions(move.played)[move.played >= 0] == 0).all()


# ---- games through the corners
def test_the_games_hold_every_kind_of_column():
    kinds = {}
    for key in ga.CORNERS:
        roots, ending, ended = ga.corner_roots(key)
        assert 8 <= roots[0].shape[0] <= 16 and ending >= 1 and ended == 1, key
        for capacity in ga.CAPACITIES:
            for move in ga.corner_game(key, capacity)[1]:
                for kind in move.kinds:
                    kinds[kind] = kinds.get(kind, 0) + 1
    for kind in ga.REQUIRED:
        assert kinds.get(kind, 0) >= 1, (kind, kinds)


@pytest.mark.parametrize("capacity", ga.CAPACITIES)
@pytest.mark.parametrize("key", ga.CORNERS)
def test_a_corner_game_equals_the_statement(key, capacity):
    h, w, k = ga.corner_geometry(key)
    model, script = ga.corner_game(key, capacity)
    b = tc.load(h, w, k, script[0].roots)
    guided = forest(b, capacity)
    replay(b, guided, script, ge.fake_network, f"{key} C = {capacity}")
    print(f"{key} C = {capacity}: kept {[move.kept.tolist() for move in script]}")
    guided.close()
    b.close()


# ---- chunk boundaries
@pytest.mark.parametrize("evaluator", list(ga.CHUNK_EVALUATORS))
def test_advances_that_cross_chunks_equal_the_statement(evaluator):
    model, script = ga.chunk_game(evaluator)
    # from the statement, before the device is looked at: more than two chunks kept, and a new root in a later chunk
    assert max(int(move.kept.max()) for move in script) > 128
    if evaluator == "narrow":
        assert any(ga.new_root_index(tree, int(c)) >= 64 and kept >= 1
                   for move in script for tree, c, kept in zip(move.finished, move.columns, move.kept))
    b = tc.load(6, 7, 4, script[0].roots)
    guided = forest(b, ga.CHUNK_CAPACITY)
    replay(b, guided, script, ga.CHUNK_EVALUATORS[evaluator], f"chunks, {evaluator}")
    guided.close()
    b.close()


# ---- a pending leaf, at the ABI level; boards not stepped, or stepped elsewhere
def advance_abi(guided, columns, kept):
    from simulator.game import _abi

    return _abi.lib().bgs_connect_guided_advance(guided.batch._handle, ctypes.c_void_p(columns.data_ptr()), guided.capacity,
                                                 ctypes.c_void_p(kept.data_ptr()), ctypes.c_void_p(guided._buffer.data_ptr()),
                                                 guided._buffer.numel())


def test_a_pending_leaf_is_dropped_or_kept_and_other_boards_restart():
    import torch

    n, capacity = 6, 40
    roots = _connect4(n)
    model = ga.GuidedAdvance(6, 7, 4, n, capacity, 320)
    b = tc.load(6, 7, 4, roots)
    guided = forest(b, capacity)
    got, want = tc.host(guided.begin()), model.step(roots, flags=ge.RESTART)
    for t in range(30):
        tc.assert_equal(got, want, f"call {t}")
        priors, values = ge.fake_network(got[0], got[1])
        got, want = tc.host(guided.step(device(priors), device(values))), model.step(roots, priors, values)
    tc.assert_equal(got, want, "call 30")
    assert all(tree["kind"] != gs.NONE for tree in ga.decoded(model))               # a leaf is pending on every tree
    with pytest.raises(RuntimeError, match=r"finish\(\) comes first"):
        guided.advance(device(np.full(n, -1, dtype=np.int32)))
    # trees 0 .. 3 by their best column, which drops the leaf; trees 4 and 5 stay, leaf included
    columns = np.where(np.arange(n) < 4, want[5], -1).astype(np.int32)
    assert (columns[:4] >= 0).all()
    kept = torch.full((n,), -7, dtype=torch.int32, device="cuda:0")
    assert advance_abi(guided, device(columns), kept) == 0
    np.testing.assert_array_equal(kept.cpu().numpy(), model.advance(columns))
    tc.assert_same_trees(guided, ga.decoded(model), "advanced with a leaf pending")
    after = ga.decoded(model)
    assert all(tree["kind"] == gs.NONE and tree["count"] >= 1 for tree in after[:4]) and all(tree["kind"] != gs.NONE for tree in after[4:])
    # boards 0 and 1 play their column, board 2 another one, board 3 none; boards 4 and 5 stay
    played = columns.copy()
    played[2], played[3] = (columns[2] + 1) % 7, -1
    assert (b.step_actions(played)[played >= 0] == 0).all()
    roots = ga.stepped(6, 7, 4, roots, played)
    priors, values = ge.fake_network(got[0], got[1])                                # the rows of the leaves that 4 and 5 still hold
    got, want = tc.host(guided.step(device(priors), device(values))), model.step(roots, priors, values)
    tc.assert_equal(got, want, "the step after the advance")
    tc.assert_same_trees(guided, ga.decoded(model), "the step after the advance")
    assert got[6][:2].tolist() == kept.cpu().numpy()[:2].tolist() and got[6][2:4].tolist() == [0, 0]      # carried, restarted
    assert (got[3][4:].sum(axis=1) == 30).all()                                     # the kept leaves were applied: 29 + 1 visits
    guided.close()
    b.close()


def _connect4(n):
    from oracle import oracle

    orc = oracle.ConnectOracle(6, 7, 4, n)
    orc.step_actions((np.arange(n) % 7).astype(np.int32))
    return orc.grid.copy(), orc.player.copy(), orc.winner.copy(), orc.plies.copy()


# ---- run(carry=False) is GuidedSearch.run
def test_run_without_carry_is_the_plain_run():
    roots = _connect4(8)
    batches = [tc.load(6, 7, 4, roots) for _ in range(2)]
    plain, kept = tc.poisoned(batches[0], 33, 256), forest(batches[1], 33, 256)
    want, got = tc.host(plain.run(torch_evaluator, 32)), tc.host(kept.run(torch_evaluator, 32))
    tc.assert_equal(got, want, "run")
    for i, (x, y) in enumerate(zip(tc.device_trees(kept), tc.device_trees(plain))):
        gs.assert_same_tree(x, y, f"tree {i}")
    with pytest.raises(RuntimeError, match="carry"):
        forest(batches[1], 33).run(torch_evaluator, 8, carry=True)
    fresh = forest(batches[1], 33)
    for call in (fresh.resume, lambda: fresh.advance(device(np.zeros(8, dtype=np.int32)))):
        with pytest.raises(RuntimeError, match="begin"):
            call()
    fresh.begin()
    with pytest.raises(RuntimeError, match="pending"):
        fresh.resume()
    fresh.close()
    for call in (fresh.resume, lambda: fresh.advance(device(np.zeros(8, dtype=np.int32)))):
        with pytest.raises(RuntimeError, match="closed"):
            call()
    for x in (plain, kept, *batches):
        x.close()


# ---- two halves of a batch equal the whole, the advance included
def test_two_parts_of_a_batch_equal_the_whole():
    key, capacity = "8x8x6", ga.SIMULATIONS + 1
    h, w, k = ga.corner_geometry(key)
    model, script = ga.corner_game(key, capacity)
    n = script[0].roots[0].shape[0]
    cut = n // 2 + 1
    parts = (slice(0, cut), slice(cut, None))
    batches = [tc.load(h, w, k, tuple(a[part] for a in script[0].roots)) for part in parts]
    searches = [forest(b, capacity) for b in batches]
    for m, move in enumerate(script):
        for part, b, guided in zip(parts, batches, searches):
            search_against(guided, [tuple(x[part] for x in call) for call in move.calls], ge.fake_network, m > 0, f"move {m} part {part}")
            np.testing.assert_array_equal(guided.advance(device(move.columns[part])).cpu().numpy(), move.kept[part])
            tc.assert_same_trees(guided, move.advanced[part], f"move {m} part {part}")
            assert (b.step_actions(move.played[part])[move.played[part] >= 0] == 0).all()
    for x in searches + batches:
        x.close()


# ---- refusals
def test_every_refusal_leaves_kept_and_trees_untouched():
    import torch

    from simulator.batch import BounceBatch, ConnectBatch, GuidedForest
    from simulator.game import _abi

    lib = _abi.lib()
    n, h, w, C = 4, 6, 7, 16
    b = ConnectBatch(h, w, 4, n, use_torch=True)
    need = b.guided_bytes(C)
    trees = torch.full((need + 256,), 0x5A, dtype=torch.uint8, device="cuda:0")
    kept = torch.full((n + 16,), 7, dtype=torch.int32, device="cuda:0")
    columns = torch.zeros(n + 16, dtype=torch.int32, device="cuda:0")

    def p(t, offset=0):
        return ctypes.c_void_p(t.data_ptr() + offset)

    def refused(word, handle=None, co=p(columns), capacity=C, ke=p(kept), tr=p(trees), size=need):
        assert lib.bgs_connect_guided_advance(b._handle if handle is None else handle, co, capacity, ke, tr, size) == _abi.BGS_ERR_ARG, word
        assert word in _abi.last_error(), (word, _abi.last_error())
        torch.cuda.synchronize()
        assert bool((kept == 7).all()) and bool((trees == 0x5A).all()), word

    grid = np.zeros((9, 6), dtype=np.int8)
    grid[1] = grid[7] = [1, 2, 3, 3, 2, 1]
    bounce = BounceBatch(grid, n)
    generic = ConnectBatch(20, 20, 5, n)
    refused("Connect", handle=bounce._handle)
    refused("bit-packed", handle=generic._handle)
    for capacity in (1, 0, -5, _abi.GUIDED_MAX_CAPACITY + 1):
        refused("capacity", capacity=capacity)
    # (a capacity the step takes and the advance does not: the size is not looked at before the bound)
    refused("at most 65536", capacity=_abi.GUIDED_ADVANCE_MAX_CAPACITY + 1, size=1 << 62)
    refused("columns is NULL", co=None)
    refused("trees is NULL", tr=None)
    refused("256-byte", tr=p(trees, 64))
    refused("columns must be 16-byte", co=p(columns, 4))
    refused("kept must be 16-byte", ke=p(kept, 8))
    refused("too small", size=need - 1)
    with pytest.raises(ValueError, match="65536"):
        GuidedForest(b, _abi.GUIDED_ADVANCE_MAX_CAPACITY + 1)
    with pytest.raises(ValueError, match="Connect"):
        GuidedForest(bounce, C)
    own = GuidedForest(b, C)
    own.run(torch_evaluator, 4)
    with pytest.raises(TypeError, match="columns"):
        own.advance(columns[:n].to(torch.int64))
    with pytest.raises(TypeError, match="columns"):
        own.advance(None)
    with pytest.raises(TypeError, match="kept"):
        own.advance(columns[:n], kept[: n - 1])
    # kept may be NULL
    assert lib.bgs_connect_guided_advance(b._handle, p(columns), C, None, ctypes.c_void_p(own._buffer.data_ptr()), own._buffer.numel()) == _abi.BGS_OK
    torch.cuda.synchronize()
    assert bool((kept == 7).all())
    own.close()
    for batch in (b, bounce, generic):
        batch.close()


# ---- an advance in a graph
def test_an_advance_replays_from_a_graph():
    """advance, the batch's device step and the resume that follows, captured once as a linear chain on the batch's stream
    and replayed for two moves with `columns` refilled in place: the trees and the outputs of the eager run"""
    import torch

    from simulator.batch import ConnectBatch, GuidedForest

    trees_n, simulations, capacity = 32, 24, 49
    stream = torch.cuda.Stream()

    def start():
        b = ConnectBatch(6, 7, 4, trees_n, use_torch=True)
        assert (b.step_actions((np.arange(trees_n) % 7).astype(np.int32)) == 0).all()
        guided = GuidedForest(b, capacity)
        guided._buffer.fill_(0xA5)
        return b, guided

    def to_finish(guided, outs):
        for t in range(simulations):
            outs = (guided.finish if t == simulations - 1 else guided.step)(*torch_evaluator(outs[0], outs[1]))
        return outs

    def choose(columns, outs):
        """in place: the best column, and every fifth tree stays"""
        columns.copy_(torch.where(torch.arange(trees_n, device=columns.device) % 5 == 4, torch.full_like(outs[5], -1), outs[5]))

    with torch.cuda.stream(stream):
        # the eager run
        b, guided = start()
        columns = torch.zeros(trees_n, dtype=torch.int32, device="cuda:0")
        kept = torch.zeros(trees_n, dtype=torch.int32, device="cuda:0")
        legal = b.legal_tensor()
        eager = []
        outs = guided.begin()
        for move in range(2):
            outs = to_finish(guided, outs)
            choose(columns, outs)
            guided.advance(columns, kept)
            b.step_actions_observe(columns, legal)
            outs = guided.resume()
            torch.cuda.synchronize()
            eager.append(([o.cpu().numpy().copy() for o in outs], kept.cpu().numpy().copy(), tc.device_trees(guided), b.grid.copy()))
        assert eager[0][1].max() > 0 and eager[1][1].max() > 0 and (eager[1][0][2] == ge.EVALUATE).any()
        guided.close()
        b.close()

        # the same game with the three calls replayed from a graph
        b, guided = start()
        legal = b.legal_tensor()
        outs = to_finish(guided, guided.begin())
        choose(columns, outs)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            guided.advance(columns, kept)
            b.step_actions_observe(columns, legal)
            outs = guided.resume()
        for move in range(2):
            if move:
                outs = to_finish(guided, outs)
                choose(columns, outs)
            graph.replay()
            torch.cuda.synchronize()
            want_outs, want_kept, want_trees, want_grid = eager[move]
            for name, got, want in zip(tc.NAMES, outs, want_outs):
                np.testing.assert_array_equal(got.cpu().numpy(), want, err_msg=f"{name}, move {move}")
            np.testing.assert_array_equal(kept.cpu().numpy(), want_kept, err_msg=f"kept, move {move}")
            np.testing.assert_array_equal(b.grid, want_grid)
            for i, (got, want) in enumerate(zip(tc.device_trees(guided), want_trees)):
                gs.assert_same_tree(got, want, f"tree {i}, move {move}")
        guided.close()
        b.close()


# ---- the agent
def host_evaluator(grid, player):
    """ge.fake_network on device tensors: the rows the statement is fed"""
    priors, values = ge.fake_network(grid.cpu().numpy(), player.cpu().numpy())
    return device(priors), device(values)


def test_the_reusing_agent_equals_the_statement():
    from simulator.game.connect import Config
    from simulator.guided import GuidedReuseAgent

    simulations, plies = 24, 3
    start = Config(6, 7, 4).sample_initial_state()
    states = [start.action_at(3).sample_next_state(), start.action_at(2).sample_next_state().action_at(2).sample_next_state()]
    agent = GuidedReuseAgent(host_evaluator, simulations=simulations, cpuct=256)
    assert agent.capacity == 2 * simulations + 1
    model = ga.GuidedAdvance(6, 7, 4, 2, agent.capacity, 256)
    kept_seen = []
    for ply in range(plies):
        grid = np.stack([s.grid for s in states])
        player = np.array([s.player for s in states], dtype=np.int8)
        roots = (grid, player, np.full(2, -1, dtype=np.int8), (grid != -1).sum(axis=(1, 2)).astype(np.int32))
        want_kept = np.zeros(2, dtype=np.int32)
        if ply:
            for columns in (own, reply):
                want_kept = model.advance(np.array(columns, dtype=np.int32))
        want = ga.search(model, roots, ge.fake_network, simulations, carry=ply > 0)[-1]
        visits, scores, best, nodes, kept = agent.search(states)
        for name, got, x in zip(tc.NAMES[3:] + ("kept",), (visits, scores, best, nodes, kept), want[3:] + (want_kept,)):
            np.testing.assert_array_equal(got, x, err_msg=f"{name}, ply {ply}")
        kept_seen.append(kept.tolist())
        # the agent's move, then a reply: the lowest column with room (state 0) or none yet (state 1 on the last ply)
        own = [int(c) for c in best]
        states = [s.action_at(c).sample_next_state() for s, c in zip(states, own)]
        reply = [int(np.flatnonzero(s.grid[-1] == -1)[0]) for s in states]
        states = [s.action_at(c).sample_next_state() for s, c in zip(states, reply)]
        assert all(not s.has_ended for s in states)
    assert kept_seen[0] == [0, 0] and max(max(k) for k in kept_seen[1:]) > 0, kept_seen
    # predict: shares of the root's visits, carried ones included
    for columns in (own, reply):
        model.advance(np.array(columns, dtype=np.int32))
    grid = np.stack([s.grid for s in states])
    roots = (grid, np.array([s.player for s in states], dtype=np.int8), np.full(2, -1, dtype=np.int8), (grid != -1).sum(axis=(1, 2)).astype(np.int32))
    want = ga.search(model, roots, ge.fake_network, simulations, carry=True)[-1]
    shares = agent.predict_many(states)
    assert (want[3].sum(axis=1) > simulations).any()
    for k, s in enumerate(states):
        assert [shares[k][a] for a in s.actions] == [want[3][k][a.column] / want[3][k].sum() for a in s.actions]
    agent.close()
