"""The PUCT search with caller-evaluated leaves for Bounce (bgs_bounce_guided_step, BounceBatch.guided_moves_search,
BounceGuidedSearchAgent) against the CPU statement of tests/bounce_guided_expected.py: leaf_grid, leaf_player, leaf_kind,
leaf_targets, visits, scores, best, nodes and used bit for bit after every call, over the corner boards of
tests/fuzz_cases.py from tree memory that holds 0xA5 in every byte.  The device is fed the rows `fake_network_moves`
computes from the device's own leaves.  tests/test_bounce_guided_expected.py states what the CPU statement holds and that
the sweeps here meet every branch.  After `begin`, a call in the middle and the last call of every run the whole trees
are read back from the caller's tensor and compared with the statement's (tests/guided_shares.py): header, edges, node
table and path in use.

Every launch is one wave a root over at most 20 roots; the CPU model, computed once a run and shared, is the slower side.

Everything here needs a real MI355X: `pytest -m gpu`.
"""

import ctypes

import numpy as np
import pytest

from oracle import oracle
from tests import bounce_guided_expected as bg
from tests import fuzz_cases as fc
from tests import guided_shares as gs
from tests.guided_torch import torch_evaluator_moves as torch_evaluator
from tests.search_bounce_expected import _actions, min_edges

pytestmark = pytest.mark.gpu

SIMULATIONS = bg.SIMULATIONS
NAMES = bg.NAMES
CORNERS = list(fc.BOUNCE_CORNERS)


def load(grid, roots):
    from simulator.batch import BounceBatch

    b = BounceBatch(grid, roots[0].shape[0], use_torch=True)
    assert (b.write_state(*roots) == 0).all()
    b.reset_steps()
    return b


def snapshot(b):
    return b.grid.tobytes(), b.player.tobytes(), b.winner.tobytes(), b.plies.tobytes()


def host(outs):
    """the nine outputs on the host; leaf_targets as the unsigned masks they are"""
    out = [x.cpu().numpy() for x in outs]
    out[3] = out[3].view(np.uint64)
    return tuple(out)


def rows(got, evaluate=bg.fake_network_moves):
    """the evaluator's rows for the leaves of a call, as device tensors"""
    import torch

    priors, values = evaluate(got[0], got[1], got[3])
    return torch.from_numpy(priors).cuda(), torch.from_numpy(values).cuda()


def assert_equal(got, want, what):
    for name, g, w in zip(NAMES, got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, f"{name} {what}"
        np.testing.assert_array_equal(g, w, err_msg=f"{name} {what}")


def poisoned(b, nodes, edges, cpuct=320, max_plies=65535):
    """a GuidedMovesSearch whose memory holds 0xA5 in every byte: the first call restarts it whatever it holds"""
    guided = b.guided_moves_search(nodes, edges, cpuct, max_plies)
    guided._buffer.fill_(0xA5)
    return guided


def device_trees(guided):
    """every tree of a GuidedMovesSearch, read back and decoded (tests/guided_shares.py)"""
    b = guided.batch
    stride = b.guided_moves_bytes(guided.nodes, guided.edges) // b.n
    assert stride == 4 * gs.bounce_share_words(guided.nodes, guided.edges)
    words = guided._buffer.cpu().numpy().view(np.uint32).reshape(b.n, stride // 4)
    return [gs.decode_bounce(words[i], guided.nodes, guided.edges) for i in range(b.n)]


def assert_same_trees(guided, want, what):
    got = device_trees(guided)
    assert len(got) == len(want)
    for i, (device, model) in enumerate(zip(got, want)):
        gs.assert_same_tree(device, model, f"{what} tree {i}")


def run_against(key, sweep):
    grid, roots, nodes, edges, cpuct, max_plies = bg.sweep_arguments(key, sweep)
    model, want = bg.sweep_expected(key, sweep)
    b = load(grid, roots)
    before = snapshot(b)
    guided = poisoned(b, nodes, edges, cpuct, max_plies)
    got = host(guided.begin())
    assert_equal(got, want[0], f"{key} {sweep} begin")
    assert_same_trees(guided, model.trees[0], f"{key} {sweep} begin")
    for t in range(SIMULATIONS):
        call = guided.finish if t == SIMULATIONS - 1 else guided.step
        got = host(call(*rows(got)))
        assert_equal(got, want[t + 1], f"{key} {sweep} call {t + 1}")
        if t + 1 in model.trees:                    # the whole trees: in the middle and after the last call
            assert_same_trees(guided, model.trees[t + 1], f"{key} {sweep} call {t + 1}")
    assert sorted(model.trees) == list(bg.TREE_CALLS)
    print(f"bounce corner {key!r} {sweep}: C = {nodes}, E = {edges}, cpuct = {cpuct}, cap = {max_plies}, nodes {got[7].tolist()}, "
          f"used {got[8].tolist()}, best {got[6].tolist()}, met {model.seen}")
    assert snapshot(b) == before and b.steps == 0               # the boards and bgs_steps are untouched
    guided.close()
    b.close()


@pytest.mark.parametrize("key", CORNERS)
def test_every_call_equals_the_statement(key):
    run_against(key, "main")


@pytest.mark.parametrize("sweep", ("two_nodes", "three_nodes", "dry_pool"))
@pytest.mark.parametrize("key", CORNERS)
def test_starved_trees_equal_the_statement(key, sweep):
    """C = 2 and 3 with the default pool: a full node table; C = 49 with E = BGS_BOUNCE_SEARCH_MIN_EDGES: a dry pool"""
    run_against(key, sweep)


@pytest.mark.parametrize("key", CORNERS)
def test_a_cap_among_the_roots_equals_the_statement(key):
    """max_plies in the middle of the roots' ply counts: roots at or beyond it have every leaf capped, the others some"""
    run_against(key, "capped")


def stepped(grid, roots, moves):
    """`roots` after `moves` int32[n, 4] (a negative row: the board stays), by the oracle"""
    orc = oracle.BounceOracle(grid, roots[0].shape[0])
    orc.grid[:], orc.player[:], orc.winner[:], orc.plies[:] = roots
    assert (orc.step_actions(moves)[moves[:, 0] >= 0] == 0).all()
    return orc.grid.copy(), orc.player.copy(), orc.winner.copy(), orc.plies.copy()


def test_stepped_boards_and_another_cap_restart_the_trees():
    """boards stepped between two calls restart only their own trees; a call under another max_plies restarts them all"""
    case = fc.bounce_case("default")
    grid, roots = case.grid, case.roots
    n = roots[0].shape[0]
    model = bg.GuidedMoves(grid, n, SIMULATIONS + 1)
    b = load(grid, roots)
    guided = poisoned(b, SIMULATIONS + 1, None)
    got, want = host(guided.begin()), model.step(roots, flags=bg.RESTART)
    assert_equal(got, want, "begin")
    cap = None
    for t in range(SIMULATIONS):
        if t == 16:      # every second running board plays its first legal move: its tree restarts, the others carry on
            moves = np.full((n, 4), -1, dtype=np.int32)
            for i in np.flatnonzero((roots[2] == -1) & (np.arange(n) % 2 == 0)):
                (sx, sy), (tx, ty) = _actions(grid, (roots[0][i], int(roots[1][i]), int(roots[3][i])))[0]
                moves[i] = (sx, sy, tx, ty)
            assert (moves[:, 0] >= 0).sum() >= 4
            assert (b.step_actions(moves)[moves[:, 0] >= 0] == 0).all()
            roots = stepped(grid, roots, moves)
        if t == 32:      # the cap changes: a capped sentinel is only true under the cap it was written with
            cap = guided.max_plies = 4096
        priors, values = rows(got)
        flags = bg.FINISH if t == SIMULATIONS - 1 else 0
        restarts = list(model.restarts)
        last, got = got, host((guided.finish if flags else guided.step)(priors, values))
        want = model.step(roots, priors.cpu().numpy(), values.cpu().numpy(), flags=flags, max_plies=cap)
        assert_equal(got, want, f"call {t + 1}")
        running = roots[2] == -1
        if t == 16:
            moved = moves[:, 0] >= 0
            assert [model.restarts[i] - restarts[i] for i in range(n)] == [int(moved[i] or not running[i]) for i in range(n)]
            assert (got[7][moved] == 0).all() and not got[4][moved].any()                  # emptied: the root is the leaf again
            assert (got[2][moved & running] == bg.EVALUATE).all() and (got[2][moved & ~running] == bg.IDLE).all()
            np.testing.assert_array_equal(got[0][moved], roots[0][moved])
            carried = ~moved & running
            assert (got[4][carried].sum(axis=(1, 2)) == 16).all() and (last[4][carried].sum(axis=(1, 2)) == 15).all()
            assert (got[7][carried] >= last[7][carried]).all() and got[7][carried].sum() > 0
        if t == 32:
            assert all(model.restarts[i] - restarts[i] == 1 for i in range(n))
            assert not got[7].any() and not got[4].any() and (got[2][running] == bg.EVALUATE).all()
    guided.close()
    b.close()


def test_two_parts_of_a_batch_equal_the_whole():
    case = fc.bounce_case("8x8")
    cut = case.roots[0].shape[0] // 2 + 1
    parts = (slice(None), slice(0, cut), slice(cut, None))
    batches = [load(case.grid, tuple(a[part] for a in case.roots)) for part in parts]
    searches = [poisoned(b, 17, None) for b in batches]
    got = [host(g.begin()) for g in searches]
    for t in range(SIMULATIONS):
        got = [host((g.finish if t == SIMULATIONS - 1 else g.step)(*rows(x))) for g, x in zip(searches, got)]
        for name, whole, first, second in zip(NAMES, *got):
            np.testing.assert_array_equal(whole, np.concatenate([first, second]), err_msg=f"{name} call {t + 1}")
    want = bg.GuidedMoves(case.grid, case.roots[0].shape[0], 17).run(case.roots, bg.fake_network_moves, SIMULATIONS)[-1]
    assert_equal(got[0], want, "8x8")
    for x in searches + batches:
        x.close()


def test_every_refusal_leaves_outputs_and_trees_untouched():
    import torch

    from simulator.batch import BounceBatch, ConnectBatch
    from simulator.game import _abi

    lib = _abi.lib()
    grid = fc.BOUNCE_CORNERS["default"]()
    h, w = grid.shape
    n, C, S = 4, 16, w * h * w
    E = min_edges(h, w) + 64
    b = BounceBatch(grid, n, use_torch=True)
    need = b.guided_moves_bytes(C, E)
    assert need % (256 * n) == 0 and need >= n * (16 * E + 12 * C + 96)     # edges of four words, a table entry and a path word a node
    assert b.guided_moves_bytes(C) == b.guided_moves_bytes(C, min_edges(h, w) + 32 * (C - 1))
    trees = torch.full((need + 256,), 0x5A, dtype=torch.uint8, device="cuda:0")
    shapes = ((n * h * w, torch.int8), (n, torch.int8), (n, torch.int32), (n * w, torch.int64), (n * S, torch.int32), (n * S, torch.int32),
              (n, torch.int32), (n, torch.int32), (n, torch.int32))
    outs = [torch.full((size + 16,), 7, dtype=dtype, device="cuda:0") for size, dtype in shapes]
    priors = torch.full((n * S + 16,), 0.5, dtype=torch.float32, device="cuda:0")
    values = torch.zeros(n + 16, dtype=torch.float32, device="cuda:0")

    def p(t, offset=0):
        return ctypes.c_void_p(t.data_ptr() + offset)

    def call(handle=None, nodes=C, edges=E, cpuct=320, max_plies=65535, flags=0, pr=p(priors), va=p(values), out=None, tr=p(trees),
             size=need):
        out = [p(o) for o in outs] if out is None else out
        return lib.bgs_bounce_guided_step(b._handle if handle is None else handle, nodes, edges, cpuct, max_plies, flags, pr, va, *out,
                                          tr, size)

    def refused(word, **kw):
        assert call(**kw) == _abi.BGS_ERR_ARG, (word, kw)
        assert word in _abi.last_error(), (word, _abi.last_error())
        torch.cuda.synchronize()
        assert all(bool((o == 7).all()) for o in outs) and bool((trees == 0x5A).all()), word

    connect = ConnectBatch(6, 7, 4, n)
    wide = np.zeros((9, 8), dtype=np.int8)      # 72 cells: a generic board
    wide[1] = wide[7] = 1
    generic = BounceBatch(wide, n)
    assert generic.generic
    size = ctypes.c_size_t(77)
    for word, other in (("Bounce batches only", connect), ("bit-packed", generic)):
        refused(word, handle=other._handle)
        assert lib.bgs_bounce_guided_bytes(other._handle, C, E, ctypes.byref(size)) == _abi.BGS_ERR_ARG and size.value == 77
    assert not hasattr(connect, "guided_moves_search")
    with pytest.raises(ValueError, match="bit-packed"):
        generic.guided_moves_search(C, 4096)
    # the Connect entry points keep refusing Bounce batches
    assert lib.bgs_connect_guided_bytes(b._handle, C, ctypes.byref(size)) == _abi.BGS_ERR_ARG and size.value == 77
    assert "Connect batches only" in _abi.last_error()
    for method in (b.guided_search, b.guided_bytes):
        with pytest.raises(ValueError, match="Connect batches only"):
            method(C)
    for nodes in (1, 0, -5, 65537):
        refused("nodes_cap", nodes=nodes)
        assert lib.bgs_bounce_guided_bytes(b._handle, nodes, E, ctypes.byref(size)) == _abi.BGS_ERR_ARG and size.value == 77
    for edges in (min_edges(h, w) - 1, 0, -1, (1 << 29) + 1):
        refused("edges", edges=edges)
        assert lib.bgs_bounce_guided_bytes(b._handle, C, edges, ctypes.byref(size)) == _abi.BGS_ERR_ARG and size.value == 77
    for cpuct in (-1, 4097):
        refused("cpuct", cpuct=cpuct)
    for max_plies in (0, -3):
        refused("max_plies", max_plies=max_plies)
    refused("flag", flags=4)
    refused("flag", flags=_abi.GUIDED_RESTART | 8)
    refused("BGS_GUIDED_FINISH", flags=_abi.GUIDED_RESTART | _abi.GUIDED_FINISH)
    refused("trees is NULL", tr=None)
    for j, name in enumerate(NAMES[:3]):
        refused(f"{name} is NULL", out=[None if x == j else p(o) for x, o in enumerate(outs)])
    refused("priors is NULL", pr=None)
    refused("values is NULL", va=None)
    refused("priors is NULL", pr=None, flags=_abi.GUIDED_FINISH)
    refused("256-byte", tr=p(trees, 64))
    refused("priors must be 16-byte", pr=p(priors, 4))
    refused("values must be 16-byte", va=p(values, 8))
    for j, name in enumerate(NAMES):
        refused(f"{name} must be 16-byte", out=[p(o, 8 if x == j else 0) for x, o in enumerate(outs)])
    refused("too small", size=need - 1)
    # the Python surface: the ranges, begin() first, the evaluator's tensors, a closed search
    with pytest.raises(ValueError, match="cpuct"):
        b.guided_moves_search(C, cpuct=4097)
    with pytest.raises(ValueError, match="max_plies"):
        b.guided_moves_search(C, max_plies=0)
    with pytest.raises(ValueError, match="nodes_cap"):
        b.guided_moves_search(1)
    with pytest.raises(ValueError, match="edges"):
        b.guided_moves_search(C, edges=3)
    own = b.guided_moves_search(C)
    assert own.edges == min_edges(h, w) + 32 * (C - 1)
    good = priors[: n * S].view(n, w, h * w)
    with pytest.raises(RuntimeError, match="begin"):
        own.step(good, values[:n])
    own.begin()
    with pytest.raises(TypeError, match="priors"):
        own.step(good.double(), values[:n])
    with pytest.raises(TypeError, match="priors"):
        own.step(priors[: n * S].view(n, S), values[:n])
    with pytest.raises(TypeError, match="values"):
        own.step(good, values[: n - 1])
    # the optional outputs may be NULL -- leaf_targets among them --, and RESTART reads neither priors nor values
    assert call(flags=_abi.GUIDED_RESTART, pr=None, va=None, out=[p(o) for o in outs[:3]] + [None] * 6) == _abi.BGS_OK
    torch.cuda.synchronize()
    assert bool((outs[2][:n] == bg.EVALUATE).all()) and all(bool((o == 7).all()) for o in outs[3:])
    assert all(bool((o[size:] == 7).all()) for o, (size, _) in zip(outs, shapes))       # nothing behind the rows of the outputs
    # ... and a step with leaf_targets alone NULL gives the other eight outputs of the step with it
    def two_steps(with_targets):
        tr = torch.full((need,), 0xA5, dtype=torch.uint8, device="cuda:0")
        for flags in (_abi.GUIDED_RESTART, 0, 0):
            out = [p(o) for o in outs]
            out[3] = out[3] if with_targets else None
            assert call(flags=flags, out=out, tr=p(tr)) == _abi.BGS_OK
        torch.cuda.synchronize()
        return [o.cpu().numpy().copy() for k, o in enumerate(outs) if k != 3]

    for x, y in zip(two_steps(True), two_steps(False)):
        np.testing.assert_array_equal(x, y)
    own.close()
    with pytest.raises(RuntimeError, match="closed"):
        own.begin()
    for batch in (b, connect, generic):
        batch.close()


def test_the_agent_equals_the_batch_call():
    from simulator.batch import BounceBatch
    from simulator.game.bounce import Config
    from simulator.guided import BounceGuidedSearchAgent, GuidedSearchAgent

    grid = fc.BOUNCE_CORNERS["default"]()
    states = [Config(grid).sample_initial_state()]
    for k in (0, 3, 1, 2, 0):
        acts = states[-1].actions
        states.append(acts[k % len(acts)].sample_next_state())
    assert not any(s.has_ended for s in states)
    agent = BounceGuidedSearchAgent(torch_evaluator, simulations=32, cpuct=256)
    assert agent.nodes == 33 and agent.edges is None
    visits, scores, best, nodes, used = agent.search(states)
    b = BounceBatch(grid, len(states), use_torch=True)
    assert (b.write_state(np.stack([s.grid for s in states]), np.array([s.player for s in states], dtype=np.int8),
                          np.full(len(states), -1, dtype=np.int8), np.array([s._plies for s in states], dtype=np.int32)) == 0).all()
    guided = b.guided_moves_search(33, cpuct=256)
    want = host(guided.run(torch_evaluator, 32))
    assert (want[2] == bg.IDLE).all() and (want[4].sum(axis=(1, 2)) == 31).all() and (want[7] > 0).all()
    for name, g, x in zip(NAMES[4:], (visits, scores, best, nodes, used), want[4:]):
        np.testing.assert_array_equal(g, x, err_msg=name)
    h, w = grid.shape

    def slot(a):
        return a._source[0] * h * w + a._target[1] * w + a._target[0]

    assert [slot(a) for a in agent.choose_many(states)] == want[6].tolist()
    shares = agent.predict_many(states)
    for k, s in enumerate(states):
        assert [shares[k][a] for a in s.actions] == [want[4][k].reshape(-1)[slot(a)] / 31 for a in s.actions]
        assert sum(shares[k].values()) == pytest.approx(1.0)
    assert slot(agent.choose(states[2])) == want[6][2] and agent.predict(states[2]) == shares[2]
    with pytest.raises(ValueError, match="Bounce states only"):
        from simulator.game.connect import Config as ConnectConfig

        agent.search([ConnectConfig(6, 7, 4).sample_initial_state()])
    with pytest.raises(ValueError, match="Connect states only"):
        GuidedSearchAgent(lambda grid, player: None).search(states[:1])
    agent.close()
    guided.close()
    b.close()
