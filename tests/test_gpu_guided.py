"""The PUCT search with caller-evaluated leaves (bgs_connect_guided_step, ConnectBatch.guided_search, GuidedSearchAgent)
against the CPU statement of tests/guided_expected.py: leaf_grid, leaf_player, leaf_kind, visits, scores, best and nodes
bit for bit after every call, over the corner boards of tests/fuzz_cases.py.  The device is fed the rows `fake_network`
computes from the device's own leaves.  tests/test_guided_expected.py states what the CPU statement holds.  After
`begin`, a call in the middle and the last call of every run the whole trees are read back from the caller's tensor and
compared with the statement's (tests/guided_shares.py): header, path and every node in use.

Everything here needs a real MI355X: `pytest -m gpu`.
"""

import ctypes
import functools

import numpy as np
import pytest

from oracle import oracle
from tests import fuzz_cases as fc
from tests import guided_expected as ge
from tests import guided_shares as gs
from tests.guided_torch import torch_evaluator

pytestmark = pytest.mark.gpu

SIMULATIONS = 48
NAMES = ("leaf_grid", "leaf_player", "leaf_kind", "visits", "scores", "best", "nodes")
CORNERS = list(fc.CONNECT_CORNERS)
CPUCT = {"6x7x7": 0, "8x8x6": 4096}           # one case each; 320 everywhere else


def load(h, w, k, roots):
    from simulator.batch import ConnectBatch

    grid, player, winner, plies = roots
    b = ConnectBatch(h, w, k, grid.shape[0], use_torch=True)
    assert (b.write_state(grid, player, winner, plies) == 0).all()
    b.reset_steps()
    return b


def snapshot(b):
    return b.grid.tobytes(), b.player.tobytes(), b.winner.tobytes(), b.plies.tobytes()


def host(outs):
    return tuple(x.cpu().numpy() for x in outs)


def rows(got, evaluate=ge.fake_network):
    """the evaluator's rows for the leaves of a call, as device tensors"""
    import torch

    priors, values = evaluate(got[0], got[1])
    return torch.from_numpy(priors).cuda(), torch.from_numpy(values).cuda()


def assert_equal(got, want, what):
    for name, g, w in zip(NAMES, got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, f"{name} {what}"
        np.testing.assert_array_equal(g, w, err_msg=f"{name} {what}")


def poisoned(b, capacity, cpuct):
    """a GuidedSearch whose memory holds 0xA5 in every byte: the first call restarts it whatever it holds"""
    guided = b.guided_search(capacity, cpuct)
    guided._buffer.fill_(0xA5)
    return guided


TREE_CALLS = (0, SIMULATIONS // 2, SIMULATIONS)       # the calls after which the whole trees are read back


@functools.lru_cache(maxsize=None)
def expected_run(key, capacity, cpuct):
    """(every call's outputs, {call: every tree after it, decoded} for TREE_CALLS) of Guided.run"""
    case = fc.connect_case(key)
    n = case.roots[0].shape[0]
    model = ge.Guided(case.h, case.w, case.k, n, capacity, cpuct)
    trees = {}

    def keep(call):
        if call in TREE_CALLS:
            trees[call] = [gs.model_tree_connect(model, i) for i in range(n)]

    calls = model.run(case.roots, ge.fake_network, SIMULATIONS, after_call=keep)
    return calls, trees


def expected(key, capacity, cpuct):
    return expected_run(key, capacity, cpuct)[0]


def device_trees(guided):
    """every tree of a GuidedSearch, read back and decoded (tests/guided_shares.py)"""
    b = guided.batch
    h, w = b.height, b.width
    stride = b.guided_bytes(guided.capacity) // b.n
    assert stride == 4 * gs.connect_share_words(h, w, guided.capacity)
    words = guided._buffer.cpu().numpy().view(np.uint32).reshape(b.n, stride // 4)
    return [gs.decode_connect(words[i], h, w, (w * (h + 1) + 63) // 64, guided.capacity) for i in range(b.n)]


def assert_same_trees(guided, want, what):
    got = device_trees(guided)
    assert len(got) == len(want)
    for i, (device, model) in enumerate(zip(got, want)):
        gs.assert_same_tree(device, model, f"{what} tree {i}")


def run_against(key, capacity, cpuct):
    case = fc.connect_case(key)
    want, trees = expected_run(key, capacity, cpuct)
    b = load(case.h, case.w, case.k, case.roots)
    before = snapshot(b)
    guided = poisoned(b, capacity, cpuct)
    got = host(guided.begin())
    assert_equal(got, want[0], f"{key} begin")
    assert_same_trees(guided, trees[0], f"{key} C = {capacity} begin")
    for t in range(SIMULATIONS):
        call = guided.finish if t == SIMULATIONS - 1 else guided.step
        got = host(call(*rows(got)))
        assert_equal(got, want[t + 1], f"{key} C = {capacity} call {t + 1}")
        if t + 1 in trees:                          # the whole trees: in the middle and after the last call
            assert_same_trees(guided, trees[t + 1], f"{key} C = {capacity} call {t + 1}")
    assert sorted(trees) == list(TREE_CALLS)
    print(f"{fc.describe(case)}: C = {capacity}, cpuct = {cpuct}, nodes {got[6].tolist()}, best {got[5].tolist()}")
    assert snapshot(b) == before and b.steps == 0               # the boards and bgs_steps are untouched
    guided.close()
    b.close()


@pytest.mark.parametrize("key", CORNERS)
def test_every_call_equals_the_statement(key):
    run_against(key, SIMULATIONS + 1, CPUCT.get(key, 320))


@pytest.mark.parametrize("capacity", (2, 3))
@pytest.mark.parametrize("key", CORNERS)
def test_trees_that_run_out_of_room_equal_the_statement(key, capacity):
    run_against(key, capacity, 320)


def stepped(case, roots, columns):
    """`roots` after `columns` (negative: the board stays), by the oracle"""
    orc = oracle.ConnectOracle(case.h, case.w, case.k, roots[0].shape[0])
    orc.grid[:], orc.player[:], orc.winner[:], orc.plies[:] = roots
    assert (orc.step_actions(columns)[columns >= 0] == 0).all()
    return orc.grid.copy(), orc.player.copy(), orc.winner.copy(), orc.plies.copy()


def test_boards_stepped_between_two_calls_restart_their_trees():
    key = "10x7x6"
    case = fc.connect_case(key)
    n = case.roots[0].shape[0]
    model = ge.Guided(case.h, case.w, case.k, n, SIMULATIONS + 1, 320)
    b = load(case.h, case.w, case.k, case.roots)
    guided = poisoned(b, SIMULATIONS + 1, 320)
    roots = case.roots
    got, want = host(guided.begin()), model.step(roots, flags=ge.RESTART)
    assert_equal(got, want, "begin")
    for t in range(SIMULATIONS):
        if t == 20:      # every second running board plays its lowest legal column: its tree restarts, the others carry on
            legal = oracle_legal(case, roots)
            columns = np.where((roots[2] == -1) & (np.arange(n) % 2 == 0), legal.argmax(axis=1), -1).astype(np.int32)
            assert (columns >= 0).sum() >= 4
            assert (b.step_actions(columns)[columns >= 0] == 0).all()
            roots = stepped(case, roots, columns)
        priors, values = rows(got)
        flags = ge.FINISH if t == SIMULATIONS - 1 else 0
        last, got = got, host((guided.finish if flags else guided.step)(priors, values))
        want = model.step(roots, priors.cpu().numpy(), values.cpu().numpy(), flags=flags)
        assert_equal(got, want, f"call {t + 1}")
        if t == 20:
            moved, running = columns >= 0, roots[2] == -1
            assert (got[6][moved] == 0).all() and not got[3][moved].any()                  # emptied: the root is the leaf again
            assert (got[2][moved & running] == ge.EVALUATE).all() and (got[2][moved & ~running] == ge.IDLE).all()
            np.testing.assert_array_equal(got[0][moved], roots[0][moved])
            # the others carry on: a visit more than a call ago, and no node fewer
            assert (got[3][~moved & running].sum(axis=1) == 20).all() and (last[3][~moved & running].sum(axis=1) == 19).all()
            assert (got[6][~moved] >= last[6][~moved]).all() and got[6][~moved].sum() > 0
    guided.close()
    b.close()


def oracle_legal(case, roots):
    orc = oracle.ConnectOracle(case.h, case.w, case.k, roots[0].shape[0])
    orc.grid[:], orc.player[:], orc.winner[:], orc.plies[:] = roots
    return orc.legal().astype(bool)


def test_two_parts_of_a_batch_equal_the_whole():
    key = "12x8x4"
    case = fc.connect_case(key)
    cut = case.roots[0].shape[0] // 2 + 1
    parts = (slice(None), slice(0, cut), slice(cut, None))
    batches = [load(case.h, case.w, case.k, tuple(a[part] for a in case.roots)) for part in parts]
    searches = [poisoned(b, 17, 320) for b in batches]
    got = [host(g.begin()) for g in searches]
    for t in range(SIMULATIONS):
        got = [host((g.finish if t == SIMULATIONS - 1 else g.step)(*rows(x))) for g, x in zip(searches, got)]
        for name, whole, first, second in zip(NAMES, *got):
            np.testing.assert_array_equal(whole, np.concatenate([first, second]), err_msg=f"{name} call {t + 1}")
    assert_equal(got[0], ge.Guided(case.h, case.w, case.k, case.roots[0].shape[0], 17, 320).run(case.roots, ge.fake_network, SIMULATIONS)[-1], key)
    for x in searches + batches:
        x.close()


def test_every_refusal_leaves_outputs_and_trees_untouched():
    import torch

    from simulator.batch import BounceBatch, ConnectBatch
    from simulator.game import _abi

    lib = _abi.lib()
    n, h, w, C = 4, 6, 7, 16
    b = ConnectBatch(h, w, 4, n, use_torch=True)
    need = b.guided_bytes(C)
    assert need % 256 == 0 and need >= n * (64 + 4 * h * w + 16 * w * C)
    trees = torch.full((need + 256,), 0x5A, dtype=torch.uint8, device="cuda:0")
    shapes = ((n * h * w, torch.int8), (n, torch.int8), (n, torch.int32), (n * w, torch.int32), (n * w, torch.int32), (n, torch.int32),
              (n, torch.int32))
    outs = [torch.full((size + 16,), 7, dtype=dtype, device="cuda:0") for size, dtype in shapes]
    priors = torch.full((n * w + 16,), 0.5, dtype=torch.float32, device="cuda:0")
    values = torch.zeros(n + 16, dtype=torch.float32, device="cuda:0")

    def p(t, offset=0):
        return ctypes.c_void_p(t.data_ptr() + offset)

    def call(handle=None, capacity=C, cpuct=320, flags=0, pr=p(priors), va=p(values), out=None, tr=p(trees), size=need):
        out = [p(o) for o in outs] if out is None else out
        return lib.bgs_connect_guided_step(b._handle if handle is None else handle, capacity, cpuct, flags, pr, va, *out, tr, size)

    def refused(word, **kw):
        assert call(**kw) == _abi.BGS_ERR_ARG, (word, kw)
        assert word in _abi.last_error(), (word, _abi.last_error())
        torch.cuda.synchronize()
        assert all(bool((o == 7).all()) for o in outs) and bool((trees == 0x5A).all()), word

    grid = np.zeros((9, 6), dtype=np.int8)
    grid[1] = grid[7] = [1, 2, 3, 3, 2, 1]
    bounce = BounceBatch(grid, n)
    generic = ConnectBatch(20, 20, 5, n)
    size = ctypes.c_size_t(77)
    for word, other in (("Connect", bounce), ("bit-packed", generic)):
        refused(word, handle=other._handle)
        assert lib.bgs_connect_guided_bytes(other._handle, C, ctypes.byref(size)) == _abi.BGS_ERR_ARG and size.value == 77
    for method in (bounce.guided_search, bounce.guided_bytes):
        with pytest.raises(ValueError, match="Connect"):
            method(C)
    with pytest.raises(ValueError, match="bit-packed"):
        generic.guided_search(C)
    for capacity in (1, 0, -5, _abi.GUIDED_MAX_CAPACITY + 1):
        refused("capacity", capacity=capacity)
        assert lib.bgs_connect_guided_bytes(b._handle, capacity, ctypes.byref(size)) == _abi.BGS_ERR_ARG and size.value == 77
    for cpuct in (-1, 4097):
        refused("cpuct", cpuct=cpuct)
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
        refused(f"{name} must be 16-byte", out=[p(o, 4 if x == j else 0) for x, o in enumerate(outs)])
    refused("too small", size=need - 1)
    # the Python surface: the range of cpuct, begin() first, the evaluator's tensors, a closed search
    with pytest.raises(ValueError, match="cpuct"):
        b.guided_search(C, cpuct=4097)
    with pytest.raises(ValueError, match="capacity"):
        b.guided_search(1)
    own = b.guided_search(C)
    with pytest.raises(RuntimeError, match="begin"):
        own.step(priors[: n * w].view(n, w), values[:n])
    own.begin()
    with pytest.raises(TypeError, match="priors"):
        own.step(priors[: n * w].view(n, w).double(), values[:n])
    with pytest.raises(TypeError, match="values"):
        own.step(priors[: n * w].view(n, w), values[: n - 1])
    # the optional outputs may be NULL, and RESTART reads neither priors nor values
    assert call(flags=_abi.GUIDED_RESTART, pr=None, va=None, out=[p(o) for o in outs[:3]] + [None] * 4) == _abi.BGS_OK
    torch.cuda.synchronize()
    assert bool((outs[2][:n] == ge.EVALUATE).all()) and all(bool((o == 7).all()) for o in outs[3:])
    own.close()
    with pytest.raises(RuntimeError, match="closed"):
        own.begin()
    for batch in (b, bounce, generic):
        batch.close()


def test_the_agent_equals_the_batch_call():
    from simulator.batch import ConnectBatch
    from simulator.game.connect import Config
    from simulator.guided import GuidedSearchAgent

    states = [Config(6, 7, 4).sample_initial_state()]
    for c in (3, 3, 2, 4, 3):
        states.append(states[-1].action_at(c).sample_next_state())
    agent = GuidedSearchAgent(torch_evaluator, simulations=32, cpuct=256)
    assert agent.capacity == 33
    visits, scores, best, nodes = agent.search(states)
    b = ConnectBatch(6, 7, 4, len(states), use_torch=True)
    assert (b.write_state(np.stack([s.grid for s in states]), np.array([s.player for s in states], dtype=np.int8),
                          np.full(len(states), -1, dtype=np.int8)) == 0).all()
    guided = b.guided_search(33, cpuct=256)
    want = host(guided.run(torch_evaluator, 32))
    assert (want[2] == ge.IDLE).all() and (want[3].sum(axis=1) == 31).all()
    for name, g, x in zip(NAMES[3:], (visits, scores, best, nodes), want[3:]):
        np.testing.assert_array_equal(g, x, err_msg=name)
    assert [a.column for a in agent.choose_many(states)] == want[5].tolist()
    shares = agent.predict_many(states)
    for k, s in enumerate(states):
        assert [shares[k][a] for a in s.actions] == [want[3][k][a.column] / 31 for a in s.actions]
    assert agent.choose(states[2]).column == want[5][2] and agent.predict(states[2]) == shares[2]
    agent.close()
    guided.close()
    b.close()
