"""The guided searches (bgs_connect_guided_step, bgs_bounce_guided_step) against their CPU statements beyond the corner
runs of tests/test_gpu_guided.py and tests/test_gpu_bounce_guided.py, everything bit for bit:

* the random keys of tests/guided_fuzz_cases.py -- random geometries, start grids and roots, small capacities and pools,
  every cpuct, boards stepped between two calls -- from tree memory that holds 0xA5: every output after every call, the
  whole trees (tests/guided_shares.py) after the last;
* primed trees: after 24 simulations the counts of every tree are scaled to a root total next to 2^19, next to 700^2 or
  to 400000 with arms at q = 4096 and q = 0 (PLANS of tests/guided_shares.py), on the device and in the statement alike,
  and 8 more calls run the arithmetic at high counts: the integer root up to 2^31, 2 s up to 2^31, the 44-bit product of
  the exploration term, the stop at BGS_GUIDED_MAX_VISITS;
* a step captured in a graph with its evaluator: 8 (evaluate, step) pairs replayed three times equal 24 eager steps, in
  every output and in every tree.

tests/test_guided_fuzz_cases.py states what the keys hold, tests/test_guided_shares.py that the comparisons here tell four
wrong statements from the right one.  The CPU statements are computed once a session and shared; they are the slower side.

Everything here needs a real MI355X: `pytest -m gpu`.
"""

import numpy as np
import pytest

from tests import bounce_guided_expected as bg
from tests import fuzz_cases as fc
from tests import guided_expected as ge
from tests import guided_fuzz_cases as gf
from tests import guided_shares as gs
from tests import test_gpu_bounce_guided as tb
from tests import test_gpu_guided as tc
from tests.guided_torch import torch_evaluator, torch_evaluator_moves
from tests.search_bounce_expected import _actions

pytestmark = pytest.mark.gpu

CALLS = gs.PRIMED_BEFORE + gs.PRIMED_AFTER


# ---- the random keys
@pytest.mark.parametrize("key", gf.connect_keys())
def test_connect_key_equals_the_statement(key):
    case = gf.connect_key(key)
    model, want = gf.connect_expected(key)
    b = tc.load(case.h, case.w, case.k, case.roots)
    guided = tc.poisoned(b, case.capacity, case.cpuct)
    got = tc.host(guided.begin())
    tc.assert_equal(got, want[0], f"key {key} begin")
    for t in range(gf.SIMULATIONS):
        if t + 1 == gf.RESTART_CALL and (case.columns >= 0).any():     # the stepped boards restart their trees, the others carry on
            assert (b.step_actions(case.columns)[case.columns >= 0] == 0).all()
        call = guided.finish if t == gf.SIMULATIONS - 1 else guided.step
        got = tc.host(call(*tc.rows(got)))
        tc.assert_equal(got, want[t + 1], f"key {key} call {t + 1}")
    tc.assert_same_trees(guided, [gs.model_tree_connect(model, i) for i in range(model.n)], f"key {key}")
    print(f"connect key {key}: {case.h}x{case.w}x{case.k}, C = {case.capacity}, cpuct = {case.cpuct}, nodes {got[6].tolist()}, {model.facts}")
    guided.close()
    b.close()


@pytest.mark.parametrize("key", gf.bounce_keys())
def test_bounce_key_equals_the_statement(key):
    case = gf.bounce_key(key)
    model, want = gf.bounce_expected(key)
    b = tb.load(case.grid, case.roots)
    guided = tb.poisoned(b, case.nodes, case.edges, case.cpuct, case.max_plies)
    got = tb.host(guided.begin())
    tb.assert_equal(got, want[0], f"key {key} begin")
    for t in range(gf.SIMULATIONS):
        call = guided.finish if t == gf.SIMULATIONS - 1 else guided.step
        got = tb.host(call(*tb.rows(got)))
        tb.assert_equal(got, want[t + 1], f"key {key} call {t + 1}")
    tb.assert_same_trees(guided, [gs.model_tree_bounce(model, i) for i in range(model.n)], f"key {key}")
    print(f"bounce key {key}: grid {case.grid.shape}, C = {case.nodes}, E = {case.edges}, cpuct = {case.cpuct}, cap = {case.max_plies}, "
          f"nodes {got[7].tolist()}, {model.facts}")
    guided.close()
    b.close()


# ---- the primed trees
def prime_device(guided, decode, encode, prime, plan, before, primed):
    """every tree of `guided` read back, compared with the statement's, primed and written back: only n and s words change"""
    import torch

    n = guided.batch.n
    words = guided._buffer.cpu().numpy().view(np.uint32).reshape(n, -1).copy()
    for i in range(n):
        tree = decode(words[i])
        gs.assert_same_tree(tree, before[i], f"tree {i} before the priming")
        assert prime(tree, gs.PLANS[plan]) == primed[i]
        words[i] = encode(tree, words[i])
    guided._buffer.copy_(torch.from_numpy(words.reshape(-1).view(np.uint8)))


def assert_the_stop(game, calls, primed):
    """running, expanded roots three visits below BGS_GUIDED_MAX_VISITS: leaves on exactly two more calls, IDLE on every
    later one, and from then on 2^19 visits and rows that no longer change"""
    was = np.array(primed)
    visits, scores = (3, 4) if game == "connect" else (4, 5)
    for t, call in enumerate(calls[gs.PRIMED_BEFORE + 1:]):
        assert ((call[2][was] != ge.IDLE) == (t < 2)).all(), t
    first = calls[gs.PRIMED_BEFORE + 3]
    for call in calls[gs.PRIMED_BEFORE + 3:]:
        assert (call[visits][was].reshape(int(was.sum()), -1).sum(axis=1) == 1 << 19).all()
        np.testing.assert_array_equal(call[visits], first[visits])
        np.testing.assert_array_equal(call[scores], first[scores])


@pytest.mark.parametrize("plan", list(gs.PLANS))
@pytest.mark.parametrize("key", gs.PRIMED_CONNECT)
def test_connect_primed_tree_equals_the_statement(key, plan):
    h, w, k, roots, capacity, cpuct = gf.primed_connect_arguments(key, plan)
    nw = (w * (h + 1) + 63) // 64
    model, want, before, _ = gf.primed_connect(key, plan)
    b = tc.load(h, w, k, roots)
    guided = tc.poisoned(b, capacity, cpuct)
    calls = [tc.host(guided.begin())]
    tc.assert_equal(calls[0], want[0], f"{key} {plan} begin")
    for t in range(CALLS):
        if t == gs.PRIMED_BEFORE:
            prime_device(guided, lambda x: gs.decode_connect(x, h, w, nw, capacity), lambda tree, x: gs.encode_connect(tree, h, w, nw, capacity, into=x),
                         gs.prime_connect, plan, before, model.primed)
        calls.append(tc.host((guided.finish if t == CALLS - 1 else guided.step)(*tc.rows(calls[-1]))))
        tc.assert_equal(calls[-1], want[t + 1], f"{key} {plan} call {t + 1}")
    tc.assert_same_trees(guided, [gs.model_tree_connect(model, i) for i in range(model.n)], f"{key} {plan}")
    if plan == "stop":
        assert_the_stop("connect", calls, model.primed)
    guided.close()
    b.close()


@pytest.mark.parametrize("plan", list(gs.PLANS))
@pytest.mark.parametrize("key", gs.PRIMED_BOUNCE)
def test_bounce_primed_tree_equals_the_statement(key, plan):
    grid, roots, nodes, cpuct = gf.primed_bounce_arguments(key, plan)
    model, want, before, _ = gf.primed_bounce(key, plan)
    b = tb.load(grid, roots)
    guided = tb.poisoned(b, nodes, None, cpuct)
    edges = guided.edges
    assert edges == bg.default_edges(*grid.shape, nodes)
    calls = [tb.host(guided.begin())]
    tb.assert_equal(calls[0], want[0], f"{key} {plan} begin")
    for t in range(CALLS):
        if t == gs.PRIMED_BEFORE:
            prime_device(guided, lambda x: gs.decode_bounce(x, nodes, edges), lambda tree, x: gs.encode_bounce(tree, nodes, edges, into=x),
                         gs.prime_bounce, plan, before, model.primed)
        calls.append(tb.host((guided.finish if t == CALLS - 1 else guided.step)(*tb.rows(calls[-1]))))
        tb.assert_equal(calls[-1], want[t + 1], f"{key} {plan} call {t + 1}")
    tb.assert_same_trees(guided, [gs.model_tree_bounce(model, i) for i in range(model.n)], f"{key} {plan}")
    if plan == "stop":
        assert_the_stop("bounce", calls, model.primed)
    guided.close()
    b.close()


# ---- a step in a graph with its evaluator
TREES, EAGER, PAIRS, REPLAYS = 64, 24, 8, 3


def graph_against_eager(torch, stream, guided, evaluate, trees_of):
    """on `stream`: begin and EAGER eager (evaluate, step) pairs, then twice begin and REPLAYS replays of a graph of PAIRS
    pairs; every output and every tree of the replayed runs equal the eager run's"""
    assert PAIRS * REPLAYS == EAGER
    outs = guided.begin()
    for _ in range(EAGER):
        outs = guided.step(*evaluate(outs))
    torch.cuda.synchronize()
    eager = [o.cpu().numpy().copy() for o in outs]
    eager_trees = trees_of(guided)
    assert (eager[2] != ge.IDLE).all() and all(tree["count"] > 1 for tree in eager_trees)
    guided.begin()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):       # a linear capture: the evaluator and the step on the batch's stream
        for _ in range(PAIRS):
            outs = guided.step(*evaluate(outs))
    for attempt in range(2):                            # twice: the graph holds no state of its own
        guided.begin()
        for _ in range(REPLAYS):
            graph.replay()
        torch.cuda.synchronize()
        for name, got, want in zip(bg.NAMES if len(eager) == 9 else tc.NAMES, outs, eager):
            np.testing.assert_array_equal(got.cpu().numpy(), want, err_msg=f"{name}, replayed run {attempt}")
        for i, (got, want) in enumerate(zip(trees_of(guided), eager_trees)):
            gs.assert_same_tree(got, want, f"tree {i}, replayed run {attempt}")


def test_connect_steps_replay_from_a_graph_with_their_evaluator():
    import torch

    from simulator.batch import ConnectBatch

    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        b = ConnectBatch(6, 7, 4, TREES, use_torch=True)
        assert (b.step_actions((np.arange(TREES) % 7).astype(np.int32)) == 0).all()       # seven different roots
        guided = b.guided_search(EAGER + 1)
        guided._buffer.fill_(0xA5)
        graph_against_eager(torch, stream, guided, lambda outs: torch_evaluator(outs[0], outs[1]), tc.device_trees)
        guided.close()
        b.close()


def test_bounce_steps_replay_from_a_graph_with_their_evaluator():
    import torch

    from simulator.batch import BounceBatch

    grid = fc.BOUNCE_CORNERS["default"]()
    start = (grid, 0, 0)
    acts = _actions(grid, start)
    moves = np.array([[sx, sy, tx, ty] for (sx, sy), (tx, ty) in (acts[i % len(acts)] for i in range(TREES))], dtype=np.int32)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        b = BounceBatch(grid, TREES, use_torch=True)
        assert (b.step_actions(moves) == 0).all()                                          # a different root a legal first move
        guided = b.guided_moves_search(EAGER + 1)
        guided._buffer.fill_(0xA5)
        graph_against_eager(torch, stream, guided, lambda outs: torch_evaluator_moves(outs[0], outs[1], outs[3]), tb.device_trees)
        guided.close()
        b.close()
