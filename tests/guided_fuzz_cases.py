"""The case table of the guided searches' fuzz (tests/test_gpu_guided_fuzz.py) and of the CPU test that states what the
table must hold (tests/test_guided_fuzz_cases.py): the random geometries, start grids and roots of tests/fuzz_cases.py
through bgs_connect_guided_step and bgs_bounce_guided_step.  No GPU import, no file I/O; not a test module.

A key is an int: random case `key` of tests/fuzz_cases.py gives the geometry or the start grid and the roots; everything
this table adds -- capacity or nodes and edges, cpuct, the cap, whether boards are stepped between two calls -- is drawn
from numpy.random.default_rng(CONNECT_BASE or BOUNCE_BASE + key), bases of this table's own: no draw of tests/fuzz_cases.py
or tests/policy_fuzz_cases.py changes, and building a key twice gives identical arrays.  BGS_FUZZ_CASES=N widens the keys
to 0 .. N - 1 as it does there.  (The corner tables go through the guided searches in tests/test_gpu_guided.py and
tests/test_gpu_bounce_guided.py.)

Connect, keys 0..15: a spread of at most 8 of the key's roots, 32 simulations, capacity from (2, 3, 5, 33), cpuct from
(0, 1, 320, 1024, 4096); on every second key the boards with an even index play their lowest legal column before call
RESTART_CALL = 12 and restart their trees.
Bounce, keys 0..11: the first 6 of the key's eval_rows, 32 simulations, nodes from (2, 3, 9, 33), edges from
(BGS_BOUNCE_SEARCH_MIN_EDGES, the default pool), cpuct as above, max_plies the case's first cap or 65535.

Bases.  Connect: 81000, the first choice, holds every condition of tests/test_guided_fuzz_cases.py.  Bounce: 85000, the
first choice, refused no edge block and met no capped leaf; of 85100, 85200, ... 85900 is the first that holds both (and
every other condition): 85100 .. 85700 refuse edge blocks but meet no cap, 85800 refuses none.

`connect_expected` / `bounce_expected` run the CPU statements under the fixed evaluators once a session and share the
result: treat everything as read-only.  `model.facts` records what the run met, for the coverage conditions."""

import functools
from collections import namedtuple

import numpy as np

from oracle import oracle
from tests import bounce_guided_expected as bg
from tests import fuzz_cases as fc
from tests import guided_expected as ge
from tests import guided_shares as gs
from tests.search_bounce_expected import min_edges

CONNECT_CASES = 16
BOUNCE_CASES = 12
CONNECT_BASE = 81000        # default_rng(base + key)
BOUNCE_BASE = 85900
SIMULATIONS = 32
RESTART_CALL = 12
CONNECT_ROOTS, BOUNCE_ROOTS = 8, 6
CAPACITIES = (2, 3, 5, 33)
NODES = (2, 3, 9, 33)
CPUCTS = (0, 1, 320, 1024, 4096)

ConnectKey = namedtuple("ConnectKey", "key h w k nw roots capacity cpuct columns roots_after")
BounceKey = namedtuple("BounceKey", "key grid roots nodes edges cpuct max_plies")


def connect_keys():
    return list(range(max(CONNECT_CASES, fc.EXTRA)))


def bounce_keys():
    return list(range(max(BOUNCE_CASES, fc.EXTRA)))


@functools.lru_cache(maxsize=None)
def connect_key(key):
    """columns: int32[n], the column every board plays before call RESTART_CALL (negative: it stays); roots_after: the
    roots from that call on"""
    case = fc.connect_case(key)
    rng = np.random.default_rng(CONNECT_BASE + key)
    roots = fc.take(case.roots, fc._spread(case.roots[0].shape[0], CONNECT_ROOTS))
    n = roots[0].shape[0]
    capacity, cpuct = int(rng.choice(CAPACITIES)), int(rng.choice(CPUCTS))
    columns = np.full(n, -1, dtype=np.int32)
    roots_after = roots
    if key % 2 == 0:
        orc = oracle.ConnectOracle(case.h, case.w, case.k, n)
        orc.grid[:], orc.player[:], orc.winner[:], orc.plies[:] = roots
        legal = orc.legal().astype(bool)
        columns = np.where((roots[2] == -1) & (np.arange(n) % 2 == 0), legal.argmax(axis=1), -1).astype(np.int32)
        assert (orc.step_actions(columns)[columns >= 0] == 0).all()
        roots_after = (orc.grid.copy(), orc.player.copy(), orc.winner.copy(), orc.plies.copy())
    return ConnectKey(key, case.h, case.w, case.k, case.nw, roots, capacity, cpuct, columns, roots_after)


@functools.lru_cache(maxsize=None)
def bounce_key(key):
    case = fc.bounce_case(key)
    rng = np.random.default_rng(BOUNCE_BASE + key)
    h, w = case.grid.shape
    roots = fc.take(case.roots, case.eval_rows[:BOUNCE_ROOTS])
    nodes = int(rng.choice(NODES))
    edges = (min_edges(h, w), bg.default_edges(h, w, nodes))[int(rng.integers(0, 2))]
    cpuct = int(rng.choice(CPUCTS))
    max_plies = (case.max_plies[0], 65535)[int(rng.integers(0, 2))]
    return BounceKey(key, case.grid, roots, nodes, edges, cpuct, max_plies)


def connect_roots_at(case, call):
    """the roots call number `call` (0: begin) runs over"""
    return case.roots_after if call >= RESTART_CALL else case.roots


def served_connect(grid, player, kind):
    """the special rows ge.fake_network serves to the EVALUATE leaves among (grid, player): {name: count}"""
    special = (ge.grid_hash(np.asarray(grid), player) % np.uint64(16)).astype(np.int64)
    full = np.asarray(grid)[:, -1, :] != -1
    served = dict.fromkeys(ge.SPECIALS, 0)
    for i in np.flatnonzero(kind == ge.EVALUATE):
        if 1 <= special[i] <= 8 and (ge.SPECIALS[special[i] - 1] != "illegal_only" or full[i].any()):
            served[ge.SPECIALS[special[i] - 1]] += 1
    return served


def _add(total, more):
    for name, count in more.items():
        total[name] = total.get(name, 0) + count


def run_connect(key, statement=ge.Guided):
    """(the Guided, every call's outputs) of the key under ge.fake_network; statement: the class that plays it"""
    case = connect_key(key)
    n = case.roots[0].shape[0]
    model = statement(case.h, case.w, case.k, n, case.capacity, case.cpuct)
    facts = {"won": 0, "full": 0, "max_depth": 0, "restarted": 0, "served": {}}
    calls = [model.step(case.roots, flags=ge.RESTART)]
    for t in range(SIMULATIONS):
        _add(facts["served"], served_connect(calls[-1][0], calls[-1][1], calls[-1][2]))
        priors, values = ge.fake_network(calls[-1][0], calls[-1][1])
        roots = connect_roots_at(case, t + 1)
        if t + 1 == RESTART_CALL:
            facts["restarted"] += int((case.columns >= 0).sum())
        calls.append(model.step(roots, priors, values, flags=ge.FINISH if t == SIMULATIONS - 1 else 0))
        for pending in model.pending:
            if pending is not None:
                facts["max_depth"] = max(facts["max_depth"], len(pending[1]))
                if pending[0] == ge.TERMINAL:
                    facts["won" if pending[2] == 0 else "full"] += 1
    facts["refused"] = model.refused
    facts["running"] = int((case.roots[2] == -1).sum())
    model.facts = facts
    return model, calls


@functools.lru_cache(maxsize=None)
def connect_expected(key):
    return run_connect(key)


def run_bounce(key, statement=bg.GuidedMoves):
    """(the GuidedMoves, every call's outputs) of the key under bg.fake_network_moves; statement: the class that plays it"""
    case = bounce_key(key)
    model = statement(case.grid, case.roots[0].shape[0], case.nodes, case.edges, case.cpuct, case.max_plies)
    before = dict(bg.SEEN)
    calls = model.run(case.roots, bg.fake_network_moves, SIMULATIONS)
    model.facts = dict(model.seen, served={name: bg.SEEN[name] - before[name] for name in bg.SPECIALS},
                       running=sum(root is not None for root in model.root))
    return model, calls


@functools.lru_cache(maxsize=None)
def bounce_expected(key):
    return run_bounce(key)


# ---- the primed runs (tests/guided_shares.py: PLANS, PRIMED_CONNECT, PRIMED_BOUNCE): PRIMED_BEFORE simulations, the counts
# of every tree scaled with the leaf of the last call still pending, PRIMED_AFTER more calls, the last with FINISH
def primed_connect_arguments(key, plan):
    """(h, w, k, roots, capacity, cpuct): at most PRIMED_ROOTS of the corner's roots; cpuct 4096 where the `extremes` plan
    meets the board of one column (P = 65536 on its only arm, the largest e term there is), 320 everywhere else"""
    case = fc.connect_case(key)
    roots = fc.take(case.roots, fc._spread(case.roots[0].shape[0], gs.PRIMED_ROOTS))
    return case.h, case.w, case.k, roots, gs.PRIMED_NODES, 4096 if plan == "extremes" and case.w == 1 else 320


def primed_bounce_arguments(key, plan):
    """(grid, roots, nodes, cpuct) with the default pool, as above"""
    case = fc.bounce_case(key)
    roots = fc.take(case.roots, fc._spread(case.roots[0].shape[0], gs.PRIMED_ROOTS))
    return case.grid, roots, gs.PRIMED_NODES, 4096 if plan == "extremes" and case.grid.shape[1] == 1 else 320


def _primed(model, roots, evaluate, tree_of, prime, load, plan):
    n = roots[0].shape[0]
    calls = [model.step(roots, flags=ge.RESTART)]
    before = after = None
    for t in range(gs.PRIMED_BEFORE + gs.PRIMED_AFTER):
        if t == gs.PRIMED_BEFORE:
            before = [tree_of(model, i) for i in range(n)]
            after = [tree_of(model, i) for i in range(n)]
            model.primed = [prime(tree, gs.PLANS[plan]) for tree in after]
            for i in range(n):
                load(model, i, after[i])
        rows = evaluate(*calls[-1])
        calls.append(model.step(roots, *rows, flags=ge.FINISH if t == gs.PRIMED_BEFORE + gs.PRIMED_AFTER - 1 else 0))
    return model, calls, before, after


@functools.lru_cache(maxsize=None)
def primed_connect(key, plan, statement=ge.Guided):
    """(the Guided, every call's outputs, the decoded trees before the priming, and after it); model.primed: which trees
    had a visit to scale"""
    h, w, k, roots, capacity, cpuct = primed_connect_arguments(key, plan)
    model = statement(h, w, k, roots[0].shape[0], capacity, cpuct)
    return _primed(model, roots, lambda *call: ge.fake_network(call[0], call[1]), gs.model_tree_connect, gs.prime_connect,
                   gs.model_load_connect, plan)


@functools.lru_cache(maxsize=None)
def primed_bounce(key, plan, statement=bg.GuidedMoves):
    grid, roots, nodes, cpuct = primed_bounce_arguments(key, plan)
    model = statement(grid, roots[0].shape[0], nodes, None, cpuct)
    return _primed(model, roots, lambda *call: bg.fake_network_moves(call[0], call[1], call[3]), gs.model_tree_bounce,
                   gs.prime_bounce, gs.model_load_bounce, plan)
