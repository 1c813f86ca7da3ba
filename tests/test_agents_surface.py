"""The surface of simulator/agents.py that needs no device: the signatures of the five public classes, what their
constructors refuse, what they say to a bad list of states before any batch is made, the proved-share rule on plain
arrays, and the two games' mapping between an action, its index in a per-root output row and its flat slot.

The signature table and every message below were written down from the agents as they were before their shared parts
were pulled together (one loader, one slot mapping, one tree-search body), and the first three parts passed against that
file unedited: they are the record that the surface did not move.  The last two parts (`_proved_shares`, and `index` /
`slot` / `action` of the per-game objects `_Connect` and `_Bounce`) exercise functions that only exist since then, so they
could not run against the earlier file; the values they expect are worked out by hand here, from the rule in the tree
agents' docstrings and the slot formula in MonteCarloAgent's.

States are built with the State constructors: no engine and no batch is involved.  Return annotations are left out of the
comparison: `predict_many` of the two tree agents is one method now, and an annotation is no part of how a method is
called.
"""

import inspect
from types import SimpleNamespace

import numpy as np
import pytest

from simulator import agents
from simulator.batch import SOLVE_DRAW, SOLVE_LOSS, SOLVE_NONE, SOLVE_UNKNOWN, SOLVE_WIN
from simulator.game import bounce, connect

CLASSES = ("MonteCarloAgent", "TreeSearchAgent", "BounceHalvingAgent", "BounceTreeSearchAgent", "SolverAgent")
MANY = "(self, states: 'Sequence', first_game: 'int' = 0)"
ONE = "(self, state, game: 'int' = 0)"
TREE = ("(self, iterations: 'int' = 256, leaf_playouts: 'int' = 64, explore: 'int' = 65536, policy: 'str' = 'uniform', "
        "seed: 'int' = 81985529216486895, device: 'int' = 0, max_plies: 'Optional[int]' = None, ")
TAIL = "prove: 'bool' = False, reuse: 'bool' = False, capacity: 'Optional[int]' = None)"
SIGNATURES = {
    ("MonteCarloAgent", "__init__"): "(self, playouts: 'int' = 256, seed: 'int' = 81985529216486895, device: 'int' = 0, "
                                     "max_plies: 'Optional[int]' = None, policy: 'str' = 'uniform', allocation: 'str' = 'flat', "
                                     "budget: 'Optional[int]' = None)",
    ("MonteCarloAgent", "bounce_values"): "(self, batch: 'BounceBatch', first_game: 'int' = 0)",
    ("MonteCarloAgent", "choose"): ONE,
    ("MonteCarloAgent", "choose_many"): MANY,
    ("MonteCarloAgent", "close"): "(self)",
    ("MonteCarloAgent", "halving_values"): "(self, batch: 'ConnectBatch', first_game: 'int' = 0)",
    ("MonteCarloAgent", "predict"): ONE,
    ("MonteCarloAgent", "predict_many"): MANY,
    ("MonteCarloAgent", "values"): "(self, batch: 'ConnectBatch', first_game: 'int' = 0)",
    ("TreeSearchAgent", "__init__"): TREE + TAIL,
    ("TreeSearchAgent", "choose"): ONE,
    ("TreeSearchAgent", "choose_many"): MANY,
    ("TreeSearchAgent", "close"): "(self)",
    ("TreeSearchAgent", "predict"): ONE,
    ("TreeSearchAgent", "predict_many"): MANY,
    ("TreeSearchAgent", "search"): MANY,
    ("TreeSearchAgent", "stones_between"): "(old: 'np.ndarray', mover: 'int', new: 'np.ndarray')",
    ("BounceHalvingAgent", "__init__"): "(self, budget: 'int' = 1024, seed: 'int' = 81985529216486895, device: 'int' = 0, "
                                        "max_plies: 'Optional[int]' = None, policy: 'str' = 'uniform')",
    ("BounceHalvingAgent", "choose"): ONE,
    ("BounceHalvingAgent", "choose_many"): MANY,
    ("BounceHalvingAgent", "close"): "(self)",
    ("BounceHalvingAgent", "predict"): ONE,
    ("BounceHalvingAgent", "predict_many"): MANY,
    ("BounceTreeSearchAgent", "__init__"): TREE + "edges: 'Optional[int]' = None, " + TAIL,
    ("BounceTreeSearchAgent", "choose"): ONE,
    ("BounceTreeSearchAgent", "choose_many"): MANY,
    ("BounceTreeSearchAgent", "close"): "(self)",
    ("BounceTreeSearchAgent", "moves_between"): "(old: 'np.ndarray', mover: 'int', new: 'np.ndarray', plies: 'int')",
    ("BounceTreeSearchAgent", "predict"): ONE,
    ("BounceTreeSearchAgent", "predict_many"): MANY,
    ("BounceTreeSearchAgent", "search"): MANY,
    ("SolverAgent", "__init__"): "(self, depth: 'Optional[int]' = None, max_nodes: 'int' = 1048576, fallback=None, device: 'int' = 0)",
    ("SolverAgent", "choose"): "(self, state)",
    ("SolverAgent", "close"): "(self)",
    ("SolverAgent", "predict"): "(self, state)",
    ("SolverAgent", "predict_many"): "(self, states: 'Sequence')",
    ("SolverAgent", "solve_many"): "(self, states: 'Sequence')",
}


# ---- signatures
def test_the_public_classes_are_the_five():
    public = [name for name, value in vars(agents).items() if inspect.isclass(value) and value.__module__ == agents.__name__
              and not name.startswith("_")]
    assert sorted(public) == sorted(CLASSES)
    assert agents.BOUNCE_MAX_PLIES == 1024


@pytest.mark.parametrize("name", CLASSES)
def test_signatures_are_the_table(name):
    cls = getattr(agents, name)
    methods = ["__init__"] + sorted(n for n, value in inspect.getmembers(cls) if not n.startswith("_") and callable(value))
    assert methods == [method for owner, method in SIGNATURES if owner == name]
    for method in methods:
        signature = inspect.signature(getattr(cls, method)).replace(return_annotation=inspect.Signature.empty)
        assert str(signature) == SIGNATURES[name, method], method
    assert cls.__doc__ and cls.__doc__.strip()


# ---- constructor refusals: one invalid argument each, the exception's type and its whole text
POLICY = "unknown playout policy 'greedy': one of ['decisive', 'uniform']"
BUDGET = "budget: a positive number of playouts a position, with allocation='halving' only"
REFUSED = [
    ("MonteCarloAgent", dict(policy="greedy"), POLICY),
    ("MonteCarloAgent", dict(policy=None), "unknown playout policy None: one of ['decisive', 'uniform']"),
    ("MonteCarloAgent", dict(allocation="ucb"), "unknown allocation 'ucb': 'flat' or 'halving'"),
    ("MonteCarloAgent", dict(budget=64), BUDGET),
    ("MonteCarloAgent", dict(allocation="halving", budget=0), BUDGET),
    ("MonteCarloAgent", dict(playouts=0), "playouts must be >= 1"),
    ("MonteCarloAgent", dict(max_plies=0), "max_plies must be >= 1"),
    ("BounceHalvingAgent", dict(policy="greedy"), POLICY),
    ("BounceHalvingAgent", dict(budget=0), "budget must be >= 1"),
    ("BounceHalvingAgent", dict(max_plies=0), "max_plies must be >= 1"),
    ("SolverAgent", dict(depth=0), "depth must be >= 1"),
    ("SolverAgent", dict(max_nodes=0), "max_nodes must be >= 1"),
    ("TreeSearchAgent", dict(prove=True, reuse=True), "prove=True with reuse=True: the forest does not prove yet"),
    ("BounceTreeSearchAgent", dict(prove=True, reuse=True), "prove=True with reuse=True: the forest does not prove"),
]
for _tree in ("TreeSearchAgent", "BounceTreeSearchAgent"):
    REFUSED += [
        (_tree, dict(policy="greedy"), POLICY),
        (_tree, dict(iterations=0), "iterations and leaf_playouts must be >= 1"),
        (_tree, dict(leaf_playouts=0), "iterations and leaf_playouts must be >= 1"),
        (_tree, dict(explore=-1), "explore must be 0 .. 2**18"),
        (_tree, dict(explore=2**18 + 1), "explore must be 0 .. 2**18"),
        (_tree, dict(max_plies=0), "max_plies must be >= 1"),
        (_tree, dict(capacity=1), "capacity must be >= 2"),
    ]


@pytest.mark.parametrize("name,arguments,text", REFUSED, ids=[f"{n}-{'-'.join(f'{k}={v}' for k, v in a.items())}" for n, a, _ in REFUSED])
def test_constructor_refusals(name, arguments, text):
    with pytest.raises(ValueError) as refusal:
        getattr(agents, name)(**arguments)
    assert str(refusal.value) == text


def test_constructors_take_the_edges_of_their_ranges_and_keep_their_attributes():
    for name in ("TreeSearchAgent", "BounceTreeSearchAgent"):
        cls = getattr(agents, name)
        least = cls(iterations=1, leaf_playouts=1, explore=0, max_plies=1, capacity=2, reuse=True, policy="decisive", seed=7, device=0)
        assert (least.iterations, least.leaf_playouts, least.explore, least.max_plies, least.capacity) == (1, 1, 0, 1, 2)
        assert (least.policy, least.seed, least.device, least.prove, least.reuse) == ("decisive", 7, 0, False, True)
        most = cls(iterations=10, explore=2**18, prove=True)
        assert (most.explore, most.capacity, most.max_plies, most.prove, most.reuse) == (2**18, 21, None, True, False)
        assert most._forests == {} and most._batches == {}
    assert agents.BounceTreeSearchAgent().edges is None and agents.BounceTreeSearchAgent(edges=300).edges == 300
    assert not hasattr(agents.TreeSearchAgent(), "edges")
    flat = agents.MonteCarloAgent(playouts=3, seed=5, max_plies=9, policy="decisive")
    assert (flat.playouts, flat.seed, flat.device, flat.max_plies, flat.policy, flat.allocation, flat.budget) == (
        3, 5, 0, 9, "decisive", "flat", None)
    halving = agents.MonteCarloAgent(allocation="halving", budget=1)
    assert (halving.allocation, halving.budget, halving.max_plies, halving._batches) == ("halving", 1, None, {})
    bounce_halving = agents.BounceHalvingAgent(budget=1, seed=5, max_plies=1, policy="decisive")
    assert (bounce_halving.budget, bounce_halving.seed, bounce_halving.device, bounce_halving.max_plies, bounce_halving.policy) == (
        1, 5, 0, 1, "decisive")
    fallback = object()
    solver = agents.SolverAgent(depth=1, max_nodes=1, fallback=fallback)
    assert (solver.depth, solver.max_nodes, solver.fallback, solver.device, solver._batches) == (1, 1, fallback, 0, {})
    assert agents.SolverAgent().depth is None


# ---- state-list refusals: all of them are made before a batch is, so constructor-built states will do
def connect_state(height=2, width=3, legal=None):
    config = connect.Config(height, width, 2)
    return connect.State(config, np.full((height, width), -1, dtype=np.int8), 0, -1, tuple(range(width)) if legal is None else legal, (0, 0))


BOUNCE_MOVES = (((0, 1), (0, 2)), ((0, 1), (1, 1)), ((1, 1), (1, 2)), ((1, 1), (0, 1)), ((1, 1), (0, 2)))


def bounce_state(height=3):
    """`height` rows and 2 columns, a piece of value 1 in both cells of row 1; the moves are not the rules' (no test here
    plays one), they are a few (source, target) pairs over both columns and two target rows"""
    grid = np.zeros((height, 2), dtype=np.int8)
    grid[1] = 1
    return bounce.State(bounce.Config(grid), grid, 0, -1, 4, BOUNCE_MOVES, (0, 0))


def entry_points(agent):
    """every public way a list of states gets into `agent`"""
    calls = [agent.predict_many, agent.choose_many if hasattr(agent, "choose_many") else agent.solve_many]
    if hasattr(agent, "search"):
        calls.append(agent.search)
    return calls


def refused(agent, states, kind, text):
    for call in entry_points(agent):
        with pytest.raises(kind) as refusal:
            call(states)
        assert str(refusal.value) == text, call.__name__
        assert type(refusal.value) is kind
    assert agent._batches == {}
    if len(states) == 1:    # ... and the one-state wrappers
        for call in (agent.predict, agent.choose):
            with pytest.raises(kind) as refusal:
                call(states[0])
            assert str(refusal.value) == text, call.__name__


SHARE = "the states must share one Config"


def test_an_empty_list_is_answered_without_a_batch():
    for name in CLASSES:
        agent = getattr(agents, name)()
        assert agent.predict_many([]) == []
        if name != "SolverAgent":
            assert agent.choose_many([]) == []
        assert agent._batches == {}


def test_tree_search_agent_refuses_before_a_batch_is_made():
    for arguments in (dict(), dict(prove=True), dict(reuse=True)):
        agent = agents.TreeSearchAgent(**arguments)
        refused(agent, [bounce_state()], ValueError, "TreeSearchAgent: Connect states only; the tree search does not cover Bounce")
        refused(agent, [bounce_state(), connect_state()], ValueError, "TreeSearchAgent: Connect states only; the tree search does not cover Bounce")
        refused(agent, [object()], TypeError, "TreeSearchAgent: Connect states, not object")
        refused(agent, ["a1"], TypeError, "TreeSearchAgent: Connect states, not str")
        refused(agent, [connect_state(2, 3), connect_state(3, 3)], ValueError, f"TreeSearchAgent: {SHARE}")
        refused(agent, [connect_state(), bounce_state()], ValueError, f"TreeSearchAgent: {SHARE}")
        refused(agent, [connect_state(), object()], ValueError, f"TreeSearchAgent: {SHARE}")
        assert agent._forests == {}


def test_bounce_tree_search_agent_refuses_before_a_batch_is_made():
    for arguments in (dict(), dict(prove=True), dict(reuse=True)):
        agent = agents.BounceTreeSearchAgent(**arguments)
        refused(agent, [connect_state()], ValueError, "BounceTreeSearchAgent: Bounce states only; Connect states: TreeSearchAgent")
        refused(agent, [connect_state(), bounce_state()], ValueError, "BounceTreeSearchAgent: Bounce states only; Connect states: TreeSearchAgent")
        refused(agent, [object()], TypeError, "BounceTreeSearchAgent: Bounce states, not object")
        refused(agent, [bounce_state(3), bounce_state(4)], ValueError, f"BounceTreeSearchAgent: {SHARE}")
        refused(agent, [bounce_state(), connect_state()], ValueError, f"BounceTreeSearchAgent: {SHARE}")
        refused(agent, [bounce_state(), object()], ValueError, f"BounceTreeSearchAgent: {SHARE}")
        assert agent._forests == {}


def test_bounce_halving_agent_refuses_before_a_batch_is_made():
    agent = agents.BounceHalvingAgent()
    elsewhere = 'BounceHalvingAgent: Bounce states only; Connect states: MonteCarloAgent(allocation="halving")'
    refused(agent, [connect_state()], ValueError, elsewhere)
    refused(agent, [connect_state(), bounce_state()], ValueError, elsewhere)
    refused(agent, [object()], TypeError, "BounceHalvingAgent: Bounce states, not object")
    refused(agent, [bounce_state(3), bounce_state(4)], ValueError, f"BounceHalvingAgent: {SHARE}")
    refused(agent, [bounce_state(), connect_state()], ValueError, f"BounceHalvingAgent: {SHARE}")
    refused(agent, [bounce_state(), object()], ValueError, f"BounceHalvingAgent: {SHARE}")


def test_monte_carlo_agent_refuses_before_a_batch_is_made():
    thing = SimpleNamespace(config=connect_state().config)      # it has a Config and is no state
    for agent in (agents.MonteCarloAgent(), agents.MonteCarloAgent(policy="decisive")):
        refused(agent, [thing], TypeError, "predict_many: Connect or Bounce states, not SimpleNamespace")
        refused(agent, [connect_state(2, 3), connect_state(3, 3)], ValueError, f"predict_many: {SHARE}")
        refused(agent, [bounce_state(3), bounce_state(4)], ValueError, f"predict_many: {SHARE}")
        refused(agent, [connect_state(), bounce_state()], ValueError, f"predict_many: {SHARE}")
        refused(agent, [bounce_state(), connect_state()], ValueError, f"predict_many: {SHARE}")
        refused(agent, [connect_state(), thing], ValueError, f"predict_many: {SHARE}")
        assert agent._policy_game is None       # a refused list binds the agent's policy to no game
    # halving: Bounce states are refused, and choose_many, which does not go through predict_many, names itself where it
    # compares the Configs and predict_many where it looks at the type
    halving = agents.MonteCarloAgent(allocation="halving")
    flat_only = "MonteCarloAgent: Bounce moves are evaluated flat, there is no halving allocation for Bounce states"
    refused(halving, [bounce_state()], ValueError, flat_only)
    refused(halving, [bounce_state(), bounce_state()], ValueError, flat_only)
    refused(halving, [thing], TypeError, "predict_many: Connect or Bounce states, not SimpleNamespace")
    for states in ([connect_state(2, 3), connect_state(3, 3)], [connect_state(), bounce_state()], [connect_state(), thing]):
        for call, who in ((halving.predict_many, "predict_many"), (halving.choose_many, "choose_many")):
            with pytest.raises(ValueError) as refusal:
                call(states)
            assert str(refusal.value) == f"{who}: {SHARE}"
    refused(halving, [bounce_state(3), bounce_state(4)], ValueError, f"predict_many: {SHARE}")
    refused(halving, [bounce_state(), connect_state()], ValueError, f"predict_many: {SHARE}")
    assert halving._batches == {}
    # an object without a Config gets no message of the agent's
    for agent in (agents.MonteCarloAgent(), halving):
        for call in entry_points(agent):
            with pytest.raises(AttributeError, match="config"):
                call([object()])


def test_solver_agent_refuses_before_a_batch_is_made():
    agent = agents.SolverAgent()
    thing = SimpleNamespace(config=connect_state().config)
    refused(agent, [thing], ValueError, "SolverAgent: Connect states that share one Config")
    refused(agent, [connect_state(2, 3), connect_state(3, 3)], ValueError, "SolverAgent: Connect states that share one Config")
    refused(agent, [connect_state(), bounce_state()], ValueError, "SolverAgent: Connect states that share one Config")
    refused(agent, [connect_state(), thing], ValueError, "SolverAgent: Connect states that share one Config")
    refused(agent, [bounce_state(3), bounce_state(4)], ValueError, "SolverAgent: Bounce states that share one Config")
    refused(agent, [bounce_state(), connect_state()], ValueError, "SolverAgent: Bounce states that share one Config")
    refused(agent, [bounce_state(), thing], ValueError, "SolverAgent: Bounce states that share one Config")
    for call in entry_points(agent):
        with pytest.raises(AttributeError, match="config"):
            call([object()])


# ---- the proved-share rule on plain arrays (new with the shared tree-search body: see the module's docstring)
WIDTH, HEIGHT = 5, 3
COLUMNS = [0, 2, 3, 4]                                        # a Connect root's legal columns, of 5
MOVES = [(0, 7), (1, 4), (1, 11), (4, 14)]                    # a Bounce root's legal (source column, target cell) pairs
VISITS = [10, 30, 20, 40]
W, D, L, U = SOLVE_WIN, SOLVE_DRAW, SOLVE_LOSS, SOLVE_UNKNOWN
PROVED_CASES = {
    "one win among open moves": ([U, W, U, U], [0.0, 1.0, 0.0, 0.0]),
    "two wins": ([W, U, W, L], [0.5, 0.0, 0.5, 0.0]),                       # each win is worth 1.0, of 2.0
    "a win beside a draw": ([D, D, W, U], [0.0, 0.0, 1.0, 0.0]),
    "some losses": ([L, U, D, L], [0.0, 30.0 / 50.0, 20.0 / 50.0, 0.0]),    # 30 and 20 visits are left, of 50
    "one loss": ([U, U, L, U], [10.0 / 80.0, 30.0 / 80.0, 0.0, 40.0 / 80.0]),
    "all lost": ([L, L, L, L], [0.1, 0.3, 0.2, 0.4]),                       # what the visits give, of 100
    "nothing proved": ([U, U, U, U], [0.1, 0.3, 0.2, 0.4]),
    "draws alone": ([D, D, D, D], [0.1, 0.3, 0.2, 0.4]),
}


def connect_root(proved):
    visits = np.full(WIDTH, 99, dtype=np.int32)               # (the illegal column's numbers must not be read)
    codes = np.full(WIDTH, SOLVE_NONE, dtype=np.int8)
    for column, v, p in zip(COLUMNS, VISITS, proved):
        visits[column], codes[column] = v, p
    return visits, codes, [(column,) for column in COLUMNS]


def bounce_root(proved):
    visits = np.full((WIDTH, HEIGHT * WIDTH), 99, dtype=np.int32)
    codes = np.full((WIDTH, HEIGHT * WIDTH), SOLVE_NONE, dtype=np.int8)
    for at, v, p in zip(MOVES, VISITS, proved):
        visits[at], codes[at] = v, p
    return visits, codes, list(MOVES)


@pytest.mark.parametrize("case", list(PROVED_CASES))
def test_proved_shares(case):
    proved, want = PROVED_CASES[case]
    got = agents._proved_shares(*connect_root(proved))
    assert list(got) == want and all(type(x) is float for x in got)
    assert list(agents._proved_shares(*bounce_root(proved))) == want      # the same numbers under Bounce's indexing
    assert abs(sum(got) - 1.0) < 1e-12


def test_proved_shares_keep_the_order_of_the_indices():
    visits, codes, at = connect_root([L, U, D, L])
    assert list(agents._proved_shares(visits, codes, at[::-1])) == [0.0, 0.4, 0.6, 0.0]


# ---- action, index in a per-root output row, flat slot (new with the per-game objects: see the module's docstring)
def test_bounce_index_and_slot_are_the_documented_formula():
    state = bounce_state()
    height, width = 3, 2
    game = agents._Bounce
    seen = set()
    for action, ((sx, sy), (tx, ty)) in zip(state.actions, BOUNCE_MOVES):
        assert game.index(action) == (sx, ty * width + tx)
        slot = game.slot(action)
        assert slot == sx * height * width + ty * width + tx and type(slot) is int
        assert game.action(state, slot) == action and game.slot(game.action(state, slot)) == slot
        assert game.action(state, np.int32(slot)) == action         # as it comes out of a `best` array
        seen.add(slot)
    assert len(seen) == len(BOUNCE_MOVES)
    for slot in (-1, np.int32(-1), -2):                             # an ended root, and HALVING_SHORT
        assert game.action(state, slot) is None


def test_connect_index_and_slot_are_the_column():
    state = connect_state(2, 3, legal=(0, 2))
    game = agents._Connect
    for action, column in zip(state.actions, (0, 2)):
        assert game.index(action) == (column,)
        assert game.slot(action) == column
        assert game.action(state, column) == action and game.action(state, np.int32(column)) == action
        assert game.slot(game.action(state, column)) == column
    assert game.action(state, -1) is None and game.action(state, np.int32(-1)) is None


def test_the_games_defaults():
    assert agents._Connect.max_plies == 2**31 - 1 and agents._Bounce.max_plies == agents.BOUNCE_MAX_PLIES
    a, b = connect_state(2, 3), connect_state(3, 3)
    assert agents._Connect.key(a.config, 4) == agents._Connect.key(connect_state(2, 3).config, 4)
    assert len({agents._Connect.key(a.config, 4), agents._Connect.key(a.config, 5), agents._Connect.key(b.config, 4),
                agents._Bounce.key(bounce_state(3).config, 4), agents._Bounce.key(bounce_state(4).config, 4),
                agents._Bounce.key(bounce_state(4).config, 5)}) == 6
    # the arrays write_state takes: the winner and the ply count are the state's own
    ended = connect.State(a.config, a.grid, 1, 0, (), (1, -1))
    grid, player, winner = agents._Connect.arrays([a, ended])
    assert grid.shape == (2, 2, 3) and grid.dtype == np.int8
    assert (player.tolist(), player.dtype, winner.tolist(), winner.dtype) == ([0, 1], np.int8, [-1, 0], np.int8)
    s = bounce_state()
    late = bounce.State(s.config, s.grid, 1, 1, 9, (), (-1, 1))
    grid, player, winner, plies = agents._Bounce.arrays([s, late])
    assert grid.shape == (2, 3, 2) and (player.tolist(), winner.tolist(), plies.tolist()) == ([0, 1], [-1, 1], [4, 9])
    assert (player.dtype, winner.dtype, plies.dtype) == (np.int8, np.int8, np.int32)
