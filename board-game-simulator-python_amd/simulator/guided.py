"""``GuidedSearchAgent`` and ``BounceGuidedSearchAgent``: PUCT tree search whose leaves are valued by the caller's
evaluator -- a policy/value network, usually -- instead of random playouts (``ConnectBatch.guided_search``,
bgs_connect_guided_step; ``BounceBatch.guided_moves_search``, bgs_bounce_guided_step).

Connect: ``evaluate(leaf_grid, leaf_player) -> (priors, values)`` sees device tensors: the leaves of all trees, int8[n, h,
w] in the batch's grid encoding (row 0 is the bottom; -1 empty, 0 and 1 the players) and int8[n] the player to move there,
and returns device tensors float32[n, w] (a weight a column: any non-negative numbers, they are normalised over the legal
columns) and float32[n] (the value for the player to move at the leaf, in [-1, 1]).

Bounce: ``evaluate(leaf_grid, leaf_player, leaf_targets) -> (priors, values)``: the grid holds the piece values (0: an
empty cell), ``leaf_targets`` int64[n, w] has bit ty * w + tx of entry x set for every legal move of the piece in column x
of the leaf's active row (zeros for a leaf that needs no evaluation), and the priors are float32[n, w, h * w], a weight a
move slot, normalised over the legal slots.

The evaluator is called once a simulation, between two launches; the trees, the descent and the statistics stay on the
device.  The agents have the shape of the agents in ``simulator.agents`` (``predict(state) -> {Action: float}``) and share
their state loading and slot mapping."""

from __future__ import annotations

from typing import Callable, Dict, List, Optional, Sequence

import numpy as np

from .agents import TreeSearchAgent, _Agent, _Bounce, _Connect, _only
from .batch import DEFAULT_CPUCT, GuidedForest


class _Guided(_Agent):
    """What the two agents share: the checks of the arguments, a search object a batch, and the reading of its outputs.
    A subclass names its game (``_game``), what it says to states that are not that game's (``_who``, ``_elsewhere``),
    how it makes the search object of a batch (``_make``) and which of `run`'s outputs `search` returns (``_report``:
    visits first, `best` third)."""

    def __init__(self, evaluate: Callable, simulations: int, cpuct: int, device: int):
        if not callable(evaluate):
            raise TypeError(f"evaluate must be callable: {self._evaluator}")
        if simulations < 1:
            raise ValueError("simulations must be >= 1")
        if not 0 <= cpuct <= 4096:
            raise ValueError("cpuct must be 0 .. 4096 (c_puct in Q8)")
        super().__init__(device)
        self.evaluate = evaluate
        self.simulations = int(simulations)
        self.cpuct = int(cpuct)
        self._searches: Dict[tuple, object] = {}      # key of the batch -> its search object

    def _run(self, states: Sequence):
        _only(self._game, states[0], self._who, self._elsewhere)
        b, _ = self._loaded(states, self._who, self._game)
        key = self._game.key(states[0].config, len(states))
        guided = self._searches.get(key)
        if guided is None:
            guided = self._searches[key] = self._make(b)
        out = guided.run(self.evaluate, self.simulations)
        return tuple(x.cpu().numpy() for x in out[self._report:])

    def predict_many(self, states: Sequence) -> List[Dict]:
        """`predict` of every state, searched together: {action: visit share}"""
        if not states:
            return []
        visits = self.search(states)[0]
        shares = []
        for k, s in enumerate(states):
            total = max(1, int(visits[k].sum()))
            shares.append({a: float(visits[k][self._game.index(a)]) / total for a in s.actions})
        return shares

    def choose_many(self, states: Sequence) -> List:
        """the launch's `best` of every state (None: no action)"""
        if not states:
            return []
        best = self.search(states)[2]
        return [self._game.action(s, slot) for s, slot in zip(states, best)]

    def predict(self, state) -> Dict:
        return self.predict_many([state])[0]

    def choose(self, state):
        return self.choose_many([state])[0]

    def close(self) -> None:
        for guided in self._searches.values():
            guided.close()
        self._searches.clear()
        super().close()


class GuidedSearchAgent(_Guided):
    """``simulations`` simulations a position, ``cpuct`` = c_puct in Q8 (320 = 1.25), trees of ``capacity`` nodes
    (default: ``simulations + 1``, room for a node a simulation).  ``predict`` returns the visit shares of the root's
    columns, ``choose`` the launch's ``best``: the most visits, then the larger score, then the lower column.  There is no
    seed: nothing in this search is random."""

    _game = _Connect
    _who = "GuidedSearchAgent values"
    _elsewhere = "covers Connect states only"
    _evaluator = "(leaf_grid, leaf_player) -> (priors, values)"
    _report = 3

    def __init__(self, evaluate: Callable, simulations: int = 128, cpuct: int = DEFAULT_CPUCT, capacity: Optional[int] = None,
                 device: int = 0):
        if capacity is not None and capacity < 2:
            raise ValueError("capacity must be >= 2")
        super().__init__(evaluate, simulations, cpuct, device)
        self.capacity = max(2, self.simulations + 1) if capacity is None else int(capacity)

    def _make(self, b):
        return b.guided_search(self.capacity, self.cpuct)

    def search(self, states: Sequence):
        """the search over `states` (Connect states that share one Config): the host copies of (visits int32[n, w],
        scores int32[n, w], best int32[n], nodes int32[n])"""
        return self._run(states)


class GuidedReuseAgent(GuidedSearchAgent):
    """``GuidedSearchAgent`` that keeps its trees from call to call (``simulator.batch.GuidedForest``,
    bgs_connect_guided_advance): the evaluations under the moves played are not paid for twice.  The agent holds a forest
    per (Config, number of states) and remembers the grids it last searched there.  Before a search it advances the tree
    at index k by the one or two stones that lead from the remembered grid k to the new one
    (``TreeSearchAgent.stones_between``: the remembered mover's stone first), in two ``advance`` calls; an equal grid is
    searched on, and any other difference passes -1, where the step's own check starts the tree anew.  So the states of
    successive calls must keep their indices.  Then ``simulations`` evaluations a tree go on top of what was kept.

    ``predict`` gives shares of the root's visits, carried ones included (they still sum to 1); ``search`` returns
    ``kept`` -- the nodes every tree held after the last advance, the root not counted; zeros on the first search -- as a
    fifth element.  ``capacity`` is the room of a tree in nodes; None: ``2 * simulations + 1``, the nodes one search can
    make plus as many carried ones.  That is the forest agent's allowance and not a measurement: a tree that is full
    stops growing until the next advance frees room."""

    _who = "GuidedReuseAgent values"

    def __init__(self, evaluate: Callable, simulations: int = 128, cpuct: int = DEFAULT_CPUCT, capacity: Optional[int] = None,
                 device: int = 0):
        super().__init__(evaluate, simulations, cpuct, capacity, device)
        if capacity is None:
            self.capacity = 2 * self.simulations + 1
        self._searched: Dict[tuple, tuple] = {}       # key of the batch -> (grids, movers) of its last search

    def _make(self, b):
        return GuidedForest(b, self.capacity, self.cpuct)

    def search(self, states: Sequence):
        """the search over `states` (Connect states that share one Config), on the trees of the last search there: the
        host copies of (visits int32[n, w], scores int32[n, w], best int32[n], nodes int32[n], kept int32[n])"""
        _only(self._game, states[0], self._who, self._elsewhere)
        b, arrays = self._loaded(states, self._who, self._game)
        key = self._game.key(states[0].config, len(states))
        forest = self._searches.get(key)
        if forest is None:
            forest = self._searches[key] = self._make(b)
        last = self._searched.get(key)
        kept = np.zeros(len(states), dtype=np.int32)
        if last is not None:
            t = b._need_torch("GuidedReuseAgent")
            plies = np.array([TreeSearchAgent.stones_between(last[0][k], int(last[1][k]), arrays[0][k]) for k in range(len(states))],
                             dtype=np.int32)
            for ply in (plies[:, 0], plies[:, 1]):      # the own move, then the reply: two calls
                kept = forest.advance(t.from_numpy(np.ascontiguousarray(ply)).to(f"cuda:{b.device}"))
            kept = kept.cpu().numpy()
        out = forest.run(self.evaluate, self.simulations, carry=last is not None)
        self._searched[key] = (arrays[0].copy(), arrays[1].copy())
        return tuple(x.cpu().numpy() for x in out[self._report:]) + (kept,)

    def close(self) -> None:
        self._searched.clear()
        super().close()


class BounceGuidedSearchAgent(_Guided):
    """The same agent for Bounce states: trees of ``nodes`` nodes (default: ``simulations + 1``) and ``edges`` pool edges
    (default: ``BounceBatch.guided_default_edges(nodes)``); a position that holds ``max_plies`` plies is valued as a draw.
    ``predict`` returns the visit shares of the root's moves, ``choose`` the launch's ``best``: the most visits, then the
    larger score, then the lower slot."""

    _game = _Bounce
    _who = "BounceGuidedSearchAgent values"
    _elsewhere = "Bounce states only; Connect states: GuidedSearchAgent"
    _evaluator = "(leaf_grid, leaf_player, leaf_targets) -> (priors, values)"
    _report = 4

    def __init__(self, evaluate: Callable, simulations: int = 128, cpuct: int = DEFAULT_CPUCT, nodes: Optional[int] = None,
                 edges: Optional[int] = None, max_plies: int = 65535, device: int = 0):
        if nodes is not None and nodes < 2:
            raise ValueError("nodes must be >= 2")
        if max_plies < 1:
            raise ValueError("max_plies must be >= 1")
        super().__init__(evaluate, simulations, cpuct, device)
        self.nodes = max(2, self.simulations + 1) if nodes is None else int(nodes)
        self.edges = None if edges is None else int(edges)
        self.max_plies = int(max_plies)

    def _make(self, b):
        return b.guided_moves_search(self.nodes, self.edges, self.cpuct, self.max_plies)

    def search(self, states: Sequence):
        """the search over `states` (Bounce states that share one Config): the host copies of (visits int32[n, w, h * w],
        scores int32[n, w, h * w], best int32[n], nodes int32[n], used int32[n])"""
        return self._run(states)
