"""``GuidedSearchAgent``: PUCT tree search over Connect positions whose leaves are valued by the caller's evaluator -- a
policy/value network, usually -- instead of random playouts (``ConnectBatch.guided_search``, bgs_connect_guided_step).

``evaluate(leaf_grid, leaf_player) -> (priors, values)`` sees device tensors: the leaves of all trees, int8[n, h, w] in the
batch's grid encoding (row 0 is the bottom; -1 empty, 0 and 1 the players) and int8[n] the player to move there, and
returns device tensors float32[n, w] (a weight a column: any non-negative numbers, they are normalised over the legal
columns) and float32[n] (the value for the player to move at the leaf, in [-1, 1]).  It is called once a simulation,
between two launches; the trees, the descent and the statistics stay on the device.

The agent has the shape of the agents in ``simulator.agents`` (``predict(state) -> {Action: float}``) and shares their
state loading."""

from __future__ import annotations

from typing import Callable, Dict, List, Optional, Sequence

from .agents import _Agent, _Connect, _only
from .batch import DEFAULT_CPUCT


class GuidedSearchAgent(_Agent):
    """``simulations`` simulations a position, ``cpuct`` = c_puct in Q8 (320 = 1.25), trees of ``capacity`` nodes
    (default: ``simulations + 1``, room for a node a simulation).  ``predict`` returns the visit shares of the root's
    columns, ``choose`` the launch's ``best``: the most visits, then the larger score, then the lower column.  There is no
    seed: nothing in this search is random."""

    _who = "GuidedSearchAgent values"
    _elsewhere = "covers Connect states only"

    def __init__(self, evaluate: Callable, simulations: int = 128, cpuct: int = DEFAULT_CPUCT, capacity: Optional[int] = None,
                 device: int = 0):
        if not callable(evaluate):
            raise TypeError("evaluate must be callable: (leaf_grid, leaf_player) -> (priors, values)")
        if simulations < 1:
            raise ValueError("simulations must be >= 1")
        if not 0 <= cpuct <= 4096:
            raise ValueError("cpuct must be 0 .. 4096 (c_puct in Q8)")
        if capacity is not None and capacity < 2:
            raise ValueError("capacity must be >= 2")
        super().__init__(device)
        self.evaluate = evaluate
        self.simulations = int(simulations)
        self.cpuct = int(cpuct)
        self.capacity = max(2, self.simulations + 1) if capacity is None else int(capacity)
        self._searches: Dict[tuple, object] = {}      # key of the batch -> its GuidedSearch

    def search(self, states: Sequence):
        """the search over `states` (Connect states that share one Config): the host copies of (visits int32[n, w],
        scores int32[n, w], best int32[n], nodes int32[n])"""
        _only(_Connect, states[0], self._who, self._elsewhere)
        b, _ = self._loaded(states, self._who, _Connect)
        key = _Connect.key(states[0].config, len(states))
        guided = self._searches.get(key)
        if guided is None:
            guided = self._searches[key] = b.guided_search(self.capacity, self.cpuct)
        out = guided.run(self.evaluate, self.simulations)
        return tuple(x.cpu().numpy() for x in out[3:])

    def predict_many(self, states: Sequence) -> List[Dict]:
        """`predict` of every state, searched together: {action: visit share}"""
        if not states:
            return []
        visits = self.search(states)[0]
        shares = []
        for k, s in enumerate(states):
            total = max(1, int(visits[k].sum()))
            shares.append({a: float(visits[k][_Connect.index(a)]) / total for a in s.actions})
        return shares

    def choose_many(self, states: Sequence) -> List:
        """the launch's `best` of every state (None: no action)"""
        if not states:
            return []
        best = self.search(states)[2]
        return [_Connect.action(s, slot) for s, slot in zip(states, best)]

    def predict(self, state) -> Dict:
        return self.predict_many([state])[0]

    def choose(self, state):
        return self.choose_many([state])[0]

    def close(self) -> None:
        for guided in self._searches.values():
            guided.close()
        self._searches.clear()
        super().close()
