"""Agents on top of the batched engine, in the shape of the reference's ``textual/examples/agent.py``:
``Agent.predict(state) -> dict[Action, float]``.

``MonteCarloAgent`` is flat Monte-Carlo: every legal column of a position is valued by ``playouts`` uniform random games
that start with it, ``(wins + draws / 2) / playouts`` for the player to move.  All columns of all positions are played
and counted in ONE launch (``ConnectBatch.evaluate_actions``).
"""

from __future__ import annotations

from typing import Dict, List, Sequence

import numpy as np

from .batch import DEFAULT_SEED, ConnectBatch
from .game import connect


class MonteCarloAgent:
    """Flat Monte-Carlo evaluation of Connect positions (``simulator.game.connect.State``).

    The playouts of the position at index k of a call are games ``((first_game + k) * width + c) * playouts + p`` of
    ``seed``: ``predict(state, game=k)`` gives what ``predict_many(states)[k]`` gives for the same ``state``.
    """

    def __init__(self, playouts: int = 256, seed: int = DEFAULT_SEED, device: int = 0):
        if playouts < 1:
            raise ValueError("playouts must be >= 1")
        self.playouts = int(playouts)
        self.seed = int(seed)
        self.device = int(device)
        self._batches: Dict[tuple, ConnectBatch] = {}

    def _batch(self, config: connect.Config, n: int) -> ConnectBatch:
        key = (config.height, config.width, config.count, n)
        b = self._batches.get(key)
        if b is None:
            b = ConnectBatch(config.height, config.width, config.count, n, device=self.device)
            self._batches[key] = b
        return b

    def values(self, batch: ConnectBatch, first_game: int = 0) -> np.ndarray:
        """float64[n, width] for the boards of `batch`: (wins + draws / 2) / playouts of every column for the player to
        move, NaN where the column is illegal or the board has ended.  Sets the batch's first_game to `first_game`; the
        boards are not modified."""
        batch.set_first_game(first_game)
        counts = batch.evaluate_actions(seed=self.seed, playouts=self.playouts).astype(np.float64)
        v = (counts[..., 0] + 0.5 * counts[..., 1]) / self.playouts
        v[batch.legal == 0] = np.nan
        return v

    def predict_many(self, states: Sequence[connect.State], first_game: int = 0) -> List[Dict[connect.Action, float]]:
        """`predict` of every state, evaluated in one call (all states must share one Config)."""
        if not states:
            return []
        config = states[0].config
        if any(s.config != config for s in states):
            raise ValueError("predict_many: the states must share one Config")
        b = self._batch(config, len(states))
        grid = np.stack([s.grid for s in states])
        player = np.array([s.player for s in states], dtype=np.int8)
        winner = np.array([-1 if not s.has_ended else int(s.to_json()["winner"]) for s in states], dtype=np.int8)
        status = b.write_state(grid, player, winner)
        if (status != 0).any():
            raise ValueError("predict_many: a state could not be loaded")
        v = self.values(b, first_game)
        return [{a: float(v[k, a.column]) for a in s.actions} for k, s in enumerate(states)]

    def predict(self, state: connect.State, game: int = 0) -> Dict[connect.Action, float]:
        """{action: value} for every action in ``state.actions`` (the keys are those Action objects)."""
        return self.predict_many([state], first_game=game)[0]

    def close(self) -> None:
        for b in self._batches.values():
            b.close()
        self._batches.clear()
