"""Agents on top of the batched engine, in the shape of the reference's ``textual/examples/agent.py``:
``Agent.predict(state) -> dict[Action, float]``.

``MonteCarloAgent`` is flat Monte-Carlo: every legal action of a position is valued by ``playouts`` random games (uniform,
or by the game's decisive-move playout policy) that start with it, ``(wins + draws / 2) / playouts`` for the player to move.  All actions of all positions are played
and counted in ONE launch: ``ConnectBatch.evaluate_actions`` for Connect states (a column each),
``BounceBatch.evaluate_moves`` for Bounce states (a (source, target) move each).

``SolverAgent`` values Connect positions exactly where it can (``ConnectBatch.solve_actions``): 1.0 for a forced win,
0.5 for a draw, 0.0 for a forced loss, and a fallback agent's value where the search was cut by its horizon or budget.
Bounce positions go to the horizon search ``BounceBatch.solve_moves`` in the same way (dispatched on the state's type).

``TreeSearchAgent`` grows a UCT tree a Connect position (``ConnectBatch.search_actions``: all positions of a call in one
launch) and plays the column with the most visits; with ``reuse=True`` it keeps the trees from call to call
(``ConnectBatch.search_forest``) and carries the subtree under the moves played into the next search.

``BounceHalvingAgent`` spends a fixed budget of playouts a Bounce position by sequential halving
(``BounceBatch.evaluate_moves_halving``) and plays the last surviving move.

``BounceTreeSearchAgent`` grows a UCT tree a Bounce position (``BounceBatch.search_moves``) and plays the move with the
most visits; with ``reuse=True`` it keeps the trees from call to call (``BounceBatch.search_moves_forest``) as
``TreeSearchAgent`` does.

What differs between the two games at this level stands once, in ``_Connect`` and ``_Bounce`` below: the key and the making
of a batch, the arrays ``write_state`` takes, the default playout cap, and the mapping between an action, its index in a
per-root output row and its flat slot.  ``_Agent`` owns an agent's batches and loads states into them (``_loaded``), and
``_TreeSearch`` is the one body of the two tree-search agents, which add their batch calls and their "between" function.
"""

from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Union

import numpy as np

from .batch import (DEFAULT_BOUNCE_SOLVE_DEPTH, DEFAULT_EXPLORE, DEFAULT_SEED, DEFAULT_SOLVE_NODES, SOLVE_BUDGET, SOLVE_DRAW, SOLVE_LOSS,
                    SOLVE_UNKNOWN, SOLVE_WIN, HALVING_SHORT, BounceBatch, ConnectBatch, playout_policy)
from .game import bounce, connect

# Bounce playouts stop at this absolute ply count unless the agent is given another cap: random Bounce games are short
# (28 plies on average), but a few in 2^18 never end, and a capped game counts as neither a win, a draw nor a loss.
BOUNCE_MAX_PLIES = 1024


class _Connect:
    """Connect, as an agent sees it."""

    name = "Connect"
    State = connect.State
    max_plies = 2**31 - 1       # the playout cap of an agent that was given none: Connect games end by themselves

    @staticmethod
    def key(config: connect.Config, n: int) -> tuple:
        """of the batch of `n` boards of `config` in an agent's cache"""
        return ("connect", config.height, config.width, config.count, n)

    @staticmethod
    def batch(config: connect.Config, n: int, device: int) -> ConnectBatch:
        return ConnectBatch(config.height, config.width, config.count, n, device=device)

    @staticmethod
    def arrays(states: Sequence) -> tuple:
        """(grid, player, winner) of `states`, as `write_state` takes them"""
        return (np.stack([s.grid for s in states]), np.array([s.player for s in states], dtype=np.int8),
                np.array([s._winner for s in states], dtype=np.int8))

    @staticmethod
    def index(action) -> tuple:
        """where `action` sits in its root's row of a per-column output"""
        return (action.column,)

    @staticmethod
    def slot(action) -> int:
        return action.column

    @staticmethod
    def action(state, slot):
        """the action of `state` in column `slot`; None for a negative one (an ended board)"""
        return state.action_at(int(slot)) if slot >= 0 else None


class _Bounce:
    """Bounce, as an agent sees it.  A move is the piece in column x of the active row going to (tx, ty): entry (x, ty *
    width + tx) of its root's row of a per-move output, slot x * height * width + ty * width + tx."""

    name = "Bounce"
    State = bounce.State
    max_plies = BOUNCE_MAX_PLIES

    @staticmethod
    def key(config: bounce.Config, n: int) -> tuple:
        grid = config.grid
        return ("bounce", grid.shape, grid.tobytes(), n)

    @staticmethod
    def batch(config: bounce.Config, n: int, device: int) -> BounceBatch:
        return BounceBatch(config.grid, n, device=device)

    @staticmethod
    def arrays(states: Sequence) -> tuple:
        """(grid, player, winner, plies) of `states`, as `write_state` takes them: the plies are the state's own count,
        because a playout's draws are keyed by the absolute ply"""
        return (np.stack([s.grid for s in states]), np.array([s.player for s in states], dtype=np.int8),
                np.array([s._winner for s in states], dtype=np.int8), np.array([s._plies for s in states], dtype=np.int32))

    @staticmethod
    def index(action) -> tuple:
        return (action._source[0], action._target[1] * action.state._grid.shape[1] + action._target[0])

    @staticmethod
    def slot(action) -> int:
        x, cell = _Bounce.index(action)
        return x * action.state._grid.size + cell

    @staticmethod
    def action(state, slot):
        """the action of `state` with flat slot `slot`; None for a negative one (an ended board)"""
        return {_Bounce.slot(a): a for a in state.actions}[int(slot)] if slot >= 0 else None


def _game_of(state):
    """the game of a state that is known to be one of the two's"""
    return _Bounce if isinstance(state, bounce.State) else _Connect


def _only(game, state, who: str, elsewhere: str) -> None:
    """refuse a `state` that is not `game`'s: the other game's with `elsewhere`, anything else by the name of its type"""
    if isinstance(state, game.State):
        return
    if isinstance(state, (connect.State, bounce.State)):
        raise ValueError(f"{who} {elsewhere}")
    raise TypeError(f"{who} {game.name} states, not {type(state).__name__}")


class _Agent:
    """What the agents share: the batches an agent holds, one a (game, Config, number of states), the loading of states
    into them, and the one-state wrappers."""

    def __init__(self, device: int):
        self.device = int(device)
        self._batches: Dict[tuple, Union[ConnectBatch, BounceBatch]] = {}

    def _cap(self, game) -> int:
        """the playout cap of a launch: the agent's own `max_plies`, else the game's default"""
        return game.max_plies if self.max_plies is None else self.max_plies

    def _loaded(self, states: Sequence, who: str, game=None, shared: Optional[str] = None):
        """(batch, arrays): the agent's batch of len(states) boards, holding `states`, and the arrays it was given
        (`game.arrays`).  The states must be `game`'s and share one Config; `who` opens the refusals, and `shared` is the
        text of that one where it is another.  Without `game` the states must be of one type, and the agent's `_game_for`
        says, after that check, which game they are."""
        config = states[0].config
        kind = type(states[0]) if game is None else game.State
        if any(not isinstance(s, kind) or s.config != config for s in states):
            raise ValueError(shared or f"{who} the states must share one Config")
        if game is None:
            game = self._game_for(states[0])
        key = game.key(config, len(states))
        b = self._batches.get(key)
        if b is None:
            b = self._batches[key] = game.batch(config, len(states), self.device)
        arrays = game.arrays(states)
        if (b.write_state(*arrays) != 0).any():
            raise ValueError(f"{who} a state could not be loaded")
        return b, arrays

    def predict(self, state, game: int = 0) -> Dict:
        """{action: value} for every action in ``state.actions`` (the keys are those Action objects): `predict_many` of
        one state, as game `game`"""
        return self.predict_many([state], first_game=game)[0]

    def choose(self, state, game: int = 0):
        """`choose_many` of one state"""
        return self.choose_many([state], first_game=game)[0]

    def close(self) -> None:
        for b in self._batches.values():
            b.close()
        self._batches.clear()


class MonteCarloAgent(_Agent):
    """Flat Monte-Carlo evaluation of Connect positions (``simulator.game.connect.State``) and Bounce positions
    (``simulator.game.bounce.State``), dispatched on the state's type.

    The playouts of the position at index k of a call are games ``((first_game + k) * width + c) * playouts + p`` of
    ``seed`` for Connect (c the column) and ``((first_game + k) * S + s) * playouts + p`` for Bounce (S = width * height *
    width, s = x * height * width + ty * width + tx for the move of the piece in column x of the active row to (tx, ty)):
    ``predict(state, game=k)`` gives what ``predict_many(states)[k]`` gives for the same ``state``.

    ``max_plies`` caps every playout at that absolute ply count (a capped playout adds nothing to the value).  None: no
    cap for Connect, whose games end by themselves, and ``BOUNCE_MAX_PLIES`` (1024) for Bounce.

    ``policy`` is the playout policy: "uniform", or "decisive".  For Connect states a decisive playout takes a winning
    column, else blocks the opponent's, else plays uniformly (``ConnectBatch.evaluate_actions(policy=...)``).  For Bounce
    states it lands in the mover's goal row when it can, else plays uniformly; there is no blocking step
    (``BounceBatch.evaluate_moves(policy=...)``).  The two games' "decisive" are different policies under one name, so an
    agent with a policy other than "uniform" stays with the game of the first states it evaluates: a state of the other
    game raises ValueError (make an agent a game).  A uniform agent takes states of either game, as before.

    ``allocation`` says how a Connect position's playouts are spread over its columns.  "flat": ``playouts`` a column.
    "halving": sequential halving (``ConnectBatch.evaluate_actions_halving``) with ``budget`` playouts a position,
    ``playouts * width`` unless ``budget`` is given -- the same total, moved round by round to the columns still in
    doubt; a column's value is ``(wins + draws / 2) / given`` over the playouts it was given.  Bounce has the flat
    allocation alone: a Bounce state with ``allocation="halving"`` raises ValueError.

    ``choose(state)`` / ``choose_many(states)`` return the action to play: flat, the best-valued action (the first in
    ``state.actions`` order on ties); halving, the last surviving column.
    """

    def __init__(self, playouts: int = 256, seed: int = DEFAULT_SEED, device: int = 0, max_plies: Optional[int] = None,
                 policy: str = "uniform", allocation: str = "flat", budget: Optional[int] = None):
        playout_policy(policy)
        if allocation not in ("flat", "halving"):
            raise ValueError(f"unknown allocation {allocation!r}: 'flat' or 'halving'")
        if budget is not None and (allocation != "halving" or budget < 1):
            raise ValueError("budget: a positive number of playouts a position, with allocation='halving' only")
        if playouts < 1:
            raise ValueError("playouts must be >= 1")
        if max_plies is not None and max_plies < 1:
            raise ValueError("max_plies must be >= 1")
        super().__init__(device)
        self.playouts = int(playouts)
        self.seed = int(seed)
        self.max_plies = None if max_plies is None else int(max_plies)
        self.policy = policy
        self.allocation = allocation
        self.budget = None if budget is None else int(budget)
        self._policy_game: Optional[str] = None   # the game whose `policy` this agent plays (set by its first states)

    def _bind(self, game: str) -> None:
        """a policy other than "uniform" is one game's: the first states evaluated say which"""
        if self.policy == "uniform":
            return
        if self._policy_game is None:
            self._policy_game = game
        elif self._policy_game != game:
            raise ValueError(f"MonteCarloAgent: this agent plays {self._policy_game}'s {self.policy!r} playout policy, which is not "
                             f"{game}'s policy of that name: make an agent of its own for {game} states")

    def _game_for(self, state):
        """the game of `state`, once the agent takes it (`_loaded` asks, before it makes a batch)"""
        if isinstance(state, bounce.State):
            if self.allocation != "flat":
                raise ValueError("MonteCarloAgent: Bounce moves are evaluated flat, there is no halving allocation for Bounce states")
        elif not isinstance(state, connect.State):
            raise TypeError(f"predict_many: Connect or Bounce states, not {type(state).__name__}")
        game = _game_of(state)
        self._bind(game.name)
        return game

    def values(self, batch: ConnectBatch, first_game: int = 0) -> np.ndarray:
        """float64[n, width] for the boards of `batch`: (wins + draws / 2) / playouts of every column for the player to
        move, NaN where the column is illegal or the board has ended.  Sets the batch's first_game to `first_game`; the
        boards are not modified."""
        if self.allocation == "halving":
            return self.halving_values(batch, first_game)[0]
        batch.set_first_game(first_game)
        cap = self._cap(_Connect)
        counts = batch.evaluate_actions(seed=self.seed, playouts=self.playouts, max_plies=cap, policy=self.policy).astype(np.float64)
        v = (counts[..., 0] + 0.5 * counts[..., 1]) / self.playouts
        v[batch.legal == 0] = np.nan
        return v

    def halving_values(self, batch: ConnectBatch, first_game: int = 0):
        """(float64[n, width], int32[n]) for the boards of `batch` under sequential halving: (wins + draws / 2) / given of
        every column (NaN where the column is illegal or the board has ended; a legal column is never given zero
        playouts) and the last surviving column (-1: an ended board).  Sets the batch's first_game to `first_game`."""
        batch.set_first_game(first_game)
        cap = self._cap(_Connect)
        budget = self.playouts * batch.width if self.budget is None else self.budget
        counts, given, best = batch.evaluate_actions_halving(seed=self.seed, budget=budget, max_plies=cap, policy=self.policy)
        v = np.full(given.shape, np.nan)
        played = given > 0
        v[played] = (counts[..., 0][played] + 0.5 * counts[..., 1][played]) / given[played]
        return v, best

    def bounce_values(self, batch: BounceBatch, first_game: int = 0) -> np.ndarray:
        """float64[n, width, height * width] for the boards of a BounceBatch: (wins + draws / 2) / playouts of the move of
        the piece in column x of the active row to cell c, for the player to move; NaN where that move is illegal or the
        board has ended.  Sets the batch's first_game to `first_game`; the boards are not modified."""
        batch.set_first_game(first_game)
        cap = self._cap(_Bounce)
        counts = batch.evaluate_moves(seed=self.seed, playouts=self.playouts, max_plies=cap, policy=self.policy).astype(np.float64)
        v = (counts[..., 0] + 0.5 * counts[..., 1]) / self.playouts
        t = batch.targets[:, : batch.width]
        cells = np.arange(batch.height * batch.width, dtype=np.uint64)
        legal = ((t[..., None] >> cells) & np.uint64(1)) != 0
        v[~legal] = np.nan
        return v

    def predict_many(self, states: Sequence, first_game: int = 0) -> List[Dict]:
        """`predict` of every state, evaluated in one call (all states must be of one game and share one Config)."""
        if not states:
            return []
        b, _ = self._loaded(states, "predict_many:")
        game = _game_of(states[0])
        v = self.bounce_values(b, first_game) if game is _Bounce else self.values(b, first_game)
        return [{a: float(v[k][game.index(a)]) for a in s.actions} for k, s in enumerate(states)]

    def choose_many(self, states: Sequence, first_game: int = 0) -> List:
        """the action to play in every state (None where it has no action): flat, the best-valued action, the first in
        ``state.actions`` order on ties; halving, the last surviving column of the same launch `predict_many` makes"""
        if not states:
            return []
        if self.allocation == "halving" and not isinstance(states[0], bounce.State):
            # (callers match these texts: the refusal of mixed Configs names choose_many, this path's others predict_many)
            b, _ = self._loaded(states, "predict_many:", shared="choose_many: the states must share one Config")
            best = self.halving_values(b, first_game)[1]
            return [_Connect.action(s, c) for s, c in zip(states, best)]
        out = []
        for s, values in zip(states, self.predict_many(states, first_game)):
            out.append(max(s.actions, key=values.get) if s.actions else None)   # (max keeps the first of equal values)
        return out


def _proved_shares(visits, proved, at: Sequence[tuple]) -> List[float]:
    """The shares `predict` gives the legal moves of one root that was searched with `prove`, in the order of `at`, the
    moves' indices in the root's rows `visits` and `proved`.  A proved win takes everything (several share it); else the
    moves proved lost get 0, unless every move is, and the others keep their visits.  The shares sum to 1."""
    share = [float(visits[i]) for i in at]
    codes = [proved[i] for i in at]
    if any(c == SOLVE_WIN for c in codes):
        share = [1.0 if c == SOLVE_WIN else 0.0 for c in codes]
    elif any(c != SOLVE_LOSS for c in codes):
        share = [0.0 if c == SOLVE_LOSS else s for c, s in zip(codes, share)]
    total = sum(share)
    return [s / total for s in share]


class _TreeSearch(_Agent):
    """The body of ``TreeSearchAgent`` and ``BounceTreeSearchAgent``.  A subclass names its game (``_game``) and what it
    says to states that are not that game's (``_who``, ``_elsewhere``) and to ``prove`` with ``reuse`` (``_no_proving_forest``),
    and makes the batch's calls: ``_launch``, ``_forest``, and ``_between`` for the plies played since the forest's last
    search.  What a search returns is the batch's tuple, in which ``visits`` and ``best`` are the second and third element
    and, with ``prove``, ``proved`` and ``done`` the last two."""

    def __init__(self, iterations: int = 256, leaf_playouts: int = 64, explore: int = DEFAULT_EXPLORE, policy: str = "uniform",
                 seed: int = DEFAULT_SEED, device: int = 0, max_plies: Optional[int] = None, prove: bool = False,
                 reuse: bool = False, capacity: Optional[int] = None):
        playout_policy(policy)
        if prove and reuse:
            raise ValueError(f"prove=True with reuse=True: {self._no_proving_forest}")
        if iterations < 1 or leaf_playouts < 1:
            raise ValueError("iterations and leaf_playouts must be >= 1")
        if not 0 <= explore <= 1 << 18:
            raise ValueError("explore must be 0 .. 2**18")
        if max_plies is not None and max_plies < 1:
            raise ValueError("max_plies must be >= 1")
        if capacity is not None and capacity < 2:
            raise ValueError("capacity must be >= 2")
        super().__init__(device)
        self.prove = bool(prove)
        self.reuse = bool(reuse)
        self.capacity = 2 * int(iterations) + 1 if capacity is None else int(capacity)
        # key of the batch -> [the forest, what was last searched there (grids, movers; for Bounce, ply counts), searches so far]
        self._forests: Dict[tuple, list] = {}
        self.iterations = int(iterations)
        self.leaf_playouts = int(leaf_playouts)
        self.explore = int(explore)
        self.policy = policy
        self.seed = int(seed)
        self.max_plies = None if max_plies is None else int(max_plies)

    def search(self, states: Sequence, first_game: int = 0):
        """the launch over `states` (states of the agent's game that share one Config): (counts, visits, best, nodes), for
        Bounce (counts, visits, best, nodes, used); with `reuse` followed by carried, with `prove` by proved and done"""
        game = self._game
        _only(game, states[0], self._who, self._elsewhere)
        b, arrays = self._loaded(states, self._who, game)
        b.set_first_game(first_game)
        arguments = dict(iterations=self.iterations, leaf_playouts=self.leaf_playouts, explore=self.explore, max_plies=self._cap(game),
                         policy=self.policy)
        if not self.reuse:
            return self._launch(b, seed=self.seed, **arguments)
        # the search of `reuse`: advance the batch's forest from what it last searched to these states, then search on
        now = arrays[:2] + arrays[3:]       # grids, movers (, ply counts)
        key = game.key(states[0].config, len(states))
        entry = self._forests.get(key)
        if entry is None:
            entry = self._forests[key] = [self._forest(b), *[None] * len(now), 0]
        forest, *last, searches = entry
        if last[0] is not None:
            plies = np.array([self._between(last, now, k) for k in range(len(states))], dtype=np.int32)
            for ply in (plies[:, 0], plies[:, 1]):
                if (ply >= 0).any():
                    forest.advance(ply)
        out = forest.search(seed=(self.seed + searches) % 2**64, **arguments)
        entry[1:] = [*now, searches + 1]
        return out

    def predict_many(self, states: Sequence, first_game: int = 0) -> List[Dict]:
        """`predict` of every state, searched in one launch"""
        if not states:
            return []
        out = self.search(states, first_game)
        visits, index = out[1], self._game.index
        shares = []
        for k, s in enumerate(states):
            actions = s.actions
            if self.prove:      # a proved win takes everything, moves proved lost nothing (unless all are)
                shares.append(dict(zip(actions, _proved_shares(visits[k], out[-2][k], [index(a) for a in actions]))))
                continue
            # a kept root's visits include the carried ones
            total = int(visits[k].sum()) if self.reuse else self.iterations * self.leaf_playouts
            shares.append({a: float(visits[k][index(a)]) / total for a in actions})
        return shares

    def choose_many(self, states: Sequence, first_game: int = 0) -> List:
        """the most visited action of every state (with `prove`, the launch's `best`), of the same launch `predict_many`
        makes (None: no action)"""
        if not states:
            return []
        best = self.search(states, first_game)[2]
        return [self._game.action(s, slot) for s, slot in zip(states, best)]

    def close(self) -> None:
        for entry in self._forests.values():
            entry[0].close()
        self._forests.clear()
        super().close()


class TreeSearchAgent(_TreeSearch):
    """UCT tree search over Connect positions (``simulator.game.connect.State``): ``ConnectBatch.search_actions`` with
    ``iterations`` iterations and ``leaf_playouts`` playouts a leaf, ``iterations * leaf_playouts`` playouts a position,
    one launch for all positions of a call.

    ``predict`` / ``predict_many`` map every action of ``state.actions`` to its share of the root's visits (the shares of
    a state sum to 1); ``choose`` / ``choose_many`` return the column with the most visits (ties: the larger 2 * wins +
    draws, then the lower column; None for a state without an action).  The playouts of the position at index k of a call
    are the games ``((first_game + k) * iterations + t) * leaf_playouts + j`` of ``seed``.  ``explore`` is about 45426 *
    C * C for a UCB1 constant C; ``policy`` is the playout policy, "uniform" or "decisive"; ``max_plies`` caps every
    playout at that absolute ply count (None: no cap).  Bounce states raise ValueError: the search covers Connect.

    ``reuse=True`` keeps the trees between calls (``ConnectBatch.search_forest``): the agent holds a forest per (Config,
    number of states) and remembers the grids it last searched there.  Before a search it advances the tree at index k by
    the one or two stones that lead from the remembered grid k to the new one -- the remembered mover's stone first, and
    the lower stone first when both share a column --, so the subtree under the moves played is carried into the search;
    an equal grid is searched on, and any other difference makes the search start that tree anew.  So the states of
    successive calls must keep their indices.  Search number m on a forest (from 0) draws with ``seed + m`` (mod 2^64),
    ``visits`` include the carried ones (the shares ``predict`` gives still sum to 1), and ``search`` returns ``carried`` --
    the nodes every tree started with -- as a fifth element.  ``capacity`` is the room of a tree in nodes; None:
    ``2 * iterations + 1``, the nodes one search can make plus as many carried ones.  That is an allowance and not a
    measurement: a tree that is full stops growing until the next advance frees room.  Without ``reuse`` the agent is
    what it was, code path included.

    ``prove=True`` searches with ``ConnectBatch.search_actions_proving``: game-end facts are kept on the edges and backed
    up by minimax, a root whose value is proved stops iterating, and ``search`` returns (counts, visits, best, nodes,
    proved, done).  ``choose`` follows that launch's ``best`` (a proved win, else the most visited column among those not
    proved lost).  ``predict`` gives a proved win 1.0 and every other column 0; otherwise the columns proved lost get 0
    and the rest are renormalised, and where every column is proved lost the shares are what the visits give.  The forest
    does not prove yet: ``prove=True`` with ``reuse=True`` raises ValueError.  Without ``prove`` the code path is what it
    was."""

    _game = _Connect
    _who = "TreeSearchAgent:"
    _elsewhere = "Connect states only; the tree search does not cover Bounce"
    _no_proving_forest = "the forest does not prove yet"

    @staticmethod
    def stones_between(old: np.ndarray, mover: int, new: np.ndarray):
        """the columns (first, second; -1: none) of the one or two stones that lead from grid `old` with `mover` to move
        to grid `new`: the mover's stone first, the lower stone first when both share a column.  (-1, -1) for equal grids
        and for any other difference."""
        rows, cols = np.nonzero(old != new)
        if not 1 <= rows.size <= 2 or (old[rows, cols] != -1).any():
            return -1, -1
        stones = [(int(r), int(c), int(new[r, c])) for r, c in zip(rows, cols)]   # (row, column, owner); row 0 is the bottom
        if len(stones) == 1:
            return (stones[0][1], -1) if stones[0][2] == mover else (-1, -1)
        if sorted(s[2] for s in stones) != [0, 1]:
            return -1, -1
        stacked = stones[0][1] == stones[1][1]
        stones.sort(key=lambda s: s[0] if stacked else s[2] != mover)
        return stones[0][1], stones[1][1]

    def _launch(self, b: ConnectBatch, **arguments):
        return (b.search_actions_proving if self.prove else b.search_actions)(**arguments)

    def _forest(self, b: ConnectBatch):
        return b.search_forest(self.capacity)

    def _between(self, last, now, k: int):
        return self.stones_between(last[0][k], int(last[1][k]), now[0][k])


class BounceHalvingAgent(_Agent):
    """Sequential halving over the moves of Bounce positions (``simulator.game.bounce.State``):
    ``BounceBatch.evaluate_moves_halving`` with ``budget`` playouts a position, one launch for all positions of a call.

    ``predict`` / ``predict_many`` map every action of ``state.actions`` to ``(wins + draws / 2) / given`` over the
    playouts the move was given (0.0 where it was given none); ``choose`` / ``choose_many`` return the last surviving move
    (None for a state without an action).  The playouts of the position at index k of a call are the games
    ``((first_game + k) * S + s) * budget + p`` of ``seed``, as for ``MonteCarloAgent`` with ``playouts = budget``.
    ``max_plies`` caps every playout at that absolute ply count; None: ``BOUNCE_MAX_PLIES`` (1024).  ``policy``:
    "uniform" or "decisive" (``BounceBatch.evaluate_moves(policy=...)``).

    A position with A legal moves needs ``budget >= BounceBatch.halving_min_budget(A)``; one that needs more raises
    ValueError.  Connect states raise ValueError: they are ``MonteCarloAgent(allocation="halving")``'s.  (A class of its
    own because ``MonteCarloAgent(allocation="halving")`` refuses Bounce states; folding the two is a later change.)"""

    def __init__(self, budget: int = 1024, seed: int = DEFAULT_SEED, device: int = 0, max_plies: Optional[int] = None,
                 policy: str = "uniform"):
        playout_policy(policy)
        if budget < 1:
            raise ValueError("budget must be >= 1")
        if max_plies is not None and max_plies < 1:
            raise ValueError("max_plies must be >= 1")
        super().__init__(device)
        self.budget = int(budget)
        self.seed = int(seed)
        self.max_plies = None if max_plies is None else int(max_plies)
        self.policy = policy

    def _evaluate(self, states: Sequence, first_game: int):
        """(counts, given, best) of the launch over `states`"""
        _only(_Bounce, states[0], "BounceHalvingAgent:", 'Bounce states only; Connect states: MonteCarloAgent(allocation="halving")')
        b, _ = self._loaded(states, "BounceHalvingAgent:", _Bounce)
        b.set_first_game(first_game)
        counts, given, best = b.evaluate_moves_halving(seed=self.seed, budget=self.budget, max_plies=self._cap(_Bounce),
                                                       policy=self.policy)
        for k in np.flatnonzero(best == HALVING_SHORT):
            moves = len(states[k].actions)
            raise ValueError(f"BounceHalvingAgent: state {k} has {moves} legal moves and needs a budget of "
                             f"{BounceBatch.halving_min_budget(moves)} playouts, this agent's is {self.budget}")
        return counts, given, best

    def predict_many(self, states: Sequence, first_game: int = 0) -> List[Dict[bounce.Action, float]]:
        """`predict` of every state, evaluated in one launch (the states must share one Config)"""
        if not states:
            return []
        counts, given, _ = self._evaluate(states, first_game)
        out = []
        for k, s in enumerate(states):
            values = {}
            for a in s.actions:
                at = (k,) + _Bounce.index(a)
                values[a] = float((counts[at][0] + 0.5 * counts[at][1]) / given[at]) if given[at] else 0.0
            out.append(values)
        return out

    def choose_many(self, states: Sequence, first_game: int = 0) -> List:
        """the last surviving move of every state, of the same launch `predict_many` makes (None: no action)"""
        if not states:
            return []
        best = self._evaluate(states, first_game)[2]
        return [_Bounce.action(s, slot) for s, slot in zip(states, best)]


class BounceTreeSearchAgent(_TreeSearch):
    """UCT tree search over Bounce positions (``simulator.game.bounce.State``): ``BounceBatch.search_moves`` with
    ``iterations`` iterations and ``leaf_playouts`` playouts a leaf, ``iterations * leaf_playouts`` playouts a position,
    one launch for all positions of a call.  The sibling of ``BounceHalvingAgent``, which spends the same playouts on one
    ply.

    ``predict`` / ``predict_many`` map every action of ``state.actions`` to its share of the root's visits (the shares of
    a state sum to 1); ``choose`` / ``choose_many`` return the move with the most visits (ties: the larger 2 * wins +
    draws, then the lower slot; None for a state without an action).  The playouts of the position at index k of a call
    are the games ``((first_game + k) * iterations + t) * leaf_playouts + j`` of ``seed``.  ``explore`` is about 45426 *
    C * C for a UCB1 constant C; ``policy`` is the playout policy, "uniform" or "decisive"; ``max_plies`` caps every
    playout at that absolute ply count (None: ``BOUNCE_MAX_PLIES``, 1024); ``edges`` is the edge pool of a position
    (None: ``BounceBatch.search_default_edges``).  Connect states raise ValueError: they are ``TreeSearchAgent``'s.

    ``reuse=True`` keeps the trees between calls (``BounceBatch.search_moves_forest``): the agent holds a forest per
    (Config, number of states) and remembers the grids, movers and ply counts it last searched there.  Before a search it
    advances the tree at index k by the one or two moves that lead from the remembered grid k to the new one -- its own
    move, then the reply --, inferred from the grid difference (``moves_between``); where the difference is not one or
    two clean piece moves it advances nothing, and the search's own check starts that tree anew.  So the states of
    successive calls must keep their indices.  Search number m on a forest (from 0) draws with ``seed + m`` (mod 2^64),
    ``visits`` include the carried ones (the shares ``predict`` gives still sum to 1), and ``search`` returns ``carried``
    -- the nodes every tree started with -- as a sixth element.  ``capacity`` is the room of a tree in nodes; None: ``2 *
    iterations + 1``, the nodes one search can make plus as many carried ones; the pool is ``edges`` or the default pool
    of ``capacity - 1`` iterations.  Both are allowances and not measurements: a tree that is full stops growing until
    the next advance frees room.  Without ``reuse`` the agent is what it was, code path included.

    ``prove=True`` searches with ``BounceBatch.search_moves_proving``: game-end facts are kept on the edges and backed up
    by minimax, a root whose value is proved stops iterating, and ``search`` returns (counts, visits, best, nodes, used,
    proved, done).  ``choose`` follows that launch's ``best`` (a proved win, else the most visited move among those not
    proved lost).  ``predict`` gives a proved win 1.0 and every other move 0; otherwise the moves proved lost get 0 and
    the rest are renormalised, and where every move is proved lost the shares are what the visits give.  The forest does
    not prove: ``prove=True`` with ``reuse=True`` raises ValueError.  Without ``prove`` the code path is what it was."""

    _game = _Bounce
    _who = "BounceTreeSearchAgent:"
    _elsewhere = "Bounce states only; Connect states: TreeSearchAgent"
    _no_proving_forest = "the forest does not prove"

    def __init__(self, iterations: int = 256, leaf_playouts: int = 64, explore: int = DEFAULT_EXPLORE, policy: str = "uniform",
                 seed: int = DEFAULT_SEED, device: int = 0, max_plies: Optional[int] = None, edges: Optional[int] = None,
                 prove: bool = False, reuse: bool = False, capacity: Optional[int] = None):
        super().__init__(iterations, leaf_playouts, explore, policy, seed, device, max_plies, prove, reuse, capacity)
        self.edges = None if edges is None else int(edges)

    @staticmethod
    def moves_between(old: np.ndarray, mover: int, new: np.ndarray, plies: int):
        """the slots (first, second; -1: none) of the one or two piece moves that lead from grid `old` with `mover` to
        move to grid `new`, `plies` (1 or 2) plies later: the mover's move first.  A clean move empties one cell and fills
        an empty one with the same value.  Two pieces of one value leave the pairing of sources and targets open; both
        pairings give the same position after the two plies, so the one whose moves are nearer to an unbounced walk
        (|dx| + |dy| = the piece's value, never backwards) is taken, and a pairing that is no legal pair of moves finds
        no such arm in the tree, which is then started anew as if nothing had been advanced.  (-1, -1) for anything else:
        equal grids, another ply difference, a reply that moved the piece just played or landed on the cell it left, two
        moves whose sources share a row (the order would be a guess), two pairings that are equally near."""
        h, w = old.shape
        ys, xs = np.nonzero(old != new)
        gone = [(int(y), int(x)) for y, x in zip(ys, xs) if old[y, x] != 0 and new[y, x] == 0]
        come = [(int(y), int(x)) for y, x in zip(ys, xs) if old[y, x] == 0 and new[y, x] != 0]
        if plies not in (1, 2) or len(gone) != plies or len(come) != plies or ys.size != 2 * plies:
            return -1, -1

        def slot(source, target):
            return source[1] * h * w + target[0] * w + target[1]

        if plies == 1:
            return (slot(gone[0], come[0]), -1) if old[gone[0]] == new[come[0]] else (-1, -1)
        if gone[0][0] == gone[1][0]:
            return -1, -1
        # player 0 picks from the lowest occupied interior row, player 1 from the highest: the mover's source is the one nearer its side
        gone.sort(key=lambda c: c[0] if mover == 0 else -c[0])

        def off(source, target, player):
            """how far the move is from an unbounced walk of `player`; None: backwards, or another value"""
            forward = target[0] - source[0] if player == 0 else source[0] - target[0]
            if forward < 0 or old[source] != new[target]:
                return None
            return abs(forward + abs(target[1] - source[1]) - int(old[source]))

        pairings = []
        for targets in (come, come[::-1]):
            offs = [off(gone[0], targets[0], mover), off(gone[1], targets[1], 1 - mover)]
            if None not in offs:
                pairings.append((sum(offs), targets))
        pairings.sort(key=lambda x: x[0])
        if not pairings or (len(pairings) == 2 and pairings[0][0] == pairings[1][0]):
            return -1, -1
        targets = pairings[0][1]
        return slot(gone[0], targets[0]), slot(gone[1], targets[1])

    def _launch(self, b: BounceBatch, **arguments):
        return (b.search_moves_proving if self.prove else b.search_moves)(edges=self.edges, **arguments)

    def _forest(self, b: BounceBatch):
        return b.search_moves_forest(self.capacity, self.edges)

    def _between(self, last, now, k: int):
        return self.moves_between(last[0][k], int(last[1][k]), now[0][k], int(now[2][k]) - int(last[2][k]))


class SolverAgent(_Agent):
    """Exact values of Connect positions (``simulator.game.connect.State``) and Bounce positions
    (``simulator.game.bounce.State``) by the batched alpha-beta solvers, dispatched on the state's type.

    ``predict(state)`` maps every action of ``state.actions`` to 1.0 (the mover can force a win after it), 0.5 (a draw
    with best play) or 0.0 (the opponent can force a win), within lines of at most ``depth`` plies (None: a full solve
    for Connect; for Bounce, whose games can cycle, the default horizon of ``BounceBatch.solve_moves``) and ``max_nodes``
    positions an action.  An action the horizon or the budget left open takes the value of ``fallback`` (e.g. a
    ``MonteCarloAgent``), or 0.5 without one.  ``choose(state)`` plays the fastest win, else the best of the draws and
    open actions, else the slowest loss.

    ``solve_many`` returns the solver's own arrays: ``[n, width]`` for Connect (indexed by column), ``[n, width, height *
    width]`` for Bounce (indexed by the source's column and the target cell ``ty * width + tx``).
    """

    def __init__(self, depth: Optional[int] = None, max_nodes: int = DEFAULT_SOLVE_NODES, fallback=None, device: int = 0):
        if depth is not None and depth < 1:
            raise ValueError("depth must be >= 1")
        if max_nodes < 1:
            raise ValueError("max_nodes must be >= 1")
        self.depth = None if depth is None else int(depth)
        self.max_nodes = int(max_nodes)
        self.fallback = fallback
        super().__init__(device)

    def solve_many(self, states: Sequence):
        """(codes, plies) of `states` (states of one game sharing one Config): int8 / int16 [n, width] for Connect,
        [n, width, height * width] for Bounce"""
        game = _game_of(states[0])
        b, _ = self._loaded(states, "SolverAgent:", game, shared=f"SolverAgent: {game.name} states that share one Config")
        if game is _Bounce:
            return b.solve_moves(depth=DEFAULT_BOUNCE_SOLVE_DEPTH if self.depth is None else self.depth, max_nodes=self.max_nodes)
        return b.solve_actions(depth=self.depth, max_nodes=self.max_nodes)

    def _values(self, states: Sequence, codes: np.ndarray) -> List[Dict]:
        """{action: value} of every state from its row of solver codes; the fallback (one call for all states) fills the
        actions the horizon or the budget left open"""
        open_ = (codes == SOLVE_UNKNOWN) | (codes == SOLVE_BUDGET)
        fill = None
        if self.fallback is not None and open_.any():
            fill = self.fallback.predict_many(list(states))
        exact = {SOLVE_WIN: 1.0, SOLVE_DRAW: 0.5, SOLVE_LOSS: 0.0}
        index = _game_of(states[0]).index
        out = []
        for k, s in enumerate(states):
            v = {}
            for a in s.actions:
                c = int(codes[(k,) + index(a)])
                v[a] = exact[c] if c in exact else (float(fill[k][a]) if fill is not None else 0.5)
            out.append(v)
        return out

    def predict_many(self, states: Sequence) -> List[Dict]:
        """`predict` of every state, solved in one call"""
        if not states:
            return []
        codes, _ = self.solve_many(states)
        return self._values(states, codes)

    def predict(self, state) -> Dict:
        """{action: value} for every action in ``state.actions``"""
        return self.predict_many([state])[0]

    def choose(self, state):
        """the fastest win, else the best-valued draw or open action, else the slowest loss"""
        codes, plies = self.solve_many([state])
        values = self._values([state], codes)[0]
        best, best_key = None, None
        for a in state.actions:
            at = (0,) + _game_of(state).index(a)
            c, p = int(codes[at]), int(plies[at])
            if c == SOLVE_WIN:
                key = (2, -p)
            elif c == SOLVE_LOSS:
                key = (0, p)
            else:
                key = (1, values[a])
            if best_key is None or key > best_key:
                best, best_key = a, key
        return best
