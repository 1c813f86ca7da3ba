"""The oracle against an independent rules spec (tests/spec_rules.py) on EVERY reachable position of small games (CPU).

tests/game_trees.py walks each game tree layer by layer, one copy of every position.  At every position the oracle and
the spec must agree on the move list (Connect: legal columns; Bounce: the target set of every piece, in the order
`state.actions` uses) and, for every move, legal or not, on the status and the child (grid, player, winner, plies,
reward).  The position counts are constants: a change of the rules fails here instead of quietly shrinking the walk.

Walks (positions, and moves checked = every position times the columns or moves tried):
  Connect, full trees: 2x3 k2 45, 3x3 k3 694, 3x4 k3 7 157, 4x3 k3 2 715, 4x4 k3 41 750, 4x4 k4 161 029;
          5x4 k4 to depth 11 (110 361 of its 1 706 255 positions).  Columns tried: -1, every column, W and W + 5.
  Bounce, full graphs: narrow 2, blocked_start 1 (settled at reset), three_next_to_goal 1 476;
          small to depth 8 (39 486 of its 151 120 positions).  Moves tried: every legal move, the skip, and illegal ones.
"""

import json
import os

import numpy as np
import pytest

from oracle import oracle
from tests import game_trees as gt
from tests import spec_rules as spec

CONNECT_WALKS = {
    # (h, w, k): (max depth or None for the whole tree, positions per layer)
    (2, 3, 2): (None, [1, 3, 9, 21, 8, 3]),
    (3, 3, 3): (None, [1, 3, 9, 24, 57, 108, 150, 176, 114, 52]),
    (3, 4, 3): (None, None),
    (4, 3, 3): (None, None),
    (4, 4, 3): (None, None),
    (4, 4, 4): (None, None),
    (5, 4, 4): (11, None),
}
CONNECT_TOTALS = {(2, 3, 2): 45, (3, 3, 3): 694, (3, 4, 3): 7157, (4, 3, 3): 2715, (4, 4, 3): 41750, (4, 4, 4): 161029,
                  (5, 4, 4): 110361}

BOUNCE_CONFIGS = {
    "narrow": [[0], [1], [0], [2], [0]],
    "blocked_start": [[0, 0], [2, 2], [2, 2], [0, 0]],
    "small": [[0, 0, 0], [1, 2, 3], [0, 0, 0], [0, 0, 0], [1, 2, 3], [0, 0, 0]],
    # a value-3 piece right below player 0's goal row, a value-1 piece alone on player 0's side
    "three_next_to_goal": [[0, 0, 0], [0, 1, 0], [0, 0, 0], [3, 0, 2], [0, 0, 0]],
}
BOUNCE_WALKS = {"narrow": (None, 2), "blocked_start": (None, 1), "small": (8, 39486), "three_next_to_goal": (None, 1476)}


def as_lists(grid):
    return grid.tolist()


# ------------------------------------------------------------------------------------------------ golden fixtures


def test_spec_reproduces_the_reference_connect_game(golden_dir):
    with open(os.path.join(golden_dir, "reference_connect.json")) as fh:
        fx = json.load(fh)
    for game in fx["games"]:
        rules = spec.Connect(*game["config"])
        grid, player, winner, plies = rules.initial()
        for pos in game["positions"]:
            assert grid == pos["grid"]
            if pos["column"] is None:
                assert winner != spec.RUNNING and rules.legal(grid, winner) == []
                continue
            assert winner == spec.RUNNING and player == pos["player"] and pos["column"] in rules.legal(grid, winner)
            status, grid, player, winner, plies = rules.step(grid, player, winner, plies, pos["column"])
            assert status == spec.OK
        assert spec.reward(winner) == game["reward"]
    js = fx["json"]
    rules = spec.Connect(*js["config_args"])
    grid, player, winner, plies = rules.initial()
    for col in js["state_after_columns"]:
        _, grid, player, winner, plies = rules.step(grid, player, winner, plies, col)
    assert (grid, player, winner) == (js["state"]["grid"], js["state"]["player"], js["state"]["winner"])
    assert js["action_column"] in rules.legal(grid, winner)


def test_spec_reproduces_the_reference_bounce_games(golden_dir):
    with open(os.path.join(golden_dir, "reference_bounce.json")) as fh:
        fx = json.load(fh)
    checked = 0
    for test in fx["tests"]:
        rules = spec.Bounce(test["positions"][0]["grid"])
        grid, player, winner, plies = rules.initial()
        for pos in test["positions"]:
            checked += 1
            assert grid == pos["grid"] and player == pos["player"] and winner == spec.RUNNING, test["name"]
            sx, sy = pos["source"]
            want = [tuple(t) for t in pos["targets"]]
            assert rules.targets(grid, player, winner, sx, sy) == set(want), (test["name"], pos["source"])
            assert [dst for src, dst in rules.actions(grid, player, winner) if src == (sx, sy)] == want
            status, grid, player, winner, plies = rules.step(grid, player, winner, plies, (sx, sy, *pos["chosen"]))
            assert status == spec.OK
        assert (winner != spec.RUNNING) == test["final"]["has_ended"], test["name"]
        assert len(rules.actions(grid, player, winner)) == test["final"]["n_actions"]
        assert spec.reward(winner) == test["final"]["reward"], test["name"]
    assert checked == 15
    js = fx["json"]
    rules = spec.Bounce(js["config"]["grid"])
    grid, player, winner, _ = rules.initial()
    assert (grid, player, winner) == (js["state"]["grid"], js["state"]["player"], js["state"]["winner"])
    assert (tuple(js["action"]["source"]), tuple(js["action"]["target"])) in rules.actions(grid, player, winner)


# ------------------------------------------------------------------------------------------------ Connect


@pytest.mark.parametrize("geom", list(CONNECT_WALKS), ids=lambda g: "x".join(map(str, g)))
def test_connect_every_position_and_move(geom):
    h, w, k = geom
    max_depth, per_layer = CONNECT_WALKS[geom]
    rules = spec.Connect(h, w, k)
    columns = [-1] + list(range(w)) + [w, w + 5]
    counts = []
    for depth, layer in gt.connect_layers(h, w, k, max_depth=max_depth):
        grid, player, winner, plies = layer
        n = grid.shape[0]
        counts.append(n)
        assert (plies == depth).all()
        legal = oracle.ConnectOracle(h, w, k, n)
        legal.grid[:], legal.winner[:] = grid, winner
        orc_legal = legal.legal()
        status, kids = gt.connect_children(h, w, k, layer, columns)
        kid_reward = oracle.reward(kids[2])
        m = len(columns)
        for i in range(n):
            g, p, wi = as_lists(grid[i]), int(player[i]), int(winner[i])
            where = f"{geom} depth {depth} board {g} player {p} winner {wi}"
            assert np.flatnonzero(orc_legal[i]).tolist() == rules.legal(g, wi), where
            for j, col in enumerate(columns):
                st, cg, cp, cw, cl = rules.step(g, p, wi, depth, col)
                r = i * m + j
                got = (int(status[r]), as_lists(kids[0][r]), int(kids[1][r]), int(kids[2][r]), int(kids[3][r]), kid_reward[r].tolist())
                assert got == (st, cg, cp, cw, cl, spec.reward(cw)), f"{where} column {col}"
    total = sum(counts)
    print(f"Connect {h}x{w} k={k}: {total} positions in {len(counts)} layers, {total * len(columns)} moves")
    assert total == CONNECT_TOTALS[geom]
    if per_layer is not None:
        assert counts == per_layer
    if max_depth is None:
        # the whole tree: its last layer holds only finished games, draws included where the board can fill
        assert len(counts) <= h * w + 1


def test_connect_full_board_outcomes_are_reached():
    """the walk reaches what random play from the start seldom does: a board-filling win next to a full-board draw"""
    h, w, k = 4, 4, 3
    last = None
    for depth, layer in gt.connect_layers(h, w, k):
        last = (depth, layer)
    depth, (grid, player, winner, plies) = last
    assert depth == h * w
    assert set(np.unique(winner).tolist()) >= {1, 2}   # the 16th stone is player 1's: wins by it, and draws


# ------------------------------------------------------------------------------------------------ Bounce


def bounce_probe_moves(rules, grid, player, winner):
    """every legal move, the skip, and illegal ones: a non-piece source, an off-board target, the origin itself, a target
    of the wrong piece, the far goal row"""
    legal = rules.actions(grid, player, winner)
    moves = [(sx, sy, tx, ty) for (sx, sy), (tx, ty) in legal]
    moves.append((-1, 0, 0, 0))
    row = rules.active_row(grid, player)
    row = 1 if row is None else row
    moves += [(0, 0, 0, 1), (0, row, rules.w, row), (0, row, 0, row), (rules.w - 1, row, 0, rules.h - 1), (0, row, 0, 0),
              (rules.w, row, 0, row), (0, row, -1, row)]
    if legal:
        (sx, sy), (tx, ty) = legal[0]
        for (ox, oy), _ in legal:
            if (ox, oy) != (sx, sy):
                moves.append((ox, oy, tx, ty) if (tx, ty) not in rules.targets(grid, player, winner, ox, oy) else (ox, oy, -1, -1))
                break
    return moves


@pytest.mark.parametrize("name", list(BOUNCE_CONFIGS))
def test_bounce_every_position_and_move(name):
    cfg = np.array(BOUNCE_CONFIGS[name], dtype=np.int8)
    max_depth, want_total = BOUNCE_WALKS[name]
    rules = spec.Bounce(BOUNCE_CONFIGS[name])
    g0, p0, w0, l0 = rules.initial()
    start = oracle.BounceOracle(cfg, 1)
    assert (as_lists(start.grid[0]), int(start.player[0]), int(start.winner[0]), int(start.plies[0])) == (g0, p0, w0, l0)
    total = moves_checked = 0
    for depth, layer, acts in gt.bounce_layers(cfg, max_depth=max_depth):
        grid, player, winner, plies = layer
        n = grid.shape[0]
        total += n
        probes = []
        for i in range(n):
            g, p, wi = as_lists(grid[i]), int(player[i]), int(winner[i])
            where = f"{name} depth {depth} board {g} player {p} winner {wi}"
            assert acts[i] == rules.actions(g, p, wi), where
            row = rules.active_row(g, p)
            if row is not None:
                probe = oracle.BounceOracle(cfg, 1)
                probe.grid[0], probe.player[0], probe.winner[0] = grid[i], player[i], winner[i]
                for x in range(rules.w):
                    assert probe.targets(0, x, row) == rules.targets(g, p, wi, x, row), f"{where} piece {x}"
            probes += [(i, m) for m in bounce_probe_moves(rules, g, p, wi)]
        status, kids = gt.bounce_children(cfg, layer, probes)
        kid_reward = oracle.reward(kids[2])
        for r, (i, move) in enumerate(probes):
            st, cg, cp, cw, cl = rules.step(as_lists(grid[i]), int(player[i]), int(winner[i]), int(plies[i]), move)
            got = (int(status[r]), as_lists(kids[0][r]), int(kids[1][r]), int(kids[2][r]), int(kids[3][r]), kid_reward[r].tolist())
            assert got == (st, cg, cp, cw, cl, spec.reward(cw)), f"{name} depth {depth} board {grid[i].tolist()} move {move}"
        moves_checked += len(probes)
    print(f"Bounce {name}: {total} positions, {moves_checked} moves")
    assert total == want_total
