"""CPU-only checks of the exact Bounce solver's plumbing and of its CPU reference (tests/solve_reference_bounce.py):
bgs_bounce_solve_moves is in the header, in both libraries' dynamic symbol tables (csrc/bgs.map) and in _abi.py; the
reference gives the answers that can be read off hand-made boards, agrees with a plain recursive search over the
independent rules spec (tests/spec_rules.py), and a deeper horizon never changes a WIN / LOSS or its plies."""

import os
import subprocess

import numpy as np

from tests import game_trees as gt
from tests import kernel_units
from tests import solve_reference_bounce as ref
from tests import spec_rules as spec
from tests.conftest import PKG, PRODUCT_LIB, ROOT, TEST_LIB
from tests.test_spec_exhaustive import BOUNCE_CONFIGS

CSRC = os.path.join(PKG, "csrc")


def _exports(path):
    out = subprocess.check_output(["nm", "-D", "--defined-only", path], text=True)
    return {line.split()[-1] for line in out.splitlines() if line.strip()}


def test_symbol_in_header_map_and_binding():
    with open(os.path.join(ROOT, "include", "bgs.h")) as f:
        text = f.read()
    assert "BGS_API int bgs_bounce_solve_moves(bgs_batch* b, int32_t depth, int64_t max_nodes, int8_t* codes, int16_t* plies," in text
    assert "#define BGS_BOUNCE_SOLVE_MAX_DEPTH 16" in text
    for path in (PRODUCT_LIB, TEST_LIB):   # what bgs.map lets through
        assert "bgs_bounce_solve_moves" in _exports(path), path
    from simulator import batch
    from simulator.game import _abi

    assert "bgs_bounce_solve_moves" in _abi.SIGNATURES
    assert _abi.SIGNATURES["bgs_bounce_solve_moves"] == _abi.SIGNATURES["bgs_connect_solve_actions"]
    assert batch.BOUNCE_SOLVE_MAX_DEPTH == 16 and batch.DEFAULT_BOUNCE_SOLVE_DEPTH == 3
    kernel_units.check_six_distinct_ids()
    assert kernel_units.units_defining("k_bounce_solve") == ["solve"] and kernel_units.units_defining("bgs::bounce_solve(") == ["solve"]


def one_root(grid, player=0):
    g = np.array(grid, dtype=np.int8)[None]
    return g, np.array([player], dtype=np.int8), np.array([-1], dtype=np.int8), np.array([player], dtype=np.int32)


def legal_slots(codes):
    return {(int(x), int(c)) for x, c in zip(*np.nonzero(codes[0] != ref.NONE))}


# ---- boards whose answers can be read off (y = 0 is the bottom row; player 0 moves up, the piece in the occupied
# interior row nearest the bottom; a piece moves exactly its value, through empty interior cells)
def test_win_in_one():
    grid = [[0], [2], [0], [0]]           # the 2 at y = 1 goes y = 2, y = 3: player 0's goal row
    for depth in (1, 2, 5):
        codes, plies = ref.solve(grid, one_root(grid), depth)
        assert legal_slots(codes) == {(0, 3)}
        assert codes[0, 0, 3] == ref.WIN and plies[0, 0, 3] == 1


def test_loss_in_two_and_an_open_move():
    # player 0 owns the 1 at (0, 1): it may go up to (0, 2) or right to (1, 1).  Then player 1 moves the 3 at (1, 3) down:
    # after (0, 2) the column below it is free, three steps reach (1, 0), its goal row: a loss in 2.  After (1, 1) that
    # column is blocked at the second step, and a goal row three rows away needs three steps straight down: nothing is
    # forced within two plies.
    grid = [[0, 0], [1, 0], [0, 0], [0, 3], [0, 0]]
    w = 2
    up, right = 2 * w + 0, 1 * w + 1
    codes, plies = ref.solve(grid, one_root(grid), 1)
    assert legal_slots(codes) == {(0, up), (0, right)}
    assert codes[0, 0, up] == ref.UNKNOWN and codes[0, 0, right] == ref.UNKNOWN and not plies.any()
    codes, plies = ref.solve(grid, one_root(grid), 2)
    assert codes[0, 0, up] == ref.LOSS and plies[0, 0, up] == 2
    assert codes[0, 0, right] == ref.UNKNOWN and plies[0, 0, right] == 0


def test_stalemate_win_at_ply_one():
    # the 1 goes to y = 2.  Player 1's only piece row is y = 3: its 2 is blocked at the first step, no move.  Player 0
    # could still move (the 1 bounces on the 2: y = 4, then y = 5, its goal row), so the move wins at once.
    grid = [[0], [1], [0], [2], [0], [0]]
    for depth in (1, 3):
        codes, plies = ref.solve(grid, one_root(grid), depth)
        assert legal_slots(codes) == {(0, 2)}
        assert codes[0, 0, 2] == ref.WIN and plies[0, 0, 2] == 1


def test_draw_at_ply_one():
    # as above on a board one row shorter: the bounce's first step would be the goal row, so player 0 cannot move either
    grid = [[0], [1], [0], [2], [0]]
    for depth in (1, 4):
        codes, plies = ref.solve(grid, one_root(grid), depth)
        assert legal_slots(codes) == {(0, 2)}
        assert codes[0, 0, 2] == ref.DRAW and plies[0, 0, 2] == 1


def test_ended_roots_and_layout():
    grid = [[0], [2], [0], [0]]
    g, p, w, l = one_root(grid)
    roots = (np.concatenate([g, g]), np.array([0, 0], dtype=np.int8), np.array([1, -1], dtype=np.int8), np.array([0, 0], dtype=np.int32))
    codes, plies = ref.solve(grid, roots, 2)
    assert codes.shape == (2, 1, 4) and codes.dtype == np.int8 and plies.dtype == np.int16
    assert (codes[0] == ref.NONE).all() and (plies[0] == 0).all()
    assert codes[1, 0, 3] == ref.WIN


# ---- the reference against a plain recursion over the rules spec
def _search(rules, grid, player, depth):
    """(sign, dist) for the side to move, `depth` plies of horizon left"""
    if depth == 0:
        return 0, 0
    best = None
    for (sx, sy), (tx, ty) in rules.actions(grid, player, spec.RUNNING):
        sign, dist = _move_value(rules, grid, player, (sx, sy, tx, ty), depth)
        key = 1000 - dist if sign == 1 else (-1000 + dist if sign == -1 else 0)
        if best is None or key > best[0]:
            best = (key, sign, dist)
    return best[1], best[2]


def _move_value(rules, grid, player, move, depth):
    status, g, p, winner, _ = rules.step(grid, player, spec.RUNNING, 0, move)
    assert status == spec.OK
    if winner == player:
        return 1, 1
    if winner != spec.RUNNING:
        return 0, 0
    s, t = _search(rules, g, p, depth - 1)
    return -s, (t + 1 if s else 0)


def test_reference_against_plain_recursion():
    checked = 0
    for name, max_depth in (("three_next_to_goal", None), ("small", 3)):
        cfg = np.array(BOUNCE_CONFIGS[name], dtype=np.int8)
        rules = spec.Bounce(BOUNCE_CONFIGS[name])
        layers = [layer for _, layer, _ in gt.bounce_layers(cfg, max_depth=max_depth)]
        pos = tuple(np.concatenate([l[j] for l in layers]) for j in range(4))
        pos = gt._take(pos, np.arange(0, pos[0].shape[0], 7))
        h, w = cfg.shape
        for depth in (1, 2, 3, 4):
            codes, plies = ref.solve(cfg, pos, depth)
            for i in range(pos[0].shape[0]):
                if pos[2][i] != -1:
                    assert (codes[i] == ref.NONE).all()
                    continue
                g, p = pos[0][i].tolist(), int(pos[1][i])
                acts = rules.actions(g, p, spec.RUNNING)
                assert int((codes[i] != ref.NONE).sum()) == len(acts)
                for (sx, sy), (tx, ty) in acts:
                    sign, dist = _move_value(rules, g, p, (sx, sy, tx, ty), depth)
                    status, _, _, winner, _ = rules.step(g, p, spec.RUNNING, 0, (sx, sy, tx, ty))
                    want = (ref.WIN, dist) if sign == 1 else (ref.LOSS, dist) if sign == -1 else \
                        (ref.DRAW, 1) if winner == 2 else (ref.UNKNOWN, 0)
                    assert (int(codes[i, sx, ty * w + tx]), int(plies[i, sx, ty * w + tx])) == want, (name, depth, g, p)
                    checked += 1
    assert checked > 2000


def test_a_deeper_horizon_keeps_every_win_and_loss():
    for name, max_depth in (("three_next_to_goal", None), ("small", 4)):
        cfg = np.array(BOUNCE_CONFIGS[name], dtype=np.int8)
        layers = [layer for _, layer, _ in gt.bounce_layers(cfg, max_depth=max_depth)]
        pos = tuple(np.concatenate([l[j] for l in layers]) for j in range(4))
        prev = None
        seen = set()
        for depth in (1, 2, 3, 4, 5, 6):
            codes, plies = ref.solve(cfg, pos, depth)
            if prev is not None:
                decided = np.isin(prev[0], [ref.WIN, ref.LOSS])
                np.testing.assert_array_equal(codes[decided], prev[0][decided])
                np.testing.assert_array_equal(plies[decided], prev[1][decided])
                np.testing.assert_array_equal(codes == ref.NONE, prev[0] == ref.NONE)
                np.testing.assert_array_equal(codes == ref.DRAW, prev[0] == ref.DRAW)
            assert (plies[np.isin(codes, [ref.WIN, ref.LOSS])] <= depth).all()
            seen |= set(np.unique(codes).tolist())
            prev = (codes, plies)
        assert {ref.WIN, ref.LOSS, ref.UNKNOWN, ref.NONE} <= seen
