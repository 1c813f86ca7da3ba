"""The case table of the differential fuzz (tests/test_gpu_fuzz.py) and of the CPU test that states what the table must
hold (tests/test_fuzz_cases.py): random geometries and start grids, and per case the root positions, solver depths,
playouts, ply caps, first-game offsets and the RNG contract.  Everything is drawn from
numpy.random.default_rng(fixed base + case) and from the oracle under seeds drawn from that generator: building a case
twice gives identical arrays.  No GPU import, no file I/O; not a test module.

A case key is an int (a random case) or a str (an entry of the corner table, always run).

Roots are in the reference layout (grid int8[n, H, W], player int8[n], winner int8[n], plies int32[n]) and mix, per
case: the start position; positions a few plies in; positions one to three plies before the end of random games; the
last positions of a scripted game that tiles the board in runs of two (Connect: it fills the whole board without a line
of three, so its end holds the few-empty-cells draws that random games on large boards never reach); ended boards, never
more than the running ones.  Duplicates are dropped.

Solver depths (sized by the CPU references, which walk the oracle from Python):
* Connect: 1-4 on every root; 5 and the full solve (depth = H * W) on the roots with at most 10 empty cells (`late`).
* Bounce: 1-3 on every root; 4 where the reference expanded fewer than BOUNCE_DEEP_NODES positions at depth 3 (with
  the branching of these grids that keeps depth 4 under about 10^4 positions; `bounce_depths` asks the reference).
"""

import functools
import os
from collections import namedtuple

import numpy as np

from oracle import oracle
from tests import game_trees as gt
from tests import mc_expected as mc

# BGS_FUZZ_CASES=N widens every sweep of test_gpu_fuzz.py
EXTRA = int(os.environ.get("BGS_FUZZ_CASES", "0"))
CONNECT_CASES = 24      # random cases of the evaluate / solve sweeps (the corner tables come on top)
BOUNCE_CASES = 16
CONNECT_BASE = 21000    # default_rng(base + case)
BOUNCE_BASE = 25000
EVAL_BOARDS = 200_000   # boards the oracle replicates comfortably for one expected-counts call
BOUNCE_DEEP_NODES = 1500
UNCAPPED = 2**31 - 1
EVAL_SEED = 0x5EED0F0E7A1A7E00
LONG = 4096             # Bounce: "uncapped" for the oracle, every position here ends well before

# playouts around the evaluation kernel's per-wave counts (kEvalGamesOneWord = 512, kEvalGamesWide = 256): one, a few,
# one below / equal / one above, and a value that gives three slices
CONNECT_PLAYOUTS = {1: (1, 7, 511, 512, 513, 1100), 2: (1, 7, 255, 256, 257, 600), 3: (1, 7, 255, 256, 257, 600)}
BOUNCE_PLAYOUTS = (1, 3, 16, 64, 300)


# ---- the geometry generators (shared with the step / rollout fuzz: the draws are pinned by its seeds)
def random_connect_geometries(rng, count):
    out = []
    while len(out) < count:
        h, w = int(rng.integers(1, 16)), int(rng.integers(1, 17))
        if w * (h + 1) > 192:
            continue
        out.append((h, w, int(rng.integers(1, 8))))
    return out


def random_bounce_grid(rng):
    while True:
        h, w = int(rng.integers(3, 12)), int(rng.integers(1, 13))
        if h * w <= 64:
            break
    grid = np.zeros((h, w), dtype=np.int8)
    density = rng.uniform(0.05, 0.7)
    max_value = int(rng.choice([1, 2, 3, 3, 3, 5, 9, 15]))
    for y in range(1, h - 1):
        for x in range(w):
            if rng.random() < density:
                grid[y, x] = int(rng.integers(1, max_value + 1))
    return grid


def random_piece_list_grid(rng):
    """A start grid the piece-list kernel takes: at most 8 columns and 16 pieces (values 1..15, a few cells each)."""
    while True:
        h, w = int(rng.integers(3, 12)), int(rng.integers(1, 9))
        if h * w <= 64:
            break
    grid = np.zeros((h, w), dtype=np.int8)
    cells = [(y, x) for y in range(1, h - 1) for x in range(w)]
    pieces = int(rng.integers(1, min(16, len(cells)) + 1))
    max_value = int(rng.choice([1, 2, 3, 3, 3, 4, 6, 15]))
    for k in rng.choice(len(cells), size=pieces, replace=False):
        y, x = cells[int(k)]
        grid[y, x] = int(rng.integers(1, max_value + 1))
    return grid


# ---- the corner tables: geometries that are always run.  name -> (h, w, k, playouts)
CONNECT_CORNERS = {
    "1x1x1": (1, 1, 1, (1, 513)),             # one cell, the first move wins
    "1x16x2": (1, 16, 2, (511, 513)),         # one row, the widest board: `next` = 16, colmask of one bit
    "15x1x4": (15, 1, 4, (7, 1100)),          # one column: fewer segments than a wave holds, half = 0
    "15x12x4": (15, 12, 4, (256,)),           # 192 bits, the tallest columns, k == 4 on three words
    "11x16x5": (11, 16, 5, (255, 257)),       # 192 bits, the widest: cell indices up to 190
    "3x13x4": (3, 13, 4, (512,)),             # k == 4 with the vertical direction impossible
    "2x7x4": (2, 7, 4, (64,)),                # k == 4 with only the horizontal direction possible
    "6x7x7": (6, 7, 7, (300,)),               # k = 7: one line a row and nothing else
    "8x8x6": (8, 8, 6, (257,)),               # two words (72 bits), general k
    "10x7x6": (10, 7, 6, (600,)),             # two words (77 bits), general k
    "5x5x6": (5, 5, 6, (1100,)),              # k above both sides: no line can ever win
    "9x9x2": (9, 9, 2, (16,)),                # k = 2 on 81 cells, two words
    "12x8x4": (12, 8, 4, (64,)),              # k == 4 on two words (104 bits)
    "9x16x3": (9, 16, 3, (7,)),               # k = 3 on three words (160 bits), w = 16
    "2x2x3": (2, 2, 3, (7,)),                 # w = 2 where no line fits: every game is a draw
    "15x4x7": (15, 4, 7, (16,)),              # 64 bits exactly in one word, shifts of up to 6 * 17 bits
}


def _grid(rows):
    return np.array(rows, dtype=np.int8)


def _bounce_8x8():
    g = np.zeros((8, 8), dtype=np.int8)
    g[1] = [1, 0, 2, 0, 0, 3, 0, 6]    # the 6 walks straight down column 7 into cell 63
    g[6] = [0, 2, 0, 1, 0, 0, 3, 0]
    return g


def _bounce_16x4():
    g = np.zeros((16, 4), dtype=np.int8)
    g[1] = [1, 2, 3, 14]               # the 14 walks straight down column 3 into cell 63
    g[5] = [2, 0, 1, 0]
    g[10] = [0, 3, 1, 0]
    g[14] = [2, 1, 3, 0]
    return g


def _bounce_4x16():
    g = np.zeros((4, 16), dtype=np.int8)
    g[1] = [1, 15, 0, 2, 9, 0, 3, 1, 0, 15, 2, 0, 4, 1, 0, 2]
    g[2] = [2, 0, 15, 1, 0, 3, 0, 7, 1, 0, 0, 15, 1, 0, 3, 1]
    return g


def _bounce_5x12():
    g = np.zeros((5, 12), dtype=np.int8)
    g[1] = [15, 1, 0, 15, 2, 0, 1, 15, 0, 3, 1, 15]
    g[2] = [0, 15, 1, 0, 0, 2, 0, 0, 15, 0, 0, 1]
    g[3] = [1, 0, 15, 2, 15, 0, 3, 1, 0, 15, 2, 0]
    return g


def _bounce_default():
    g = np.zeros((9, 6), dtype=np.int8)
    g[1] = g[7] = [1, 2, 3, 3, 2, 1]
    return g


BOUNCE_CORNERS = {
    "8x8": _bounce_8x8,                                              # 64 cells, a piece that reaches cell 63
    "16x4": _bounce_16x4,                                            # 64 cells, 16 rows, cell 63 again
    "4x16": _bounce_4x16,                                            # 64 cells, 16 columns, values 15
    "5x12": _bounce_5x12,                                            # 12 columns, values 15
    "7x1": lambda: _grid([[0], [2], [0], [1], [0], [3], [0]]),       # one column
    "default": _bounce_default,                                      # the 9x6 default board
}

ConnectCase = namedtuple("ConnectCase", "key h w k nw roots late depths playouts max_plies first_game per_ply eval_rows")
BounceCase = namedtuple("BounceCase", "key grid nc roots playouts max_plies first_game eval_rows")


def concat(layers):
    return tuple(np.concatenate([l[j] for l in layers]) for j in range(4))


def _snap(orc, idx=None):
    layer = (orc.grid.copy(), orc.player.copy(), orc.winner.copy(), orc.plies.copy())
    return layer if idx is None else gt._take(layer, idx)


def _mix(parts, unique, running_cap, ended_cap):
    """the distinct positions of `parts`: up to running_cap running ones, then ended ones -- never more than the running"""
    layer = concat(parts)
    layer = gt._take(layer, unique(layer))
    run = np.flatnonzero(layer[2] == -1)[:running_cap]
    end = np.flatnonzero(layer[2] != -1)[: min(ended_cap, run.size)]
    return gt._take(layer, np.concatenate([run, end]))


def _spread(n, count):
    """`count` of n row indices, evenly spread (all of them when count >= n)"""
    return np.unique(np.linspace(0, n - 1, max(1, min(n, count))).round().astype(np.int64))


# ---- Connect
def tiled_game(h, w, k, last=4):
    """the last `last` running positions of the scripted game in which cell (x, y) goes to player (x // 2 + y) % 2:
    runs of two in every direction.  The columns are taken greedily, lowest first; the game stops where it ends or where
    no column offers the mover one of its cells."""
    orc = oracle.ConnectOracle(h, w, k, 1)
    height = [0] * w
    hist = []
    for ply in range(h * w):
        col = next((x for x in sorted(range(w), key=lambda x: height[x]) if height[x] < h and (x // 2 + height[x]) % 2 == ply % 2), None)
        if col is None:
            break
        hist = (hist + [_snap(orc)])[-last:]
        orc.step_actions(np.int32([col]))
        height[col] += 1
        if orc.winner[0] != -1:
            break
    return concat(hist)


def connect_roots(h, w, k, rng):
    seed = int(rng.integers(0, 1 << 62))
    parts = [_snap(oracle.ConnectOracle(h, w, k, 1))]
    n = 8
    orc = oracle.ConnectOracle(h, w, k, n)
    target = rng.integers(1, 7, n)
    for ply in range(1, 7):                       # a few plies in (ended already on the smallest boards)
        orc.step_random(seed)
        parts.append(_snap(orc, np.flatnonzero(target == ply)))
    parts.append(tiled_game(h, w, k))
    parts.append(gt.end_games(h, w, k, 16, seed + 1, last=3))
    orc = oracle.ConnectOracle(h, w, k, 6)
    orc.rollout(seed + 2)
    parts.append(_snap(orc))
    # (the reference's cost grows with width ** depth: fewer roots on the wide boards)
    return _mix(parts, lambda l: gt._unique_rows(l[0]), max(12, min(36, 288 // w)), 6)


def connect_keys():
    return list(range(max(CONNECT_CASES, EXTRA))) + list(CONNECT_CORNERS)


@functools.lru_cache(maxsize=None)
def connect_case(key):
    if isinstance(key, str):
        h, w, k, playouts = CONNECT_CORNERS[key]
        rng = np.random.default_rng(CONNECT_BASE + 500_000 + list(CONNECT_CORNERS).index(key))
    else:
        rng = np.random.default_rng(CONNECT_BASE + key)
        (h, w, k), = random_connect_geometries(rng, 1)
        playouts = None
    nw = (w * (h + 1) + 63) // 64
    roots = connect_roots(h, w, k, rng)
    if playouts is None:
        playouts = (int(rng.choice(CONNECT_PLAYOUTS[nw])),)
    running = roots[2] == -1
    empty = (roots[0] < 0).sum(axis=(1, 2))
    late = np.flatnonzero(running & (empty <= 10))
    depths = (1, 2, 3, 4)
    first_game = int(rng.integers(0, 1 << 40))
    per_ply = bool(rng.integers(0, 2))
    # a cap in the middle of the roots' ply counts: the later roots start at or beyond it, the earlier ones are cut short
    cap = UNCAPPED if rng.random() < 0.5 else int(np.median(roots[3][running])) + int(rng.integers(1, 8))
    eval_rows = tuple(_spread(roots[0].shape[0], EVAL_BOARDS // (w * p)) for p in playouts)
    return ConnectCase(key, h, w, k, nw, roots, late, depths, playouts, cap, first_game, per_ply, eval_rows)


def connect_solves(case):
    """[(depth, rows of case.roots)]: depths 1-4 on every root, 5 and the full solve on the late ones"""
    every = np.arange(case.roots[0].shape[0])
    out = [(d, every) for d in case.depths]
    if case.late.size:
        out += [(5, case.late), (case.h * case.w, case.late)]
    return out


# ---- Bounce
def bounce_end_games(grid, n, seed, last=3, max_plies=300):
    """the positions `last`, ..., 1 plies before the end of n oracle games played from the start (the games still running
    after max_plies give none)"""
    orc = oracle.BounceOracle(grid, n)
    hist, picked = [], [gt._take(_snap(orc), np.zeros(0, dtype=np.int64))]
    for _ in range(max_plies):
        if orc.ended.all():
            break
        hist = (hist + [_snap(orc)])[-last:]
        before = orc.ended.copy()
        orc.step_random(seed)
        done = np.flatnonzero(orc.ended & ~before)
        for snap in hist:
            picked.append(gt._take(snap, done))
    layer = concat(picked)
    return gt._take(layer, np.flatnonzero(layer[2] == -1))


def bounce_roots(grid, rng):
    seed = int(rng.integers(0, 1 << 62))
    parts = [_snap(oracle.BounceOracle(grid, 1))]
    n = 8
    orc = oracle.BounceOracle(grid, n)
    target = rng.integers(1, 6, n)
    for ply in range(1, 6):
        orc.step_random(seed)
        parts.append(_snap(orc, np.flatnonzero(target == ply)))
    parts.append(bounce_end_games(grid, 8, seed + 1))
    orc = oracle.BounceOracle(grid, 4)
    orc.rollout(seed + 2, max_plies=LONG)
    parts.append(_snap(orc))
    return _mix(parts, lambda l: gt._unique_rows(l[0], l[1]), 16, 4)


def bounce_keys():
    return list(range(max(BOUNCE_CASES, EXTRA))) + list(BOUNCE_CORNERS)


def _start_runs(grid):
    return oracle.BounceOracle(grid, 1).winner[0] == -1


@functools.lru_cache(maxsize=None)
def bounce_case(key):
    if isinstance(key, str):
        grid = BOUNCE_CORNERS[key]()
        rng = np.random.default_rng(BOUNCE_BASE + 500_000 + list(BOUNCE_CORNERS).index(key))
    else:
        rng = np.random.default_rng(BOUNCE_BASE + key)
        grid = random_bounce_grid(rng)
        while not _start_runs(grid):      # (an empty or blocked start grid has no running root at all: draw again)
            grid = random_bounce_grid(rng)
    h, w = grid.shape
    assert h * w <= 64 and grid.max() <= 15
    roots = bounce_roots(grid, rng)
    playouts = int(rng.choice(BOUNCE_PLAYOUTS))
    first_game = int(rng.integers(0, 1 << 40))
    cap = int(np.median(roots[3])) + int(rng.integers(1, 40))
    eval_rows = _spread(roots[0].shape[0], 8)
    return BounceCase(key, grid, 1 if w <= 8 else 3, roots, playouts, (cap, LONG), first_game, eval_rows)


@functools.lru_cache(maxsize=None)
def bounce_reference(key, depth):
    """(codes, plies, positions expanded) of tests/solve_reference_bounce.solve on the case's roots"""
    from tests import solve_reference_bounce as ref

    case = bounce_case(key)
    stats = {}
    codes, plies = ref.solve(case.grid, case.roots, depth, stats=stats)
    return codes, plies, stats.get("nodes", 0)


def bounce_depths(key):
    return (1, 2, 3) + ((4,) if bounce_reference(key, 3)[2] < BOUNCE_DEEP_NODES else ())


def take(layer, idx):
    return gt._take(layer, np.asarray(idx, dtype=np.int64))


def connect_eval_expected(case, j):
    """(roots, counts, env-steps) of the case's j-th playout count from the oracle"""
    roots = take(case.roots, case.eval_rows[j])
    counts, steps = mc.connect_expected(case.h, case.w, case.k, roots, EVAL_SEED, case.first_game, case.playouts[j], case.max_plies,
                                        case.per_ply)
    return roots, counts, steps


def bounce_eval_expected(case, max_plies):
    """(roots, counts, env-steps) from the oracle: one replicated batch where it is small, slot by slot where it is not"""
    roots = take(case.roots, case.eval_rows)
    h, w = case.grid.shape
    small = w * h * w * case.playouts * roots[0].shape[0] <= EVAL_BOARDS
    counts, steps = (mc.expected if small else mc.expected_by_slot)(case.grid, roots, EVAL_SEED, case.first_game, case.playouts, max_plies)
    return roots, counts, steps


def describe(case):
    if isinstance(case, ConnectCase):
        return f"connect case {case.key!r} {case.h}x{case.w}x{case.k} (NW={case.nw}, {case.roots[0].shape[0]} roots)"
    return f"bounce case {case.key!r} grid {case.grid.tolist()} ({case.roots[0].shape[0]} roots)"
