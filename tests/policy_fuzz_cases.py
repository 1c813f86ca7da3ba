"""The case table of the policy, halving and tree-search sweeps (tests/test_gpu_fuzz_policy.py) and of the CPU test that
states what the table must hold (tests/test_policy_fuzz_cases.py): the corner geometries and random cases of
tests/fuzz_cases.py once more, this time through the launches that play the decisive policy, halve or search --
evaluate_actions / evaluate_moves with policy="decisive", evaluate_actions_halving / evaluate_moves_halving,
search_actions / search_moves, their proving variants and the forest's restart.  No GPU import, no file I/O; not a test
module.

A key is an int (random case `key` of tests/fuzz_cases.py: its geometry or start grid and its root mix) or a str (an entry
of fuzz_cases.CONNECT_CORNERS / BOUNCE_CORNERS, always run).  The geometry and the roots come from fuzz_cases' cached
cases; everything this table adds -- the RNG contract, first_game, the cap, playouts, budgets and search shapes -- is
drawn from numpy.random.default_rng(CONNECT_BASE or BOUNCE_BASE + key), bases of this table's own: no draw of
tests/fuzz_cases.py changes, and building a key twice gives identical arrays.  BGS_FUZZ_CASES=N widens the random keys
to 0 .. N - 1 as it does there.

Where the fuzz keys of these launches live:
* here: Connect keys 0..15 and the 16 corners (evaluate_actions decisive, halving, search_actions, the forest restart;
  search_actions_proving on the corners only); Bounce keys 0..11 and the 6 corners (evaluate_moves decisive, halving;
  search_moves and search_moves_proving on the corners only);
* tests/search_prove_expected.py (fuzz_keys, fuzz_case): 8 random Connect keys of search_actions_proving, base 47000;
* tests/test_gpu_search_bounce.py (FUZZ_KEYS, _fuzz_arguments): random Bounce keys 0..7 of search_moves, which
  tests/test_gpu_search_bounce_prove.py runs through search_moves_proving too;
* tests/fuzz_cases.py: the uniform evaluation and the exact solvers, 24 + 16 random keys and the corners.

Connect roots.  A spread (fuzz_cases._spread) of the key's roots -- the start, positions a few plies in, positions one
to three plies before the end of random games, ended boards, never more than the running ones -- and, on the corners, the
last min(w + 1, 8) positions of the tiled game, whose columns fill up one by one: roots with w, ..., 2, 1 legal columns.
At most EVAL_ROOTS roots for the evaluation and the halving, SEARCH_ROOTS for the searches, WIDE_SEARCH_ROOTS for the
decisive searches on three words (the CPU model's cost: about 26 us a decisive playout ply).  One corner of exactly 192
bits ("15x12x4", LADDER) halves on the last w positions of the tiled game instead: twelve roots with 12, 11, ..., 1 legal
columns, the only way to hold every column count of a three-word board in twelve roots.  Its mid-game roots are halved
under the wide budget below.

Wide halving budgets (WIDE): for one corner each of NW = 1, 2, 3 a second budget with budget // rounds(w) > 512 on two
roots -- the 256-lane team of the halving kernel; every other budget here stays with the wave team.

Bounce roots: the first 4 of the key's eval_rows.  Both caps of the case; the halving budgets are min_budget(A) and 4 * A
for the largest arm count A among the roots (with more than 16 arms 4 * A is below A * R(A): that root is SHORT)."""

import functools
from collections import namedtuple

import numpy as np

from tests import bounce_halving_expected as bh
from tests import bounce_policy_expected as bp
from tests import fuzz_cases as fc
from tests import game_trees as gt
from tests import halving_expected as he
from tests import policy_expected as pe
from tests import search_bounce_expected as sb
from tests import search_bounce_prove_expected as sbp
from tests import search_expected as se
from tests import search_prove_expected as sp

CONNECT_CASES = 16      # random keys (the corner table comes on top)
BOUNCE_CASES = 12
CONNECT_BASE = 61000    # default_rng(base + key); corners: base + 500 000 + their index
BOUNCE_BASE = 65000
SEED = fc.EVAL_SEED
UNCAPPED = fc.UNCAPPED
POLICIES = ("uniform", "decisive")
EVAL_ROOTS, SEARCH_ROOTS, WIDE_SEARCH_ROOTS, TILED_ROOTS = 12, 8, 4, 8
CONNECT_PLAYOUTS, CORNER_PLAYOUTS = (1, 3, 8), 4
BOUNCE_PLAYOUTS = (1, 3, 6)
LADDER = ("15x12x4",)
# corner -> the budget of the 256-lane team: budget // rounds(w) > 512
WIDE = {"3x13x4": 2100, "12x8x4": 1600, "15x12x4": 2100}
# (T, P) of the Bounce searches, by the key's index: those of the fuzz of tests/test_gpu_search_bounce.py
BOUNCE_SHAPES = ((32, 8), (64, 4), (16, 16), (256, 1), (5, 51))

ConnectKey = namedtuple("ConnectKey", "key h w k nw roots halving_roots search_roots per_ply first_game max_plies playouts budget "
                                      "iterations leaf_playouts explore wide")
BounceKey = namedtuple("BounceKey", "key grid roots playouts max_plies first_game budgets iterations leaf_playouts explore min_pool")


def connect_keys():
    return list(range(max(CONNECT_CASES, fc.EXTRA))) + list(fc.CONNECT_CORNERS)


def connect_corner_keys():
    return list(fc.CONNECT_CORNERS)


def bounce_keys():
    return list(range(max(BOUNCE_CASES, fc.EXTRA))) + list(fc.BOUNCE_CORNERS)


def bounce_corner_keys():
    return list(fc.BOUNCE_CORNERS)


def _rng(key, base, corners):
    return np.random.default_rng(base + (500_000 + list(corners).index(key) if isinstance(key, str) else key))


def _thin(layer, count):
    """at most `count` rows of `layer`: a spread of its running rows and, of count // 6 ended ones, no more than those"""
    run, end = np.flatnonzero(layer[2] == -1), np.flatnonzero(layer[2] != -1)
    ended = min(end.size, count // 6)
    run = run[fc._spread(run.size, count - ended)]
    return fc.take(layer, np.concatenate([run, end[: min(ended, run.size)]]))


def _distinct(layer):
    """the distinct boards of `layer`, in its order"""
    return fc.take(layer, np.sort(gt._unique_rows(layer[0])))


# ---- Connect
@functools.lru_cache(maxsize=None)
def connect_key(key):
    case = fc.connect_case(key)
    h, w, k = case.h, case.w, case.k
    rng = _rng(key, CONNECT_BASE, fc.CONNECT_CORNERS)
    corner = isinstance(key, str)
    if corner:
        tiled = fc.tiled_game(h, w, k, last=min(w + 1, TILED_ROOTS))
        roots = _distinct(fc.concat([_thin(case.roots, EVAL_ROOTS - tiled[0].shape[0]), tiled]))
    else:
        roots = _thin(case.roots, EVAL_ROOTS)
    halving_roots = fc.tiled_game(h, w, k, last=w) if key in LADDER else roots
    search_roots = _thin(roots, SEARCH_ROOTS)
    running = roots[2] == -1
    per_ply = bool(rng.integers(0, 2))
    first_game = int(rng.integers(0, 1 << 40))
    cap = UNCAPPED if rng.random() < 0.5 else int(np.median(roots[3][running])) + int(rng.integers(1, 8))
    playouts = CORNER_PLAYOUTS if corner else int(rng.choice(CONNECT_PLAYOUTS))
    least = he.min_budget(w)
    budget = int(rng.choice([least, 2 * least + 1, 5 * least]))
    T, P = int(rng.integers(8, 41)), int(rng.choice([1, 3, 8]))
    explore = int(rng.choice([0, 20000, 65536]))
    wide = None
    if key in WIDE:
        # a late root with every column open, and the root with the fewest (but two or more) open columns
        legal = he.legal_columns(h, w, k, roots).sum(axis=1)
        every = np.flatnonzero(legal == w)
        few = np.flatnonzero(legal >= 2)
        rows = [int(every[np.argmax(roots[3][every])]), int(few[np.argmin(legal[few])])]
        assert rows[0] != rows[1] and WIDE[key] // he.rounds(w) > 512
        wide = (WIDE[key], fc.take(roots, rows))
    return ConnectKey(key, h, w, k, case.nw, roots, halving_roots, search_roots, per_ply, first_game, cap, playouts, budget, T, P,
                      explore, wide)


def connect_search_roots(case, policy):
    """the roots of the key's searches: fewer under the decisive policy on three words"""
    if policy == "decisive" and case.nw == 3:
        return _thin(case.search_roots, WIDE_SEARCH_ROOTS)
    return case.search_roots


@functools.lru_cache(maxsize=None)
def connect_eval_expected(key):
    """(counts, env-steps, {class: plies}) of evaluate_actions(policy="decisive") on case.roots: treat as read-only"""
    c = connect_key(key)
    return pe.connect_policy_expected(c.h, c.w, c.k, c.roots, SEED, c.first_game, c.playouts, c.max_plies, c.per_ply)


@functools.lru_cache(maxsize=None)
def connect_halving_expected(key, policy, wide=False):
    """(counts, given, best, env-steps, seen) of evaluate_actions_halving on case.halving_roots (wide: on case.wide)"""
    c = connect_key(key)
    budget, roots = c.wide if wide else (c.budget, c.halving_roots)
    return he.halving_expected(c.h, c.w, c.k, roots, SEED, c.first_game, budget, c.max_plies, c.per_ply, policy)


def _search_arguments(c, policy):
    return (c.h, c.w, c.k, connect_search_roots(c, policy), SEED, c.first_game, c.iterations, c.leaf_playouts, c.explore, c.max_plies,
            c.per_ply, policy)


@functools.lru_cache(maxsize=None)
def connect_search_expected(key, policy):
    """(counts, visits, best, nodes, env-steps, seen) of search_actions on connect_search_roots"""
    return se.search_expected(*_search_arguments(connect_key(key), policy))


@functools.lru_cache(maxsize=None)
def connect_prove_expected(key, policy):
    """(counts, visits, best, nodes, proved, done, env-steps, seen) of search_actions_proving on connect_search_roots"""
    return sp.search_expected(*_search_arguments(connect_key(key), policy))


# ---- Bounce
@functools.lru_cache(maxsize=None)
def bounce_key(key):
    case = fc.bounce_case(key)
    rng = _rng(key, BOUNCE_BASE, fc.BOUNCE_CORNERS)
    index = list(fc.BOUNCE_CORNERS).index(key) if isinstance(key, str) else key
    roots = fc.take(case.roots, case.eval_rows[:4])
    playouts = int(rng.choice(BOUNCE_PLAYOUTS))
    first_game = int(rng.integers(0, 1 << 40))
    arms = max([len(a) for a in bp.root_actions(case.grid, roots)] + [1])
    T, P = BOUNCE_SHAPES[index % len(BOUNCE_SHAPES)]
    return BounceKey(key, case.grid, roots, playouts, (int(case.max_plies[0]), fc.LONG), first_game, (bh.min_budget(arms), 4 * arms),
                     T, P, sb.DEFAULT_EXPLORE, index % 2 == 0)


def bounce_edges(case):
    h, w = case.grid.shape
    return sb.min_edges(h, w) if case.min_pool else sb.default_edges(h, w, case.iterations)


@functools.lru_cache(maxsize=None)
def bounce_eval_expected(key, cap):
    """(counts, env-steps, {class: plies}) of evaluate_moves(policy="decisive") under case.max_plies[cap]"""
    c = bounce_key(key)
    return bp.bounce_policy_expected(c.grid, c.roots, SEED, c.first_game, c.playouts, c.max_plies[cap])


@functools.lru_cache(maxsize=None)
def bounce_halving_expected(key, j, policy):
    """(counts, given, best, env-steps, seen) of evaluate_moves_halving with case.budgets[j] under case.max_plies[j]"""
    c = bounce_key(key)
    return bh.bounce_halving_expected(c.grid, c.roots, SEED, c.first_game, c.budgets[j], c.max_plies[j], policy)


def bounce_search_cap(case):
    """the short cap on the even corners, the long one on the odd ones"""
    return case.max_plies[0] if list(fc.BOUNCE_CORNERS).index(case.key) % 2 == 0 else min(case.max_plies[1], sb.LONG)


def _bounce_search_arguments(c, policy):
    return (c.grid, c.roots, SEED, c.first_game, c.iterations, c.leaf_playouts, c.explore, bounce_search_cap(c), policy, bounce_edges(c))


@functools.lru_cache(maxsize=None)
def bounce_search_expected(key, policy):
    """(counts, visits, best, nodes, used, env-steps, seen) of search_moves on a corner key"""
    return sb.search_bounce_expected(*_bounce_search_arguments(bounce_key(key), policy))


@functools.lru_cache(maxsize=None)
def bounce_prove_expected(key, policy):
    """(counts, visits, best, nodes, used, proved, done, env-steps, seen) of search_moves_proving on a corner key"""
    return sbp.search_bounce_prove_expected(*_bounce_search_arguments(bounce_key(key), policy))


def describe(case):
    if isinstance(case, ConnectKey):
        return (f"connect key {case.key!r} {case.h}x{case.w}x{case.k} (NW={case.nw}) per_ply {case.per_ply} first_game {case.first_game} "
                f"max_plies {case.max_plies}")
    return f"bounce key {case.key!r} grid {case.grid.tolist()} first_game {case.first_game}"
