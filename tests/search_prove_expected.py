"""The CPU statement of bgs_connect_search_actions_proving (include/bgs.h), built on tests/search_expected.py -- its Node,
its selection arithmetic, its oracle steps and playouts, its root builders -- and the case table of
tests/test_gpu_search_prove.py.  No GPU import; not a test module.

On top of the plain search's tree every edge has a tag, seen from the player to move at its node: OPEN, WIN, DRAW or
LOSS.  The selection runs over the legal columns whose tag is OPEN; an edge that ends the game is tagged when it is
played; after such an iteration the tags go up the path while the node at hand has a value (step 7); a root whose value
is not OPEN runs no further iteration.  The playouts of iteration t of all roots go through one oracle batch, as in
search_expected, under the game ids of the T that was asked for."""

import functools
from collections import namedtuple

import numpy as np

from oracle import oracle
from tests import fuzz_cases as fc
from tests import game_trees as gt
from tests import search_expected as se
from tests.search_expected import Node, _legal, _play, _step, count_nodes, select

OPEN, WIN, DRAW, LOSS = 0, 1, 2, 3
# the solver's codes (include/bgs.h): what `proved` holds
SOLVE_NONE, SOLVE_LOSS, SOLVE_DRAW, SOLVE_WIN, SOLVE_UNKNOWN, SOLVE_BUDGET = -2, -1, 0, 1, 2, 3
CODE = {OPEN: SOLVE_UNKNOWN, WIN: SOLVE_WIN, DRAW: SOLVE_DRAW, LOSS: SOLVE_LOSS}
NEGATED = {WIN: LOSS, LOSS: WIN, DRAW: DRAW}
TALLIES = ("selections", "tied_selections", "terminal_leaves", "capped_leaves", "max_depth", "best_ties", "tags_set", "tags_backed_up",
           "deepest_backup", "excluded_top", "stopped_early", "decided_win", "decided_draw", "decided_loss")

View = namedtuple("View", "legal n s")      # what search_expected.select reads of a node


class ProvingNode(Node):
    def __init__(self, position, legal):
        super().__init__(position, legal)
        self.tag = [OPEN] * len(legal)


def value(node):
    tags = [node.tag[c] for c in node.legal]
    for what in (WIN, OPEN, DRAW):
        if what in tags:
            return what
    return LOSS


def select_open(node, explore, seen):
    """search_expected.select over the legal columns whose tag is OPEN; counts the selections in which the plain rule,
    over all legal columns, would have taken a tagged column"""
    candidates = [c for c in node.legal if node.tag[c] == OPEN]
    assert candidates, "the descent stands on a node without an OPEN column"
    col = select(View(candidates, node.n, node.s), explore, seen)
    if len(candidates) < len(node.legal) and all(node.n[c] for c in candidates):
        aside = dict.fromkeys(("selections", "tied_selections"), 0)
        seen["excluded_top"] += int(node.tag[select(View(node.legal, node.n, node.s), explore, aside)] != OPEN)
    return col


def search_trees(h, w, k, roots, seed, first_game, iterations, leaf_playouts, explore, max_plies, per_ply, policy="uniform"):
    """(trees, counts int64[n, w, 3], done int64[n], env-steps, seen): search_expected.search_trees with the tags"""
    assert iterations >= 1 and leaf_playouts >= 1 and iterations * leaf_playouts <= se.MAX_PLAYOUTS and 0 <= explore <= se.MAX_EXPLORE
    grid, player, winner, plies = roots
    n = grid.shape[0]
    T, P = iterations, leaf_playouts
    trees = []
    for i in range(n):
        if winner[i] != -1:
            trees.append(None)
            continue
        position = (grid[i].copy(), int(player[i]), int(plies[i]))
        trees.append(ProvingNode(position, _legal(h, w, k, position)))
    counts = np.zeros((n, w, 3), dtype=np.int64)
    done = np.array([0 if tree is None else T for tree in trees], dtype=np.int64)
    over = [tree is None for tree in trees]
    steps = 0
    seen = dict.fromkeys(TALLIES, 0)
    seen["capped"] = np.zeros((n, w), dtype=np.int64)
    for t in range(T):
        paths, leaves, ids, owner, outcome, tagged = {}, [], [], [], {}, set()
        for i in range(n):
            if over[i]:
                continue
            if value(trees[i]) != OPEN:                     # step 0
                over[i], done[i] = True, t
                seen["stopped_early"] += 1
                continue
            node, path = trees[i], []
            while True:
                c = select_open(node, explore, seen)
                path.append((node, c))
                if c not in node.edge:
                    node.edge[c] = _step(h, w, k, node.position, c)
                won, after = node.edge[c]
                if won != -1:                               # the edge ends the game: a fact
                    seen["terminal_leaves"] += 1
                    outcome[i] = [won] * P
                    assert node.tag[c] == OPEN and won in (2, node.position[1])
                    node.tag[c] = DRAW if won == 2 else WIN
                    seen["tags_set"] += 1
                    tagged.add(i)
                    break
                if node.n[c] == 0:
                    node.child[c] = ProvingNode(after, _legal(h, w, k, after))
                    if after[2] >= max_plies:               # capped at once: not an end, no tag
                        seen["capped_leaves"] += 1
                        outcome[i] = [-1] * P
                    else:
                        for j in range(P):
                            leaves.append(after)
                            ids.append((((first_game + i) * T + t) * P + j) & se.MASK64)
                            owner.append(i)
                    break
                node = node.child[c]
            paths[i] = path
            seen["max_depth"] = max(seen["max_depth"], len(path))
        if leaves:
            won, played = _play(h, w, k, leaves, ids, seed, max_plies, per_ply, policy)
            steps += played
            for i, x in zip(owner, won.tolist()):
                outcome.setdefault(i, []).append(x)
        for i, path in paths.items():
            result = np.array(outcome[i])
            assert result.size == P
            mover = int(player[i])
            tally = {who: int((result == who).sum()) for who in (0, 1, 2)}
            counts[i, path[0][1]] += (tally[mover], tally[2], tally[1 - mover])
            seen["capped"][i, path[0][1]] += int((result == -1).sum())
            for node, c in path:
                node.n[c] += P
                node.s[c] += 2 * tally[node.position[1]] + tally[2]
            if i in tagged:                                 # step 7
                levels = 0
                for k_ in range(len(path) - 1, -1, -1):
                    what = value(path[k_][0])
                    if what == OPEN:
                        break
                    if k_ == 0:
                        seen[{WIN: "decided_win", DRAW: "decided_draw", LOSS: "decided_loss"}[what]] += 1
                        break
                    above, c = path[k_ - 1]
                    assert above.tag[c] == OPEN
                    above.tag[c] = NEGATED[what]
                    levels += 1
                seen["tags_backed_up"] += levels
                seen["deepest_backup"] = max(seen["deepest_backup"], levels)
    return trees, counts, done, steps, seen


def _outputs(w, trees, counts, done, steps, seen):
    n = len(trees)
    seen = dict(seen)
    visits = np.zeros((n, w), dtype=np.int64)
    best = np.full(n, -1, dtype=np.int64)
    nodes = np.zeros(n, dtype=np.int64)
    proved = np.full((n, w), SOLVE_NONE, dtype=np.int8)
    for i, root in enumerate(trees):
        if root is None:
            continue
        visits[i] = root.n
        nodes[i] = count_nodes(root)
        for c in root.legal:
            proved[i, c] = CODE[root.tag[c]]
        won = [c for c in root.legal if root.tag[c] == WIN]
        assert len(won) <= 1
        among = [c for c in root.legal if root.tag[c] != LOSS] or root.legal
        ranked = sorted(among, key=lambda c: (-root.n[c], -root.s[c], c))
        best[i] = won[0] if won else ranked[0]
        seen["best_ties"] += int(not won and len(ranked) > 1 and root.n[ranked[0]] == root.n[ranked[1]])
    return (counts.astype(np.int32), visits.astype(np.int32), best.astype(np.int32), nodes.astype(np.int32), proved,
            done.astype(np.int32), steps, seen)


def search_expected(h, w, k, roots, seed, first_game, iterations, leaf_playouts, explore, max_plies, per_ply, policy="uniform"):
    """(counts int32[n, w, 3], visits int32[n, w], best int32[n], nodes int32[n], proved int8[n, w], done int32[n],
    env-steps, seen).  seen: search_expected's tallies and "capped", and "tags_set" (step 4), "tags_backed_up" (step 7),
    "deepest_backup" (the most tags one step 7 wrote: the levels a fact went up), "excluded_top" (selections in which a
    tagged column had the top U of the plain rule), "stopped_early" (roots with done < T), "decided_win" / "decided_draw"
    / "decided_loss" (roots whose value step 7 found)"""
    return _outputs(w, *search_trees(h, w, k, roots, seed, first_game, iterations, leaf_playouts, explore, max_plies, per_ply, policy))


# ---- hand-made roots
def _after(h, w, k, columns):
    orc = oracle.ConnectOracle(h, w, k, 1)
    for c in columns:
        assert orc.step_actions(np.int32([c]))[0] == 0 and (orc.winner[0] == -1)
    return orc.grid.copy(), orc.player.copy(), orc.winner.copy(), orc.plies.copy()


@functools.lru_cache(maxsize=None)
def hand_roots_3x5x3():
    """3 x 5, three in a row: the start; a win in one (the mover holds b1 c1 with a1 and d1 empty); a position where
    every column loses in two (the opponent holds b1 c1 with both ends empty, the mover one stone on b2: whatever it
    plays, the other end wins); the positions one and two plies before those; and the last five positions of random
    games"""
    lines = ([], [1, 1, 2, 2], [1, 1, 2], [1, 1], [1, 2, 2])
    ends = gt.end_games(3, 5, 3, 12, 77003, last=5)
    ends = fc.take(ends, np.arange(min(ends[0].shape[0], 12)))
    return fc.concat([_after(3, 5, 3, line) for line in lines] + [ends])


@functools.lru_cache(maxsize=None)
def hand_roots_2x2x3():
    """2 x 2, three in a row (a corner board of tests/fuzz_cases.py): no line fits, so the last empty cells force a
    draw from every position"""
    return fc.concat([_after(2, 2, 3, line) for line in ([], [0], [0, 0], [0, 1], [0, 1, 1], [1, 1, 0])])


@functools.lru_cache(maxsize=None)
def hand_roots_1x1x1():
    """1 x 1, one in a row (a corner board of tests/fuzz_cases.py): the first move wins"""
    return _after(1, 1, 1, [])


@functools.lru_cache(maxsize=None)
def end_game_roots_6x7x4():
    """6 x 7 x 4 end-games: the positions 4 to 12 plies before the end of random games, up to 24 of them, running and
    with at most 12 empty cells -- the roots the CPU solver is asked about"""
    layer = gt.end_games(6, 7, 4, 24, 77001, last=10)
    empty = (layer[0] < 0).sum(axis=(1, 2))
    rows = np.flatnonzero((layer[2] == -1) & (empty <= 12) & (empty >= 5))
    rows = rows[np.unique(np.linspace(0, rows.size - 1, 20).round().astype(np.int64))]
    return fc.take(layer, rows)


@functools.lru_cache(maxsize=None)
def spread_roots_12x13x5():
    """12 x 13 x 5, three words: every third root of tests/search_expected.py's mix, eight running boards -- four in the
    opening (2, 4, 5 and 18 stones: three of them inside a 4-ply block) and four a few plies before the board is full"""
    mixed = se._case_roots(12, 13, 5)
    return fc.take(mixed, np.arange(1, mixed[0].shape[0], 3))


# ---- the cases of the GPU comparison: cases of tests/search_expected.py on its root mix, and the hand-made roots
Case = namedtuple("Case", "name h w k iterations playouts explore cap first_game roots")
BASE = (9, 8, 0, 1, 2, 10, 11)      # of search_expected.CASES: 2x5x3, 5x6x3, 6x7x4 (48 x 16, 200 x 1, 12 x 70 capped), 6x12x4, 12x13x5
CASES = tuple(Case(se.case_id(c), c.h, c.w, c.k, c.iterations, c.playouts, c.explore, c.cap, c.first_game, functools.partial(se.case_roots, c))
              for c in (se.CASES[j] for j in BASE)) + (
    Case("hand-3x5x3-T40-P4", 3, 5, 3, 40, 4, 65536, None, 3, hand_roots_3x5x3),
    Case("hand-2x2x3-T24-P2", 2, 2, 3, 24, 2, 65536, None, 0, hand_roots_2x2x3),
    Case("hand-1x1x1-T4-P3", 1, 1, 1, 4, 3, 65536, None, 0, hand_roots_1x1x1),
    Case("ends-6x7x4-T96-P4", 6, 7, 4, 96, 4, 65536, None, 11, end_game_roots_6x7x4),
    Case("spread-12x13x5-T16-P8-capped", 12, 13, 5, 16, 8, 65536, 12, 3, spread_roots_12x13x5),   # the cap cuts the opening roots' games
)
DECISIVE = (1, 2)                   # the cases that run under the decisive policy too: 5x6x3 and 6x7x4 48 x 16
PER_PLY = (1,)                      # ... under the per-ply RNG contract too
PER_PLY_BOTH = (11,)                # ... under the per-ply contract in both policies: the three-word spread
RUNS = ([(j, "uniform", False) for j in range(len(CASES))] + [(j, "decisive", False) for j in DECISIVE]
        + [(j, "uniform", True) for j in PER_PLY] + [(j, policy, True) for j in PER_PLY_BOTH for policy in ("uniform", "decisive")])
SOLVED_EMPTY = 12                   # roots with at most this many empty cells are checked against the exact solvers


def run_id(run):
    j, policy, per_ply = run
    return f"{CASES[j].name}-{policy}" + ("-per-ply" if per_ply else "")


def case_roots(case):
    roots = case.roots()
    assert roots[0].shape[0] <= 24
    return roots


def case_max_plies(case, roots=None):
    if case.cap is None:
        return se.UNCAPPED
    roots = case_roots(case) if roots is None else roots
    return int(np.median(roots[3][roots[2] == -1])) + case.cap


@functools.lru_cache(maxsize=None)
def case_trees(index, per_ply=False, policy="uniform"):
    """search_trees of CASES[index], computed once a session and shared: treat everything as read-only"""
    case = CASES[index]
    roots = case_roots(case)
    return search_trees(case.h, case.w, case.k, roots, se.SEED, case.first_game, case.iterations, case.playouts, case.explore,
                        case_max_plies(case, roots), per_ply, policy)


@functools.lru_cache(maxsize=None)
def case_expected(index, per_ply=False, policy="uniform"):
    """search_expected of CASES[index], from case_trees: treat the arrays as read-only"""
    return _outputs(CASES[index].w, *case_trees(index, per_ply, policy))


@functools.lru_cache(maxsize=None)
def plain_expected(index, per_ply=False, policy="uniform"):
    """tests/search_expected.py's answer for the same run: the base cases share its cache"""
    case = CASES[index]
    if index < len(BASE):
        return se.case_expected(BASE[index], per_ply, policy)
    roots = case_roots(case)
    return se.search_expected(case.h, case.w, case.k, roots, se.SEED, case.first_game, case.iterations, case.playouts, case.explore,
                              case_max_plies(case, roots), per_ply, policy)


# ---- the fuzz sweep of tests/test_gpu_search_prove.py: random geometries and root sets from the generators of
# tests/fuzz_cases.py; BGS_FUZZ_CASES widens it
FUZZ_CASES = 8
FUZZ_BASE = 47000
FuzzCase = namedtuple("FuzzCase", "key h w k roots iterations playouts explore max_plies first_game per_ply policy")


def fuzz_keys():
    return list(range(max(FUZZ_CASES, fc.EXTRA)))


@functools.lru_cache(maxsize=None)
def fuzz_case(key):
    rng = np.random.default_rng(FUZZ_BASE + key)
    (h, w, k), = fc.random_connect_geometries(rng, 1)
    mixed = fc.connect_roots(h, w, k, rng)
    roots = fc.take(mixed, np.arange(min(mixed[0].shape[0], 16)))
    running = roots[2] == -1
    T, P = int(rng.integers(8, 41)), int(rng.choice([1, 3, 8]))
    cap = se.UNCAPPED if rng.random() < 0.7 or not running.any() else int(np.median(roots[3][running])) + int(rng.integers(1, 8))
    return FuzzCase(key, h, w, k, roots, T, P, int(rng.choice([0, 20000, 65536])), cap, int(rng.integers(0, 1 << 40)),
                    bool(rng.integers(0, 2)), str(rng.choice(["uniform", "decisive"])))


def fuzz_expected(case):
    return search_expected(case.h, case.w, case.k, case.roots, se.SEED, case.first_game, case.iterations, case.playouts,
                           case.explore, case.max_plies, case.per_ply, case.policy)
