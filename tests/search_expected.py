"""The CPU statement of bgs_connect_search_actions (include/bgs.h), built on the oracle's public API alone, and the case
table of tests/test_gpu_search.py.  No GPU import; not a test module.

A Python tree per root: a node holds n[c], s[c] and child[c] for every column, and (the model's convenience; the kernel
rebuilds it) its position.  Iteration t of every running root descends by the rule of the header -- the lowest legal
column with n = 0, else the largest U(c) = Q(c) + E(c), ties to the lowest column -- until an edge ends the game or
reaches a position without a node.  The playouts of iteration t of ALL roots then go through one ConnectOracle batch,
in the lock step of tests/policy_expected.py: every ply takes the candidate list (policy_expected.candidates; the legal
columns under the uniform policy), picks the index with oracle.connect_sample_index (oracle.sample_index under the
per-ply contract) under the playout's own game id G = ((first_game + i) * T + t) * P + j and calls orc.step_actions.
Env-steps are the oracle's ply counts past the leaf's."""

import functools
import math
from collections import namedtuple

import numpy as np

from oracle import oracle
from tests import fuzz_cases as fc
from tests.policy_expected import candidates

UNCAPPED = 2**31 - 1
SEED = 0x5EED0F0E7A1A7E00
MASK64 = 2**64 - 1
MAX_EXPLORE = 1 << 18
MAX_PLAYOUTS = 1 << 29          # T * P
DEFAULT_EXPLORE = 65536


def lg(total):
    """256 * e + ((256 * N) >> e) - 256, e = floor(log2 N): a piecewise-linear log2 in Q8"""
    e = int(total).bit_length() - 1
    return 256 * e + ((int(total) << 8) >> e) - 256


def isqrt(x):
    return math.isqrt(x)


def q_term(s, n):
    return (s * 2048) // n


def e_term(explore, total, n):
    return isqrt((explore * lg(total)) // n)


class Node:
    def __init__(self, position, legal):
        w = len(legal)
        self.position = position            # (grid int8[h, w], player, plies) of a running board
        self.legal = [c for c in range(w) if legal[c]]
        self.n, self.s, self.child = [0] * w, [0] * w, [None] * w
        self.edge = {}                      # c -> (winner after c, position after c), filled when the edge is first played


def select(node, explore, seen):
    """the column iteration takes at `node`"""
    fresh = [c for c in node.legal if node.n[c] == 0]
    if fresh:
        return fresh[0]
    total = sum(node.n[c] for c in node.legal)
    u = [q_term(node.s[c], node.n[c]) + e_term(explore, total, node.n[c]) for c in node.legal]
    top = max(u)
    seen["selections"] += 1
    if explore == 0 and "greedy" in seen:
        seen["greedy"].append(([q_term(node.s[c], node.n[c]) for c in node.legal], list(node.legal), node.legal[u.index(top)]))
    seen["tied_selections"] += int(u.count(top) > 1)
    return node.legal[u.index(top)]         # (index: the first, so the lowest column)


def _step(h, w, k, position, col):
    """(winner, position) after `col` on `position`, by the oracle"""
    grid, player, plies = position
    orc = oracle.ConnectOracle(h, w, k, 1)
    orc.grid[0], orc.player[0], orc.winner[0], orc.plies[0] = grid, player, -1, plies
    assert orc.step_actions(np.int32([col]))[0] == 0
    return int(orc.winner[0]), (orc.grid[0].copy(), int(orc.player[0]), int(orc.plies[0]))


def _legal(h, w, k, position):
    grid, player, plies = position
    orc = oracle.ConnectOracle(h, w, k, 1)
    orc.grid[0], orc.player[0], orc.winner[0], orc.plies[0] = grid, player, -1, plies
    return orc.legal()[0].astype(bool)


def _play(h, w, k, leaves, ids, seed, max_plies, per_ply, policy):
    """(winner int8[len(leaves)], env-steps): the running position leaves[j] played on as game ids[j]"""
    orc = oracle.ConnectOracle(h, w, k, len(leaves), per_ply=per_ply)
    for j, (grid, player, plies) in enumerate(leaves):
        orc.grid[j], orc.player[j], orc.winner[j], orc.plies[j] = grid, player, -1, plies
    start = orc.plies.astype(np.int64).copy()
    sample = oracle.sample_index if per_ply else oracle.connect_sample_index
    while True:
        live = np.flatnonzero((orc.winner == -1) & (orc.plies < max_plies))
        if live.size == 0:
            break
        # (the uniform policy's candidate list is the legal columns: candidates(orc, live, True)[0] without its win tests)
        chosen = orc.legal()[live].astype(bool) if policy == "uniform" else candidates(orc, live)[0]
        size = chosen.sum(axis=1)
        idx = np.array([sample(seed, ids[r], int(p), int(s)) for r, p, s in zip(live, orc.plies[live], size)])
        move = np.full(orc.n, -1, dtype=np.int32)
        move[live] = (np.cumsum(chosen, axis=1) > idx[:, None]).argmax(axis=1)   # the idx-th candidate, ascending
        assert (orc.step_actions(move)[live] == 0).all()
    return orc.winner.copy(), int((orc.plies.astype(np.int64) - start).sum())


def search_trees(h, w, k, roots, seed, first_game, iterations, leaf_playouts, explore, max_plies, per_ply, policy="uniform"):
    """(trees, counts int64[n, w, 3], env-steps, seen): trees[i] is the root Node of board i, None for an ended board.
    seen["capped"] int64[n, w]: the playouts through every root column that the cap left unfinished (at once or in
    mid-game); seen["greedy"]: with explore = 0, the UCB selections as (Q of the legal columns, the column taken)"""
    assert iterations >= 1 and leaf_playouts >= 1 and iterations * leaf_playouts <= MAX_PLAYOUTS and 0 <= explore <= MAX_EXPLORE
    grid, player, winner, plies = roots
    n = grid.shape[0]
    T, P = iterations, leaf_playouts
    trees = []
    for i in range(n):
        if winner[i] != -1:
            trees.append(None)
            continue
        position = (grid[i].copy(), int(player[i]), int(plies[i]))
        trees.append(Node(position, _legal(h, w, k, position)))
    counts = np.zeros((n, w, 3), dtype=np.int64)
    steps = 0
    seen = dict.fromkeys(("selections", "tied_selections", "terminal_leaves", "capped_leaves", "max_depth", "best_ties"), 0)
    seen["capped"] = np.zeros((n, w), dtype=np.int64)
    seen["greedy"] = []
    for t in range(T):
        paths, leaves, ids, owner, outcome = {}, [], [], [], {}
        for i in range(n):
            if trees[i] is None:
                continue
            node, path = trees[i], []
            while True:
                c = select(node, explore, seen)
                path.append((node, c))
                if c not in node.edge:
                    node.edge[c] = _step(h, w, k, node.position, c)
                won, after = node.edge[c]
                if won != -1:                               # the edge ends the game: P playouts with that outcome
                    seen["terminal_leaves"] += 1
                    outcome[i] = [won] * P
                    break
                if node.n[c] == 0:                          # a new node for the position after c
                    node.child[c] = Node(after, _legal(h, w, k, after))
                    if after[2] >= max_plies:               # capped at once: no game, every playout scores 0
                        seen["capped_leaves"] += 1
                        outcome[i] = [-1] * P
                    else:
                        for j in range(P):
                            leaves.append(after)
                            ids.append((((first_game + i) * T + t) * P + j) & MASK64)
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
    return trees, counts, steps, seen


def count_nodes(root):
    total, stack = 0, [root]
    while stack:
        node = stack.pop()
        for child in node.child:
            if child is not None:
                total += 1
                stack.append(child)
    return total


def _outputs(w, trees, counts, steps, seen):
    n = len(trees)
    seen = dict(seen)
    visits = np.zeros((n, w), dtype=np.int64)
    best = np.full(n, -1, dtype=np.int64)
    nodes = np.zeros(n, dtype=np.int64)
    for i, root in enumerate(trees):
        if root is None:
            continue
        visits[i] = root.n
        ranked = sorted(root.legal, key=lambda c: (-root.n[c], -root.s[c], c))
        best[i] = ranked[0]
        seen["best_ties"] += int(len(ranked) > 1 and root.n[ranked[0]] == root.n[ranked[1]])
        nodes[i] = count_nodes(root)
    return counts.astype(np.int32), visits.astype(np.int32), best.astype(np.int32), nodes.astype(np.int32), steps, seen


def search_expected(h, w, k, roots, seed, first_game, iterations, leaf_playouts, explore, max_plies, per_ply, policy="uniform"):
    """(counts int32[n, w, 3], visits int32[n, w], best int32[n], nodes int32[n], env-steps, seen).  seen counts the UCB
    "selections", the "tied_selections" (the top two U equal, so the column order decided), the "terminal_leaves", the
    "capped_leaves", the "max_depth" of a path in edges and the "best_ties" (two root columns with the most visits); "capped" int64[n, w] and
    "greedy" are search_trees' own"""
    return _outputs(w, *search_trees(h, w, k, roots, seed, first_game, iterations, leaf_playouts, explore, max_plies, per_ply, policy))


# ---- the cases of the GPU comparison.  Roots: a spread of fuzz_cases.connect_roots (the start, positions a few plies in,
# positions one to three plies before the end of random games, ended boards) and the last positions of its tiled game,
# whose columns fill up one by one: roots with W, ..., 3, 2, 1 legal columns and trees that run out of leaves.  At most 24
# roots a case.  cap: None, or plies past the median ply count of the running roots.
Case = namedtuple("Case", "h w k iterations playouts explore cap first_game")
CASES = (
    Case(6, 7, 4, 48, 16, 65536, None, 5),
    Case(6, 7, 4, 200, 1, 65536, None, 0),         # classic UCT: many U ties, deep paths
    Case(6, 7, 4, 12, 70, 65536, 3, 1 << 33),      # P above a wave: the refill path; game ids beyond 32 bits; capped
    Case(6, 7, 4, 7, 8, 65536, None, 0),           # T = columns: expansion only
    Case(6, 7, 4, 8, 8, 65536, None, 0),           # the first UCB choice
    Case(6, 7, 4, 1, 64, 65536, None, 0),          # a single iteration
    Case(6, 7, 4, 40, 8, 0, None, 0),              # pure exploitation
    Case(6, 7, 4, 40, 8, 262144, None, 0),         # the ceiling of `explore`
    Case(5, 6, 3, 64, 8, 65536, None, 0),          # count 3, short games: terminal edges near the root
    Case(2, 5, 3, 40, 4, 65536, None, 0),          # the general bit search; trees exhausted
    Case(6, 12, 4, 24, 16, 65536, None, 0),        # two words
    Case(12, 13, 5, 16, 8, 65536, None, 0),        # three words
)
DECISIVE = (0, 1, 2, 11)                           # the cases that run under the decisive policy too
PER_PLY = (0, 8)                                   # ... under the per-ply RNG contract too
RUNS = ([(j, "uniform", False) for j in range(len(CASES))] + [(j, "decisive", False) for j in DECISIVE]
        + [(j, "uniform", True) for j in PER_PLY])
RUNNING_ROOTS, ENDED_ROOTS, TILED_ROOTS = 14, 2, 8


def case_id(case):
    text = f"{case.h}x{case.w}x{case.k}-T{case.iterations}-P{case.playouts}"
    if case.explore != DEFAULT_EXPLORE:
        text += f"-e{case.explore}"
    return text + ("-capped" if case.cap is not None else "")


def run_id(run):
    j, policy, per_ply = run
    return f"{case_id(CASES[j])}-{policy}" + ("-per-ply" if per_ply else "")


@functools.lru_cache(maxsize=None)
def _case_roots(h, w, k):
    rng = np.random.default_rng(43000 + 100 * h + w + 7 * k)
    mixed = fc.connect_roots(h, w, k, rng)
    running, ended = np.flatnonzero(mixed[2] == -1), np.flatnonzero(mixed[2] != -1)
    tiled = fc.tiled_game(h, w, k, last=min(w + 1, TILED_ROOTS))
    roots = fc.concat([fc.take(mixed, running[:RUNNING_ROOTS]), fc.take(mixed, ended[:ENDED_ROOTS]), tiled])
    assert roots[0].shape[0] <= 24
    return roots


def case_roots(case):
    return _case_roots(case.h, case.w, case.k)


def case_max_plies(case, roots=None):
    if case.cap is None:
        return UNCAPPED
    roots = case_roots(case) if roots is None else roots
    return int(np.median(roots[3][roots[2] == -1])) + case.cap


@functools.lru_cache(maxsize=None)
def case_trees(index, per_ply=False, policy="uniform"):
    """search_trees of CASES[index], computed once a session and shared: treat everything as read-only"""
    case = CASES[index]
    roots = case_roots(case)
    return search_trees(case.h, case.w, case.k, roots, SEED, case.first_game, case.iterations, case.playouts, case.explore,
                        case_max_plies(case, roots), per_ply, policy)


@functools.lru_cache(maxsize=None)
def case_expected(index, per_ply=False, policy="uniform"):
    """search_expected of CASES[index], from case_trees: treat the arrays as read-only"""
    return _outputs(CASES[index].w, *case_trees(index, per_ply, policy))
