"""The CPU statement of bgs_bounce_search_moves (include/bgs.h), built on the oracle's public API alone, and the case
table of tests/test_gpu_search_bounce.py.  No GPU import; not a test module.

A Python tree per root: a node holds n[a], s[a] and child[a] for every arm -- its legal moves in the oracle's canonical
order, which is ascending slot x * H * W + ty * W + tx -- and (the model's convenience; the kernel rebuilds it) its
position.  Every root has a pool of E edges: the root takes A(root) of them, a node A(node) when it is made.  Iteration t
of every running root descends by the rule of the header -- the lowest arm with n = 0, else the largest U(a) = Q(a) +
E(a), ties to the lowest arm -- until an edge ends the game, reaches a position that holds the cap, or has no child.  An
edge without a child gets its node if and only if used + A(p') <= E; either way the playouts start from p'.

The playouts of iteration t of ALL roots then go through one BounceOracle batch in the lock step of
tests/bounce_halving_expected.py::_play: every ply of a running board below the cap takes the canonical list L, keeps the
moves into the mover's goal row when the policy is decisive and there are any, and plays element
oracle.sample_index(seed, G, plies, size) of that list under the playout's own game id G = ((first_game + i) * T + t) * P
+ j.  Env-steps are the oracle's ply counts past the leaf's."""

import functools
from collections import namedtuple

import numpy as np

from oracle import oracle
from tests.bounce_halving_expected import candidates
from tests.bounce_policy_expected import GRIDS as POLICY_GRIDS
from tests.bounce_policy_expected import MASK64, SEED, short_cap
from tests.mc_expected import make_roots
from tests.search_expected import DEFAULT_EXPLORE, MAX_EXPLORE, MAX_PLAYOUTS, e_term, isqrt, lg, q_term  # noqa: F401

LONG = 1024
MAX_PLIES = 65535          # plies are 16-bit: the cap is clamped to this, and a root that holds it has no arms

# 18 columns on three rows: the one geometry here whose move list needs three words of counts (NC = 3); every other grid
# of the table needs one (up to 8 columns) or two (9 .. 16).  One interior row: a piece moves sideways or into a goal row.
FLAT = np.array([[0] * 18, [2, 0, 3, 0, 0, 2, 0, 0, 4, 0, 3, 0, 0, 2, 0, 0, 3, 2], [0] * 18], dtype=np.int8)
GRIDS = dict(POLICY_GRIDS, flat=FLAT)


def min_edges(h, w):
    """BGS_BOUNCE_SEARCH_MIN_EDGES(h, w): the most arms a position of the geometry can have"""
    return w * w * (h - 2) if h >= 3 else 1


def default_edges(h, w, iterations):
    """the pool BounceBatch.search_moves takes with edges=None"""
    least = min_edges(h, w)
    return min((iterations + 1) * least, least + 32 * iterations)


def count_words(w):
    """the words of 8-bit per-column counts the move list of a board of w columns needs (the kernel's NC, at least)"""
    return (w + 7) // 8


class Node:
    def __init__(self, position, actions, first_visit=True):
        a = len(actions)
        self.position = position            # (grid int8[h, w], player, plies) of a running board
        self.actions = actions              # [((sx, sy), (tx, ty))], canonical order
        self.n, self.s, self.child = [0] * a, [0] * a, [None] * a
        self.edge = {}                      # a -> (winner after a, position after a), filled when the edge is first played
        self.first_visit = first_visit      # the node was made the first time its edge was taken


def select(node, explore, seen):
    """the arm an iteration takes at `node`"""
    arms = range(len(node.actions))
    fresh = [a for a in arms if node.n[a] == 0]
    if fresh:
        return fresh[0]
    total = sum(node.n)
    u = [q_term(node.s[a], node.n[a]) + e_term(explore, total, node.n[a]) for a in arms]
    top = max(u)
    seen["selections"] += 1
    seen["tied_selections"] += int(u.count(top) > 1)
    return u.index(top)                     # (index: the first, so the lowest arm)


def _probe(grid, position):
    grid_now, player, plies = position
    orc = oracle.BounceOracle(grid, 1)
    orc.grid[0], orc.player[0], orc.winner[0], orc.plies[0] = grid_now, player, -1, plies
    return orc


def _actions(grid, position):
    return _probe(grid, position).actions(0)


def _step(grid, position, action):
    """(winner, position) after `action` on `position`, by the oracle (a blocked side to move is settled there)"""
    orc = _probe(grid, position)
    (sx, sy), (tx, ty) = action
    assert orc.step_actions(np.int32([[sx, sy, tx, ty]]))[0] == 0
    return int(orc.winner[0]), (orc.grid[0].copy(), int(orc.player[0]), int(orc.plies[0]))


def _play(grid, leaves, ids, seed, max_plies, uniform):
    """(winner int8[len(leaves)], env-steps): the running position leaves[j] played on as game ids[j]"""
    h = grid.shape[0]
    orc = oracle.BounceOracle(grid, len(leaves))
    for j, (grid_now, player, plies) in enumerate(leaves):
        orc.grid[j], orc.player[j], orc.winner[j], orc.plies[j] = grid_now, player, -1, plies
    steps = 0
    lists = {}   # (board, player) -> L: boards repeat among the playouts of a leaf
    while True:
        active = np.flatnonzero((orc.winner == -1) & (orc.plies < max_plies))
        if active.size == 0:
            break
        moves = np.full((len(leaves), 4), -1, dtype=np.int32)
        for k in active:
            mover = int(orc.player[k])
            key = (orc.grid[k].tobytes(), mover)
            if key not in lists:
                lists[key] = orc.actions(int(k))
            cand = candidates(lists[key], mover, h, uniform)
            (sx, sy), (tx, ty) = cand[oracle.sample_index(seed, ids[k], int(orc.plies[k]), len(cand))]
            moves[k] = (sx, sy, tx, ty)
        assert (orc.step_actions(moves)[active] == 0).all()
        steps += int(active.size)
    return orc.winner.copy(), steps


def slot_of(action, h, w):
    (sx, _), (tx, ty) = action
    return sx * h * w + ty * w + tx


def search_trees(grid, roots, seed, first_game, iterations, leaf_playouts, explore, max_plies, policy="uniform", edges=None):
    """(trees, counts int64[n, S, 3], used int64[n], env-steps, seen): trees[i] is the root Node of board i, None for a
    board that has ended, has no move or holds 65535 plies.  seen counts the UCB "selections", the "tied_selections" (the
    top two U equal, so the arm order decided), the terminal leaves by a move into a "goal_leaves" row and by a
    "blocked_leaves" side, the "capped_leaves" (capped at once), the "cut_playouts" (playouts the cap cut in mid-game),
    the "pool_full" events (a node that did not fit), the "late_nodes" (nodes made after a larger one of their root did
    not fit), the "max_depth" of a path in edges; seen["capped"] int64[n, S]: the playouts through every root slot that
    the cap left unfinished (at once or in mid-game)"""
    assert iterations >= 1 and leaf_playouts >= 1 and iterations * leaf_playouts <= MAX_PLAYOUTS and 0 <= explore <= MAX_EXPLORE
    g, player, winner, plies = roots
    h, w = grid.shape
    n, S = g.shape[0], w * h * w
    T, P = iterations, leaf_playouts
    E = default_edges(h, w, T) if edges is None else edges
    assert E >= min_edges(h, w)
    cap = min(int(max_plies), MAX_PLIES)
    trees, used = [], np.zeros(n, dtype=np.int64)
    for i in range(n):
        position = (g[i].copy(), int(player[i]), int(plies[i]))
        acts = _actions(grid, position) if winner[i] == -1 and plies[i] < MAX_PLIES else []
        trees.append(Node(position, acts) if acts else None)
        used[i] = len(acts)
        assert used[i] <= E
    counts = np.zeros((n, S, 3), dtype=np.int64)
    steps = 0
    seen = dict.fromkeys(("selections", "tied_selections", "goal_leaves", "blocked_leaves", "capped_leaves", "cut_playouts",
                          "pool_full", "late_nodes", "max_depth", "best_ties"), 0)
    seen["capped"] = np.zeros((n, S), dtype=np.int64)
    full = np.zeros(n, dtype=bool)          # some node of root i did not fit its pool
    for t in range(T):
        paths, leaves, ids, owner, outcome = {}, [], [], [], {}
        for i in range(n):
            if trees[i] is None:
                continue
            node, path = trees[i], []
            while True:
                a = select(node, explore, seen)
                path.append((node, a))
                if a not in node.edge:
                    node.edge[a] = _step(grid, node.position, node.actions[a])
                won, after = node.edge[a]
                if won != -1:                               # the edge ends the game: P playouts with that outcome
                    goal = node.actions[a][1][1] in (0, h - 1)
                    seen["goal_leaves" if goal else "blocked_leaves"] += 1
                    outcome[i] = [won] * P
                    break
                if after[2] >= cap:                         # capped at once: no node, no game, every playout scores 0
                    seen["capped_leaves"] += 1
                    outcome[i] = [-1] * P
                    break
                if node.child[a] is not None:
                    node = node.child[a]
                    continue
                acts = _actions(grid, after)
                assert acts                                 # (a running position has a move: the oracle settles blocked sides)
                if used[i] + len(acts) <= E:
                    node.child[a] = Node(after, acts, first_visit=node.n[a] == 0)
                    used[i] += len(acts)
                    seen["late_nodes"] += int(full[i])
                else:
                    seen["pool_full"] += 1
                    full[i] = True
                for j in range(P):
                    leaves.append(after)
                    ids.append((((first_game + i) * T + t) * P + j) & MASK64)
                    owner.append(i)
                break
            paths[i] = path
            seen["max_depth"] = max(seen["max_depth"], len(path))
        if leaves:
            won, played = _play(grid, leaves, ids, seed, cap, policy == "uniform")
            steps += played
            seen["cut_playouts"] += int((won == -1).sum())
            for i, x in zip(owner, won.tolist()):
                outcome.setdefault(i, []).append(x)
        for i, path in paths.items():
            result = np.array(outcome[i])
            assert result.size == P
            mover = int(player[i])
            tally = {who: int((result == who).sum()) for who in (0, 1, 2)}
            slot = slot_of(path[0][0].actions[path[0][1]], h, w)
            counts[i, slot] += (tally[mover], tally[2], tally[1 - mover])
            seen["capped"][i, slot] += int((result == -1).sum())
            for node, a in path:
                node.n[a] += P
                node.s[a] += 2 * tally[node.position[1]] + tally[2]
    return trees, counts, used, steps, seen


def all_nodes(root):
    """every node of the tree below (and with) `root`"""
    out, stack = [], [root]
    while stack:
        node = stack.pop()
        out.append(node)
        stack.extend(c for c in node.child if c is not None)
    return out


def _outputs(grid, trees, counts, used, steps, seen):
    h, w = grid.shape
    n, S = len(trees), w * h * w
    seen = dict(seen)
    visits = np.zeros((n, S), dtype=np.int64)
    best = np.full(n, -1, dtype=np.int64)
    nodes = np.zeros(n, dtype=np.int64)
    for i, root in enumerate(trees):
        if root is None:
            continue
        slots = [slot_of(a, h, w) for a in root.actions]
        assert slots == sorted(slots)
        visits[i, slots] = root.n
        ranked = sorted((a for a in range(len(slots)) if root.n[a] > 0), key=lambda a: (-root.n[a], -root.s[a], slots[a]))
        best[i] = slots[ranked[0]]
        seen["best_ties"] += int(len(ranked) > 1 and root.n[ranked[0]] == root.n[ranked[1]])
        nodes[i] = len(all_nodes(root)) - 1
    shape = (n, w, h * w)
    return (counts.reshape(shape + (3,)).astype(np.int32), visits.reshape(shape).astype(np.int32), best.astype(np.int32),
            nodes.astype(np.int32), used.astype(np.int32), steps, seen)


def search_bounce_expected(grid, roots, seed, first_game, iterations, leaf_playouts, explore, max_plies, policy="uniform", edges=None):
    """(counts int32[n, W, H * W, 3], visits int32[n, W, H * W], best int32[n], nodes int32[n], used int32[n], env-steps,
    seen): seen as search_trees gives it, and "best_ties" (two root arms with the most visits)"""
    return _outputs(grid, *search_trees(grid, roots, seed, first_game, iterations, leaf_playouts, explore, max_plies, policy, edges))


# ---- the cases of the GPU comparison: roots from make_roots(grid, n, roots_seed) (the start, positions a few and many
# plies in, boards played to the end), at most 8 a case, T * P <= 1024: the smallest shapes that reach each branch.
# cap_past: None (1024 plies), or plies past the least ply count of a running root.  edges: None (the default pool) or
# "min" (BGS_BOUNCE_SEARCH_MIN_EDGES exactly).
Case = namedtuple("Case", "name grid n roots_seed iterations playouts explore cap_past first_game edges policies")
BOTH = ("uniform", "decisive")
CASES = (
    Case("default", "default", 8, 5, 48, 16, DEFAULT_EXPLORE, None, 5, None, BOTH),                # the baseline
    Case("uct", "default", 8, 5, 200, 1, DEFAULT_EXPLORE, None, 0, None, ("uniform",)),            # classic UCT: U ties, deep paths
    Case("refill", "default", 4, 5, 3, 300, DEFAULT_EXPLORE, None, 0, None, ("uniform",)),         # P above the team's lanes
    Case("ids", "small", 8, 6, 24, 8, DEFAULT_EXPLORE, None, 2**33, None, ("uniform",)),           # game ids beyond 32 bits
    Case("capped", "small", 8, 6, 40, 8, DEFAULT_EXPLORE, 3, 1, None, BOTH),                       # capped at once, cut in mid-game
    Case("expansion", "default", 8, 5, 8, 8, DEFAULT_EXPLORE, None, 0, None, ("uniform",)),        # T <= the arms of a root
    Case("exploit", "default", 8, 5, 40, 8, 0, None, 0, None, ("uniform",)),                       # pure exploitation
    Case("ceiling", "default", 8, 5, 40, 8, MAX_EXPLORE, None, 0, None, ("uniform",)),             # the ceiling of `explore`
    Case("pool", "default", 8, 5, 64, 4, DEFAULT_EXPLORE, None, 3, "min", ("uniform",)),           # the pool runs dry, edges retried
    Case("narrow", "narrow", 8, 9, 32, 8, DEFAULT_EXPLORE, None, 7, None, ("uniform",)),           # a root with one arm
    Case("blocked_start", "blocked_start", 8, 10, 48, 8, DEFAULT_EXPLORE, None, 5, None, ("uniform",)),
    Case("crowded", "crowded", 6, 8, 48, 8, DEFAULT_EXPLORE, None, 3, None, ("uniform",)),         # blocked sides inside the tree
    Case("wide", "wide", 6, 11, 96, 8, DEFAULT_EXPLORE, None, 5, None, BOTH),                      # 12 columns: two count words, 71 arms
    Case("tall_wide", "tall_wide", 6, 12, 64, 8, DEFAULT_EXPLORE, None, 2**33, None, ("decisive",)),      # 9 columns, long games
    Case("flat", "flat", 6, 13, 40, 8, DEFAULT_EXPLORE, None, 5, None, ("uniform",)),              # 18 columns: three count words
)
BY_NAME = {c.name: c for c in CASES}
RUNS = [(c.name, p) for c in CASES for p in c.policies]


@functools.lru_cache(maxsize=None)
def _roots(grid_name, n, roots_seed):
    return make_roots(GRIDS[grid_name], n, roots_seed)


def case_grid(case):
    return GRIDS[case.grid]


def case_roots(case):
    return _roots(case.grid, case.n, case.roots_seed)


def case_max_plies(case, roots=None):
    roots = case_roots(case) if roots is None else roots
    return LONG if case.cap_past is None else short_cap(roots, case.cap_past)


def case_edges(case):
    h, w = case_grid(case).shape
    return min_edges(h, w) if case.edges == "min" else default_edges(h, w, case.iterations)


@functools.lru_cache(maxsize=None)
def case_trees(name, policy="uniform"):
    """search_trees of the case, computed once a session and shared: treat everything as read-only"""
    case = BY_NAME[name]
    roots = case_roots(case)
    return search_trees(case_grid(case), roots, SEED, case.first_game, case.iterations, case.playouts, case.explore,
                        case_max_plies(case, roots), policy, case_edges(case))


@functools.lru_cache(maxsize=None)
def case_expected(name, policy="uniform"):
    """search_bounce_expected of the case, from case_trees: treat the arrays as read-only"""
    return _outputs(case_grid(BY_NAME[name]), *case_trees(name, policy))
