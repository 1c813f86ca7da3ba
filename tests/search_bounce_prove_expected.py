"""The CPU statement of bgs_bounce_search_moves_proving (include/bgs.h), built on tests/search_bounce_expected.py -- its
Node, its oracle steps and playouts, its selection arithmetic, its case table and helpers -- and the hand-made cases of
tests/test_gpu_search_bounce_prove.py.  No GPU import; not a test module.

On top of the plain search's tree every edge has a tag, seen from the player to move at its node: OPEN, WIN, DRAW or
LOSS.  The selection runs over the arms whose tag is OPEN (a capped arm is OPEN for good); an edge that ends the game is
tagged when it is played; after such an iteration the tags go up the path while the node at hand has a value (step 7); a
root whose value is not OPEN runs no further iteration.  The playouts of iteration t of all roots go through one oracle
batch, as in search_bounce_expected, under the game ids of the T that was asked for.

Beside the tag the model keeps the HEIGHT of its proof in plies: 1 for an edge that ends the game, 1 + the height of the
child's WIN arm for a LOSS edge, 1 + the largest height among the child's arms for a WIN or a backed-up DRAW edge.  A
horizon solver of that depth sees the whole proof."""

import functools
from collections import namedtuple

import numpy as np

from tests import search_bounce_expected as sb
from tests.mc_expected import make_roots
from tests.search_bounce_expected import (BY_NAME, CASES, MASK64, MAX_PLIES, RUNS, SEED, Node, _actions, _play, _step,  # noqa: F401
                                          all_nodes, default_edges, e_term, min_edges, q_term, slot_of)

OPEN, WIN, DRAW, LOSS = 0, 1, 2, 3
# the solver's codes (include/bgs.h): what `proved` holds
SOLVE_NONE, SOLVE_LOSS, SOLVE_DRAW, SOLVE_WIN, SOLVE_UNKNOWN, SOLVE_BUDGET = -2, -1, 0, 1, 2, 3
CODE = {OPEN: SOLVE_UNKNOWN, WIN: SOLVE_WIN, DRAW: SOLVE_DRAW, LOSS: SOLVE_LOSS}
NEGATED = {WIN: LOSS, LOSS: WIN, DRAW: DRAW}
TALLIES = ("selections", "tied_selections", "goal_leaves", "blocked_leaves", "drawn_leaves", "capped_leaves", "cut_playouts", "pool_full",
           "late_nodes", "max_depth", "best_ties", "tags_set", "tags_backed_up", "deepest_backup", "draws_backed_up", "excluded_top",
           "capped_only_selections", "stopped_early", "decided_win", "decided_draw", "decided_loss", "decided_draw_with_loss",
           "decided_loss_all_arms", "max_height")


class ProvingNode(Node):
    def __init__(self, position, actions):
        super().__init__(position, actions)
        self.tag = [OPEN] * len(actions)
        self.height = [0] * len(actions)    # plies of the proof below (and with) a tagged edge
        self.capped = set()                 # the arms whose position holds the cap


def value(node):
    for what in (WIN, OPEN, DRAW):
        if what in node.tag:
            return what
    return LOSS


def _rule(node, arms, explore):
    """(arm, the top U is shared) by the plain rule over `arms`, ascending"""
    fresh = [a for a in arms if node.n[a] == 0]
    if fresh:
        return fresh[0], None
    total = sum(node.n[a] for a in arms)
    u = [q_term(node.s[a], node.n[a]) + e_term(explore, total, node.n[a]) for a in arms]
    top = max(u)
    return arms[u.index(top)], u.count(top) > 1


def select_open(node, explore, seen):
    """the arm an iteration takes at `node`: the plain rule over the OPEN arms.  Counts the selections in which that rule,
    over all arms, would have taken a tagged one, and those in which every OPEN arm is capped"""
    everything = list(range(len(node.actions)))
    candidates = [a for a in everything if node.tag[a] == OPEN]
    assert candidates, "the descent stands on a node without an OPEN arm"
    assert all(node.n[a] > 0 for a in everything if node.tag[a] != OPEN)
    arm, tied = _rule(node, candidates, explore)
    if tied is not None:
        seen["selections"] += 1
        seen["tied_selections"] += int(tied)
        if len(candidates) < len(everything):
            seen["excluded_top"] += int(node.tag[_rule(node, everything, explore)[0]] != OPEN)
    seen["capped_only_selections"] += int(all(a in node.capped for a in candidates))
    return arm


def search_trees(grid, roots, seed, first_game, iterations, leaf_playouts, explore, max_plies, policy="uniform", edges=None):
    """(trees, counts int64[n, S, 3], used int64[n], done int64[n], env-steps, seen): search_bounce_expected.search_trees
    with the tags"""
    assert iterations >= 1 and leaf_playouts >= 1 and iterations * leaf_playouts <= sb.MAX_PLAYOUTS and 0 <= explore <= sb.MAX_EXPLORE
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
        trees.append(ProvingNode(position, acts) if acts else None)
        used[i] = len(acts)
        assert used[i] <= E
    counts = np.zeros((n, S, 3), dtype=np.int64)
    done = np.array([0 if tree is None else T for tree in trees], dtype=np.int64)
    over = [tree is None for tree in trees]
    steps = 0
    seen = dict.fromkeys(TALLIES, 0)
    seen["capped"] = np.zeros((n, S), dtype=np.int64)
    seen["tagged_roots"] = np.zeros(n, dtype=bool)      # some edge of root i's tree was tagged
    full = np.zeros(n, dtype=bool)
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
                a = select_open(node, explore, seen)
                path.append((node, a))
                if a not in node.edge:
                    node.edge[a] = _step(grid, node.position, node.actions[a])
                won, after = node.edge[a]
                if won != -1:                               # the edge ends the game: a fact
                    goal = node.actions[a][1][1] in (0, h - 1)
                    seen["goal_leaves" if goal else ("drawn_leaves" if won == 2 else "blocked_leaves")] += 1
                    outcome[i] = [won] * P
                    assert node.tag[a] == OPEN and won in (2, node.position[1])
                    node.tag[a], node.height[a] = (DRAW if won == 2 else WIN), 1
                    seen["tags_set"] += 1
                    seen["tagged_roots"][i] = True
                    tagged.add(i)
                    break
                if after[2] >= cap:                         # capped at once: not an end, no tag, OPEN for good
                    seen["capped_leaves"] += 1
                    node.capped.add(a)
                    outcome[i] = [-1] * P
                    break
                if node.child[a] is not None:
                    node = node.child[a]
                    continue
                acts = _actions(grid, after)
                assert acts
                if used[i] + len(acts) <= E:
                    node.child[a] = ProvingNode(after, acts)
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
            if i in tagged:                                 # step 7
                levels = 0
                for k in range(len(path) - 1, -1, -1):
                    at = path[k][0]
                    what = value(at)
                    if what == OPEN:
                        break
                    if k == 0:
                        seen[{WIN: "decided_win", DRAW: "decided_draw", LOSS: "decided_loss"}[what]] += 1
                        seen["decided_draw_with_loss"] += int(what == DRAW and LOSS in at.tag)
                        seen["decided_loss_all_arms"] += int(what == LOSS and len(at.tag) > 1)
                        break
                    above, a = path[k - 1]
                    assert above.tag[a] == OPEN and above.child[a] is at
                    above.tag[a] = NEGATED[what]
                    above.height[a] = 1 + (at.height[at.tag.index(WIN)] if what == WIN else max(at.height))
                    levels += 1
                    seen["draws_backed_up"] += int(what == DRAW)
                seen["tags_backed_up"] += levels
                seen["deepest_backup"] = max(seen["deepest_backup"], levels)
    return trees, counts, used, done, steps, seen


def _outputs(grid, trees, counts, used, done, steps, seen):
    h, w = grid.shape
    n, S = len(trees), w * h * w
    seen = dict(seen)
    visits = np.zeros((n, S), dtype=np.int64)
    best = np.full(n, -1, dtype=np.int64)
    nodes = np.zeros(n, dtype=np.int64)
    proved = np.full((n, S), SOLVE_NONE, dtype=np.int8)
    height = np.zeros((n, S), dtype=np.int64)
    for i, root in enumerate(trees):
        if root is None:
            continue
        slots = [slot_of(a, h, w) for a in root.actions]
        assert slots == sorted(slots)
        arms = range(len(slots))
        visits[i, slots] = root.n
        proved[i, slots] = [CODE[tag] for tag in root.tag]
        height[i, slots] = root.height
        won = [a for a in arms if root.tag[a] == WIN]
        assert len(won) <= 1
        among = [a for a in arms if root.tag[a] != LOSS] or list(arms)
        ranked = sorted((a for a in among if root.n[a] > 0), key=lambda a: (-root.n[a], -root.s[a], slots[a]))
        best[i] = slots[won[0]] if won else slots[ranked[0]]
        seen["best_ties"] += int(not won and len(ranked) > 1 and root.n[ranked[0]] == root.n[ranked[1]])
        nodes[i] = len(all_nodes(root)) - 1
    shape = (n, w, h * w)
    seen["height"] = height.reshape(shape)
    seen["max_height"] = int(height.max()) if height.size else 0
    return (counts.reshape(shape + (3,)).astype(np.int32), visits.reshape(shape).astype(np.int32), best.astype(np.int32),
            nodes.astype(np.int32), used.astype(np.int32), proved.reshape(shape), done.astype(np.int32), steps, seen)


def search_bounce_prove_expected(grid, roots, seed, first_game, iterations, leaf_playouts, explore, max_plies, policy="uniform", edges=None):
    """(counts int32[n, W, H * W, 3], visits int32[n, W, H * W], best, nodes, used int32[n], proved int8[n, W, H * W], done
    int32[n], env-steps, seen).  seen: the tallies of search_bounce_expected, and "drawn_leaves" (edges after which
    neither side can move), "tags_set" (step 4), "tags_backed_up" (step 7), "deepest_backup" (the most tags one step 7
    wrote: the levels a fact went up), "draws_backed_up", "excluded_top" (selections in which the plain rule, over all
    arms, would have taken a tagged arm), "capped_only_selections" (selections at a node whose every OPEN arm holds the
    cap), "stopped_early" (roots with done < T), "decided_win" / "decided_draw" / "decided_loss" (roots whose value step 7
    found), "decided_draw_with_loss" (of those, drawn roots with an arm tagged LOSS), "decided_loss_all_arms" (lost roots
    with more than one arm), "tagged_roots" bool[n] (some edge of the root's tree was tagged), "height" int64[n, W, H * W]
    (the plies of the proof of every tagged root slot, 0 elsewhere) and "max_height\""""
    return _outputs(grid, *search_trees(grid, roots, seed, first_game, iterations, leaf_playouts, explore, max_plies, policy, edges))


# ---- hand-made cases beside the table of tests/search_bounce_expected.py (reused unchanged): at most 8 roots, T * P <= 1024
HandCase = namedtuple("HandCase", "name grid roots iterations playouts explore max_plies first_game edges policies")



@functools.lru_cache(maxsize=None)
def _hand_roots(grid_name, n, roots_seed):
    return make_roots(sb.GRIDS[grid_name], n, roots_seed)


# "draws": the crowded grid (blocked sides inside the tree) from the one make_roots seed of 0 .. 299, at 8 roots and 32 x 4,
# whose search backs a DRAW up (three times, one of them four levels) and decides a root DRAW that also holds a LOSS arm;
# no seed of the narrow, blocked_start and small grids does either.
HAND_CASES = (
    HandCase("draws", sb.GRIDS["crowded"], _hand_roots("crowded", 8, 142), 32, 4, sb.DEFAULT_EXPLORE, sb.LONG, 3, None, ("uniform",)),
)
HAND_BY_NAME = {c.name: c for c in HAND_CASES}


def hand_runs():
    return [(c.name, p) for c in HAND_CASES for p in c.policies]


@functools.lru_cache(maxsize=None)
def case_trees(name, policy="uniform"):
    """search_trees of the case of the plain table, computed once a session and shared: treat everything as read-only"""
    case = BY_NAME[name]
    roots = sb.case_roots(case)
    return search_trees(sb.case_grid(case), roots, SEED, case.first_game, case.iterations, case.playouts, case.explore,
                        sb.case_max_plies(case, roots), policy, sb.case_edges(case))


@functools.lru_cache(maxsize=None)
def case_expected(name, policy="uniform"):
    """search_bounce_prove_expected of the case, from case_trees: treat the arrays as read-only"""
    return _outputs(sb.case_grid(BY_NAME[name]), *case_trees(name, policy))


@functools.lru_cache(maxsize=None)
def hand_trees(name, policy="uniform"):
    c = HAND_BY_NAME[name]
    return search_trees(c.grid, c.roots, SEED, c.first_game, c.iterations, c.playouts, c.explore, c.max_plies, policy, c.edges)


@functools.lru_cache(maxsize=None)
def hand_expected(name, policy="uniform"):
    return _outputs(HAND_BY_NAME[name].grid, *hand_trees(name, policy))
