"""The CPU statement of bgs_bounce_forest_search / bgs_bounce_forest_advance (include/bgs.h), built on
tests/search_bounce_expected.py (Node, select, the oracle's step and playouts, the slot of an action, the grids and the
root makers), and the chains of tests/test_gpu_bounce_forest.py.  No GPU import; not a test module.

A Forest holds a persistent Python tree per board: the nodes in use in the order they were made (node 0 is the root; an
empty list is an emptied tree), the edges in use, and the cap the tree was grown under.  Every node carries `first`, the
offset of its edge block in the tree's pool, so that the layout the kernel keeps -- blocks contiguous and ascending with
the node index -- can be checked on the model.  `search` makes the carried check of the header, empties the trees that
fail it and runs the iterations of search_bounce_expected.search_trees (restated here: that loop cannot be imported
piecemeal) with the forest's step 4: a node is made if and only if the edge has no child, the tree holds fewer than C
nodes and used + A(p') <= E.  `advance` re-roots a tree at the child of the root's arm with the given slot, or empties it.

A CHAIN is a list of moves over one set of roots.  A move is (seed, T, P, rule, cap): every tree is searched, then every
running board advances its tree and steps its board by what the rule gives (one ply or two), so boards end along the way.
run_chain records, move by move, the roots, the expected outputs and the plies: the GPU test replays them."""

import functools
from collections import namedtuple

import numpy as np

from oracle import oracle
from tests import search_bounce_expected as sb
from tests.search_bounce_expected import GRIDS, MAX_PLIES, Node, _actions, _play, _roots, _step, select, slot_of

# one column tall enough that games last: every position has one arm, so a carried tree is a chain of one-arm nodes
COLUMN = np.array([[0], [1], [0], [0], [0], [0], [0], [1], [0]], dtype=np.int8)
GRIDS = dict(GRIDS, column=COLUMN)
SEED = sb.SEED
MASK64 = sb.MASK64
LONG = sb.LONG
MAX_NODES = 65536           # BGS_BOUNCE_FOREST_MAX_NODES


class Forest:
    def __init__(self, grid, n, nodes_cap, edges):
        h, w = grid.shape
        assert 2 <= nodes_cap <= MAX_NODES and edges >= sb.min_edges(h, w)
        self.grid, self.n, self.capacity, self.edges = grid, n, nodes_cap, edges
        self.nodes = [[] for _ in range(n)]     # the nodes of tree i in index order; []: emptied
        self.used = [0] * n                     # pool edges in use
        self.cap = [0] * n                      # the effective cap the tree's sentinels were written under
        # what the chains must reach (tests/test_bounce_forest_expected.py)
        self.seen = dict.fromkeys(("no_room_nodes", "no_room_edges", "emptied_no_child", "emptied_sentinel", "emptied_cap",
                                   "emptied_position", "most_kept", "overlapping_moves"), 0)

    def root(self, i):
        return self.nodes[i][0] if self.nodes[i] else None

    def _new_node(self, i, position, actions):
        node = Node(position, actions)
        node.first = self.used[i]
        node.stopped = {}                       # arm -> the playouts of the iterations that ended at this edge
        self.nodes[i].append(node)
        self.used[i] += len(actions)
        return node

    def search(self, roots, seed, first_game, iterations, leaf_playouts, explore, max_plies, policy="uniform", restart=False):
        """(counts, visits, best, nodes, used, carried, env-steps) of one launch over `roots` (grid, player, winner, plies)"""
        g, player, winner, plies = roots
        h, w = self.grid.shape
        n, S = self.n, w * h * w
        T, P = iterations, leaf_playouts
        assert T >= 1 and P >= 1 and T * P <= sb.MAX_PLAYOUTS and 0 <= explore <= sb.MAX_EXPLORE and g.shape[0] == n
        C, E = self.capacity, self.edges
        cap = min(int(max_plies), MAX_PLIES)
        carried = np.zeros(n, dtype=np.int64)
        for i in range(n):
            position = (g[i].copy(), int(player[i]), int(plies[i]))
            acts = _actions(self.grid, position) if winner[i] == -1 and plies[i] < MAX_PLIES else []
            root = self.root(i)
            same = root is not None and np.array_equal(root.position[0], g[i]) and root.position[2] == int(plies[i])
            keep = not restart and bool(acts) and same and self.cap[i] == cap and sum(root.n) + T * P < 2**31
            if keep:
                assert root.position[1] == int(player[i]) and 1 <= len(self.nodes[i]) <= C and len(acts) <= self.used[i] <= E
                carried[i] = len(self.nodes[i]) - 1
                continue
            if not restart and bool(acts) and root is not None:
                self.seen["emptied_position" if not same else "emptied_cap"] += 1
            self.nodes[i], self.used[i], self.cap[i] = [], 0, cap
            if acts:
                self._new_node(i, position, acts)
        counts = np.zeros((n, S, 3), dtype=np.int64)
        steps = 0
        seen = dict.fromkeys(("selections", "tied_selections"), 0)
        for t in range(T):
            paths, leaves, ids, owner, outcome = {}, [], [], [], {}
            for i in range(n):
                if not self.nodes[i]:
                    continue
                node, path = self.nodes[i][0], []
                while True:
                    a = select(node, explore, seen)
                    path.append((node, a))
                    if a not in node.edge:
                        node.edge[a] = _step(self.grid, node.position, node.actions[a])
                    won, after = node.edge[a]
                    if won != -1:                               # the edge ends the game: P playouts with that outcome
                        outcome[i] = [won] * P
                        break
                    if after[2] >= cap:                         # capped at once: no node, no game, every playout scores 0
                        outcome[i] = [-1] * P
                        break
                    if node.child[a] is not None:
                        node = node.child[a]
                        continue
                    acts = _actions(self.grid, after)
                    assert acts
                    if len(self.nodes[i]) < C and self.used[i] + len(acts) <= E:
                        node.child[a] = self._new_node(i, after, acts)
                    elif len(self.nodes[i]) >= C:
                        self.seen["no_room_nodes"] += 1
                    else:
                        self.seen["no_room_edges"] += 1
                    for j in range(P):
                        leaves.append(after)
                        ids.append((((first_game + i) * T + t) * P + j) & MASK64)
                        owner.append(i)
                    break
                paths[i] = path
                assert len(path) <= len(self.nodes[i])          # the descent path fits C words
            if leaves:
                won, played = _play(self.grid, leaves, ids, seed, cap, policy == "uniform")
                steps += played
                for i, x in zip(owner, won.tolist()):
                    outcome.setdefault(i, []).append(x)
            for i, path in paths.items():
                result = np.array(outcome[i])
                assert result.size == P
                mover = int(player[i])
                tally = {who: int((result == who).sum()) for who in (0, 1, 2)}
                counts[i, slot_of(path[0][0].actions[path[0][1]], h, w)] += (tally[mover], tally[2], tally[1 - mover])
                for node, a in path:
                    node.n[a] += P
                    node.s[a] += 2 * tally[node.position[1]] + tally[2]
                node, a = path[-1]                              # the playouts that went no further than this edge
                node.stopped[a] = node.stopped.get(a, 0) + P
        visits = np.zeros((n, S), dtype=np.int64)
        best = np.full(n, -1, dtype=np.int64)
        nodes = np.zeros(n, dtype=np.int64)
        for i in range(n):
            root = self.root(i)
            if root is None:
                continue
            slots = [slot_of(a, h, w) for a in root.actions]
            visits[i, slots] = root.n
            ranked = sorted((a for a in range(len(slots)) if root.n[a] > 0), key=lambda a: (-root.n[a], -root.s[a], slots[a]))
            best[i] = slots[ranked[0]]
            nodes[i] = len(self.nodes[i]) - 1
        shape = (n, w, h * w)
        return (counts.reshape(shape + (3,)).astype(np.int32), visits.reshape(shape).astype(np.int32), best.astype(np.int32),
                nodes.astype(np.int32), np.array(self.used, dtype=np.int32), carried.astype(np.int32), steps)

    def advance(self, slots):
        """kept int32[n]: re-root tree i at the child of its root's arm with slot slots[i], or empty it; a negative slot
        leaves it"""
        h, w = self.grid.shape
        kept = np.zeros(self.n, dtype=np.int32)
        for i, slot in enumerate(np.asarray(slots).tolist()):
            if slot >= 0:
                root, child = self.root(i), None
                if root is not None:
                    arm = [a for a, action in enumerate(root.actions) if slot_of(action, h, w) == slot]
                    if arm:
                        child = root.child[arm[0]]
                        if child is None:
                            won, after = root.edge.get(arm[0], (-1, (None, 0, 0)))
                            sentinel = won != -1 or (arm[0] in root.edge and after[2] >= self.cap[i])
                            self.seen["emptied_sentinel" if sentinel else "emptied_no_child"] += 1
                if child is None:
                    self.nodes[i], self.used[i] = [], 0
                else:
                    inside = {id(node) for node in sb.all_nodes(child)}
                    stay = [node for node in self.nodes[i] if id(node) in inside]      # the relative order is kept
                    assert stay[0] is child
                    at = 0
                    for node in stay:       # blocks are packed from edge 0, to offsets that never exceed the old ones
                        assert at <= node.first
                        self.seen["overlapping_moves"] += int(at < node.first < at + len(node.actions))
                        node.first = at
                        at += len(node.actions)
                    self.nodes[i], self.used[i] = stay, at
                    self.seen["most_kept"] = max(self.seen["most_kept"], len(stay) - 1)
            kept[i] = max(len(self.nodes[i]) - 1, 0)
        return kept

    def check(self):
        """the invariants of the layout: every tree's blocks contiguous and ascending, children above their parents, an
        edge's n the sum over its child, the counts within the forest's room"""
        for i, nodes in enumerate(self.nodes):
            index = {id(node): v for v, node in enumerate(nodes)}
            at = 0
            for v, node in enumerate(nodes):
                assert node.first == at
                at += len(node.actions)
                for a, child in enumerate(node.child):
                    if child is not None:
                        assert index[id(child)] > v
                        assert node.n[a] == sum(child.n) + node.stopped[a] > sum(child.n)    # (what made the child, or found no room, stopped here)
                    else:
                        assert node.n[a] == node.stopped.get(a, 0)
            assert at == self.used[i] <= self.edges and len(nodes) <= self.capacity
            assert len(sb.all_nodes(nodes[0])) == len(nodes) if nodes else self.used[i] == 0


# ---- chains.  Rules, for every running board (an ended board gets -1):
#   "best"     one ply: the search's best slot for the tree and for the board;
#   "best2"    two plies: best, then the reply -- the most visited arm of the new root (ties: the lowest slot), or the lowest
#              legal move where the tree was emptied by the first ply;
#   "deep"     one ply: the root's arm with the largest subtree (ties: the lowest slot), the best slot where no arm has a node:
#              boards whose best move ends the game at once still carry something;
#   "high"     one ply: the last legal move, usually never expanded;
#   "desync"   as "best", but the board of the first running root with two legal moves steps by another move than its tree
#              advances by: the next search must start that tree anew.
# A move's `cap` (None: the chain's) is its max_plies as plies past the least ply count of a running root of the chain.
Move = namedtuple("Move", "seed iterations playouts rule cap", defaults=(None,))
Chain = namedtuple("Chain", "name grid n roots_seed nodes edges explore cap policy first_game moves")
Record = namedtuple("Record", "roots max_plies counts visits best nodes used carried steps plies desynced")
#   Record.plies: [(tree slots int32[n], board moves int32[n, 4], kept int32[n])]


def _moves(base, *steps):
    return tuple(Move((SEED + base + m) & MASK64, *step) for m, step in enumerate(steps))


E0 = sb.DEFAULT_EXPLORE
CHAINS = (
    Chain("default", "default", 8, 5, 97, None, E0, None, "uniform", 5,
          _moves(100, (48, 16, "best"), (48, 16, "best2"), (48, 16, "best"), (48, 16, "high"), (24, 16, "best"))),
    Chain("decisive", "default", 8, 5, 65, None, E0, None, "decisive", 0, _moves(200, (32, 16, "best"), (32, 16, "desync"), (32, 16, "best"))),
    Chain("wide", "wide", 6, 11, 401, None, sb.MAX_EXPLORE, None, "uniform", 3, _moves(300, (400, 2, "deep"), (100, 2, "deep"), (100, 2, "best"))),
    Chain("narrow", "narrow", 8, 9, 33, None, E0, None, "uniform", 7, _moves(400, (32, 8, "best"), (32, 8, "best"), (32, 8, "best"))),
    Chain("column", "column", 2, None, 17, None, E0, None, "uniform", 7, _moves(450, (12, 4, "best"), (12, 4, "best2"), (12, 4, "best"))),   # one-arm nodes carried
    Chain("crowded", "crowded", 6, 8, 97, None, E0, None, "uniform", 3, _moves(500, (48, 8, "best"), (48, 8, "best"), (48, 8, "best2"), (48, 8, "best"))),
    Chain("two_nodes", "default", 8, 5, 2, None, E0, None, "uniform", 0, _moves(600, (40, 4, "best"), (40, 4, "best"), (40, 4, "best"))),      # C = 2
    Chain("min_edges", "default", 8, 5, 129, "min", E0, None, "uniform", 3, _moves(700, (64, 4, "best"), (64, 4, "best"), (64, 4, "best"))),   # edges run out
    Chain("few_nodes", "default", 8, 5, 12, None, E0, None, "uniform", 1, _moves(800, (40, 8, "best"), (40, 8, "best"), (40, 8, "best"))),     # nodes run out
    Chain("capped", "small", 8, 6, 81, None, E0, 3, "uniform", 1,
          _moves(900, (40, 8, "best"), (40, 8, "best"), (40, 8, "best", 5), (40, 8, "best", 5))),          # the cap changes at the third move
    Chain("ids", "small", 8, 6, 49, None, E0, None, "uniform", 2**33, _moves(1000, (24, 8, "best"), (24, 8, "best2"), (24, 8, "best"))),
    # trees of several hundred nodes on two roots: a re-rooting over many chunks that keeps more than 256 nodes
    Chain("large", "default", 2, 5, 2048, None, 0, None, "uniform", 0, _moves(1100, (1000, 1, "best"), (100, 1, "best"), (100, 1, "best"))),
    # the decisive playout policy in a kept tree off the default grid: 12 columns (three count words) and a grid of run-time geometry
    Chain("wide_decisive", "wide", 4, 3, 129, None, E0, None, "decisive", 3, _moves(1200, (100, 2, "deep"), (40, 2, "deep"), (40, 2, "best"))),
    Chain("small_decisive", "small", 4, 6, 33, None, E0, None, "decisive", 1, _moves(1300, (16, 4, "best"), (16, 4, "best"), (16, 4, "best"))),
)
BY_NAME = {c.name: c for c in CHAINS}
# the game of BounceTreeSearchAgent(reuse=True) against a scripted reply (the most visited arm of its tree): seeds SEED, SEED + 1, ...,
# C = 2 T + 1, the default pool of 2 T iterations, from the start of the default grid, the default cap of 1024 plies
AGENT_STATES = 2
AGENT_CHAINS = (
    Chain("agent", "default", AGENT_STATES, None, 257, None, 8192, None, "uniform", 4,
          _moves(0, (128, 8, "best2"), (128, 8, "best2"), (128, 8, "best2"))),
)
ANCHORS = ("default", "pool", "narrow", "wide", "capped")     # the cases of search_bounce_expected a restart with C = T + 1 must reproduce


def chain_grid(chain):
    return GRIDS[chain.grid]


def chain_edges(chain):
    h, w = chain_grid(chain).shape
    return sb.min_edges(h, w) if chain.edges == "min" else sb.default_edges(h, w, chain.nodes - 1)


def chain_roots(chain):
    if chain.roots_seed is None:        # the start position
        orc = oracle.BounceOracle(chain_grid(chain), chain.n)
        return orc.grid.copy(), orc.player.copy(), orc.winner.copy(), orc.plies.astype(np.int32).copy()
    return _roots(chain.grid, chain.n, chain.roots_seed)


def move_max_plies(chain, move, roots):
    past = chain.cap if move.cap is None else move.cap
    return LONG if past is None else sb.short_cap(roots, past)


def _most_visited(root, h, w):
    played = [a for a in range(len(root.actions)) if root.n[a] > 0]
    return max(played, key=lambda a: (root.n[a], -a)) if played else None


def _ply(rule, forest, orc, best, reply):
    """(tree slots, board moves, index of the desynchronised board or -1) of one ply of `rule`"""
    h, w = forest.grid.shape
    n = orc.n
    tree = np.full(n, -1, dtype=np.int32)
    board = np.full((n, 4), -1, dtype=np.int32)
    desynced = -1
    for i in np.flatnonzero(orc.winner == -1):
        acts = orc.actions(int(i))
        if not acts:
            continue
        by_slot = {slot_of(a, h, w): a for a in acts}
        if reply and rule == "best2":
            root = forest.root(i)
            arm = None if root is None else _most_visited(root, h, w)
            action = acts[0] if arm is None else root.actions[arm]
        elif rule == "deep":
            root = forest.root(i)
            sizes = [0 if c is None else len(sb.all_nodes(c)) for c in root.child]
            action = root.actions[sizes.index(max(sizes))] if max(sizes) else by_slot[int(best[i])]
        elif rule == "high":
            action = acts[-1]
        else:
            action = by_slot[int(best[i])]
        tree[i] = slot_of(action, h, w)
        if rule == "desync" and not reply and desynced < 0 and len(acts) >= 2:
            desynced = int(i)
            action = next(a for a in acts if a != action)
        (sx, sy), (tx, ty) = action
        board[i] = (sx, sy, tx, ty)
    return tree, board, desynced


def run_chain(chain, roots):
    """(records, forest): a Record a move.  Record.roots are the boards the move searches"""
    grid = chain_grid(chain)
    g, player, winner, plies = roots
    n = g.shape[0]
    orc = oracle.BounceOracle(grid, n)
    orc.grid[:], orc.player[:], orc.winner[:], orc.plies[:] = g, player, winner, plies
    forest = Forest(grid, n, chain.nodes, chain_edges(chain))
    records = []
    for m, move in enumerate(chain.moves):
        before = (orc.grid.copy(), orc.player.copy(), orc.winner.copy(), orc.plies.astype(np.int32).copy())
        cap = move_max_plies(chain, move, roots)
        out = forest.search(before, move.seed, chain.first_game, move.iterations, move.playouts, chain.explore, cap, chain.policy,
                            restart=(m == 0))
        forest.check()
        plies_done, desynced = [], -1
        for reply in ((False, True) if move.rule == "best2" else (False,)):
            tree, board, d = _ply(move.rule, forest, orc, out[2], reply)
            desynced = d if d >= 0 else desynced
            kept = forest.advance(tree)
            forest.check()
            assert (kept <= out[3]).all()
            status = orc.step_actions(board)
            assert (status[board[:, 0] >= 0] == 0).all()
            plies_done.append((tree, board, kept))
        records.append(Record(before, cap, *out, plies_done, desynced))
    return records, forest


@functools.lru_cache(maxsize=None)
def chain_expected(name, agent=False):
    """run_chain of the chain of that name, once a session: read-only"""
    chain = AGENT_CHAINS[0] if agent else BY_NAME[name]
    return run_chain(chain, chain_roots(chain))


@functools.lru_cache(maxsize=None)
def anchor_expected(name, policy="uniform", spare=0):
    """(counts, visits, best, nodes, used, carried, env-steps) of a restart with C = T + 1 + spare and the case's pool on the
    case of search_bounce_expected.CASES of that name"""
    case = sb.BY_NAME[name]
    roots = sb.case_roots(case)
    forest = Forest(sb.case_grid(case), roots[0].shape[0], case.iterations + 1 + spare, sb.case_edges(case))
    return forest.search(roots, SEED, case.first_game, case.iterations, case.playouts, case.explore, sb.case_max_plies(case, roots),
                         policy, restart=True)
