"""The CPU statement of bgs_connect_forest_search / bgs_connect_forest_advance (include/bgs.h), built on
tests/search_expected.py (Node, select, the oracle's step, legal columns and playouts), and the chains of
tests/test_gpu_forest.py.  No GPU import; not a test module.

A Forest holds a persistent Python tree per board: the root Node (None: an emptied tree) and the nodes in use.  `search`
makes the carried check of the header, empties the trees that fail it and runs the iterations of
search_expected.search_trees with step 4 read as the forest reads it: a node is made when the edge has no child and the
tree holds fewer than `capacity` nodes; the playouts start from the position after the edge either way.  `advance`
re-roots a tree at the child of the root's edge, or empties it.

A CHAIN is a list of moves over one set of roots.  A move is (seed, T, P, rule): every tree is searched, then every
running board advances its tree and steps its board by the columns the rule gives (one ply or two), so boards end along
the way.  run_chain records, move by move, the roots, the expected outputs and the columns: the GPU test replays them."""

import functools
from collections import namedtuple

import numpy as np

from oracle import oracle
from tests import search_expected as se
from tests.search_expected import Node, _legal, _play, _step, select

SEED = se.SEED
MASK64 = se.MASK64


class Forest:
    def __init__(self, h, w, k, n, capacity):
        assert capacity >= 2
        self.h, self.w, self.k, self.n, self.capacity = h, w, k, n, capacity
        self.root = [None] * n          # the root Node of tree i; None: emptied
        self.count = [0] * n            # nodes in use, the root counted
        self.refused = 0                # edges taken whose node did not fit
        self.replayed = 0               # ... of them, edges that had been refused before

    def search(self, roots, seed, first_game, iterations, leaf_playouts, explore, max_plies, per_ply=False, policy="uniform",
               restart=False):
        """(counts, visits, best, nodes, carried, env-steps) of one launch over `roots` (grid, player, winner, plies)"""
        h, w, k, n = self.h, self.w, self.k, self.n
        T, P = iterations, leaf_playouts
        assert T >= 1 and P >= 1 and T * P <= se.MAX_PLAYOUTS and 0 <= explore <= se.MAX_EXPLORE
        grid, player, winner, plies = roots
        assert grid.shape[0] == n
        carried = np.zeros(n, dtype=np.int64)
        for i in range(n):
            root = self.root[i]
            keep = (not restart and winner[i] == -1 and root is not None and np.array_equal(root.position[0], grid[i])
                    and sum(root.n) + T * P < 2**31)
            if keep:
                carried[i] = self.count[i] - 1
            elif winner[i] != -1:
                self.root[i], self.count[i] = None, 0
            else:
                position = (grid[i].copy(), int(player[i]), int(plies[i]))
                self.root[i], self.count[i] = Node(position, _legal(h, w, k, position)), 1
        counts = np.zeros((n, w, 3), dtype=np.int64)
        steps = 0
        seen = dict.fromkeys(("selections", "tied_selections"), 0)
        late = [set() for _ in range(n)]    # the edges of tree i whose node did not fit in this launch
        for t in range(T):
            paths, leaves, ids, owner, outcome = {}, [], [], [], {}
            for i in range(n):
                if self.root[i] is None:
                    continue
                node, path = self.root[i], []
                while True:
                    c = select(node, explore, seen)
                    path.append((node, c))
                    if c not in node.edge:
                        node.edge[c] = _step(h, w, k, node.position, c)
                    won, after = node.edge[c]
                    if won != -1:                               # the edge ends the game: P playouts with that outcome
                        outcome[i] = [won] * P
                        break
                    if node.child[c] is None:                   # no node for the position after c: one is made if it fits
                        if self.count[i] < self.capacity:
                            node.child[c] = Node(after, _legal(h, w, k, after))
                            self.count[i] += 1
                        else:
                            self.refused += 1
                            self.replayed += int((id(node), c) in late[i])
                            late[i].add((id(node), c))
                        if after[2] >= max_plies:               # capped at once: no game, every playout scores 0
                            outcome[i] = [-1] * P
                        else:
                            for j in range(P):
                                leaves.append(after)
                                ids.append((((first_game + i) * T + t) * P + j) & MASK64)
                                owner.append(i)
                        break
                    node = node.child[c]
                paths[i] = path
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
                for node, c in path:
                    node.n[c] += P
                    node.s[c] += 2 * tally[node.position[1]] + tally[2]
        visits = np.zeros((n, w), dtype=np.int64)
        best = np.full(n, -1, dtype=np.int64)
        nodes = np.zeros(n, dtype=np.int64)
        for i, root in enumerate(self.root):
            if root is None:
                continue
            visits[i] = root.n
            best[i] = sorted(root.legal, key=lambda c: (-root.n[c], -root.s[c], c))[0]
            nodes[i] = self.count[i] - 1
            assert nodes[i] == se.count_nodes(root)
        return tuple(a.astype(np.int32) for a in (counts, visits, best, nodes, carried)) + (steps,)

    def advance(self, columns):
        """kept int32[n]: re-root tree i at the child of its root's edge columns[i], or empty it; a negative column leaves it"""
        kept = np.zeros(self.n, dtype=np.int32)
        for i, c in enumerate(np.asarray(columns).tolist()):
            root = self.root[i]
            if c >= 0:
                child = root.child[c] if root is not None and c < self.w else None
                self.root[i] = child
                self.count[i] = 0 if child is None else 1 + se.count_nodes(child)
            kept[i] = max(self.count[i] - 1, 0)
        return kept


# ---- chains.  Rules, for every running board (an ended board gets -1, -1):
#   "best"     one ply: the search's best column for the tree and for the board;
#   "best2"    two plies: best, then the reply -- the most visited column of the new root (ties: the lowest), or the lowest
#              legal column where the tree was emptied by the first ply;
#   "high"     one ply: the highest legal column (never played when T is below the number of legal columns);
#   "desync"   as "best", but the board of the first running root with two legal columns steps by another column than
#              its tree advances by: the next search must start that tree anew.
Move = namedtuple("Move", "seed iterations playouts rule")
Chain = namedtuple("Chain", "h w k capacity explore cap policy per_ply first_game moves take", defaults=(None,))   # take: the first roots only
Record = namedtuple("Record", "roots counts visits best nodes carried steps plies desynced")   # plies: [(tree columns, board columns, kept)]


def _moves(base, *steps):
    return tuple(Move((SEED + base + m) & MASK64, t, p, rule) for m, (t, p, rule) in enumerate(steps))


CHAINS = (
    Chain(6, 7, 4, 97, 65536, None, "uniform", False, 5, _moves(100, (48, 16, "best"), (48, 16, "best2"), (48, 16, "best"), (48, 16, "best"))),
    Chain(6, 7, 4, 12, 65536, None, "decisive", False, 0, _moves(200, (20, 8, "best"), (20, 8, "best"), (20, 8, "best"))),      # full trees
    Chain(6, 7, 4, 25, 65536, 3, "uniform", False, 1 << 33, _moves(300, (12, 70, "best"), (12, 70, "desync"), (12, 70, "best"))),  # capped
    Chain(5, 6, 3, 129, 65536, None, "uniform", True, 0, _moves(400, (64, 8, "best2"), (64, 8, "best"), (64, 8, "best"), (64, 8, "best"))),
    Chain(2, 5, 3, 2, 65536, None, "uniform", False, 0, _moves(500, (40, 4, "best"), (40, 4, "high"), (40, 4, "best"))),           # C = 2
    Chain(6, 12, 4, 49, 65536, None, "uniform", False, 0, _moves(600, (24, 16, "best"), (24, 16, "best2"), (24, 16, "best")), 12),  # two words
    Chain(12, 13, 5, 33, 65536, None, "decisive", False, 0, _moves(700, (4, 8, "high"), (16, 8, "best"), (16, 8, "best")), 8),       # three words
    # trees of several hundred nodes on two roots: a re-rooting over many chunks that keeps more than a chunk's nodes
    Chain(6, 7, 4, 1024, 65536, None, "uniform", False, 0, _moves(800, (700, 1, "best"), (150, 1, "best"), (150, 1, "best")), 2),
)
# the self-play games of TreeSearchAgent(reuse=True): seeds SEED, SEED + 1, ..., capacity 2 T + 1, from the start position
AGENT_STATES = 3
AGENT_CHAINS = (
    Chain(6, 7, 4, 65, 40000, None, "uniform", False, 4, _moves(0, (32, 16, "best"), (32, 16, "best"), (32, 16, "best2"), (32, 16, "best"))),
)
ANCHORS = (0, 2, 9, 10)          # the cases of search_expected a restart with C = T + 1 must reproduce


def chain_id(chain):
    text = f"{chain.h}x{chain.w}x{chain.k}-C{chain.capacity}-" + "+".join(f"T{m.iterations}P{m.playouts}{m.rule}" for m in chain.moves)
    text += f"-{chain.policy}" + ("-per-ply" if chain.per_ply else "") + ("-capped" if chain.cap is not None else "")
    return text + (f"-{chain.take}roots" if chain.take else "")


def chain_roots(chain):
    roots = se._case_roots(chain.h, chain.w, chain.k)
    return roots if chain.take is None else tuple(a[:chain.take] for a in roots)


def start_roots(chain, n):
    orc = oracle.ConnectOracle(chain.h, chain.w, chain.k, n)
    return orc.grid.copy(), orc.player.copy(), orc.winner.copy(), orc.plies.copy()


def chain_max_plies(chain, roots):
    if chain.cap is None:
        return se.UNCAPPED
    return int(np.median(roots[3][roots[2] == -1])) + chain.cap


def _columns(rule, forest, orc, best, reply):
    """(tree columns, board columns, index of the desynchronised board or -1) of one ply of `rule`"""
    n = orc.n
    running = orc.winner == -1
    legal = orc.legal().astype(bool)
    tree = np.full(n, -1, dtype=np.int32)
    desynced = -1
    for i in np.flatnonzero(running):
        if reply:
            root = forest.root[i]
            played = [] if root is None else [c for c in root.legal if root.n[c] > 0]
            tree[i] = max(played, key=lambda c: (root.n[c], -c)) if played else int(np.flatnonzero(legal[i])[0])
        elif rule == "high":
            tree[i] = int(np.flatnonzero(legal[i])[-1])
        else:
            tree[i] = best[i]
    board = tree.copy()
    if rule == "desync" and not reply:
        desynced = int(next(i for i in np.flatnonzero(running) if legal[i].sum() >= 2))
        board[desynced] = next(c for c in np.flatnonzero(legal[desynced]) if c != tree[desynced])
    return tree, board, desynced


def run_chain(chain, roots):
    """(records, forest): a Record a move.  Record.roots are the boards the move searches"""
    grid, player, winner, plies = roots
    n = grid.shape[0]
    orc = oracle.ConnectOracle(chain.h, chain.w, chain.k, n, per_ply=chain.per_ply)
    orc.grid[:], orc.player[:], orc.winner[:], orc.plies[:] = grid, player, winner, plies
    cap = chain_max_plies(chain, roots)
    forest = Forest(chain.h, chain.w, chain.k, n, chain.capacity)
    records = []
    for m, move in enumerate(chain.moves):
        before = (orc.grid.copy(), orc.player.copy(), orc.winner.copy(), orc.plies.astype(np.int32).copy())
        out = forest.search(before, move.seed, chain.first_game, move.iterations, move.playouts, chain.explore, cap, chain.per_ply,
                            chain.policy, restart=(m == 0))
        steps, desynced = [], -1
        for reply in ((False, True) if move.rule == "best2" else (False,)):
            tree, board, d = _columns(move.rule, forest, orc, out[2], reply)
            desynced = d if d >= 0 else desynced
            kept = forest.advance(tree)
            status = orc.step_actions(board)
            assert (status[board >= 0] == 0).all()
            steps.append((tree, board, kept))
        records.append(Record(before, *out, steps, desynced))
    return records, forest


@functools.lru_cache(maxsize=None)
def chain_expected(index, agent=False):
    """run_chain of CHAINS[index] (AGENT_CHAINS[index] from the start position), once a session: read-only"""
    chain = AGENT_CHAINS[index] if agent else CHAINS[index]
    return run_chain(chain, start_roots(chain, AGENT_STATES) if agent else chain_roots(chain))


@functools.lru_cache(maxsize=None)
def anchor_expected(index, per_ply=False, policy="uniform"):
    """(counts, visits, best, nodes, carried, env-steps) of a restart with C = T + 1 on search_expected.CASES[index]"""
    case = se.CASES[index]
    roots = se.case_roots(case)
    forest = Forest(case.h, case.w, case.k, roots[0].shape[0], case.iterations + 1)
    return forest.search(roots, SEED, case.first_game, case.iterations, case.playouts, case.explore, se.case_max_plies(case, roots),
                         per_ply, policy, restart=True)
