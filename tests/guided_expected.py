"""The CPU statement of bgs_connect_guided_step (include/bgs.h): Python trees over the oracle's `legal` and `step_actions`
(through tests/search_expected.py's _legal and _step), the quantisation of the caller's rows with np.float32 operations
exactly as the header words them, and `fake_network`, the fixed host evaluator of tests/test_gpu_guided.py.  No GPU
import; not a test module.

A Guided holds, per board, what a tree's share holds between two calls: the root Node (None: an emptied tree), the nodes
in use and the pending leaf (its kind, its path of (node, column) pairs and, for an EVALUATE leaf, its position and legal
columns).  `step` is one call: check, apply, report, select, in that order, board by board."""

import math

import numpy as np

from tests.search_expected import _legal, _step

RESTART, FINISH = 1, 2
EVALUATE, TERMINAL, IDLE = 0, 1, 2
MAX_CAPACITY = 1 << 20
MAX_VISITS = 1 << 19
F32 = np.float32


# ---- the quantisation of the caller's rows
def prior_weights(row, legal):
    """w[c] of the header for the legal columns of a leaf (a list of columns); row: float32[width]"""
    weights = {}
    for c in legal:
        x = F32(row[c])
        weights[c] = int(np.floor(np.minimum(x, F32(1.0)) * F32(65536.0))) if x > 0 else 0     # (NaN > 0 is false)
    if sum(weights.values()) == 0:
        weights = {c: 1 for c in legal}
    return weights


def prior_shares(row, legal, width):
    """P[c] for every column: floor(w[c] * 65536 / W), 0 for an illegal column"""
    weights = prior_weights(row, legal)
    total = sum(weights.values())
    return [(weights[c] * 65536) // total if c in weights else 0 for c in range(width)]


def value_sigma(x):
    """sigma = 1024 + v of the header; x: one float32"""
    x = F32(x)
    if np.isnan(x):
        return 1024
    x = np.minimum(np.maximum(x, F32(-1.0)), F32(1.0))
    return 1024 + int(x * F32(1024.0))          # (int: truncated toward zero)


def q_term(s, n):
    return (2 * s) // n if n else 2048


def e_term(cpuct, share, total, n):
    return ((cpuct * share * math.isqrt((total + 1) << 12)) >> 19) // (1 + n)


class Node:
    def __init__(self, position, legal):
        w = len(legal)
        self.position = position            # (grid int8[h, w], player, plies) of a running board
        self.legal = [c for c in range(w) if legal[c]]
        self.n, self.s, self.child, self.P = [0] * w, [0] * w, [None] * w, [0] * w
        self.edge = {}                      # c -> (winner after c, position after c), filled when the edge is first played


class Guided:
    def __init__(self, h, w, k, n, capacity, cpuct):
        assert 2 <= capacity <= MAX_CAPACITY and 0 <= cpuct <= 4096
        self.h, self.w, self.k, self.n, self.capacity, self.cpuct = h, w, k, n, capacity, cpuct
        self.root = [None] * n              # the root Node of tree i; None: emptied
        self.count = [0] * n                # nodes in use, the root counted
        self.expanded = [False] * n         # the root has its P
        self.pending = [None] * n           # (kind, path, sigma of a TERMINAL leaf, position of an EVALUATE leaf, its legal columns)
        self.applied = [0] * n              # applied leaves that were not the root, since the tree was last emptied
        self.made = []                      # (tree, node): every node made by an application, for the tests
        self.refused = 0                    # EVALUATE leaves whose node did not fit

    # the four rules below are methods so that tests/test_guided_shares.py can state a wrong version of each
    @staticmethod
    def stopped(total):
        """the root selects nothing once it holds this many visits"""
        return total >= MAX_VISITS

    @staticmethod
    def credit(sigma, own, depth):
        """what edge `depth` of the path (0: the root's) receives: own, the edge's mover is the leaf's"""
        return sigma if own else 2048 - sigma

    @staticmethod
    def accumulate(s, x):
        return s + x

    def explore(self, share, total, n):
        return e_term(self.cpuct, share, total, n)

    def select(self, node):
        """the column the descent takes at `node`: the largest U, ties to the lowest column"""
        total = sum(node.n[c] for c in node.legal)
        u = [q_term(node.s[c], node.n[c]) + self.explore(node.P[c], total, node.n[c]) for c in node.legal]
        return node.legal[u.index(max(u))]

    def step(self, roots, priors=None, values=None, flags=0):
        """one call over `roots` (grid, player, winner, plies): (leaf_grid int8[n, h, w], leaf_player int8[n], leaf_kind
        int32[n], visits int32[n, w], scores int32[n, w], best int32[n], nodes int32[n])"""
        h, w, k, n = self.h, self.w, self.k, self.n
        assert flags in (0, RESTART, FINISH)
        grid, player, winner, plies = roots
        assert grid.shape == (n, h, w)
        out_grid = grid.astype(np.int8).copy()
        out_player = (np.asarray(plies) & 1).astype(np.int8)         # (ply & 1: the mover of a running board)
        out_kind = np.full(n, IDLE, dtype=np.int32)
        visits = np.zeros((n, w), dtype=np.int32)
        scores = np.zeros((n, w), dtype=np.int32)
        best = np.full(n, -1, dtype=np.int32)
        nodes = np.zeros(n, dtype=np.int32)
        for i in range(n):
            # 1. the check
            root = self.root[i]
            live = (not flags & RESTART and winner[i] == -1 and root is not None and 1 <= self.count[i] <= self.capacity
                    and np.array_equal(root.position[0], grid[i]))
            if not live:
                self.pending[i], self.expanded[i], self.applied[i] = None, False, 0
                if winner[i] != -1:
                    self.root[i], self.count[i] = None, 0
                else:
                    position = (grid[i].copy(), int(player[i]), int(plies[i]))
                    self.root[i], self.count[i] = Node(position, _legal(h, w, k, position)), 1
                root = self.root[i]
            # 2. the application
            if self.pending[i] is not None:
                kind, path, sigma, position, legal = self.pending[i]
                self.pending[i] = None
                if kind == EVALUATE:
                    shares = prior_shares(priors[i], legal, w)
                    sigma = value_sigma(values[i])
                    if not path:
                        root.P = shares
                        self.expanded[i] = True
                    else:
                        parent, c = path[-1]
                        if parent.child[c] is None and self.count[i] < self.capacity:
                            node = Node(position, [c in legal for c in range(w)])
                            node.P = shares
                            parent.child[c] = node
                            self.count[i] += 1
                            self.made.append((i, node))
                        elif parent.child[c] is None:
                            self.refused += 1
                if path:
                    self.applied[i] += 1
                leaf_mover = (root.position[2] + len(path)) & 1
                for depth, (node, c) in enumerate(path):
                    node.n[c] += 1
                    node.s[c] = self.accumulate(node.s[c], self.credit(sigma, (node.position[2] & 1) == leaf_mover, depth))
            # 3. the report
            if root is not None:
                visits[i], scores[i] = root.n, root.s
                nodes[i] = self.count[i] - 1
                if sum(root.n) > 0:
                    best[i] = sorted(range(w), key=lambda c: (-root.n[c], -root.s[c], c))[0]
            # 4. the selection
            if root is None or flags & FINISH or self.stopped(sum(root.n)):
                continue
            if not self.expanded[i]:
                self.pending[i] = (EVALUATE, [], None, root.position, list(root.legal))
                out_kind[i] = EVALUATE
                continue
            node, path = root, []
            while True:
                c = self.select(node)
                path.append((node, c))
                if c not in node.edge:
                    node.edge[c] = _step(h, w, k, node.position, c)
                won, after = node.edge[c]
                if won != -1:                               # the leaf ended the game: the last edge won, or filled the board
                    self.pending[i] = (TERMINAL, path, 1024 if won == 2 else 0, None, None)
                    out_kind[i] = TERMINAL
                    break
                if node.child[c] is None:
                    legal = _legal(h, w, k, after)
                    self.pending[i] = (EVALUATE, path, None, after, [x for x in range(w) if legal[x]])
                    out_kind[i] = EVALUATE
                    break
                node = node.child[c]
            out_grid[i], out_player[i] = after[0], (root.position[2] + len(path)) & 1
        return out_grid, out_player, out_kind, visits, scores, best, nodes

    def run(self, roots, evaluate, simulations, after_call=None):
        """GuidedSearch.run: RESTART, simulations - 1 plain steps and FINISH, `evaluate` between them; returns every call's
        outputs.  after_call(number of the call, 0 for begin): called behind every call, for the tests that look at the trees"""
        calls = [self.step(roots, flags=RESTART)]
        if after_call:
            after_call(0)
        for t in range(simulations):
            priors, values = evaluate(calls[-1][0], calls[-1][1])
            calls.append(self.step(roots, priors, values, flags=FINISH if t == simulations - 1 else 0))
            if after_call:
                after_call(t + 1)
        return calls


def count_nodes(root):
    return 0 if root is None else sum(1 + count_nodes(ch) for ch in root.child if ch is not None)


# ---- the fixed host evaluator
SPECIALS = ("nan_prior", "negative_prior", "inf_prior", "zero_row", "illegal_only", "value_high", "value_low", "value_nan")
SEEN = dict.fromkeys(SPECIALS, 0)       # how often fake_network injected each special row, for the tests
_MASK = (1 << 64) - 1


def _mix(x):
    """splitmix64's finaliser on uint64 arrays"""
    with np.errstate(over="ignore"):
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return x ^ (x >> np.uint64(31))


def grid_hash(grid, player):
    """uint64[n]: an integer hash of every (grid, player)"""
    n = grid.shape[0]
    cells = (grid.reshape(n, -1).astype(np.int64) + 2).astype(np.uint64)
    coef = _mix(np.arange(1, cells.shape[1] + 1, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)) | np.uint64(1)
    with np.errstate(over="ignore"):
        return _mix((cells * coef[None, :]).sum(axis=1, dtype=np.uint64) + np.asarray(player).astype(np.uint64) * np.uint64(0xD1B54A32D192ED03))


def fake_network(grid, player):
    """(priors float32[n, w], values float32[n]) of the leaves (grid int8[n, h, w], player int8[n]): exact float32
    fractions k / 2^24 from an integer hash of the grid, and on a fixed schedule -- leaf hash mod 16 = 1 .. 8 -- the
    special rows of SPECIALS: a NaN prior, a negative prior, +inf, an all-zero row, priors only on illegal columns (full
    ones; where there is none the row stays as it is), and the values 1.5, -3 and NaN"""
    grid = np.asarray(grid)
    n, h, w = grid.shape
    key = grid_hash(grid, player)
    with np.errstate(over="ignore"):
        per_column = _mix(key[:, None] + np.arange(1, w + 1, dtype=np.uint64)[None, :] * np.uint64(0x9E3779B97F4A7C15))
        per_value = _mix(key ^ np.uint64(0xA5A5A5A5A5A5A5A5))
    priors = (per_column >> np.uint64(40)).astype(np.float32) / F32(1 << 24)                  # k / 2^24, k < 2^24
    values = ((per_value >> np.uint64(40)).astype(np.int64) - (1 << 23)).astype(np.float32) / F32(1 << 23)   # [-1, 1)
    special = (key % np.uint64(16)).astype(np.int64)
    column = ((key >> np.uint64(8)) % np.uint64(w)).astype(np.int64)
    full = grid[:, h - 1, :] != -1
    for i in range(n):
        kind = special[i]
        if not 1 <= kind <= 8:
            continue
        name = SPECIALS[kind - 1]
        if name == "nan_prior":
            priors[i, column[i]] = np.nan
        elif name == "negative_prior":
            priors[i, column[i]] = -priors[i, column[i]] - F32(0.25)
        elif name == "inf_prior":
            priors[i, column[i]] = np.inf
        elif name == "zero_row":
            priors[i] = 0
        elif name == "illegal_only":
            if not full[i].any():
                continue
            priors[i, ~full[i]] = 0
        elif name == "value_high":
            values[i] = 1.5
        elif name == "value_low":
            values[i] = -3.0
        else:
            values[i] = np.nan
        SEEN[name] += 1
    return priors, values


def constant_network(grid, player):
    """uniform priors, value 0"""
    n, _, w = np.asarray(grid).shape
    return np.full((n, w), F32(1.0) / F32(w), dtype=np.float32), np.zeros(n, dtype=np.float32)
