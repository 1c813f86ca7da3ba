"""The CPU statement of bgs_bounce_guided_step (include/bgs.h): Python trees over the oracle -- through
tests/search_bounce_expected.py's _actions, _step and slot_of --, the quantisation and the selection terms of
tests/guided_expected.py (value_sigma, q_term, e_term) with `prior_shares` over slots, and `fake_network_moves`, the fixed
host evaluator of tests/test_gpu_bounce_guided.py.  No GPU import; not a test module.

A GuidedMoves holds, per board, what a tree's share holds between two calls: the root Node (None: an emptied tree), the
nodes and the pool edges in use, the cap the tree was grown under and the pending leaf (its kind, its path of (node, arm)
pairs, the sigma of a TERMINAL leaf and the position of an EVALUATE leaf).  `step` is one call: check, apply, report,
select, in that order, board by board.  `seen` records what the runs met, for the coverage conditions of
tests/test_bounce_guided_expected.py."""

import numpy as np

from tests import guided_expected as ge
from tests.guided_expected import EVALUATE, FINISH, IDLE, MAX_VISITS, RESTART, TERMINAL, e_term, q_term, value_sigma  # noqa: F401
from tests.search_bounce_expected import MAX_PLIES, _actions, _step, min_edges, slot_of

MAX_NODES = 65536          # BGS_BOUNCE_FOREST_MAX_NODES
MAX_EDGES = 1 << 29        # BGS_BOUNCE_FOREST_MAX_EDGES
F32 = np.float32
NAMES = ("leaf_grid", "leaf_player", "leaf_kind", "leaf_targets", "visits", "scores", "best", "nodes", "used")


def default_edges(h, w, nodes):
    """the pool BounceBatch.guided_moves_search takes with edges=None"""
    return min_edges(h, w) + 32 * (nodes - 1)


# ---- the quantisation of the caller's rows
def prior_weights(row, legal):
    """w[slot] of the header for the legal slots of a leaf (a list of slots); row: float32[S]"""
    weights = {}
    for slot in legal:
        x = F32(row[slot])
        weights[slot] = int(np.floor(np.minimum(x, F32(1.0)) * F32(65536.0))) if x > 0 else 0     # (NaN > 0 is false)
    if sum(weights.values()) == 0:
        weights = {slot: 1 for slot in legal}
    return weights


def prior_shares(row, legal):
    """P of every legal slot, in the order of `legal`: floor(w * 65536 / W)"""
    weights = prior_weights(row, legal)
    total = sum(weights.values())
    return [(weights[slot] * 65536) // total for slot in legal]


def target_masks(actions, w):
    """uint64[w]: bit ty * w + tx of entry sx for every action, the layout of bgs_bounce_read_targets"""
    out = [0] * w
    for (sx, _), (tx, ty) in actions:
        out[sx] |= 1 << (ty * w + tx)
    return np.array(out, dtype=np.uint64)


class Node:
    def __init__(self, position, actions, h, w):
        a = len(actions)
        self.position = position            # (grid int8[h, w], player, plies) of a running board
        self.actions = actions              # [((sx, sy), (tx, ty))], canonical order: ascending slot
        self.slots = [slot_of(x, h, w) for x in actions]
        assert self.slots == sorted(self.slots)
        self.n, self.s, self.child, self.P = [0] * a, [0] * a, [None] * a, [0] * a
        self.edge = {}                      # a -> (winner after a, position after a), filled when the edge is first played


def new_seen():
    return {"made": 0, "refused_nodes": 0, "refused_edges": 0, "goal": 0, "blocked": 0, "draw": 0, "cap": 0, "max_depth": 0,
            "max_leaf_arms": 0, "evaluated": 0}


class GuidedMoves:
    def __init__(self, grid, n, nodes, edges=None, cpuct=320, max_plies=MAX_PLIES):
        h, w = grid.shape
        edges = default_edges(h, w, nodes) if edges is None else edges
        assert 2 <= nodes <= MAX_NODES and min_edges(h, w) <= edges <= MAX_EDGES and 0 <= cpuct <= 4096 and max_plies >= 1
        self.grid, self.h, self.w, self.n = grid, h, w, n
        self.nodes, self.edges, self.cpuct, self.cap = nodes, edges, cpuct, min(int(max_plies), MAX_PLIES)
        self.root = [None] * n              # the root Node of tree i; None: emptied
        self.count = [0] * n                # nodes in use, the root counted
        self.used = [0] * n                 # pool edges in use
        self.grown_under = [None] * n       # the cap the tree was emptied under
        self.expanded = [False] * n         # the root's arms have their P
        self.pending = [None] * n           # (kind, path, sigma of a TERMINAL leaf, (position, actions) of an EVALUATE leaf)
        self.restarts = [0] * n             # how often the tree was emptied
        self.made = []                      # (tree, node): every node made by an application, in order, for the tests
        self.seen = new_seen()

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
        """the arm the descent takes at `node`: the largest U, ties to the lowest arm"""
        total = min(sum(node.n), MAX_VISITS)
        u = [q_term(node.s[a], node.n[a]) + self.explore(node.P[a], total, node.n[a]) for a in range(len(node.actions))]
        return u.index(max(u))

    def step(self, roots, priors=None, values=None, flags=0, max_plies=None):
        """one call over `roots` (grid, player, winner, plies): the nine outputs in the order of NAMES.  max_plies: this
        call's cap, when it is not the one the object was made with"""
        h, w, n = self.h, self.w, self.n
        S = w * h * w
        assert flags in (0, RESTART, FINISH)
        cap = self.cap if max_plies is None else min(int(max_plies), MAX_PLIES)
        grid, player, winner, plies = roots
        assert grid.shape == (n, h, w)
        out_grid = grid.astype(np.int8).copy()
        out_player = (np.asarray(plies) & 1).astype(np.int8)
        out_kind = np.full(n, IDLE, dtype=np.int32)
        out_targets = np.zeros((n, w), dtype=np.uint64)
        visits = np.zeros((n, S), dtype=np.int32)
        scores = np.zeros((n, S), dtype=np.int32)
        best = np.full(n, -1, dtype=np.int32)
        nodes = np.zeros(n, dtype=np.int32)
        used = np.zeros(n, dtype=np.int32)
        priors = None if priors is None else np.asarray(priors).reshape(n, S)
        for i in range(n):
            # 1. the check
            root = self.root[i]
            position = (grid[i].copy(), int(player[i]), int(plies[i]))
            acts = _actions(self.grid, position) if winner[i] == -1 and plies[i] < MAX_PLIES else []
            live = (not flags & RESTART and bool(acts) and root is not None and 1 <= self.count[i] <= self.nodes
                    and len(acts) <= self.used[i] <= self.edges and np.array_equal(root.position[0], grid[i])
                    and root.position[2] == int(plies[i]) and self.grown_under[i] == cap)
            if not live:
                self.pending[i], self.expanded[i] = None, False
                self.restarts[i] += 1
                if acts:
                    self.root[i], self.count[i], self.used[i], self.grown_under[i] = Node(position, acts, h, w), 1, len(acts), cap
                else:
                    self.root[i], self.count[i], self.used[i], self.grown_under[i] = None, 0, 0, None
                root = self.root[i]
            # 2. the application
            if self.pending[i] is not None:
                kind, path, sigma, leaf = self.pending[i]
                self.pending[i] = None
                if kind == EVALUATE:
                    after, leaf_acts = leaf
                    leaf_slots = [slot_of(x, h, w) for x in leaf_acts]
                    shares = prior_shares(priors[i], leaf_slots)
                    sigma = value_sigma(values[i])
                    self.seen["evaluated"] += 1
                    if not path:
                        root.P = shares
                        self.expanded[i] = True
                    else:
                        parent, a = path[-1]
                        if parent.child[a] is None:
                            if self.count[i] >= self.nodes:
                                self.seen["refused_nodes"] += 1
                            elif self.used[i] + len(leaf_acts) > self.edges:
                                self.seen["refused_edges"] += 1
                            else:
                                node = Node(after, leaf_acts, h, w)
                                node.P = shares
                                parent.child[a] = node
                                self.count[i] += 1
                                self.used[i] += len(leaf_acts)
                                self.seen["made"] += 1
                                self.made.append((i, node))
                leaf_mover = (root.position[2] + len(path)) & 1
                for depth, (node, a) in enumerate(path):
                    node.n[a] += 1
                    node.s[a] = self.accumulate(node.s[a], self.credit(sigma, (node.position[2] & 1) == leaf_mover, depth))
            # 3. the report
            if root is not None:
                visits[i, root.slots], scores[i, root.slots] = root.n, root.s
                nodes[i], used[i] = self.count[i] - 1, self.used[i]
                ranked = sorted((a for a in range(len(root.slots)) if root.n[a] > 0), key=lambda a: (-root.n[a], -root.s[a], a))
                if ranked:
                    best[i] = root.slots[ranked[0]]
            # 4. the selection
            if root is None or flags & FINISH or self.stopped(sum(root.n)):
                continue
            if not self.expanded[i]:
                self.pending[i] = (EVALUATE, [], None, (root.position, root.actions))
                out_kind[i], out_targets[i] = EVALUATE, target_masks(root.actions, w)
                self.seen["max_leaf_arms"] = max(self.seen["max_leaf_arms"], len(root.actions))
                continue
            node, path = root, []
            while True:
                a = self.select(node)
                path.append((node, a))
                if a not in node.edge:
                    node.edge[a] = _step(self.grid, node.position, node.actions[a])
                won, after = node.edge[a]
                if won != -1:                               # the edge ends the game: its mover won, or a draw
                    goal = node.actions[a][1][1] in (0, h - 1)
                    self.seen["goal" if goal else ("draw" if won == 2 else "blocked")] += 1
                    assert won == 2 or won == (node.position[2] & 1)
                    self.pending[i] = (TERMINAL, path, 1024 if won == 2 else 0, None)
                    out_kind[i] = TERMINAL
                    break
                if after[2] >= cap:                         # the position runs and holds the cap: no node, now or later
                    assert node.child[a] is None
                    self.seen["cap"] += 1
                    self.pending[i] = (TERMINAL, path, 1024, None)
                    out_kind[i] = TERMINAL
                    break
                if node.child[a] is not None:
                    node = node.child[a]
                    continue
                leaf_acts = _actions(self.grid, after)
                assert leaf_acts                            # (a running position has a move: the oracle settles blocked sides)
                self.pending[i] = (EVALUATE, path, None, (after, leaf_acts))
                out_kind[i], out_targets[i] = EVALUATE, target_masks(leaf_acts, w)
                self.seen["max_leaf_arms"] = max(self.seen["max_leaf_arms"], len(leaf_acts))
                break
            self.seen["max_depth"] = max(self.seen["max_depth"], len(path))
            out_grid[i], out_player[i] = after[0], (root.position[2] + len(path)) & 1
        shape = (n, w, h * w)
        return out_grid, out_player, out_kind, out_targets, visits.reshape(shape), scores.reshape(shape), best, nodes, used

    def run(self, roots, evaluate, simulations, after_call=None):
        """GuidedMovesSearch.run: RESTART, simulations - 1 plain steps and FINISH, `evaluate` between them; returns every
        call's outputs.  after_call(number of the call, 0 for begin): called behind every call, for the tests that look at
        the trees"""
        calls = [self.step(roots, flags=RESTART)]
        if after_call:
            after_call(0)
        for t in range(simulations):
            priors, values = evaluate(calls[-1][0], calls[-1][1], calls[-1][3])
            calls.append(self.step(roots, priors, values, flags=FINISH if t == simulations - 1 else 0))
            if after_call:
                after_call(t + 1)
        return calls


def count_nodes(root):
    return 0 if root is None else sum(1 + count_nodes(ch) for ch in root.child if ch is not None)


def walk(root):
    if root is not None:
        yield root
        for child in root.child:
            yield from walk(child)


# ---- the fixed host evaluator
SPECIALS = ge.SPECIALS
SEEN = dict.fromkeys(SPECIALS, 0)       # how often fake_network_moves served each special row to a leaf with legal slots


def legal_slots(targets_row, h, w):
    """the legal slots of a leaf from its target masks uint64[w], ascending"""
    return [x * h * w + c for x in range(w) for c in range(h * w) if (int(targets_row[x]) >> c) & 1]


def fake_network_moves(grid, player, targets):
    """(priors float32[n, w, h * w], values float32[n]) of the leaves (grid int8[n, h, w], player int8[n], targets
    uint64[n, w]): exact float32 fractions k / 2^24 from guided_expected's integer hash of the grid, and on the same fixed
    schedule -- leaf hash mod 16 = 1 .. 8 -- the special rows of SPECIALS: a NaN, a negative and a +inf prior on a legal
    slot, an all-zero row, priors on illegal slots only, and the values 1.5, -3 and NaN.  A leaf without a legal slot (a
    TERMINAL or IDLE row, which the search ignores) keeps its plain row and is not counted in SEEN"""
    grid = np.asarray(grid)
    targets = np.asarray(targets).astype(np.uint64)
    n, h, w = grid.shape
    S = w * h * w
    key = ge.grid_hash(grid, player)
    with np.errstate(over="ignore"):
        per_slot = ge._mix(key[:, None] + np.arange(1, S + 1, dtype=np.uint64)[None, :] * np.uint64(0x9E3779B97F4A7C15))
        per_value = ge._mix(key ^ np.uint64(0xA5A5A5A5A5A5A5A5))
    priors = (per_slot >> np.uint64(40)).astype(np.float32) / F32(1 << 24)                    # k / 2^24, k < 2^24
    values = ((per_value >> np.uint64(40)).astype(np.int64) - (1 << 23)).astype(np.float32) / F32(1 << 23)   # [-1, 1)
    special = (key % np.uint64(16)).astype(np.int64)
    pick = (key >> np.uint64(8)).astype(np.uint64)
    for i in range(n):
        kind = special[i]
        if not 1 <= kind <= 8 or not targets[i].any():
            continue
        legal = legal_slots(targets[i], h, w)
        slot = legal[int(pick[i] % np.uint64(len(legal)))]
        name = SPECIALS[kind - 1]
        if name == "nan_prior":
            priors[i, slot] = np.nan
        elif name == "negative_prior":
            priors[i, slot] = -priors[i, slot] - F32(0.25)
        elif name == "inf_prior":
            priors[i, slot] = np.inf
        elif name == "zero_row":
            priors[i] = 0
        elif name == "illegal_only":
            priors[i, legal] = 0
        elif name == "value_high":
            values[i] = 1.5
        elif name == "value_low":
            values[i] = -3.0
        else:
            values[i] = np.nan
        SEEN[name] += 1
    return priors.reshape(n, w, h * w), values


def constant_network_moves(grid, player, targets):
    """uniform priors, value 0"""
    n, h, w = np.asarray(grid).shape
    return np.full((n, w, h * w), F32(1.0) / F32(w * h * w), dtype=np.float32), np.zeros(n, dtype=np.float32)


# ---- the runs of the GPU comparison (tests/test_gpu_bounce_guided.py), whose coverage tests/test_bounce_guided_expected.py
# asserts on this model: the six corner boards of tests/fuzz_cases.py with their roots (at most 20 a board), 48 simulations
SIMULATIONS = 48
NODES = SIMULATIONS + 1
CPUCT = {"16x4": 0, "5x12": 4096}         # one board each; 320 everywhere else
# (name, nodes, edges: None the default pool / "min" BGS_BOUNCE_SEARCH_MIN_EDGES, capped: the case's first max_plies)
SWEEPS = (("main", NODES, None, False), ("two_nodes", 2, None, False), ("three_nodes", 3, None, False),
          ("dry_pool", NODES, "min", False), ("capped", NODES, None, True))


def sweep_arguments(key, sweep):
    """(grid, roots, nodes, edges, cpuct, max_plies) of run (corner `key`, SWEEPS entry named `sweep`)"""
    from tests import fuzz_cases as fc

    case = fc.bounce_case(key)
    _, nodes, edges, capped = next(s for s in SWEEPS if s[0] == sweep)
    h, w = case.grid.shape
    edges = min_edges(h, w) if edges == "min" else default_edges(h, w, nodes)
    cpuct = CPUCT.get(key, 320) if sweep == "main" else 320
    return case.grid, case.roots, nodes, edges, cpuct, case.max_plies[0] if capped else MAX_PLIES


TREE_CALLS = (0, SIMULATIONS // 2, SIMULATIONS)       # the calls after which the GPU comparison reads the whole trees back


def run_with_trees(model, roots, evaluate, simulations, tree_calls=TREE_CALLS):
    """model.run, with model.trees[call] = every tree after call number `call` (0: begin) in the decoded form of
    tests/guided_shares.py"""
    from tests import guided_shares as gs       # (it imports this module)

    model.trees = {}

    def keep(call):
        if call in tree_calls:
            model.trees[call] = [gs.model_tree_bounce(model, i) for i in range(roots[0].shape[0])]

    return model.run(roots, evaluate, simulations, after_call=keep)


_SWEEPS_DONE = {}


def sweep_expected(key, sweep):
    """(the GuidedMoves, every call's outputs) of the run under fake_network_moves, computed once a session and shared:
    treat everything as read-only.  model.trees: the whole trees after the calls of TREE_CALLS"""
    if (key, sweep) not in _SWEEPS_DONE:
        grid, roots, nodes, edges, cpuct, max_plies = sweep_arguments(key, sweep)
        model = GuidedMoves(grid, roots[0].shape[0], nodes, edges, cpuct, max_plies)
        before = dict(SEEN)
        calls = run_with_trees(model, roots, fake_network_moves, SIMULATIONS)
        model.served = {name: SEEN[name] - before[name] for name in SPECIALS}     # the special rows this run was fed
        _SWEEPS_DONE[key, sweep] = (model, calls)
    return _SWEEPS_DONE[key, sweep]
