"""The CPU statement of bgs_connect_guided_advance (include/bgs.h) on top of tests/guided_expected.Guided, and the scripted
games that tests/test_guided_advance_expected.py (CPU) and tests/test_gpu_guided_advance.py (MI355X) play with it.  No GPU
import; not a test module.

`GuidedAdvance.advance(columns) -> kept` is the header's text, tree by tree.  The new root leaves `made`, so that
tests/guided_shares.model_tree_connect lists it once, as node 0, and the rest in the order it was made: what a
compaction that keeps the order gives.

A scripted game (`play`) is a list of moves over one set of roots: a search (`begin` on the first move, `resume` on the
later ones, then plain steps and `finish`, under an evaluator), an advance by columns chosen on the CPU from the
statement's own trees -- KINDS says what a column can be --, and the boards stepped by the columns that can be played.
Everything the device must reproduce is recorded: every call's outputs, every tree after `finish` and after `advance`,
`kept`, the columns and their kinds."""

import functools
from collections import namedtuple

import numpy as np

from oracle import oracle
from tests import fuzz_cases as fc
from tests import guided_expected as ge
from tests import guided_shares as gs
from tests.search_expected import _legal, _step

ADVANCE_MAX_CAPACITY = 65536

# what the column of an advance can be, seen from the tree it meets
KINDS = ("best",            # the root's most visited column, and it has a child: the subtree is kept
         "child",           # another column with a child
         "untouched",       # c < 0
         "never_played",    # a legal column without a visit
         "full_column",     # a column without room
         "width",           # c = width
         "wins",            # an edge that wins: terminal, no child
         "fills",           # an edge that fills the board: terminal, no child
         "did_not_fit",     # a visited edge to a running position whose node found no room
         "empty")           # c >= 0 on a tree that is empty already (an ended board, or emptied before)
REQUIRED = ("best", "untouched", "never_played", "full_column", "width", "wins", "fills")


class GuidedAdvance(ge.Guided):
    def __init__(self, h, w, k, n, capacity, cpuct):
        super().__init__(h, w, k, n, capacity, cpuct)
        assert capacity <= ADVANCE_MAX_CAPACITY

    def empty(self, i):
        self.root[i], self.count[i], self.pending[i], self.expanded[i], self.applied[i] = None, 0, None, False, 0

    def advance(self, columns):
        """kept int32[n]; the boards are not looked at"""
        assert len(columns) == self.n
        kept = np.zeros(self.n, dtype=np.int32)
        for i, c in enumerate(int(x) for x in columns):
            root = self.root[i]
            if c < 0:                                       # untouched, a pending leaf included
                kept[i] = self.count[i] - 1 if root is not None else 0
                continue
            child = None
            if root is not None and 1 <= self.count[i] <= self.capacity and c < self.w and root.position[0][self.h - 1, c] == -1:
                child = root.child[c]
            if child is None:                               # anything else: emptied
                self.empty(i)
                continue
            at = next(j for j, (t, node) in enumerate(self.made) if node is child)
            assert self.made[at][0] == i
            del self.made[at]
            # a plain drop by the side to move: the position the child was made for
            dropped = root.position[0].copy()
            dropped[int((dropped[:, c] != -1).sum()), c] = root.position[2] & 1
            assert np.array_equal(dropped, child.position[0])
            self.root[i], self.count[i], self.pending[i], self.expanded[i] = child, ge.count_nodes(child) + 1, None, True
            kept[i] = self.count[i] - 1
        return kept


def count_tree(root):
    """the nodes of a tree, the root counted"""
    return 0 if root is None else 1 + ge.count_nodes(root)


def stepped(h, w, k, roots, columns):
    """`roots` (grid, player, winner, plies) after `columns` (negative: the board stays), by the oracle"""
    orc = oracle.ConnectOracle(h, w, k, roots[0].shape[0])
    orc.grid[:], orc.player[:], orc.winner[:], orc.plies[:] = roots
    assert (orc.step_actions(np.asarray(columns, dtype=np.int32))[np.asarray(columns) >= 0] == 0).all()
    return orc.grid.copy(), orc.player.copy(), orc.winner.copy(), orc.plies.copy()


def playable(h, w, roots, columns):
    """`columns` where the board runs and the column has room, -1 elsewhere: what the boards can be stepped by"""
    grid, _, winner, _ = roots
    out = np.full(len(columns), -1, dtype=np.int32)
    for i, c in enumerate(int(x) for x in columns):
        if 0 <= c < w and winner[i] == -1 and grid[i][h - 1, c] == -1:
            out[i] = c
    return out


def column_kinds(model, i):
    """{kind: column} for tree i of the statement: what an advance could be given there"""
    h, w, k = model.h, model.w, model.k
    root = model.root[i]
    if root is None:
        return {"untouched": -1, "empty": 0}
    found = {"untouched": -1, "width": w}
    order = sorted(range(w), key=lambda c: (-root.n[c], -root.s[c], c))
    legal = _legal(h, w, k, root.position)
    for c in order:
        if not legal[c]:
            found.setdefault("full_column", c)
            continue
        won, _ = _step(h, w, k, root.position, c)
        if won in (0, 1):
            found.setdefault("wins", c)
        elif won == 2:
            found.setdefault("fills", c)
        elif root.child[c] is not None:
            found.setdefault("best" if c == order[0] and root.n[c] > 0 else "child", c)
        elif root.n[c] == 0:
            found.setdefault("never_played", c)
        else:
            found.setdefault("did_not_fit", c)
    return found


# the order in which tree i of move m looks for a kind it can be given: rotated by 3 * i + m, so that neighbours differ
WISHES = ("best", "untouched", "wins", "best", "never_played", "fills", "best", "full_column", "child", "width", "best", "did_not_fit",
          "empty")


def choose_columns(model, move):
    columns, kinds = np.zeros(model.n, dtype=np.int32), []
    for i in range(model.n):
        found = column_kinds(model, i)
        at = (3 * i + move) % len(WISHES)
        kind = next(kind for kind in WISHES[at:] + WISHES[:at] if kind in found)
        columns[i] = found[kind]
        kinds.append(kind)
    return columns, kinds


Move = namedtuple("Move", "roots calls finished columns kinds kept advanced played")


def decoded(model):
    return [gs.model_tree_connect(model, i) for i in range(model.n)]


def search(model, roots, evaluate, simulations, carry):
    """every call's outputs of GuidedForest.run(evaluate, simulations, carry): begin or resume, steps, finish"""
    zeros = np.zeros((model.n, model.w), dtype=np.float32), np.zeros(model.n, dtype=np.float32)
    calls = [model.step(roots, *zeros, flags=0) if carry else model.step(roots, flags=ge.RESTART)]
    for t in range(simulations):
        priors, values = evaluate(calls[-1][0], calls[-1][1])
        calls.append(model.step(roots, priors, values, flags=ge.FINISH if t == simulations - 1 else 0))
    return calls


def play(h, w, k, roots, capacity, simulations, moves, evaluate=ge.fake_network, cpuct=320, columns_of=choose_columns):
    """(the statement, [Move]): `moves` times search, advance by columns_of(model, move) -> (columns, kinds), step the boards
    by the columns that can be played"""
    model = GuidedAdvance(h, w, k, roots[0].shape[0], capacity, cpuct)
    script = []
    for m in range(moves):
        calls = search(model, roots, evaluate, simulations, carry=m > 0)
        finished = decoded(model)
        columns, kinds = columns_of(model, m)
        kept = model.advance(columns)
        played = playable(h, w, roots, columns)
        script.append(Move(roots, calls, finished, columns, kinds, kept, decoded(model), played))
        roots = stepped(h, w, k, roots, played)
    return model, script


# ---- the corner games of tests/test_gpu_guided_advance.py
CORNERS = ("15x1x4", "1x16x2", "11x16x5", "8x8x6", "2x2x3", "6x7x4")
SIMULATIONS, MOVES, ROOTS = 24, 4, 12
CAPACITIES = (3, SIMULATIONS + 1, 2 * SIMULATIONS + 1)


def corner_geometry(key):
    return (6, 7, 4) if key == "6x7x4" else fc.CONNECT_CORNERS[key][:3]


@functools.lru_cache(maxsize=None)
def corner_roots(key):
    """at most ROOTS roots of the corner at different plies: a board one move from its end and an ended board first (where
    the corner's roots hold them), then a spread of the rest"""
    h, w, k = corner_geometry(key)
    roots = fc.connect_roots(h, w, k, np.random.default_rng(97000 + CORNERS.index(key))) if key == "6x7x4" else fc.connect_case(key).roots
    n = roots[0].shape[0]
    ending = []
    for i in np.flatnonzero(roots[2] == -1):
        position = (roots[0][i], int(roots[1][i]), int(roots[3][i]))
        if any(_step(h, w, k, position, c)[0] != -1 for c in np.flatnonzero(_legal(h, w, k, position))):
            ending.append(int(i))
    ended = [int(i) for i in np.flatnonzero(roots[2] != -1)]
    first = ending[:3] + ended[:1]
    rest = [int(i) for i in fc._spread(n, ROOTS) if i not in first]
    return fc.take(roots, np.array((first + rest)[:ROOTS], dtype=np.int64)), len(ending[:3]), len(ended[:1])


@functools.lru_cache(maxsize=None)
def corner_game(key, capacity):
    h, w, k = corner_geometry(key)
    return play(h, w, k, corner_roots(key)[0], capacity, SIMULATIONS, MOVES)


# ---- the chunk boundaries: Connect4, 2 roots, about 300 simulations, capacity 301
CHUNK_SIMULATIONS, CHUNK_CAPACITY = 300, 301


def narrow_network(grid, player):
    """a prior that sits on one column -- the lowest with room --, 1 / 80 of it on the others, value 0: a deep chain of nodes
    made one after the other, and siblings that get their first visit only when the favoured column holds 80 (with Q equal
    everywhere, E(c) is proportional to P[c] / (1 + n[c])): nodes made late, with children made later still"""
    grid = np.asarray(grid)
    n, h, w = grid.shape
    priors = np.full((n, w), 1.0 / 80, dtype=np.float32)
    for i in range(n):
        room = np.flatnonzero(grid[i, h - 1] == -1)
        if room.size:
            priors[i, room[0]] = 1.0
    return priors, np.zeros(n, dtype=np.float32)


CHUNK_EVALUATORS = {"fake": ge.fake_network, "narrow": narrow_network}


def new_root_index(tree, column):
    """the index the root's child of `column` has in a decoded tree (0: none)"""
    return tree["nodes"][0]["child"][column] if tree["count"] and 0 <= column < len(tree["nodes"][0]["child"]) else 0


def chunk_columns(model, move):
    """tree 0: the column whose subtree is the largest; tree 1: among the children whose node index is 64 or more the one
    with the largest subtree, and without such a child the one with the highest index"""
    trees = decoded(model)
    columns = np.full(model.n, -1, dtype=np.int32)
    for i, tree in enumerate(trees):
        root = model.root[i]
        with_child = [c for c in range(model.w) if root is not None and root.child[c] is not None]
        if not with_child:
            continue
        if i == 0:
            columns[i] = max(with_child, key=lambda c: (count_tree(root.child[c]), -c))
        else:
            late = [c for c in with_child if new_root_index(tree, c) >= 64]
            columns[i] = (max(late, key=lambda c: (count_tree(root.child[c]), -c)) if late else
                          max(with_child, key=lambda c: (new_root_index(tree, c), -c)))
    return columns, ["child" if c >= 0 else "untouched" for c in columns]


@functools.lru_cache(maxsize=None)
def chunk_game(evaluator):
    orc = oracle.ConnectOracle(6, 7, 4, 2)
    orc.step_actions(np.int32([3, -1]))
    roots = orc.grid.copy(), orc.player.copy(), orc.winner.copy(), orc.plies.copy()
    return play(6, 7, 4, roots, CHUNK_CAPACITY, CHUNK_SIMULATIONS, 2, evaluate=CHUNK_EVALUATORS[evaluator], columns_of=chunk_columns)
