"""What tests/search_prove_expected.py -- the CPU statement of bgs_connect_search_actions_proving and the case table of
tests/test_gpu_search_prove.py -- holds: the table reaches every branch the proving search adds, a root without a tag
is the plain search's, and every tag at a root is right, checked twice without the model's own bookkeeping: by a
certificate walk over the oracle's `legal` and `step`, and against the CPU solver of tests/solve_reference.py.  No GPU."""

import numpy as np
import pytest

from tests import search_expected as se
from tests import search_prove_expected as sp
from tests import solve_reference as sr


def _run(run):
    index, policy, per_ply = run
    return sp.CASES[index], sp.case_roots(sp.CASES[index]), sp.case_trees(index, per_ply, policy)[0], sp.case_expected(index, per_ply, policy)


def test_the_codes_are_the_solvers():
    assert (sp.SOLVE_NONE, sp.SOLVE_LOSS, sp.SOLVE_DRAW, sp.SOLVE_WIN, sp.SOLVE_UNKNOWN, sp.SOLVE_BUDGET) == (
        sr.NONE, sr.LOSS, sr.DRAW, sr.WIN, sr.UNKNOWN, sr.BUDGET)


def test_the_value_of_a_node():
    node = sp.ProvingNode(None, [True, True, False, True])
    assert node.legal == [0, 1, 3] and sp.value(node) == sp.OPEN             # a column never visited is OPEN
    node.tag = [sp.LOSS, sp.DRAW, sp.WIN, sp.OPEN]                            # (column 2 is illegal: its tag does not count)
    assert sp.value(node) == sp.OPEN
    node.tag[3] = sp.LOSS
    assert sp.value(node) == sp.DRAW
    node.tag[1] = sp.LOSS
    assert sp.value(node) == sp.LOSS
    node.tag[0] = sp.WIN
    assert sp.value(node) == sp.WIN
    node.tag[1] = sp.OPEN
    assert sp.value(node) == sp.WIN                                           # a win beats an open column


@pytest.mark.parametrize("run", sp.RUNS, ids=sp.run_id)
def test_every_tree_keeps_the_books(run):
    case, roots, trees, (counts, visits, best, nodes, proved, done, steps, seen) = _run(run)
    T, P = case.iterations, case.playouts
    running = roots[2] == -1
    assert roots[0].shape[0] <= 24 and T * P <= 1024
    np.testing.assert_array_equal(visits.sum(axis=1), done * P)               # every iteration run is P visits of the root
    assert (done[~running] == 0).all() and (done[running] >= 1).all() and (done <= T).all() and (nodes <= done).all()
    assert (proved[~running] == sp.SOLVE_NONE).all() and (best[~running] == -1).all() and (counts[~running] == 0).all()
    np.testing.assert_array_equal(counts.sum(axis=2), visits - seen["capped"])
    for i, root in enumerate(trees):
        if root is None:
            continue
        tags = {c: root.tag[c] for c in root.legal}
        assert all(proved[i, c] == sp.SOLVE_NONE for c in range(case.w) if c not in tags)
        assert all(proved[i, c] == sp.CODE[tag] for c, tag in tags.items())
        won = [c for c, tag in tags.items() if tag == sp.WIN]
        alive = [c for c, tag in tags.items() if tag != sp.LOSS]
        if won:
            assert won == [int(best[i])]
        elif alive:
            assert best[i] in alive and visits[i, best[i]] == visits[i, alive].max()
        else:
            assert visits[i, best[i]] == visits[i].max()
        if done[i] < T:                                                       # stopped: the root's value is not OPEN
            assert sp.value(root) != sp.OPEN
        # a tagged edge is never entered again: below a decided node nothing is OPEN-and-reachable through a tagged edge,
        # and every node's tagged columns are legal ones that were visited
        stack = [root]
        while stack:
            node = stack.pop()
            assert all(node.tag[c] == sp.OPEN for c in range(case.w) if c not in node.legal)
            assert all(node.n[c] >= P for c in node.legal if node.tag[c] != sp.OPEN)
            stack.extend(child for child in node.child if child is not None)


def test_the_table_reaches_every_branch():
    total = dict.fromkeys(sp.TALLIES, 0)
    tagged_undecided = untagged = 0
    for run in sp.RUNS:
        case, roots, trees, out = _run(run)
        proved, done, seen = out[4], out[5], out[7]
        for key in total:
            total[key] = max(total[key], seen[key]) if key in ("max_depth", "deepest_backup") else total[key] + seen[key]
        for i, root in enumerate(trees):
            if root is None:
                continue
            tags = _tags_below(root)
            untagged += int(tags == 0)
            tagged_undecided += int(tags > 0 and done[i] == case.iterations and sp.value(root) == sp.OPEN)
    print(total, "tagged and undecided", tagged_undecided, "untagged", untagged)
    assert total["decided_win"] >= 1 and total["decided_draw"] >= 1 and total["decided_loss"] >= 1
    assert total["deepest_backup"] >= 3                   # a fact that went up three levels in one step 7
    assert total["excluded_top"] >= 1                     # the exclusion changed a selection
    assert total["stopped_early"] >= 1 and total["tags_set"] >= 1 and total["capped_leaves"] >= 1
    assert tagged_undecided >= 1 and untagged >= 1
    assert {(c.w * (c.h + 1) + 63) // 64 for c in sp.CASES} == {1, 2, 3}
    assert {sp.CASES[j].playouts for j, _, _ in sp.RUNS} >= {1, 70}
    assert any(policy == "decisive" for _, policy, _ in sp.RUNS) and any(per_ply for _, _, per_ply in sp.RUNS)


def _tags_below(root):
    """the tagged edges of a whole tree"""
    total, stack = 0, [root]
    while stack:
        node = stack.pop()
        total += sum(tag != sp.OPEN for tag in node.tag)
        stack.extend(child for child in node.child if child is not None)
    return total


@pytest.mark.parametrize("run", sp.RUNS, ids=sp.run_id)
def test_a_root_without_a_tag_is_the_plain_search(run):
    """while no edge of a root's tree is tagged its state is the plain search's, bit for bit: the six outputs of such a
    root are tests/search_expected.py's four, the whole path of UNKNOWNs and done = T"""
    index, policy, per_ply = run
    case, roots, trees, (counts, visits, best, nodes, proved, done, _, _) = _run(run)
    plain = sp.plain_expected(index, per_ply, policy)
    for i, root in enumerate(trees):
        if root is None:
            for got, want in zip((counts, visits, best, nodes), plain[:4]):
                np.testing.assert_array_equal(got[i], want[i])
            continue
        if _tags_below(root):
            continue
        for got, want in zip((counts, visits, best, nodes), plain[:4]):
            np.testing.assert_array_equal(got[i], want[i], err_msg=f"root {i}")
        assert done[i] == case.iterations
        assert all(proved[i, c] == (sp.SOLVE_UNKNOWN if c in root.legal else sp.SOLVE_NONE) for c in range(case.w))


# ---- the certificate walk: the oracle's legal() and step() alone say whether a tag holds
def _certify(h, w, k, position, node, c, tag):
    mover = position[1]
    won, after = se._step(h, w, k, position, c)
    if won != -1:
        return (tag == sp.WIN and won == mover) or (tag == sp.DRAW and won == 2)
    child = node.child[c]
    if child is None:
        return False
    legal = [x for x in range(w) if se._legal(h, w, k, after)[x]]
    tags = [child.tag[x] for x in legal]
    if tag == sp.LOSS:                                    # the reply has a certified win
        return any(t == sp.WIN and _certify(h, w, k, after, child, x, sp.WIN) for x, t in zip(legal, tags))
    if tag == sp.WIN:                                     # every reply is a certified loss
        return bool(legal) and all(t == sp.LOSS and _certify(h, w, k, after, child, x, sp.LOSS) for x, t in zip(legal, tags))
    # DRAW: no reply is open or wins, one draws, and each is what it says
    return (bool(legal) and all(t in (sp.DRAW, sp.LOSS) for t in tags) and sp.DRAW in tags
            and all(_certify(h, w, k, after, child, x, t) for x, t in zip(legal, tags)))


@pytest.mark.parametrize("run", sp.RUNS, ids=sp.run_id)
def test_every_tag_at_a_root_has_a_certificate(run):
    case, roots, trees, out = _run(run)
    checked = 0
    for i, root in enumerate(trees):
        if root is None:
            continue
        position = (roots[0][i].copy(), int(roots[1][i]), int(roots[3][i]))
        for c in range(case.w):
            if root.tag[c] != sp.OPEN:
                assert _certify(case.h, case.w, case.k, position, root, c, root.tag[c]), (i, c, root.tag[c])
                checked += 1
    print(f"{sp.run_id(run)}: {checked} tags certified")


def test_tagged_columns_equal_the_cpu_solver():
    """every root with at most 12 empty cells: its tagged columns carry the full-depth code of tests/solve_reference.py;
    the table holds at least 6 such roots with a tag"""
    roots_with_a_tag = 0
    for run in sp.RUNS:
        case, roots, trees, out = _run(run)
        proved = out[4]
        empty = (roots[0] < 0).sum(axis=(1, 2))
        rows = np.flatnonzero((roots[2] == -1) & (empty <= sp.SOLVED_EMPTY))
        if rows.size == 0:
            continue
        codes, _ = sr.solve(case.h, case.w, case.k, tuple(a[rows] for a in roots), case.h * case.w)
        for j, i in enumerate(rows):
            tagged = np.flatnonzero((proved[i] != sp.SOLVE_UNKNOWN) & (proved[i] != sp.SOLVE_NONE))
            np.testing.assert_array_equal(proved[i, tagged], codes[j, tagged], err_msg=f"{sp.run_id(run)} root {i}")
            assert ((codes[j] == sr.NONE) == (proved[i] == sp.SOLVE_NONE)).all()
            roots_with_a_tag += int(tagged.size > 0)
    print("roots checked against the solver that hold a tag:", roots_with_a_tag)
    assert roots_with_a_tag >= 6


def test_two_shards_equal_the_whole():
    case = sp.CASES[1]
    roots = sp.case_roots(case)
    cut = roots[0].shape[0] // 2
    tail = (case.iterations, case.playouts, case.explore, se.UNCAPPED, False, "decisive")
    whole = sp.search_expected(case.h, case.w, case.k, roots, se.SEED, 100, *tail)
    lo = sp.search_expected(case.h, case.w, case.k, tuple(a[:cut] for a in roots), se.SEED, 100, *tail)
    hi = sp.search_expected(case.h, case.w, case.k, tuple(a[cut:] for a in roots), se.SEED, 100 + cut, *tail)
    for x, y, z in zip(lo[:6], hi[:6], whole[:6]):
        np.testing.assert_array_equal(np.concatenate([x, y]), z)
    assert lo[6] + hi[6] == whole[6]


def test_the_hand_made_roots_are_decided_as_they_were_made():
    names = [c.name for c in sp.CASES]
    hand = names.index("hand-3x5x3-T40-P4")
    *_, best, _, proved, done, _, _ = sp.case_expected(hand)
    T = sp.CASES[hand].iterations
    # root 1: a win in one, found by the expansion (column 0 is the lowest winning column): one iteration
    assert proved[1, 0] == sp.SOLVE_WIN and best[1] == 0 and done[1] == 1
    # root 2: every column loses in two
    assert (proved[2] == sp.SOLVE_LOSS).all() and 1 <= done[2] < T and best[2] >= 0
    # 2 x 2, no line fits: every root is decided, nothing wins or loses, the last empty cells force the draw
    small = names.index("hand-2x2x3-T24-P2")
    *_, proved, done, _, _ = sp.case_expected(small)
    assert (done < sp.CASES[small].iterations).all()
    assert np.isin(proved, (sp.SOLVE_DRAW, sp.SOLVE_NONE)).all() and (proved == sp.SOLVE_DRAW).any(axis=1).all()
    # 1 x 1 x 1: the first move wins
    *_, best, _, proved, done, _, _ = sp.case_expected(names.index("hand-1x1x1-T4-P3"))
    assert proved.tolist() == [[sp.SOLVE_WIN]] and best.tolist() == [0] and done.tolist() == [1]
