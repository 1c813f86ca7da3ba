"""CPU-only checks of tests/guided_shares.py: the codec of the guided trees' shares, the validity of the primed trees, and
four mutants of the CPU statements -- each a wrong version of one rule, a subclass of the statement with that rule's method
replaced -- that the new comparisons of tests/test_gpu_guided_fuzz.py must tell from the statement.  A mutant plays the
device's part: it runs on its own leaves, and its outputs and trees are compared with the statement's as the GPU test
compares the device's.

The plans (PLANS in tests/guided_shares.py): `stop` primes a root to 2^19 - 3 visits, so that the last selecting call
has (N + 1) << 12 = 2^31 and the next finds the root stopped; `squares` to 700^2 - 3, so that N + 1 crosses a perfect
square; `extremes` to 400000 with one root arm at s = 2048 n and one at s = 0, the top-up at sigma = 2048.

Every statement a mutant is compared with is computed by the unchanged classes, and a mutant is a class of its own that
runs outside the caches of tests/guided_fuzz_cases.py: no test here depends on another having run, and nothing a mutant
computed is ever shared."""

import math

import numpy as np
import pytest

from tests import bounce_guided_expected as bg
from tests import guided_expected as ge
from tests import guided_fuzz_cases as gf
from tests import guided_shares as gs

GEOMETRIES_CONNECT = gs.PRIMED_CONNECT[:3]        # NW = 1, 2, 3
GEOMETRIES_BOUNCE = gs.PRIMED_BOUNCE[:3]          # 9x6, 8x8, 4x16


# ---- the codec
def test_the_share_lengths_are_the_kernels():
    assert gs.connect_share_words(6, 7, 49) == (16 + 42 + 49 * 28 + 63) // 64 * 64
    assert gs.connect_share_words(1, 1, 2) == 64 and gs.connect_share_words(15, 12, 1 << 20) == (16 + 180 + (48 << 20) + 63) // 64 * 64
    assert gs.bounce_share_words(49, 252 + 32 * 48) == (32 + 4 * (252 + 32 * 48) + 3 * 49 + 63) // 64 * 64
    assert gs.bounce_share_words(2, 1) == 64


@pytest.mark.parametrize("key", GEOMETRIES_CONNECT)
def test_the_connect_codec_round_trips(key):
    h, w, k, roots, capacity, _ = gf.primed_connect_arguments(key, "squares")
    nw = (w * (h + 1) + 63) // 64
    model, _, before, after = gf.primed_connect(key, "squares")
    final = [gs.model_tree_connect(model, i) for i in range(model.n)]
    pending = 0
    for tree in before + after + final:
        share = gs.encode_connect(tree, h, w, nw, capacity)
        assert share.dtype == np.uint32 and share.shape == (gs.connect_share_words(h, w, capacity),)
        assert gs.decode_connect(share, h, w, nw, capacity) == tree
        np.testing.assert_array_equal(gs.encode_connect(gs.decode_connect(share, h, w, nw, capacity), h, w, nw, capacity, into=share), share)
        other = gs.encode_connect(tree, h, w, nw, capacity, into=np.zeros_like(share))
        gs.assert_same_tree(gs.decode_connect(other, h, w, nw, capacity), tree, key)
        # nothing is written beyond what is in use: the nodes beyond the count, the path beyond its length
        used = 16 + h * w + 4 * w * tree["count"]
        assert (share[used:] == gs.POISON).all() and (share[16 + tree["depth"]: 16 + h * w] == gs.POISON).all()
        pending += tree["kind"] != gs.NONE
    assert pending > 0 and any(t["kind"] == gs.EVALUATE and t["depth"] > 0 for t in before)
    assert all(t["kind"] == gs.NONE for t in final)


@pytest.mark.parametrize("key", GEOMETRIES_BOUNCE)
def test_the_bounce_codec_round_trips(key):
    grid, roots, nodes, _ = gf.primed_bounce_arguments(key, "squares")
    edges = bg.default_edges(*grid.shape, nodes)
    model, _, before, after = gf.primed_bounce(key, "squares")
    final = [gs.model_tree_bounce(model, i) for i in range(model.n)]
    for tree in before + after + final:
        share = gs.encode_bounce(tree, nodes, edges)
        assert share.dtype == np.uint32 and share.shape == (gs.bounce_share_words(nodes, edges),)
        assert gs.decode_bounce(share, nodes, edges) == tree
        np.testing.assert_array_equal(gs.encode_bounce(gs.decode_bounce(share, nodes, edges), nodes, edges, into=share), share)
        other = gs.encode_bounce(tree, nodes, edges, into=np.zeros_like(share))
        gs.assert_same_tree(gs.decode_bounce(other, nodes, edges), tree, key)
        assert (share[24:32] == gs.POISON).all() and (share[32 + 4 * tree["used"]: 32 + 4 * edges] == gs.POISON).all()
        assert (share[32 + 4 * edges + 2 * tree["count"]: 32 + 4 * edges + 2 * nodes] == gs.POISON).all()
        assert (share[32 + 4 * edges + 2 * nodes + tree["depth"]:] == gs.POISON).all()
        # the tree is well formed: every node's block inside the edges in use, the root's first, blocks back to back
        assert [first for first, _ in tree["table"]] == list(np.cumsum([0] + [arms for _, arms in tree["table"]])[:-1])
        assert sum(arms for _, arms in tree["table"]) == tree["used"]
    assert any(t["kind"] != gs.NONE and t["depth"] > 0 for t in before)
    sentinels = sum(e["child"] >= gs.EDGE_ENDED for t in final for e in t["edges"])
    children = sum(0 < e["child"] < gs.EDGE_ENDED for t in final for e in t["edges"])
    print(key, "sentinels", sentinels, "children", children)
    assert sentinels > 0 and children > 0


def test_the_comparison_sees_every_defined_word_and_no_other():
    model, _, before, _ = gf.primed_connect("8x8x6", "squares")
    tree = next(t for t in before if t["kind"] == gs.EVALUATE and t["depth"] > 1 and t["count"] > 2)
    for change in (lambda t: t["nodes"][2]["s"].__setitem__(3, t["nodes"][2]["s"][3] + 1),
                   lambda t: t["nodes"][1]["child"].__setitem__(0, t["nodes"][1]["child"][0] ^ 1),
                   lambda t: t["nodes"][2]["P"].__setitem__(7, 5), lambda t: t["path"].__setitem__(1, (0, 0)),
                   lambda t: t.__setitem__("legal", t["legal"] ^ 1), lambda t: t.__setitem__("expanded", 0)):
        other = {**tree, "nodes": [{k: list(v) for k, v in node.items()} for node in tree["nodes"]], "path": list(tree["path"])}
        change(other)
        with pytest.raises(AssertionError, match="differs"):
            gs.assert_same_tree(other, tree, "changed")
    idle = {**tree, "kind": gs.WON}
    gs.assert_same_tree({**idle, "legal": 77}, idle, "legal bits of a TERMINAL leaf")
    model, _, before, _ = gf.primed_bounce("default", "squares")
    tree = next(t for t in before if t["kind"] == gs.EVALUATE and t["depth"] > 1)
    for name in ("n", "s", "child", "P", "source", "target"):
        other = {**tree, "edges": [dict(e) for e in tree["edges"]]}
        other["edges"][-1][name] += 1
        with pytest.raises(AssertionError, match="differs"):
            gs.assert_same_tree(other, tree, name)
    with pytest.raises(AssertionError, match="differs"):
        gs.assert_same_tree({**tree, "leaf_ply": tree["leaf_ply"] + 1}, tree, "leaf_ply")
    ended = {**tree, "kind": gs.FULL}
    gs.assert_same_tree({**ended, "leaf_ply": 9, "leaf_planes": [1, 2, 3, 4]}, ended, "the leaf of a TERMINAL kind")


# ---- the primed trees
PRIMED = [("connect", key, plan) for plan in gs.PLANS for key in gs.PRIMED_CONNECT] + \
         [("bounce", key, plan) for plan in gs.PLANS for key in gs.PRIMED_BOUNCE]


def primed(game, key, plan, statement=None):
    run = gf.primed_connect if game == "connect" else gf.primed_bounce
    return run(key, plan) if statement is None else run.__wrapped__(key, plan, statement)


def totals(game, call):
    return call[3].sum(axis=1) if game == "connect" else call[4].sum(axis=(1, 2))


@pytest.mark.parametrize("game,key,plan", PRIMED, ids=lambda x: str(x))
def test_a_primed_tree_is_a_state_of_the_statement(game, key, plan):
    model, calls, before, after = primed(game, key, plan)
    assert any(model.primed) and len(calls) == 1 + gs.PRIMED_BEFORE + gs.PRIMED_AFTER
    for i, (x, y) in enumerate(zip(before, after)):
        gs.assert_valid_priming(x, y)
        blocks = [n["n"] for n in y["nodes"]] if game == "connect" else [[e["n"] for e in y["edges"][f: f + a]] for f, a in y["table"]]
        if model.primed[i]:
            assert sum(blocks[0]) == gs.PLANS[plan].target and x["expanded"] == 1 and x["kind"] != gs.NONE
        else:
            assert x == y and (not blocks or sum(blocks[0]) == 0)
    was = np.array(model.primed)
    assert (calls[gs.PRIMED_BEFORE][2][was] != ge.IDLE).all() and (totals(game, calls[gs.PRIMED_BEFORE])[was] == gs.PRIMED_BEFORE - 1).all()
    handed = [(call[2][was] != ge.IDLE) for call in calls[gs.PRIMED_BEFORE + 1:]]
    if plan == "stop":       # leaves on exactly two more calls, then idle, the root at 2^19 visits and unchanged
        assert [bool(x.all()) for x in handed] == [True, True] + [False] * (gs.PRIMED_AFTER - 2) and not any(x.any() for x in handed[2:])
        for call in calls[gs.PRIMED_BEFORE + 3:]:
            assert (totals(game, call)[was] == 1 << 19).all()
            for j in (3, 4) if game == "connect" else (4, 5):
                np.testing.assert_array_equal(call[j], calls[gs.PRIMED_BEFORE + 3][j])
    else:
        assert all(x.all() for x in handed[:-1]) and not handed[-1].any()
        assert (totals(game, calls[-1])[was] == gs.PLANS[plan].target + gs.PRIMED_AFTER).all()
    if plan == "squares":    # N + 1 crosses 700^2 during the calls
        assert gs.PLANS[plan].target + 1 < 700 * 700 <= gs.PLANS[plan].target + gs.PRIMED_AFTER
    if plan == "extremes":   # q at 4096 and at 0 beside large n; score rows near 2^30
        scores = calls[-1][4 if game == "connect" else 5]
        assert 1 << 28 < scores.max() < 1 << 30                 # (float32 holds integers exactly up to 2^24)
        for i, tree in enumerate(after):
            if model.primed[i]:
                arms = [(n, s) for n, s in zip(tree["nodes"][0]["n"], tree["nodes"][0]["s"])] if game == "connect" else \
                       [(e["n"], e["s"]) for e in tree["edges"][: tree["table"][0][1]]]
                assert any(n > 0 and s == 2048 * n for n, s in arms)
                assert sum(n > 0 for n, _ in arms) < 2 or any(n > 0 and s == 0 for n, s in arms)


# ---- the mutants
def trees_differ(game, model, other):
    tree_of, defined = (gs.model_tree_connect, gs.defined_connect) if game == "connect" else (gs.model_tree_bounce, gs.defined_bounce)
    return any(defined(tree_of(model, i)) != defined(tree_of(other, i)) for i in range(model.n))


def differs(game, statement, mutant):
    """the comparison of a primed run: every call's outputs, and the whole trees at the end"""
    (model, calls), (other, got) = statement[:2], mutant[:2]
    return any(not np.array_equal(a, b) for x, y in zip(calls, got) for a, b in zip(x, y)) or trees_differ(game, model, other)


def mutants(**rules):
    """(a Guided, a GuidedMoves) with `rules` in place of the statement's methods of those names"""
    return type("MutantGuided", (ge.Guided,), rules), type("MutantGuidedMoves", (bg.GuidedMoves,), rules)


def caught(plan, classes):
    """per game: the cases of `plan` on which the mutant differs from the statement"""
    out = {}
    for game, keys, cls in (("connect", gs.PRIMED_CONNECT, classes[0]), ("bounce", gs.PRIMED_BOUNCE, classes[1])):
        assert cls not in (ge.Guided, bg.GuidedMoves)
        out[game] = [key for key in keys if differs(game, primed(game, key, plan), primed(game, key, plan, cls))]
    return out


def test_the_stop_plan_catches_a_stop_tested_with_greater():
    found = caught("stop", mutants(stopped=staticmethod(lambda total: total > ge.MAX_VISITS)))
    assert found == {"connect": list(gs.PRIMED_CONNECT), "bounce": list(gs.PRIMED_BOUNCE)}      # a third leaf, on every case


def signed_e_term(cpuct, share, total, n):
    x = ((total + 1) << 12) & 0xFFFFFFFF
    x = x - (1 << 32) if x >= 1 << 31 else x                # (N + 1) << 12 as a signed 32-bit value
    root = math.isqrt(x) if x >= 0 else 0                   # (the square root of a negative float is NaN, as an integer 0)
    return ((cpuct * share * root) >> 19) // (1 + n)


def test_the_stop_plan_catches_a_signed_square_root_argument():
    assert signed_e_term(320, 4000, 1000, 7) == ge.e_term(320, 4000, 1000, 7)
    assert signed_e_term(320, 4000, (1 << 19) - 2, 7) == ge.e_term(320, 4000, (1 << 19) - 2, 7)
    assert signed_e_term(320, 4000, (1 << 19) - 1, 7) == 0 < ge.e_term(320, 4000, (1 << 19) - 1, 7)
    found = caught("stop", mutants(explore=lambda self, share, total, n: signed_e_term(self.cpuct, share, total, n)))
    print(found)
    # (not on the boards of one column: their only arm is taken whatever U is)
    assert found["connect"] and found["bounce"]


def test_the_extremes_plan_catches_scores_summed_in_float32():
    found = caught("extremes", mutants(accumulate=staticmethod(lambda s, x: int(np.float32(s) + np.float32(x)))))
    print(found)
    # (not on every case: where every leaf ends the game, as on the 4x16 and 7x1 Bounce boards, the scores are multiples of
    # 1024, which float32 adds exactly up to 2^34)
    assert found["connect"] and found["bounce"]


def test_the_whole_tree_comparison_catches_a_wrong_perspective_three_edges_down():
    connect, bounce = mutants(credit=staticmethod(lambda sigma, own, depth: sigma if own or depth >= 2 else 2048 - sigma))
    found = {"connect": [key for key in range(gf.CONNECT_CASES) if trees_differ("connect", gf.connect_expected(key)[0], gf.run_connect(key, connect)[0])],
             "bounce": [key for key in range(gf.BOUNCE_CASES) if trees_differ("bounce", gf.bounce_expected(key)[0], gf.run_bounce(key, bounce)[0])]}
    print(found)
    assert found["connect"] and found["bounce"]
    # ... and only there: the mutant is the statement on every key whose paths stay above three edges
    for keys, run in ((found["connect"], gf.connect_expected), (found["bounce"], gf.bounce_expected)):
        assert all(run(key)[0].facts["max_depth"] >= 3 for key in keys)


def test_a_header_word_beyond_its_range_is_seen():
    """the decoders keep the header words as they are: a count or a path length beyond the capacity is not a full tree's"""
    model, _, before, _ = gf.primed_connect("8x8x6", "squares")
    h, w, k, roots, capacity, _ = gf.primed_connect_arguments("8x8x6", "squares")
    tree = next(t for t in before if t["depth"] > 0)
    share = gs.encode_connect(tree, h, w, 2, capacity)
    for word, name in ((0, "count"), (2, "depth")):
        bad = share.copy()
        bad[word] = 0xA5A5A5A5
        with pytest.raises(AssertionError, match=name):
            gs.assert_same_tree(gs.decode_connect(bad, h, w, 2, capacity), tree, "poisoned header")
    grid, roots, nodes, _ = gf.primed_bounce_arguments("default", "squares")
    edges = bg.default_edges(*grid.shape, nodes)
    tree = next(t for t in gf.primed_bounce("default", "squares")[2] if t["depth"] > 0)
    share = gs.encode_bounce(tree, nodes, edges)
    for word, name in ((0, "count"), (1, "used"), (13, "depth")):
        bad = share.copy()
        bad[word] = 0xA5A5A5A5
        with pytest.raises(AssertionError, match=name):
            gs.assert_same_tree(gs.decode_bounce(bad, nodes, edges), tree, "poisoned header")
