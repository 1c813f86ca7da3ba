"""The exact Bounce solver (bgs_bounce_solve_moves, BounceBatch.solve_moves, SolverAgent on Bounce states) against the CPU
reference of tests/solve_reference_bounce.py, bit for bit: codes and plies of every slot of every position.

Everything here needs a real MI355X: `pytest -m gpu`.
"""

import ctypes
import functools

import numpy as np
import pytest

from oracle import oracle
from tests import game_trees as gt
from tests import solve_reference_bounce as ref
from tests.test_gpu_parity import BOUNCE_GRIDS
from tests.test_spec_exhaustive import BOUNCE_CONFIGS, BOUNCE_WALKS

pytestmark = pytest.mark.gpu

MAX_DEPTH = 16          # BGS_BOUNCE_SOLVE_MAX_DEPTH
BUDGET = 1 << 22        # no position of the small grids or of the shallow horizons here comes near it
SEED = 0xB0A2CE501E
DEFAULT = BOUNCE_GRIDS["default"]


def concat(layers):
    return tuple(np.concatenate([l[j] for l in layers]) for j in range(4))


@functools.lru_cache(maxsize=None)
def walk(name):
    cfg = np.array(BOUNCE_CONFIGS[name], dtype=np.int8)
    pos = concat([layer for _, layer, _ in gt.bounce_layers(cfg, max_depth=BOUNCE_WALKS[name][0])])
    assert pos[0].shape[0] == BOUNCE_WALKS[name][1]
    return cfg, pos


def load(cfg, pos, use_torch=None):
    from simulator.batch import BounceBatch

    b = BounceBatch(cfg, pos[0].shape[0], use_torch=use_torch)
    assert (b.write_state(pos[0], pos[1], pos[2], pos[3]) == 0).all()
    return b


def random_roots(grid, per, plies_list, seed):
    """distinct running positions of `per` oracle games after each of `plies_list` random plies"""
    out = []
    for plies in plies_list:
        orc = oracle.BounceOracle(grid, per)
        for _ in range(plies):
            orc.step_random(seed + plies)
        out.append((orc.grid.copy(), orc.player.copy(), orc.winner.copy(), orc.plies.copy()))
    pos = concat(out)
    pos = gt._take(pos, np.flatnonzero(pos[2] == -1))
    return gt._take(pos, gt._unique_rows(pos[0], pos[1]))


def assert_same(got, want, what):
    (codes, plies), (want_c, want_p) = got, want
    bad = np.flatnonzero((codes != want_c).any(axis=(1, 2)) | (plies != want_p).any(axis=(1, 2)))
    if bad.size:
        i = bad[0]
        at = np.argwhere((codes[i] != want_c[i]) | (plies[i] != want_p[i]))[:6]
        detail = [(tuple(a), int(codes[i][tuple(a)]), int(want_c[i][tuple(a)]), int(plies[i][tuple(a)]), int(want_p[i][tuple(a)])) for a in at]
        raise AssertionError(f"{what}: {bad.size} boards differ, first {i}: (slot, code, want, plies, want) {detail}")


# ---- 1. every position of the exhaustive walks.  The documented maximum horizon where the CPU reference stays
# affordable: the three full graphs (a layer never holds more than the graph's positions); the "small" walk's layers at
# depth 16 would each approach its 151 120 positions, one Python call a position.
@pytest.mark.parametrize("name", list(BOUNCE_CONFIGS))
def test_exact_on_every_walked_position(name):
    cfg, pos = walk(name)
    b = load(cfg, pos)
    for depth in (1, 2, 3, 4) + (() if name == "small" else (MAX_DEPTH,)):
        got = b.solve_moves(depth=depth, max_nodes=BUDGET)
        assert not (got[0] == ref.BUDGET).any()
        assert_same(got, ref.solve(cfg, pos, depth), f"{name} depth {depth}")
    b.close()


# ---- 1b. the deepest stack together with the refill from the queue: depth 16 on the "small" walk (more reply tasks than
# a wave has lanes, fewer waves a CU) under a small budget.  The reference is affordable to depth 4 here; a deeper
# horizon never changes a WIN / LOSS or its plies, so wherever the depth-16 search stayed inside its budget it must
# repeat every depth-4 WIN / LOSS, and every WIN / LOSS it finds within 4 plies must be the depth-4 answer.
def test_deepest_stack_under_a_budget():
    cfg, pos = walk("small")
    want_c, want_p = ref.solve(cfg, pos, 4)
    b = load(cfg, pos)
    codes, plies = b.solve_moves(depth=MAX_DEPTH, max_nodes=200)
    b.close()
    hit = codes == ref.BUDGET
    assert hit.any() and (plies[hit] == 0).all()
    np.testing.assert_array_equal(codes == ref.NONE, want_c == ref.NONE)
    np.testing.assert_array_equal(codes == ref.DRAW, want_c == ref.DRAW)
    decided = np.isin(want_c, [ref.WIN, ref.LOSS]) & ~hit
    assert decided.sum() > 10000
    np.testing.assert_array_equal(codes[decided], want_c[decided])
    np.testing.assert_array_equal(plies[decided], want_p[decided])
    short = np.isin(codes, [ref.WIN, ref.LOSS]) & (plies <= 4)
    np.testing.assert_array_equal(codes[short], want_c[short])
    np.testing.assert_array_equal(plies[short], want_p[short])
    assert (np.isin(codes, [ref.WIN, ref.LOSS]) & (plies > 4)).any()   # and the deep levels were really used


# ---- 2. the packed grids of the parity tests, 12 and 8 columns among them.  Sized by the CPU reference (it walks the
# oracle one position a Python call).  Roots / positions expanded at depth 3 / seconds for depths 1-3, measured on the
# development host: default 88 / 31 019 / 6.5 s; small 27 / 293 / 0.3 s; big_values 22 / 2 574 / 0.8 s; crowded 121 / 1 462 /
# 0.4 s; wide 27 / 34 075 / 15.6 s; narrow and blocked_start: no game runs for 4 plies, the start position stands in.
# crowded's set (the reference's answer over depths 1-3): LOSS, DRAW and UNKNOWN with plies 0-3 but only a handful of WINs
# -- its games are decided by stalemates, not goal landings -- so the full class mix is asserted on the four grids below
# and crowded's own set is pinned to what it holds: LOSS and UNKNOWN.
GAMES = {"crowded": 256, "wide": 64}   # games a ply count (32 elsewhere): few games of these two grids run for long


@pytest.mark.parametrize("name", list(BOUNCE_GRIDS))
def test_exact_on_packed_grids(name):
    grid = BOUNCE_GRIDS[name]
    pos = random_roots(grid, GAMES.get(name, 32), (4, 10, 16, 24), SEED)
    if pos[0].shape[0] == 0:   # narrow, blocked_start: no game runs for 4 plies; the start position (blocked_start's is
        orc = oracle.BounceOracle(grid, 3)   # settled at reset: every slot NONE)
        pos = (orc.grid.copy(), orc.player.copy(), orc.winner.copy(), orc.plies.copy())
    b = load(grid, pos)
    classes, lengths = set(), set()
    for depth in (1, 2, 3):
        want = ref.solve(grid, pos, depth)
        assert_same(b.solve_moves(depth=depth, max_nodes=BUDGET), want, f"{name} depth {depth}")
        classes |= set(np.unique(want[0]).tolist())
        lengths |= set(np.unique(want[1]).tolist())
    b.close()
    if name in ("default", "small", "big_values", "wide"):
        # on the reference's answer: the comparison above cannot have passed on an empty class
        assert {ref.WIN, ref.LOSS, ref.UNKNOWN, ref.NONE} <= classes, classes
        assert {1, 2, 3} <= lengths, lengths
    if name == "crowded":
        assert {ref.LOSS, ref.UNKNOWN, ref.NONE} <= classes and 2 in lengths, (classes, lengths)


# ---- 3. one ply of negamax at scale: every move's answer follows from the row of the board after it.
# d = 3 and max_nodes = 2^20: a default-board position has at most 6 movable pieces x 54 cells = 324 moves, so a depth-3
# search visits at most 1 + 324 + 324^2 = 105 301 positions and a depth-2 search 325: neither side can run out of budget,
# the excluded share is 0 (asserted below, with the `nodes` the call reports).
def test_one_ply_consistency_at_scale():
    from simulator.game import _abi

    n, d, max_nodes = 1 << 14, 3, 1 << 20
    pos = random_roots(DEFAULT, 1 << 13, (6, 10, 14), SEED + 3)
    assert pos[0].shape[0] >= n
    pos = gt._take(pos, np.arange(n))
    h, w = DEFAULT.shape
    b = load(DEFAULT, pos)
    codes, plies = b.solve_moves(depth=d, max_nodes=max_nodes)
    nodes = ctypes.c_uint64(0)
    scratch = np.empty(codes.shape, dtype=np.int8)
    assert _abi.lib().bgs_bounce_solve_moves(b._handle, d, max_nodes, ctypes.c_void_p(scratch.ctypes.data), None,
                                             ctypes.byref(nodes), 0) == _abi.BGS_OK
    t = b.targets
    legal = ((t[:, :w, None] >> np.arange(h * w, dtype=np.uint64)) & np.uint64(1)) != 0
    row = t[:, w].astype(np.int64)
    np.testing.assert_array_equal(codes != ref.NONE, legal)
    tasks = int(legal.sum())
    assert 0 < nodes.value <= tasks * 105301
    assert not (codes == ref.BUDGET).any()
    flat_legal = legal.reshape(n, -1)
    order = np.argsort(~flat_legal, axis=1, kind="stable")   # every board's legal slots first, ascending
    count = flat_legal.sum(axis=1)
    checked = excluded = 0
    kid = load(DEFAULT, pos)
    for k in range(int(count.max())):
        has = count > k
        slot = order[:, k]
        x, c = slot // (h * w), slot % (h * w)
        moves = np.stack([x, row, c % w, c // w], -1).astype(np.int32)
        moves[~has] = -1
        assert (kid.write_state(pos[0], pos[1], pos[2], pos[3]) == 0).all()
        status = kid.step_actions(moves)
        assert (status[has] == 0).all()
        kc, kp = kid.solve_moves(depth=d - 1, max_nodes=max_nodes)
        winner = kid.winner
        idx = np.flatnonzero(has)
        got_c, got_p = codes[idx, x[idx], c[idx]], plies[idx, x[idx], c[idx]]
        ended = winner[idx] != -1
        won = ended & (winner[idx] == pos[1][idx])
        drawn = ended & (winner[idx] == 2)
        assert (ended == (won | drawn)).all()
        assert (got_c[won] == ref.WIN).all() and (got_p[won] == 1).all()
        assert (got_c[drawn] == ref.DRAW).all() and (got_p[drawn] == 1).all()
        kcg = kc[idx].reshape(idx.size, -1).astype(np.int64)
        kpg = kp[idx].reshape(idx.size, -1).astype(np.int64)
        out = (got_c == ref.BUDGET) | (kcg == ref.BUDGET).any(axis=1)
        excluded += int((out & ~ended).sum())
        go = np.flatnonzero(~ended & ~out)
        key = np.where(kcg == ref.WIN, 1000 - kpg, np.where(kcg == ref.LOSS, -1000 + kpg, np.where(kcg == ref.NONE, -10**6, 0)))
        j = np.argmax(key[go], axis=1)
        bc, bp = kcg[go, j], kpg[go, j]
        want_c = np.where(bc == ref.WIN, ref.LOSS, np.where(bc == ref.LOSS, ref.WIN, ref.UNKNOWN))
        want_p = np.where(np.isin(bc, [ref.WIN, ref.LOSS]), bp + 1, 0)
        np.testing.assert_array_equal(got_c[go], want_c)
        np.testing.assert_array_equal(got_p[go], want_p)
        checked += go.size
    assert checked + excluded > 0 and excluded < 0.01 * tasks
    assert checked > n * 8
    print(f"one ply at scale: {tasks} moves of {n} roots, {checked} re-derived, {excluded} excluded, {nodes.value} nodes")


# ---- 4. the budget, edge cases and invariants
def test_budget():
    cfg, pos = walk("three_next_to_goal")
    want_c, want_p = ref.solve(cfg, pos, 4)
    b = load(cfg, pos)
    for max_nodes in (1, 2, 7):
        codes, plies = b.solve_moves(depth=4, max_nodes=max_nodes)
        hit = codes == ref.BUDGET
        assert hit.any()
        assert (plies[hit] == 0).all()
        np.testing.assert_array_equal(codes[~hit], want_c[~hit])
        np.testing.assert_array_equal(plies[~hit], want_p[~hit])
    codes, plies = b.solve_moves(depth=4, max_nodes=BUDGET)
    assert not (codes == ref.BUDGET).any()
    np.testing.assert_array_equal(codes, want_c)
    b.close()


def test_ended_boards_illegal_slots_and_invariants():
    cfg, pos = walk("three_next_to_goal")
    h, w = cfg.shape
    b = load(cfg, pos)
    before = (b.grid.copy(), b.player.copy(), b.winner.copy(), b.plies.copy())
    b.reset_steps()
    codes, plies = b.solve_moves()
    assert codes.shape == (pos[0].shape[0], w, h * w) and codes.dtype == np.int8 and plies.dtype == np.int16
    ended = pos[2] != -1
    assert ended.any()
    assert (codes[ended] == ref.NONE).all() and (plies[ended] == 0).all()
    acts = gt.bounce_actions(cfg, pos)
    legal = np.zeros(codes.shape, dtype=bool)
    for i, a in enumerate(acts):
        for (sx, sy), (tx, ty) in a:
            legal[i, sx, ty * w + tx] = True
    np.testing.assert_array_equal(codes != ref.NONE, legal)
    assert (plies[~legal] == 0).all()
    for a, c in zip(before, (b.grid, b.player, b.winner, b.plies)):
        np.testing.assert_array_equal(a, c)
    assert b.steps == 0
    # a board without a legal move that is still marked running cannot be loaded (write_state settles it): the blocked
    # start position is the library's own example, every slot NONE
    blocked = np.array(BOUNCE_CONFIGS["blocked_start"], dtype=np.int8)
    bb = load(*walk("blocked_start"))
    cb, pb = bb.solve_moves()
    assert (cb == ref.NONE).all() and (pb == 0).all() and cb.shape == (1, 2, blocked.size)
    bb.close()
    # no dependence on first_game, on the ply counter beyond its parity, on splitting the batch
    b.set_first_game(12345)
    c2, p2 = b.solve_moves()
    np.testing.assert_array_equal(c2, codes)
    np.testing.assert_array_equal(p2, plies)
    c3, p3 = b.solve_moves(with_plies=False)
    assert p3 is None
    np.testing.assert_array_equal(c3, codes)
    later = load(cfg, (pos[0], pos[1], pos[2], pos[3] + 1000))
    c4, p4 = later.solve_moves()
    np.testing.assert_array_equal(c4, codes)
    np.testing.assert_array_equal(p4, plies)
    later.close()
    third = pos[0].shape[0] // 3
    for part in (np.arange(third), np.arange(third, pos[0].shape[0])):
        s = load(cfg, gt._take(pos, part))
        cs, ps = s.solve_moves()
        np.testing.assert_array_equal(cs, codes[part])
        np.testing.assert_array_equal(ps, plies[part])
        s.close()
    one = load(cfg, gt._take(pos, np.array([7])))
    np.testing.assert_array_equal(one.solve_moves()[0], codes[7:8])
    b.close()


# ---- 5. the device path
def test_device_path_and_stream_order():
    import torch

    pos = random_roots(DEFAULT, 512, (8, 12), SEED + 5)
    n = pos[0].shape[0]
    h, w = DEFAULT.shape
    host = load(DEFAULT, pos)
    dev = load(DEFAULT, pos, use_torch=True)
    t = host.targets
    moves = np.full((n, 4), -1, dtype=np.int32)
    for i in range(n):   # every board's first legal move
        x = next(x for x in range(w) if t[i, x])
        c = int(t[i, x]).bit_length() - 1
        moves[i] = (x, int(t[i, w]), c % w, c // w)
    assert (host.step_actions(moves) == 0).all()
    want_c, want_p = host.solve_moves(max_nodes=BUDGET)
    dev.step_actions(torch.from_numpy(moves).cuda(), want_status=False)   # same stream, no synchronisation in between
    codes, plies = dev.solve_moves_tensor(max_nodes=BUDGET)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(codes.cpu().numpy(), want_c)
    np.testing.assert_array_equal(plies.cpu().numpy(), want_p)
    out_c = torch.full((n, w, h * w), 99, dtype=torch.int8, device="cuda:0")
    got_c, got_p = dev.solve_moves_tensor(codes=out_c, with_plies=False, max_nodes=BUDGET)
    assert got_p is None and got_c is out_c
    torch.cuda.synchronize()
    np.testing.assert_array_equal(out_c.cpu().numpy(), want_c)
    with pytest.raises(TypeError):
        dev.solve_moves_tensor(codes=torch.zeros((n, w, h * w), dtype=torch.int16, device="cuda:0"))
    with pytest.raises(TypeError):
        dev.solve_moves_tensor(plies=torch.zeros((n, w), dtype=torch.int16, device="cuda:0"))


# ---- 6. refusals
def test_refusals():
    import torch
    from simulator.batch import BounceBatch, ConnectBatch
    from simulator.game import _abi

    lib = _abi.lib()
    n = 64
    h, w = DEFAULT.shape
    cells = n * w * h * w
    codes = np.zeros(cells, dtype=np.int8)
    cp = ctypes.c_void_p(codes.ctypes.data)
    connect = ConnectBatch(6, 7, 4, n)
    assert lib.bgs_bounce_solve_moves(connect._handle, 3, 100, cp, None, None, 0) == _abi.BGS_ERR_ARG
    with pytest.raises(ValueError, match="Bounce"):
        connect.solve_moves()
    big = np.zeros((9, 8), dtype=np.int8)   # 72 cells: generic
    big[1] = big[7] = 1
    generic = BounceBatch(big, n)
    assert generic.generic
    assert lib.bgs_bounce_solve_moves(generic._handle, 3, 100, cp, None, None, 0) == _abi.BGS_ERR_ARG
    valued = DEFAULT.copy()
    valued[1, 0] = 16                       # a value above 15: generic
    generic2 = BounceBatch(valued, n)
    assert generic2.generic
    assert lib.bgs_bounce_solve_moves(generic2._handle, 3, 100, cp, None, None, 0) == _abi.BGS_ERR_ARG
    b = BounceBatch(DEFAULT, n, use_torch=True)
    assert lib.bgs_bounce_solve_moves(b._handle, 0, 100, cp, None, None, 0) == _abi.BGS_ERR_ARG
    assert lib.bgs_bounce_solve_moves(b._handle, MAX_DEPTH + 1, 100, cp, None, None, 0) == _abi.BGS_ERR_ARG
    with pytest.raises(Exception, match=str(MAX_DEPTH)):
        b.solve_moves(depth=MAX_DEPTH + 1)
    assert lib.bgs_bounce_solve_moves(b._handle, 3, 0, cp, None, None, 0) == _abi.BGS_ERR_ARG
    assert lib.bgs_bounce_solve_moves(b._handle, 3, 100, None, None, None, 0) == _abi.BGS_ERR_ARG
    buf = torch.zeros(cells * 3 + 64, dtype=torch.int8, device="cuda:0")
    base = buf.data_ptr()
    assert base % 16 == 0
    ok_nodes = torch.zeros(2, dtype=torch.int64, device="cuda:0")
    assert lib.bgs_bounce_solve_moves(b._handle, 3, 100, ctypes.c_void_p(base + 1), None, None, 1) == _abi.BGS_ERR_ARG
    assert lib.bgs_bounce_solve_moves(b._handle, 3, 100, ctypes.c_void_p(base), ctypes.c_void_p(base + cells + 2), None,
                                      1) == _abi.BGS_ERR_ARG
    assert lib.bgs_bounce_solve_moves(b._handle, 3, 100, ctypes.c_void_p(base), None,
                                      ctypes.c_void_p(ok_nodes.data_ptr() + 4), 1) == _abi.BGS_ERR_ARG
    # the well-formed calls go through, at the maximum too, and count the same positions on the host and the device path
    b.reset()
    assert lib.bgs_bounce_solve_moves(b._handle, MAX_DEPTH, 50, cp, None, None, 0) == _abi.BGS_OK
    nodes = ctypes.c_uint64(0)
    assert lib.bgs_bounce_solve_moves(b._handle, 4, 1 << 20, cp, None, ctypes.byref(nodes), 0) == _abi.BGS_OK
    assert nodes.value > 0
    assert lib.bgs_bounce_solve_moves(b._handle, 4, 1 << 20, ctypes.c_void_p(base), None, ctypes.c_void_p(ok_nodes.data_ptr()),
                                      1) == _abi.BGS_OK
    torch.cuda.synchronize()
    assert int(ok_nodes[0]) == nodes.value
    np.testing.assert_array_equal(buf[:cells].cpu().numpy(), codes)


# ---- 7. the agent
def _states(cfg, pos, idx):
    from simulator.game.bounce import Config, State

    config = Config(cfg)
    return [State.from_json({"grid": pos[0][i].tolist(), "player": int(pos[1][i]), "winner": int(pos[2][i])}, config) for i in idx]


def test_solver_agent_values_and_choice():
    from simulator.agents import SolverAgent

    cfg, pos = walk("small")
    h, w = cfg.shape
    idx = np.flatnonzero(pos[2] == -1)[::97]
    sub = gt._take(pos, idx)
    want_c, want_p = ref.solve(cfg, sub, 3)
    states = _states(cfg, pos, idx)
    agent = SolverAgent(depth=3)
    values = agent.predict_many(states)
    seen = set()
    for i, s in enumerate(states):
        assert list(values[i]) == s.actions
        slot = {a: (a._source[0], a._target[1] * w + a._target[0]) for a in s.actions}
        for a, v in values[i].items():
            c = int(want_c[i][slot[a]])
            seen.add(c)
            assert v == {ref.WIN: 1.0, ref.DRAW: 0.5, ref.LOSS: 0.0, ref.UNKNOWN: 0.5}[c]
        if i % 5 == 0:
            pick = agent.choose(s)
            c, p = int(want_c[i][slot[pick]]), int(want_p[i][slot[pick]])
            all_c = [int(want_c[i][slot[a]]) for a in s.actions]
            if ref.WIN in all_c:
                assert c == ref.WIN and p == min(int(want_p[i][slot[a]]) for a in s.actions if want_c[i][slot[a]] == ref.WIN)
            elif any(x != ref.LOSS for x in all_c):
                assert c != ref.LOSS
            else:
                assert p == max(int(want_p[i][slot[a]]) for a in s.actions)
    assert {ref.WIN, ref.LOSS, ref.UNKNOWN} <= seen
    assert agent.predict(states[0]) == values[0]
    # depth=None is the Bounce default horizon
    np.testing.assert_array_equal(SolverAgent().solve_many(states[:8])[0], want_c[:8])
    agent.close()


def test_solver_agent_fallback():
    from simulator.agents import MonteCarloAgent, SolverAgent

    pos = random_roots(DEFAULT, 16, (10,), SEED + 7)
    states = _states(DEFAULT, pos, range(min(8, pos[0].shape[0])))
    w = DEFAULT.shape[1]
    mc = MonteCarloAgent(playouts=32)
    agent = SolverAgent(depth=2, fallback=mc)
    codes, _ = agent.solve_many(states)
    assert (codes == ref.UNKNOWN).any()
    mixed = agent.predict_many(states)
    mc_values = mc.predict_many(states)
    exact = {ref.WIN: 1.0, ref.DRAW: 0.5, ref.LOSS: 0.0}
    for i, s in enumerate(states):
        assert list(mixed[i]) == s.actions
        for a in s.actions:
            c = int(codes[i, a._source[0], a._target[1] * w + a._target[0]])
            assert mixed[i][a] == (mc_values[i][a] if c == ref.UNKNOWN else exact[c])
    alone = SolverAgent(depth=2).predict_many(states)
    for i, s in enumerate(states):
        for a in s.actions:
            if codes[i, a._source[0], a._target[1] * w + a._target[0]] == ref.UNKNOWN:
                assert alone[i][a] == 0.5
