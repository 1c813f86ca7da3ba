"""The exact Connect solver (bgs_connect_solve_actions, ConnectBatch.solve_actions, SolverAgent) against the CPU
reference of tests/solve_reference.py, bit for bit: codes and plies of every column of every position.

Everything here needs a real MI355X: `pytest -m gpu`.
"""

import ctypes
import functools

import numpy as np
import pytest

from oracle import oracle
from tests import game_trees as gt
from tests import solve_reference as ref

pytestmark = pytest.mark.gpu

CONNECT_FULL = [(2, 3, 2), (3, 3, 3), (3, 4, 3), (4, 3, 3), (4, 4, 3), (4, 4, 4)]
BUDGET = 1 << 22        # no test position here comes near it (small boards, end-games, shallow horizons)
SEED = 0x50171E5EED


def concat(layers):
    return tuple(np.concatenate([l[j] for l in layers]) for j in range(4))


@functools.lru_cache(maxsize=None)
def all_positions(h, w, k):
    return concat([layer for _, layer in gt.connect_layers(h, w, k)])


def load(h, w, k, pos, use_torch=None):
    from simulator.batch import ConnectBatch

    b = ConnectBatch(h, w, k, pos[0].shape[0], use_torch=use_torch)
    assert (b.write_state(pos[0], pos[1], pos[2], pos[3]) == 0).all()
    return b


def at_empty(h, w, k, n, empties, seed):
    """running positions of random oracle games with a number of empty cells in `empties` (distinct boards, at most n)"""
    orc = oracle.ConnectOracle(h, w, k, n)
    picked = []
    for ply in range(h * w):
        if h * w - ply in empties:
            picked.append(gt._take((orc.grid, orc.player, orc.winner, orc.plies), np.flatnonzero(orc.winner == -1)))
        if orc.ended.all():
            break
        orc.step_random(seed)
    pos = concat(picked)
    return gt._take(pos, gt._unique_rows(pos[0]))


def mid_game(h, w, k, n, plies, seed):
    orc = oracle.ConnectOracle(h, w, k, n)
    for _ in range(plies):
        orc.step_random(seed)
    pos = (orc.grid, orc.player, orc.winner, orc.plies)
    return gt._take(pos, gt._unique_rows(pos[0]))


def check(h, w, k, pos, depth, max_nodes=BUDGET):
    b = load(h, w, k, pos)
    codes, plies = b.solve_actions(depth=depth, max_nodes=max_nodes)
    want_c, want_p = ref.solve(h, w, k, pos, depth)
    b.close()
    return codes, plies, want_c, want_p


# ---- 1. every reachable position of the small geometries
@pytest.mark.parametrize("geom", CONNECT_FULL, ids=lambda g: "x".join(map(str, g)))
def test_exact_on_every_small_position(geom):
    h, w, k = geom
    pos = all_positions(h, w, k)
    for depth in (h * w, 1, 2, 3, 5):
        codes, plies, want_c, want_p = check(h, w, k, pos, depth)
        bad = np.flatnonzero((codes != want_c).any(axis=1) | (plies != want_p).any(axis=1))
        assert bad.size == 0, (geom, depth, bad[:5], codes[bad[:3]], want_c[bad[:3]], plies[bad[:3]], want_p[bad[:3]])


# ---- 1b. a horizon beyond the board's cells is the same full solve (the launcher clamps it; the stack is sized by it)
@pytest.mark.parametrize("geom", CONNECT_FULL, ids=lambda g: "x".join(map(str, g)))
def test_depth_beyond_the_board_is_a_full_solve(geom):
    h, w, k = geom
    pos = all_positions(h, w, k)
    b = load(h, w, k, pos)
    want_c, want_p = b.solve_actions(depth=h * w, max_nodes=BUDGET)
    for depth in (h * w + 1, h * w + 2, 2**31 - 1):
        codes, plies = b.solve_actions(depth=depth, max_nodes=BUDGET)
        np.testing.assert_array_equal(codes, want_c)
        np.testing.assert_array_equal(plies, want_p)
    b.close()
    ref_c, ref_p = ref.solve(h, w, k, gt._take(pos, np.array([0])), h * w)
    np.testing.assert_array_equal(want_c[:1], ref_c)
    np.testing.assert_array_equal(want_p[:1], ref_p)


# ---- 2. the big boards: one, two and three words a plane.  6x7 end-games at 6-10 empty cells are solved in full; on the
# larger boards random games end long before so few empty cells, and their positions a few plies before the end of a
# random game are solved at the horizon the mid-game positions get
@pytest.mark.parametrize("geom,mid_plies,depth", [((6, 7, 4), 12, 5), ((8, 8, 4), 16, 5), ((12, 13, 5), 30, 4)],
                         ids=["6x7x4", "8x8x4", "12x13x5"])
def test_exact_on_big_boards(geom, mid_plies, depth):
    h, w, k = geom
    if (h, w) == (6, 7):
        late = at_empty(h, w, k, 4096, {6, 8, 10}, SEED ^ h)
        late = gt._take(late, np.arange(min(300, late[0].shape[0])))
        assert late[0].shape[0] >= 200 and ((late[0] < 0).sum(axis=(1, 2)) <= 10).all()
        codes, plies, want_c, want_p = check(h, w, k, late, h * w)
        assert not np.isin(codes, [ref.UNKNOWN, ref.BUDGET]).any()
    else:
        late = gt.end_games(h, w, k, 200, SEED ^ h)
        codes, plies, want_c, want_p = check(h, w, k, late, depth)
        assert (codes == ref.WIN).any() and (codes == ref.LOSS).any()
    np.testing.assert_array_equal(codes, want_c)
    np.testing.assert_array_equal(plies, want_p)
    mid = mid_game(h, w, k, 200, mid_plies, SEED ^ w)
    for d in range(1, depth + 1):
        codes, plies, want_c, want_p = check(h, w, k, mid, d)
        np.testing.assert_array_equal(codes, want_c)
        np.testing.assert_array_equal(plies, want_p)


# ---- 3. one ply of negamax at scale: every column's answer follows from the row of the board after it
def test_one_ply_consistency_at_scale():
    h, w, k = 6, 7, 4
    n = 1 << 16
    pos = at_empty(h, w, k, 1 << 18, {12, 13, 14}, SEED)
    assert pos[0].shape[0] >= n
    pos = gt._take(pos, np.arange(n))
    depth = 12
    b = load(h, w, k, pos)
    codes, plies = b.solve_actions(depth=depth, max_nodes=1 << 16)
    empty = (pos[0] < 0).sum(axis=(1, 2))
    checked = 0
    for c in range(w):
        kid = load(h, w, k, pos)
        status = kid.step_actions(np.full(n, c, dtype=np.int32))
        legal = status == 0
        assert ((codes[:, c] == ref.NONE) == ~legal).all()
        kc, kp = kid.solve_actions(depth=depth - 1, max_nodes=1 << 16)
        winner = kid.winner
        ended = winner != -1
        won = legal & ended & (winner != 2)
        drawn = legal & (winner == 2)
        assert (codes[won, c] == ref.WIN).all() and (plies[won, c] == 1).all()
        assert (codes[drawn, c] == ref.DRAW).all() and (plies[drawn, c] == 1).all()
        go = np.flatnonzero(legal & ~ended & (codes[:, c] != ref.BUDGET) & ~(kc == ref.BUDGET).any(axis=1))
        kcg, kpg = kc[go].astype(np.int64), kp[go].astype(np.int64)
        key = np.where(kcg == ref.WIN, 1000 - kpg, np.where(kcg == ref.LOSS, -1000 + kpg,
                       np.where(kcg == ref.NONE, -10**6, 0)))
        j = np.argmax(key, axis=1)
        bc, bp = kcg[np.arange(go.size), j], kpg[np.arange(go.size), j]
        want_c = np.where(bc == ref.WIN, ref.LOSS, np.where(bc == ref.LOSS, ref.WIN, bc))
        want_p = np.where(np.isin(bc, [ref.WIN, ref.LOSS]), bp + 1, np.where(bc == ref.DRAW, empty[go], 0))
        np.testing.assert_array_equal(codes[go, c], want_c)
        np.testing.assert_array_equal(plies[go, c], want_p)
        checked += go.size
        kid.close()
    assert checked > n * 3
    assert (codes == ref.BUDGET).mean() < 0.01


# ---- 4. the budget
def test_budget():
    h, w, k = 4, 4, 4
    pos = all_positions(h, w, k)
    want_c, want_p = ref.solve(h, w, k, pos, h * w)
    b = load(h, w, k, pos)
    for max_nodes in (1, 3, 40):
        codes, plies = b.solve_actions(max_nodes=max_nodes)
        hit = codes == ref.BUDGET
        assert hit.any()
        assert (plies[hit] == 0).all()
        np.testing.assert_array_equal(codes[~hit], want_c[~hit])
        np.testing.assert_array_equal(plies[~hit], want_p[~hit])
    codes, plies = b.solve_actions(max_nodes=BUDGET)
    assert not (codes == ref.BUDGET).any()
    np.testing.assert_array_equal(codes, want_c)


# ---- 5. edge cases and invariants
def test_ended_boards_illegal_columns_and_invariants():
    h, w, k = 4, 4, 3
    pos = all_positions(h, w, k)
    b = load(h, w, k, pos)
    before = (b.grid.copy(), b.player.copy(), b.winner.copy(), b.plies.copy())
    b.reset_steps()
    codes, plies = b.solve_actions()
    ended = pos[2] != -1
    assert (codes[ended] == ref.NONE).all() and (plies[ended] == 0).all()
    full_col = (pos[0][:, h - 1, :] >= 0)
    assert (codes[full_col] == ref.NONE).all() and (plies[full_col] == 0).all()
    assert (codes[~ended[:, None] & ~full_col] != ref.NONE).all()
    for a, c in zip(before, (b.grid, b.player, b.winner, b.plies)):
        np.testing.assert_array_equal(a, c)
    assert b.steps == 0
    # no dependence on first_game, on the RNG contract, on splitting the batch, or on the plies buffer
    b.set_first_game(12345)
    b.set_rng_contract("per-ply")
    c2, p2 = b.solve_actions()
    np.testing.assert_array_equal(c2, codes)
    np.testing.assert_array_equal(p2, plies)
    c3, p3 = b.solve_actions(with_plies=False)
    assert p3 is None
    np.testing.assert_array_equal(c3, codes)
    half = pos[0].shape[0] // 3
    for part in (np.arange(half), np.arange(half, pos[0].shape[0])):
        s = load(h, w, k, gt._take(pos, part))
        cs, ps = s.solve_actions()
        np.testing.assert_array_equal(cs, codes[part])
        np.testing.assert_array_equal(ps, plies[part])
        s.close()
    one = load(h, w, k, gt._take(pos, np.array([7])))
    np.testing.assert_array_equal(one.solve_actions()[0], codes[7:8])


# ---- 6. the device path
def test_device_path_and_stream_order():
    import torch

    h, w, k = 6, 7, 4
    pos = at_empty(h, w, k, 4096, {9, 10, 11}, SEED + 1)
    n = pos[0].shape[0]
    host = load(h, w, k, pos)
    dev = load(h, w, k, pos, use_torch=True)
    cols = ((np.arange(n) * 3) % w).astype(np.int32)
    host.step_actions(cols)
    want_c, want_p = host.solve_actions(max_nodes=BUDGET)
    dev.step_actions(torch.from_numpy(cols).cuda(), want_status=False)   # same stream, no synchronisation in between
    codes, plies = dev.solve_actions_tensor(max_nodes=BUDGET)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(codes.cpu().numpy(), want_c)
    np.testing.assert_array_equal(plies.cpu().numpy(), want_p)
    out_c = torch.full((n, w), 99, dtype=torch.int8, device="cuda:0")
    got_c, got_p = dev.solve_actions_tensor(codes=out_c, with_plies=False, max_nodes=BUDGET)
    assert got_p is None and got_c is out_c
    np.testing.assert_array_equal(out_c.cpu().numpy(), want_c)


# ---- 7. refusals
def test_refusals():
    import torch
    from simulator.batch import BounceBatch, ConnectBatch
    from simulator.game import _abi

    lib = _abi.lib()
    codes = np.zeros(64 * 16, dtype=np.int8)
    cp = ctypes.c_void_p(codes.ctypes.data)
    grid = np.zeros((9, 6), dtype=np.int8)
    grid[1] = grid[7] = [1, 2, 3, 3, 2, 1]
    bounce = BounceBatch(grid, 64)
    assert lib.bgs_connect_solve_actions(bounce._handle, 10, 100, cp, None, None, 0) == _abi.BGS_ERR_ARG
    with pytest.raises(ValueError, match="Connect"):
        bounce.solve_actions()
    generic = ConnectBatch(15, 16, 4, 64)
    assert generic.generic
    assert lib.bgs_connect_solve_actions(generic._handle, 10, 100, cp, None, None, 0) == _abi.BGS_ERR_ARG
    b = ConnectBatch(6, 7, 4, 64, use_torch=True)
    assert lib.bgs_connect_solve_actions(b._handle, 0, 100, cp, None, None, 0) == _abi.BGS_ERR_ARG
    assert lib.bgs_connect_solve_actions(b._handle, 10, 0, cp, None, None, 0) == _abi.BGS_ERR_ARG
    assert lib.bgs_connect_solve_actions(b._handle, 10, 100, None, None, None, 0) == _abi.BGS_ERR_ARG
    buf = torch.zeros(64 * 7 * 2 + 64, dtype=torch.int8, device="cuda:0")
    base = buf.data_ptr()
    assert base % 16 == 0
    ok_nodes = torch.zeros(2, dtype=torch.int64, device="cuda:0")
    assert lib.bgs_connect_solve_actions(b._handle, 10, 100, ctypes.c_void_p(base + 1), None, None, 1) == _abi.BGS_ERR_ARG
    assert lib.bgs_connect_solve_actions(b._handle, 10, 100, ctypes.c_void_p(base), ctypes.c_void_p(base + 64 * 7 + 2),
                                         None, 1) == _abi.BGS_ERR_ARG
    assert lib.bgs_connect_solve_actions(b._handle, 10, 100, ctypes.c_void_p(base), None,
                                         ctypes.c_void_p(ok_nodes.data_ptr() + 4), 1) == _abi.BGS_ERR_ARG
    # the well-formed device call goes through and counts the positions it visited
    b.reset()
    nodes = ctypes.c_uint64(0)
    assert lib.bgs_connect_solve_actions(b._handle, 6, 1000, cp, None, ctypes.byref(nodes), 0) == _abi.BGS_OK
    assert nodes.value > 0
    assert lib.bgs_connect_solve_actions(b._handle, 6, 1000, ctypes.c_void_p(base), None,
                                         ctypes.c_void_p(ok_nodes.data_ptr()), 1) == _abi.BGS_OK
    torch.cuda.synchronize()
    assert int(ok_nodes[0]) == nodes.value


# ---- 8. the agent
def _states(h, w, k, pos):
    from simulator.game.connect import Config, State

    cfg = Config(h, w, k)
    return [State.from_json({"grid": pos[0][i].tolist(), "player": int(pos[1][i]), "winner": int(pos[2][i])}, cfg)
            for i in range(pos[0].shape[0])]


def test_solver_agent_values_every_position():
    from simulator.agents import SolverAgent

    h, w, k = 4, 4, 3
    pos = all_positions(h, w, k)
    run = gt._take(pos, np.flatnonzero(pos[2] == -1))
    want_c, want_p = ref.solve(h, w, k, run, h * w)
    states = _states(h, w, k, run)
    agent = SolverAgent()
    values = agent.predict_many(states)
    for i, s in enumerate(states):
        assert list(values[i]) == s.actions
        for act, v in values[i].items():
            assert v == {ref.WIN: 1.0, ref.DRAW: 0.5, ref.LOSS: 0.0}[int(want_c[i, act.column])]
    agent.close()


def test_solver_agent_choose_everywhere():
    """choose() on every running 4x4x3 position, in one batch per call"""
    from simulator.agents import SolverAgent

    h, w, k = 4, 4, 3
    pos = all_positions(h, w, k)
    run = gt._take(pos, np.flatnonzero(pos[2] == -1))
    want_c, want_p = ref.solve(h, w, k, run, h * w)
    agent = SolverAgent()
    rank = {ref.WIN: 2, ref.DRAW: 1, ref.LOSS: 0}
    for i, s in enumerate(_states(h, w, k, run)):
        c = agent.choose(s).column
        legal = [a.column for a in s.actions]
        best = max(rank[int(want_c[i, x])] for x in legal)
        assert rank[int(want_c[i, c])] == best
        same = [x for x in legal if rank[int(want_c[i, x])] == best]
        if best == 2:
            assert want_p[i, c] == min(want_p[i, x] for x in same)
        if best == 0:
            assert want_p[i, c] == max(want_p[i, x] for x in same)
    agent.close()


def test_solver_agent_fallback():
    from simulator.agents import MonteCarloAgent, SolverAgent

    pos = mid_game(6, 7, 4, 8, 4, SEED)
    states = _states(6, 7, 4, pos)
    mc = MonteCarloAgent(playouts=64)
    agent = SolverAgent(depth=2, fallback=mc)
    codes, _ = agent.solve_many(states)
    assert (codes == ref.UNKNOWN).any()
    mixed = agent.predict_many(states)
    mc_values = mc.predict_many(states)
    exact = {ref.WIN: 1.0, ref.DRAW: 0.5, ref.LOSS: 0.0}
    for i, s in enumerate(states):
        assert list(mixed[i]) == s.actions
        for a in s.actions:
            c = int(codes[i, a.column])
            assert mixed[i][a] == (mc_values[i][a] if c == ref.UNKNOWN else exact[c])
    alone = SolverAgent(depth=2).predict_many(states)
    for i, s in enumerate(states):
        assert all(alone[i][a] == 0.5 for a in s.actions if codes[i, a.column] == ref.UNKNOWN)
