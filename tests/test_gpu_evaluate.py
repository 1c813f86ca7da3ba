"""Flat Monte-Carlo evaluation (bgs_connect_evaluate_actions, ConnectBatch.evaluate_actions, MonteCarloAgent) against
the CPU oracle.  The expected counts are built from the oracle as it is: root i replicated width * playouts times,
stepped by its column (illegal columns leave the board and drop out of the count), then rollout(seed,
first_game * width * playouts, max_plies), the winners counted relative to the root's player.

Everything here needs a real MI355X: `pytest -m gpu`.
"""

import ctypes

import numpy as np
import pytest

from oracle import oracle
from tests.mc_expected import connect_expected as expected

pytestmark = pytest.mark.gpu

SEED = 0x5EED0F0E7A1A7E00
ONE_WORD = [(4, 4, 3), (6, 7, 4), (7, 8, 4)]
MULTI_WORD = [(6, 12, 4), (12, 13, 5), (10, 16, 5)]


def make_roots(h, w, k, n, seed):
    """n positions in the reference layout: the start, random mid-game positions, boards with full columns, ended
    boards (grid, player, winner, plies)."""
    rng = np.random.default_rng(seed)
    orc = oracle.ConnectOracle(h, w, k, n)
    kind = np.arange(n) % 4   # 0 start, 1 mid-game, 2 full columns, 3 played to the end
    target = np.where(kind == 1, rng.integers(1, h * w // 2, n), 0)
    fill = np.where(kind == 2, rng.integers(0, w, n), -1)
    for ply in range(h * w):
        legal = orc.legal()
        cols = np.full(n, -1, dtype=np.int32)
        for i in range(n):
            if orc.winner[i] != -1 or not legal[i].any():
                continue
            if kind[i] == 1 and ply >= target[i]:
                continue
            if kind[i] == 0:
                continue
            if kind[i] == 2:
                if ply < h and legal[i, fill[i]]:
                    cols[i] = fill[i]          # one column filled, alternating stones: no vertical run
                elif ply < h + 2 * (i % 3):
                    cols[i] = rng.choice(np.flatnonzero(legal[i]))
                continue
            cols[i] = rng.choice(np.flatnonzero(legal[i]))
        if (cols < 0).all():
            break
        orc.step_actions(cols)
    return orc.grid.copy(), orc.player.copy(), orc.winner.copy(), orc.plies.copy()


def load(h, w, k, roots, per_ply=False, first_game=0, use_torch=None):
    from simulator.batch import ConnectBatch

    grid, player, winner, plies = roots
    b = ConnectBatch(h, w, k, grid.shape[0], use_torch=use_torch)
    assert (b.write_state(grid, player, winner, plies) == 0).all()
    if per_ply:
        b.set_rng_contract("per-ply")
    b.set_first_game(first_game)
    b.reset_steps()
    return b


def snapshot(b):
    return b.grid.tobytes(), b.player.tobytes(), b.winner.tobytes(), b.plies.tobytes()


@pytest.mark.parametrize("geom", ONE_WORD + MULTI_WORD, ids=lambda g: "x".join(map(str, g)))
@pytest.mark.parametrize("playouts", [1, 7, 64, 300])
def test_counts_equal_the_oracle(geom, playouts):
    h, w, k = geom
    roots = make_roots(h, w, k, 12, seed=h * 100 + w + playouts)
    first_game = 5
    for per_ply in (False, True):
        for cap in (None, 3):
            max_plies = 2**31 - 1 if cap is None else int(roots[3].min()) + cap
            b = load(h, w, k, roots, per_ply, first_game)
            before = snapshot(b)
            got = b.evaluate_actions(seed=SEED, playouts=playouts, max_plies=max_plies)
            want, steps = expected(h, w, k, roots, SEED, first_game, playouts, max_plies, per_ply)
            what = f"{geom} P={playouts} per_ply={per_ply} max_plies={max_plies}"
            np.testing.assert_array_equal(got, want, err_msg=what)
            assert b.steps == steps, what
            assert snapshot(b) == before, what
            b.close()


@pytest.mark.parametrize("geom,playouts", [((6, 7, 4), 700), ((12, 13, 5), 1000)])
def test_playouts_spanning_waves_equal_the_oracle(geom, playouts):
    """more playouts than a wave takes: a (root, column) is split over waves (one atomic per wave and counter)"""
    h, w, k = geom
    roots = make_roots(h, w, k, 4, seed=7)
    b = load(h, w, k, roots, first_game=3)
    got = b.evaluate_actions(seed=SEED, playouts=playouts)
    want, steps = expected(h, w, k, roots, SEED, 3, playouts, 2**31 - 1, False)
    np.testing.assert_array_equal(got, want)
    assert b.steps == steps


def test_sharded_batches_give_the_whole_batch():
    h, w, k = 6, 7, 4
    roots = make_roots(h, w, k, 64, seed=11)
    whole = load(h, w, k, roots, first_game=100).evaluate_actions(seed=SEED, playouts=32)
    half = [tuple(a[s] for a in roots) for s in (slice(0, 32), slice(32, 64))]
    lo = load(h, w, k, half[0], first_game=100).evaluate_actions(seed=SEED, playouts=32)
    hi = load(h, w, k, half[1], first_game=132).evaluate_actions(seed=SEED, playouts=32)
    np.testing.assert_array_equal(np.concatenate([lo, hi]), whole)


@pytest.mark.parametrize("playouts", [48, 600])
def test_device_path_writes_everything_in_stream_order(playouts):
    import torch

    h, w, k, n = 6, 7, 4, 256
    roots = make_roots(h, w, k, n, seed=13)
    b = load(h, w, k, roots, use_torch=True)
    ref = load(h, w, k, roots)
    stream = torch.cuda.Stream(device=0)
    b.set_stream(stream.cuda_stream)
    cols = torch.as_tensor((np.arange(n) * 3) % w, dtype=torch.int32)
    with torch.cuda.stream(stream):
        legal = torch.empty((n, w), dtype=torch.uint8, device="cuda:0")
        d_cols = cols.to("cuda:0", non_blocking=False)
        out = torch.full((n, w, 3), -1, dtype=torch.int32, device="cuda:0")
        b.step_actions_observe(d_cols, legal)
        b.evaluate_actions_tensor(out, seed=SEED, playouts=playouts)
    stream.synchronize()
    got = out.cpu().numpy()
    assert (got >= 0).all()
    # the same position on the default stream: the boards after the step, through the host path and the oracle
    ref.step_actions(cols.numpy().astype(np.int32), want_status=False)
    assert snapshot(ref) == snapshot(b)
    np.testing.assert_array_equal(got, ref.evaluate_actions(seed=SEED, playouts=playouts))
    want, _ = expected(h, w, k, (ref.grid, ref.player, ref.winner, ref.plies), SEED, 0, playouts, 2**31 - 1, False)
    np.testing.assert_array_equal(got, want)


def test_full_size_connect4_against_the_oracle():
    """2^14 roots x 7 columns x 64 playouts = 7.3 M playouts"""
    from simulator.batch import ConnectBatch

    h, w, k, n, playouts = 6, 7, 4, 1 << 14, 64
    b = ConnectBatch(h, w, k, n)
    b.step_random(seed=SEED ^ 1, plies=3)
    b.step_random(seed=SEED ^ 2, plies=5)
    roots = (b.grid, b.player, b.winner, b.plies)
    b.reset_steps()
    got = b.evaluate_actions(seed=SEED, playouts=playouts)
    want, steps = expected(h, w, k, roots, SEED, 0, playouts, 2**31 - 1, False)
    np.testing.assert_array_equal(got, want)
    assert b.steps == steps


def _state_after(columns, config=(6, 7, 4)):
    from simulator.game.connect import Config

    s = Config(*config).sample_initial_state()
    for c in columns:
        s = s.action_at(c).sample_next_state()
    return s


def test_monte_carlo_agent():
    from simulator.agents import MonteCarloAgent

    agent = MonteCarloAgent(playouts=128, seed=SEED)
    win_now = _state_after([0, 1, 0, 1, 0, 1])        # player 0 to move, column 0 wins at once
    values = agent.predict(win_now)
    assert list(values) == win_now.actions
    assert values[win_now.action_at(0)] == 1.0
    assert max(values, key=values.get).column == 0
    full_col = _state_after([3, 3, 3, 3, 3, 3, 2])    # column 3 is full: not among the actions
    v = agent.predict(full_col)
    assert list(v) == full_col.actions and all(a.column != 3 for a in v)
    assert all(0.0 <= x <= 1.0 for x in v.values())

    states = [_state_after(cs) for cs in ([], [3], [3, 3, 2], [0, 1, 0, 1, 0, 1], [3, 3, 3, 3, 3, 3, 2])]
    many = agent.predict_many(states)
    for g, (s, m) in enumerate(zip(states, many)):
        one = agent.predict(s, game=g)
        assert list(m) == s.actions and m == one
    agent.close()


def test_refusals():
    from simulator.batch import BounceBatch, ConnectBatch
    from simulator.game import _abi

    grid = np.zeros((9, 6), dtype=np.int8)
    grid[1] = grid[7] = [1, 2, 3, 3, 2, 1]
    bounce = BounceBatch(grid, 64)
    with pytest.raises(ValueError, match="Connect"):
        bounce.evaluate_actions()
    out = np.zeros(64 * 6 * 3, dtype=np.int32)
    assert _abi.lib().bgs_connect_evaluate_actions(bounce._handle, 1, 8, 100, ctypes.c_void_p(out.ctypes.data), 0) == _abi.BGS_ERR_ARG
    assert "Connect" in _abi.last_error()
    with pytest.raises(ValueError, match="bit-packed"):
        ConnectBatch(20, 20, 5, 4).evaluate_actions()
    b = ConnectBatch(6, 7, 4, 4)
    with pytest.raises(ValueError, match="playouts"):
        b.evaluate_actions(playouts=0)
    with pytest.raises(ValueError, match="max_plies"):
        b.evaluate_actions(max_plies=0)
    import torch

    t = torch.zeros(4 * 7 * 3 + 1, dtype=torch.int32, device="cuda:0")
    rc = _abi.lib().bgs_connect_evaluate_actions(b._handle, 1, 8, 100, ctypes.c_void_p(t.data_ptr() + 4), 1)
    assert rc == _abi.BGS_ERR_ARG and "aligned" in _abi.last_error()
