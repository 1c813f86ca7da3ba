"""Flat Monte-Carlo evaluation of Bounce boards (bgs_bounce_evaluate_moves, BounceBatch.evaluate_moves, MonteCarloAgent on
Bounce states) against the CPU oracle.  The expected counts are built from the oracle as it is: root i replicated S * P
times (S = W * H * W slots), every copy stepped by its slot's move (slot s = x * H * W + c: the piece in column x of the
active row to cell c; a refused move drops the copy), then rollout(seed, first_game * S * P, max_plies), the winners
counted relative to the root's player.

Everything here needs a real MI355X: `pytest -m gpu`.
"""

import ctypes

import numpy as np
import pytest

from tests.mc_expected import active_rows, expected, expected_by_slot, make_roots, slot_moves  # noqa: F401
from tests.test_gpu_parity import BOUNCE_GRIDS

pytestmark = pytest.mark.gpu

SEED = 0x5EED0F0E7A1A7E00
LONG = 4096     # "uncapped" for the oracle: every test position ends well before (or is capped the same on both sides)


def load(grid, roots, first_game=0, use_torch=None):
    from simulator.batch import BounceBatch

    b = BounceBatch(grid, roots[0].shape[0], use_torch=use_torch)
    assert (b.write_state(*roots) == 0).all()
    b.set_first_game(first_game)
    b.reset_steps()
    return b


def snapshot(b):
    return b.grid.tobytes(), b.player.tobytes(), b.winner.tobytes(), b.plies.tobytes()


@pytest.mark.parametrize("name", list(BOUNCE_GRIDS))
@pytest.mark.parametrize("playouts", [1, 7, 64, 300])
def test_counts_equal_the_oracle(name, playouts):
    grid = BOUNCE_GRIDS[name]
    n = 12 if playouts <= 64 else 4
    roots = make_roots(grid, n, seed=len(name) * 100 + playouts)
    first_game = 5
    for max_plies in (int(roots[3].min()) + 40, 200, LONG):
        b = load(grid, roots, first_game)
        before = snapshot(b)
        got = b.evaluate_moves(seed=SEED, playouts=playouts, max_plies=max_plies)
        want, steps = expected(grid, roots, SEED, first_game, playouts, max_plies)
        what = f"{name} P={playouts} max_plies={max_plies}"
        np.testing.assert_array_equal(got, want, err_msg=what)
        assert b.steps == steps, what
        assert snapshot(b) == before, what
        # ended roots and illegal slots are 0, 0, 0
        ended = roots[2] != -1
        assert not got[ended].any(), what
        b.close()


def test_roots_without_a_move_give_nothing():
    grid = BOUNCE_GRIDS["blocked_start"]
    roots = make_roots(grid, 4, seed=1)
    b = load(grid, roots)
    assert (b.winner != -1).all()
    assert not b.evaluate_moves(seed=SEED, playouts=8).any()
    assert b.steps == 0


def test_segments_spanning_waves_and_capped_playouts():
    """more playouts than a chunk: a (root, slot) is split over waves; a short cap leaves playouts capped"""
    grid = BOUNCE_GRIDS["default"]
    roots = make_roots(grid, 4, seed=7)
    b = load(grid, roots, first_game=3)
    got = b.evaluate_moves(seed=SEED, playouts=1500, max_plies=int(roots[3].max()) + 12)
    want, steps = expected_by_slot(grid, roots, SEED, 3, 1500, int(roots[3].max()) + 12)
    np.testing.assert_array_equal(got, want)
    assert b.steps == steps
    lsum = got.sum(-1)
    assert (lsum[got.any(-1)] < 1500).any()   # some capped playouts


def test_sharded_batches_give_the_whole_batch():
    grid = BOUNCE_GRIDS["default"]
    roots = make_roots(grid, 48, seed=11)
    whole = load(grid, roots, first_game=100).evaluate_moves(seed=SEED, playouts=16, max_plies=1024)
    half = [tuple(a[s] for a in roots) for s in (slice(0, 20), slice(20, 48))]
    lo = load(grid, half[0], first_game=100).evaluate_moves(seed=SEED, playouts=16, max_plies=1024)
    hi = load(grid, half[1], first_game=120).evaluate_moves(seed=SEED, playouts=16, max_plies=1024)
    np.testing.assert_array_equal(np.concatenate([lo, hi]), whole)


@pytest.mark.parametrize("playouts", [24, 700])
def test_device_path_writes_everything_in_stream_order(playouts):
    import torch

    grid = BOUNCE_GRIDS["default"]
    n = 64
    roots = make_roots(grid, n, seed=13)
    b = load(grid, roots, use_torch=True)
    ref = load(grid, roots)
    stream = torch.cuda.Stream(device=0)
    b.set_stream(stream.cuda_stream)
    shape = (n, 6, 54, 3)
    with torch.cuda.stream(stream):
        out = torch.full(shape, -1, dtype=torch.int32, device="cuda:0")
        b.step_random(seed=SEED ^ 5, plies=2)      # enqueued before the evaluation on the same stream
        b.evaluate_moves_tensor(out, seed=SEED, playouts=playouts, max_plies=512)
    stream.synchronize()
    got = out.cpu().numpy()
    assert (got >= 0).all()
    ref.step_random(seed=SEED ^ 5, plies=2)
    assert snapshot(ref) == snapshot(b)
    np.testing.assert_array_equal(got, ref.evaluate_moves(seed=SEED, playouts=playouts, max_plies=512))
    want, _ = expected_by_slot(grid, (ref.grid, ref.player, ref.winner, ref.plies), SEED, 0, playouts, 512)
    np.testing.assert_array_equal(got, want)


def test_full_size_default_board_against_the_oracle():
    """about 10^6 playouts on the default board, mid-game roots, cap 1024: the run holds capped playouts"""
    from simulator.batch import BounceBatch

    n, playouts = 1024, 48
    b = BounceBatch(BOUNCE_GRIDS["default"], n)
    b.step_random(seed=SEED ^ 1, plies=3)
    b.step_random(seed=SEED ^ 2, plies=4)
    roots = (b.grid, b.player, b.winner, b.plies)
    b.reset_steps()
    got = b.evaluate_moves(seed=SEED, playouts=playouts, max_plies=1024)
    want, steps = expected_by_slot(BOUNCE_GRIDS["default"], roots, SEED, 0, playouts, 1024)
    np.testing.assert_array_equal(got, want)
    assert b.steps == steps
    t = b.targets[:, :6]
    legal = ((t[..., None] >> np.arange(54, dtype=np.uint64)) & np.uint64(1)) != 0
    assert legal.sum() * playouts > 700_000
    per_slot = got.sum(-1)
    assert (per_slot[~legal] == 0).all()
    assert (per_slot[legal] < playouts).any(), "no capped playout: the straggler path was not exercised"


def test_monte_carlo_agent_on_bounce_states():
    from simulator.agents import BOUNCE_MAX_PLIES, MonteCarloAgent
    from simulator.game.bounce import Config

    config = Config(BOUNCE_GRIDS["default"])
    states = [config.sample_initial_state()]
    rng = np.random.default_rng(3)
    for _ in range(5):
        s = states[-1]
        for _ in range(int(rng.integers(1, 4))):
            if s.has_ended:
                break
            acts = s.actions
            s = acts[int(rng.integers(len(acts)))].sample_next_state()
        if not s.has_ended:
            states.append(s)
    agent = MonteCarloAgent(playouts=32, seed=SEED)
    many = agent.predict_many(states)
    for g, (s, m) in enumerate(zip(states, many)):
        assert list(m) == s.actions
        assert m == agent.predict(s, game=g)
        assert all(0.0 <= v <= 1.0 for v in m.values())
    # the values are the oracle's counts
    g = np.stack([s.grid for s in states])
    roots = (g, np.array([s.player for s in states], np.int8), np.full(len(states), -1, np.int8),
             np.array([s._plies for s in states], np.int32))
    want, _ = expected_by_slot(config.grid, roots, SEED, 0, 32, BOUNCE_MAX_PLIES)
    for k, s in enumerate(states):
        for a in s.actions:
            (sx, _), (tx, ty) = a._source, a._target
            wdl = want[k, sx, ty * 6 + tx]
            assert many[k][a] == (wdl[0] + 0.5 * wdl[1]) / 32
    agent.close()


def test_refusals():
    import torch

    from simulator.batch import BounceBatch, ConnectBatch
    from simulator.game import _abi

    grid = BOUNCE_GRIDS["default"]
    b = BounceBatch(grid, 4)
    with pytest.raises(ValueError, match="Connect"):
        b.evaluate_actions()
    with pytest.raises(ValueError, match="playouts"):
        b.evaluate_moves(playouts=0)
    with pytest.raises(ValueError, match="max_plies"):
        b.evaluate_moves(max_plies=0)
    t = torch.zeros(4 * 6 * 54 * 3 + 4, dtype=torch.int32, device="cuda:0")
    rc = _abi.lib().bgs_bounce_evaluate_moves(b._handle, 1, 8, 100, ctypes.c_void_p(t.data_ptr() + 4), 1)
    assert rc == _abi.BGS_ERR_ARG and "aligned" in _abi.last_error()
    c = ConnectBatch(6, 7, 4, 4)
    out = np.zeros(4 * 7 * 42 * 3, dtype=np.int32)
    assert _abi.lib().bgs_bounce_evaluate_moves(c._handle, 1, 8, 100, ctypes.c_void_p(out.ctypes.data), 0) == _abi.BGS_ERR_ARG
    assert "Bounce" in _abi.last_error()
    wide = np.zeros((9, 8), dtype=np.int8)   # 72 cells: a generic board
    wide[1] = wide[7] = 1
    with pytest.raises(ValueError, match="bit-packed"):
        BounceBatch(wide, 4).evaluate_moves()
    big = np.zeros((3, 21), dtype=np.int8)   # S = 21 * 63; 2^22 boards x S x (2^31 - 1) playouts > 2^63
    big[1] = 1
    huge = BounceBatch(big, 1 << 22)
    with pytest.raises(ValueError, match="overflows"):
        huge.evaluate_moves(playouts=2**31 - 1)
    huge.close()
