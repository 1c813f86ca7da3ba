"""GPU tests of the deferred opening of the Connect4(6,7,4) rollout (csrc/connect_kernels.hip: open_games_deferred, refetch;
docs/EXPERIMENTS.md §27): the lock-step opening plays plies 5 .. 16 without per-ply tests, one whole-board run test per
player stands for them, and the games it flags are parked at an earlier state and replayed by the refill loop.

From the initial state, uncapped, seed 0x0123456789ABCDEF, against the CPU oracle: boards, winners, rewards, has_ended and
the env-step count, the fused outcome codes and the host arrays of a RewardSink, through the one-step launch (with and
without fused codes) and through grouped executor calls (connect_group=2, whose odd last step is a one-step launch).
The shapes are one game, one short of and one past a wave's 64 lanes, a ragged batch (a short last chunk and a partial last
opening, first game 77) and 2^16 games.  The class of every game -- ended inside the speculative plies, a column full
before their last draw, replayed past the eight parked words, flagged only at stage 2, drawn -- is derived from the oracle
alone (capped rollouts of 11, 12, 15 and 16 plies), and the samples are asserted to hold enough of each."""

import functools

import numpy as np
import pytest

from tests.knobs import knobs
from oracle import oracle

pytestmark = pytest.mark.gpu

SEED = 0x0123456789ABCDEF
SHAPES = [(1, 0), (63, 0), (65, 0), (6000, 77), (1 << 16, 0)]
DRAW = 2   # the oracle's winner of a full board without a run


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def expected(n, first, seed=SEED):
    """the oracle's full rollout: grid, winner, reward, ended, plies, env-steps (computed once, never modified)"""
    orc = oracle.ConnectOracle(6, 7, 4, n)
    steps = orc.rollout(seed, first_game=first)
    return _frozen(orc.grid.copy(), orc.winner.copy(), orc.reward.copy(), orc.ended.copy(), orc.plies.copy()) + (steps,)


@functools.lru_cache(maxsize=None)
def classes(n, first):
    """every game's class under seed SEED, from the oracle alone"""
    def capped(cap):
        orc = oracle.ConnectOracle(6, 7, 4, n)
        orc.rollout(SEED, first_game=first, max_plies=cap)
        assert int(orc.plies.max()) <= cap
        return orc.ended.copy(), (orc.grid != -1).sum(axis=1).max(axis=1)   # ended, the tallest column (empty cell -1)

    ended11, tall11 = capped(11)
    ended12, _ = capped(12)
    ended15, tall15 = capped(15)
    ended16, _ = capped(16)
    _, winner, _, _, plies, _ = expected(n, first)
    column11 = ~ended12 & ~ended11 & (tall11 == 6)          # a column full after 11 plies, and the game goes on
    stage1 = ended12 | (~ended11 & (tall11 == 6))
    stage2 = ~stage1 & (ended16 | (~ended15 & (tall15 == 6)))
    return {
        "ended within 12 plies": ended12,
        "column full after 11 plies and still running": column11,
        "... longer than 36 plies (the words run out)": column11 & (plies > 36),
        "... longer than 40 plies": column11 & (plies > 40),
        "flagged only at stage 2": stage2,
        "flagged only at stage 2, by a column alone, and goes on": stage2 & ~ended16,
        "boards played full (42 plies)": plies == 42,
        "draws": winner == DRAW,
    }


AT_LEAST = {
    (1 << 16, 0): {"ended within 12 plies": 1000, "column full after 11 plies and still running": 100,
                   "... longer than 36 plies (the words run out)": 10, "... longer than 40 plies": 3,
                   "flagged only at stage 2": 1000, "flagged only at stage 2, by a column alone, and goes on": 1000,
                   "boards played full (42 plies)": 50, "draws": 50},
    (6000, 77): {"ended within 12 plies": 100, "column full after 11 plies and still running": 10},
}


def check_classes(n, first):
    for name, least in AT_LEAST.get((n, first), {}).items():
        count = int(classes(n, first)[name].sum())
        print(f"n = {n}, first game {first}: {name}: {count} (at least {least})")
        assert count >= least, name


def _check(b, n, first, what, calls=1):
    grid, winner, reward, ended, plies, steps = expected(n, first)
    np.testing.assert_array_equal(b.winner, winner, err_msg=f"{what}: winner")
    np.testing.assert_array_equal(b.grid, grid, err_msg=f"{what}: grid")
    np.testing.assert_array_equal(b.reward, reward, err_msg=f"{what}: reward")
    np.testing.assert_array_equal(b.has_ended, ended, err_msg=f"{what}: has_ended")
    np.testing.assert_array_equal(b.plies, plies, err_msg=f"{what}: plies")
    assert b.steps == calls * steps == calls * int(plies.sum()), what


@pytest.mark.parametrize("n,first", SHAPES)
def test_one_step_launch(n, first):
    """the kernel without fused codes; a repeat of the call leaves identical arrays"""
    from simulator.batch import ConnectBatch

    check_classes(n, first)
    b = ConnectBatch(6, 7, 4, n, device=0)
    b.set_first_game(first)
    b.rollout(SEED, from_initial=True)
    _check(b, n, first, f"n = {n}")
    b.rollout(SEED, from_initial=True)
    _check(b, n, first, f"n = {n}, repeated", calls=2)
    b.close()


@pytest.mark.parametrize("n,first", SHAPES)
def test_one_step_launch_with_fused_codes(n, first):
    """the kernel that writes the 2-bit outcome codes itself: into a device buffer, and into a RewardSink's slot"""
    import torch
    from simulator.batch import ConnectBatch, RewardSink, expand_outcomes_host

    check_classes(n, first)
    reward = expected(n, first)[2]
    b = ConnectBatch(6, 7, 4, n, use_torch=True)
    b.set_first_game(first)
    nbytes = (n + 3) // 4
    for call in (1, 2):
        buf = torch.full(((n + 63) // 64 * 16,), 0xAA, dtype=torch.uint8, device="cuda")
        b.rollout_outcomes_tensor(buf, SEED, from_initial=True)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(expand_outcomes_host(buf[:nbytes].cpu().numpy(), n), reward, err_msg=f"codes, call {call}")
        _check(b, n, first, f"n = {n}, fused codes, call {call}", calls=call)
    sink = RewardSink(n, slots=2, threads=2)
    for call in (3, 4):
        host = np.full((n, 2), 9, dtype=np.int8)
        sink.wait(sink.rollout(b, host, SEED, from_initial=True))
        np.testing.assert_array_equal(host, reward, err_msg=f"host array, call {call}")
        _check(b, n, first, f"n = {n}, sink, call {call}", calls=call)
    sink.close()
    b.close()


def _grouped(n, first, plan, depth=3, slots=8):
    import torch
    from simulator.batch import ConnectBatch, RewardSink
    from simulator.pipeline import RolloutExecutor

    old = knobs.get("connect_group")
    knobs["connect_group"] = "2"
    try:
        batches = []
        for _ in range(depth):
            with torch.cuda.stream(torch.cuda.Stream()):
                b = ConnectBatch(6, 7, 4, n, use_torch=True)
            b.set_first_game(first)
            batches.append(b)
        hosts = [np.full((n, 2), 9, dtype=np.int8) for _ in range(slots)]
        sink = RewardSink(n, slots=slots, threads=3)
        exe = RolloutExecutor(batches, sink=sink, host_arrays=hosts, seed0=SEED)
        for count, handover in plan:
            exe.enqueue(count, handover)
        exe.drain()
        out = {
            "steps": exe.steps, "handovers": exe.handovers, "hosts": [h.copy() for h in hosts],
            "grid": [b.grid.copy() for b in batches], "winner": [b.winner.copy() for b in batches],
            "reward": [b.reward.copy() for b in batches], "ended": [b.has_ended.copy() for b in batches],
            "env_steps": [b.steps for b in batches],
        }
        exe.close()
        sink.close()
        for b in batches:
            b.close()
        return out
    finally:
        if old is None:
            knobs.pop("connect_group", None)
        else:
            knobs["connect_group"] = old


@pytest.mark.parametrize("n,first", SHAPES)
def test_grouped_launch(n, first):
    """connect_group=2: calls of 4 and 3 steps are launches of 2 + 2 and 2 + 1 steps -- the last step a one-step launch.
    Step s is batch s % 3 with seed SEED + s (step 0 plays the sample whose classes are counted): every host array, and
    what every batch is left with, against the oracle; a repeat leaves identical arrays."""
    check_classes(n, first)
    depth, plan = 3, [(4, True), (3, True)]
    total = sum(count for count, _ in plan)
    got = _grouped(n, first, plan, depth)
    assert got["steps"] == got["handovers"] == total
    for s in range(total):
        np.testing.assert_array_equal(got["hosts"][s], expected(n, first, SEED + s)[2], err_msg=f"hand-over {s}")
    for k in range(depth):
        mine = [s for s in range(total) if s % depth == k]
        grid, winner, reward, ended, _, _ = expected(n, first, SEED + mine[-1])
        np.testing.assert_array_equal(got["grid"][k], grid, err_msg=f"batch {k}: grid")
        np.testing.assert_array_equal(got["winner"][k], winner, err_msg=f"batch {k}: winner")
        np.testing.assert_array_equal(got["reward"][k], reward, err_msg=f"batch {k}: reward")
        np.testing.assert_array_equal(got["ended"][k], ended, err_msg=f"batch {k}: has_ended")
        assert got["env_steps"][k] == sum(expected(n, first, SEED + s)[5] for s in mine), f"batch {k}: env-steps"
    again = _grouped(n, first, plan, depth)
    for key in ("hosts", "grid", "winner", "reward", "ended"):
        for k, (x, y) in enumerate(zip(got[key], again[key])):
            np.testing.assert_array_equal(x, y, err_msg=f"repeat: {key} {k}")
    assert got["env_steps"] == again["env_steps"]
