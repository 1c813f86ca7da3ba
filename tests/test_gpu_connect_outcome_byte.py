"""GPU tests of the outcome byte of the Connect4(6,7,4) rollout (csrc/connect_unit.h: connect_outcome4; connect_kernels.hip:
k_connect_rollout_opened and k_connect_rollout_opened_steps; docs/EXPERIMENTS.md §29): a game that ends leaves its stones
and a run flag, and status, rewards, 2-bit codes and env-steps are derived from those bytes when a chunk is flushed.

From the initial state, uncapped, against the CPU oracle: boards, winner, rewards, has_ended, plies, the env-steps of every
batch, the fused codes and the host arrays of a RewardSink -- through the one-step launch with and without fused codes,
and through five-step executor calls with connect_group=2 (launches of 2 + 2 + 1 steps) and connect_group=3 (3 + 2): both
slice parities, a transition into a step while the one before is still pending, and a last launch that writes boards.
The shapes are one game, one short of and one past a wave's 64 lanes, a ragged batch and 2^16 games, the last two from
game 77 on.  The classes an outcome rule can get wrong are counted from the oracle alone for every seed played at 2^16:
draws, full boards that are won (a stones-only rule would call them draws), the shortest games, and games ending at each
of the four ply positions of a block."""

import functools

import numpy as np
import pytest

from tests.knobs import knobs
from oracle import oracle

pytestmark = pytest.mark.gpu

SEED = 0x0123456789ABCDEF   # bench.py's
SHAPES = [(1, 0), (63, 0), (65, 0), (6000, 77), (1 << 16, 77)]
DRAW = 2   # the oracle's winner of a full board without a run
CALL = 5   # steps of the grouped call: seeds SEED .. SEED + 4
# at 2^16 games from game 77 on, seeds SEED .. SEED + 4 give 140 .. 174 draws, 35 .. 60 full boards won, 1027 .. 1103
# seven-ply games and 14328 .. 18486 games ending at each ply position (the oracle, counted on the CPU)
AT_LEAST = {"draws": 100, "full boards that are won": 30, "games of seven plies": 500,
            "ending at ply position 0": 10_000, "ending at ply position 1": 10_000,
            "ending at ply position 2": 10_000, "ending at ply position 3": 10_000}


@functools.lru_cache(maxsize=None)
def expected(n, first, seed=SEED):
    """the oracle's full rollout: grid, winner, reward, ended, plies, env-steps (computed once, never modified)"""
    orc = oracle.ConnectOracle(6, 7, 4, n)
    steps = orc.rollout(seed, first_game=first)
    arrays = (orc.grid.copy(), orc.winner.copy(), orc.reward.copy(), orc.ended.copy(), orc.plies.copy())
    for a in arrays:
        a.setflags(write=False)
    return arrays + (steps,)


def check_classes(n, first, seed=SEED):
    if n != 1 << 16:
        return
    _, winner, _, _, plies, _ = expected(n, first, seed)
    counts = {"draws": winner == DRAW, "full boards that are won": (plies == 42) & (winner != DRAW),
              "games of seven plies": plies == 7}
    for k in range(4):
        counts[f"ending at ply position {k}"] = (plies - 1) % 4 == k
    for name, least in AT_LEAST.items():
        count = int(counts[name].sum())
        print(f"n = {n}, first game {first}, seed + {seed - SEED}: {name}: {count} (at least {least})")
        assert count >= least, (name, seed - SEED)


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
    """the kernel without fused codes; a repeat of the call adds the same env-steps and leaves identical arrays"""
    from simulator.batch import ConnectBatch

    check_classes(n, first)
    b = ConnectBatch(6, 7, 4, n, device=0)
    b.set_first_game(first)
    for call in (1, 2):
        b.rollout(SEED, from_initial=True)
        _check(b, n, first, f"n = {n}, call {call}", calls=call)
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
    buf = torch.full(((n + 63) // 64 * 16,), 0xAA, dtype=torch.uint8, device="cuda")
    b.rollout_outcomes_tensor(buf, SEED, from_initial=True)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(expand_outcomes_host(buf[:nbytes].cpu().numpy(), n), reward, err_msg="codes")
    _check(b, n, first, f"n = {n}, fused codes")
    sink = RewardSink(n, slots=2, threads=2)
    host = np.full((n, 2), 9, dtype=np.int8)
    sink.wait(sink.rollout(b, host, SEED, from_initial=True))
    np.testing.assert_array_equal(host, reward, err_msg="host array")
    _check(b, n, first, f"n = {n}, sink", calls=2)
    sink.close()
    b.close()


def _grouped(group, n, first, plan, depth=3, slots=8):
    import torch
    from simulator.batch import ConnectBatch, RewardSink
    from simulator.pipeline import RolloutExecutor

    old = knobs.get("connect_group")
    knobs["connect_group"] = str(group)
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
            "plies": [b.plies.copy() for b in batches], "env_steps": [b.steps for b in batches],
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


@pytest.mark.parametrize("group", [2, 3])
@pytest.mark.parametrize("n,first", SHAPES)
def test_grouped_five_step_call(n, first, group):
    """Step s is batch s % 3 with seed SEED + s.  Every host array, what every batch is left with -- steps 3, 4 and 2 write
    the boards of batches 0, 1 and 2; with connect_group=2 step 4 is a one-step launch -- and the env-steps of every batch."""
    for s in range(CALL):
        check_classes(n, first, SEED + s)
    depth = 3
    got = _grouped(group, n, first, [(CALL, True)], depth)
    assert got["steps"] == got["handovers"] == CALL
    for s in range(CALL):
        np.testing.assert_array_equal(got["hosts"][s], expected(n, first, SEED + s)[2], err_msg=f"hand-over {s}")
    for k in range(depth):
        mine = [s for s in range(CALL) if s % depth == k]
        grid, winner, reward, ended, plies, _ = expected(n, first, SEED + mine[-1])
        np.testing.assert_array_equal(got["grid"][k], grid, err_msg=f"batch {k}: grid")
        np.testing.assert_array_equal(got["winner"][k], winner, err_msg=f"batch {k}: winner")
        np.testing.assert_array_equal(got["reward"][k], reward, err_msg=f"batch {k}: reward")
        np.testing.assert_array_equal(got["ended"][k], ended, err_msg=f"batch {k}: has_ended")
        np.testing.assert_array_equal(got["plies"][k], plies, err_msg=f"batch {k}: plies")
        assert got["env_steps"][k] == sum(expected(n, first, SEED + s)[5] for s in mine), f"batch {k}: env-steps"
