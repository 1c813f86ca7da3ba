"""GPU tests of the leaner lock-step opening of the Connect4(6,7,4) rollout (connect_kernels.hip: open_games_deferred,
NibblePlies::cheap / cheap_first, open_games_per_ply; docs/EXPERIMENTS.md §40): the blind ply's position as a multiply-add
and a subtract, ply 0 written out for the empty board, and the slot's words parked in the pieces they lie in registers as.
Results are bit for bit what they were, so everything is compared with the CPU oracle -- boards, winner, has_ended, plies,
rewards, env-steps and the 2-bit codes -- under the default contract and, for the one-step kernel, under the strict one
(open_games_per_ply and NibblePlies::cheap):

  * 333 games in chunks of 128: three waves, the first two refill their pool inside the chunk, the last is ragged;
  * 6000 games from game 77 on: through the executor (grouped launches, five steps, depth 3) and in one launch.  Of the
    games of a batch 13.5 % are flagged at the opening's stage 1, 21.3 % at stage 2 and 1.3 % have a column closed after
    11 plies (tools/refill_model.py), so every park and the replay are taken hundreds of times;
  * 128 games from game 2^32 - 40 on: the lanes of a wave differ in the HIGH word of the game id, which is a word of the
    philox counter.

The run-time geometry 6x5x4 (NibblePlies::cheap with the board's sizes in SGPRs) is compared with the any-geometry kernel
on the same seeds."""

import functools

import numpy as np
import pytest

from tests.knobs import knobs
from oracle import oracle

pytestmark = pytest.mark.gpu

SEED = 0x0123456789ABCDEF   # bench.py's
CARRY = 2**32 - 40
CALL, DEPTH = 5, 3
# (n, first game, chunk knob or None)
SMALL_CHUNKS = (333, 3 << 34, "128")
RAGGED = (6000, 77, None)
ACROSS_CARRY = (128, CARRY, None)


@functools.lru_cache(maxsize=None)
def expected(n, first, seed, per_ply=False):
    """the oracle's rollout of n games of 6x7x4 from the initial state (computed once, read-only)"""
    orc = oracle.ConnectOracle(6, 7, 4, n, per_ply=per_ply)
    steps = orc.rollout(seed, first_game=first)
    out = {"grid": orc.grid.copy(), "winner": orc.winner.copy(), "reward": orc.reward.copy(), "ended": orc.ended.copy(),
           "plies": orc.plies.copy()}
    # the 2-bit codes: 1 / 2 the winner's, 3 a draw (every game has ended: no cap), four games a byte
    assert out["ended"].all()
    code = np.where(out["reward"][:, 0] > 0, 1, np.where(out["reward"][:, 1] > 0, 2, 3)).astype(np.uint8)
    code = np.concatenate([code, np.zeros(-n % 4, dtype=np.uint8)]).reshape(-1, 4)
    out["codes"] = (code[:, 0] | (code[:, 1] << 2) | (code[:, 2] << 4) | (code[:, 3] << 6)).astype(np.uint8)
    for a in out.values():
        a.setflags(write=False)
    out["steps"] = steps
    assert steps == int(out["plies"].sum())
    return out


def _check_batch(b, want, what, calls=1):
    np.testing.assert_array_equal(b.grid, want["grid"], err_msg=f"{what}: grid")
    np.testing.assert_array_equal(b.winner, want["winner"], err_msg=f"{what}: winner")
    np.testing.assert_array_equal(b.has_ended, want["ended"], err_msg=f"{what}: has_ended")
    np.testing.assert_array_equal(b.plies, want["plies"], err_msg=f"{what}: plies")
    np.testing.assert_array_equal(b.reward, want["reward"], err_msg=f"{what}: reward")
    assert b.steps == calls * want["steps"], f"{what}: env-steps"


def _one_step(shape, contract, monkeypatch):
    """the one-step kernel without and with fused codes, on one batch: two launches"""
    import torch
    from simulator.batch import ConnectBatch, expand_outcomes_host

    n, first, chunk = shape
    if chunk is not None:
        monkeypatch.setitem(knobs, "rollout_chunk", chunk)
    want = expected(n, first, SEED, contract == "per-ply")
    b = ConnectBatch(6, 7, 4, n, use_torch=True)
    b.set_rng_contract(contract)
    b.set_first_game(first)
    b.rollout(SEED, from_initial=True)
    _check_batch(b, want, f"{contract}, n = {n} from game {first}")
    buf = torch.full(((n + 63) // 64 * 16,), 0xAA, dtype=torch.uint8, device="cuda")
    b.rollout_outcomes_tensor(buf, SEED, from_initial=True)
    torch.cuda.synchronize()
    packed = buf[: (n + 3) // 4].cpu().numpy()
    np.testing.assert_array_equal(packed, want["codes"], err_msg="codes")
    np.testing.assert_array_equal(expand_outcomes_host(packed, n), want["reward"], err_msg="codes, expanded")
    _check_batch(b, want, f"{contract}, n = {n} from game {first}, fused codes", calls=2)
    b.close()


@pytest.mark.parametrize("contract", ["per-block", "per-ply"])
@pytest.mark.parametrize("shape", [SMALL_CHUNKS, RAGGED, ACROSS_CARRY], ids=["chunks-of-128", "ragged-6000", "carry"])
def test_one_step_kernel_equals_the_oracle(shape, contract, monkeypatch):
    _one_step(shape, contract, monkeypatch)


def _grouped(group, n, first):
    """a five-step executor call with hand-over on three batches under connect_group=`group`; what a caller can read"""
    import torch
    from simulator.batch import ConnectBatch, RewardSink
    from simulator.pipeline import RolloutExecutor

    old = knobs.get("connect_group")
    knobs["connect_group"] = str(group)
    try:
        batches = []
        for _ in range(DEPTH):
            with torch.cuda.stream(torch.cuda.Stream()):
                b = ConnectBatch(6, 7, 4, n, use_torch=True)
            b.set_first_game(first)
            batches.append(b)
        hosts = [np.full((n, 2), 9, dtype=np.int8) for _ in range(8)]
        sink = RewardSink(n, slots=8, threads=3)
        exe = RolloutExecutor(batches, sink=sink, host_arrays=hosts, seed0=SEED)
        exe.enqueue(CALL, True)
        exe.drain()
        assert exe.steps == exe.handovers == CALL
        for s in range(CALL):
            np.testing.assert_array_equal(hosts[s], expected(n, first, SEED + s)["reward"], err_msg=f"hand-over {s}")
        for k, b in enumerate(batches):
            mine = [s for s in range(CALL) if s % DEPTH == k]
            want = dict(expected(n, first, SEED + mine[-1]))
            want["steps"] = sum(expected(n, first, SEED + s)["steps"] for s in mine)
            _check_batch(b, want, f"group {group}, batch {k}")
        exe.close()
        sink.close()
        for b in batches:
            b.close()
    finally:
        if old is None:
            knobs.pop("connect_group", None)
        else:
            knobs["connect_group"] = old


@pytest.mark.parametrize("group", [2, 3])
@pytest.mark.parametrize("shape", [RAGGED, ACROSS_CARRY], ids=["ragged-6000", "carry"])
def test_grouped_launches_equal_the_oracle(shape, group):
    """Step s is batch s % 3 with seed SEED + s: every host array, the boards the last step on each batch leaves, and the
    env-steps of every batch.  connect_group = 2: launches of 2 + 2 + 1 steps; 3: 3 + 2."""
    n, first, _ = shape
    _grouped(group, n, first)


def _run_6x5(contract, codes):
    import torch
    from simulator.batch import ConnectBatch

    n = 333
    b = ConnectBatch(6, 5, 4, n)
    b.set_rng_contract(contract)
    b.set_first_game(3 << 34)
    packed = torch.zeros((n + 63) // 64 * 16, dtype=torch.uint8, device="cuda")
    if codes:
        b.rollout_outcomes_tensor(packed, SEED ^ 78, from_initial=True)
        torch.cuda.synchronize()
    else:
        b.rollout(SEED ^ 78, from_initial=True)
    out = {"grid": b.grid.copy(), "winner": b.winner.copy(), "ended": b.has_ended.copy(), "plies": b.plies.copy(),
           "reward": b.reward.copy(), "steps": b.steps, "codes": packed.cpu().numpy()[: (n + 3) // 4].copy()}
    b.close()
    return out


@pytest.mark.parametrize("contract", ["per-block", "per-ply"])
def test_run_time_geometry_equals_the_any_geometry_kernel(contract, monkeypatch):
    """6x5x4, 333 games in chunks of 128, with one to four opening blocks, with and without fused codes."""
    monkeypatch.setitem(knobs, "rollout_chunk", "128")
    monkeypatch.setitem(knobs, "rollout_generic", "1")
    want = _run_6x5(contract, codes=True)
    monkeypatch.delitem(knobs, "rollout_generic")
    assert want["steps"] > 0 and want["ended"].all()
    for opening in ("1", "2", "3", "4"):
        monkeypatch.setitem(knobs, "rollout_opening", opening)
        for codes in (False, True):
            got = _run_6x5(contract, codes)
            what = f"6x5x4 {contract} opening {opening} codes {codes}"
            for name in ("grid", "winner", "ended", "plies", "reward"):
                np.testing.assert_array_equal(got[name], want[name], err_msg=f"{name} {what}")
            assert got["steps"] == want["steps"], what
            if codes:
                np.testing.assert_array_equal(got["codes"], want["codes"], err_msg=f"codes {what}")
