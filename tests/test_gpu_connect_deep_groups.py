"""GPU tests of deep grouped Connect launches (bgs_pipeline.hip, connect_group_plan.h, the sink's ring in bgs_host.hip):
launches of up to eight steps on a sink whose ring of 32 code slots is larger than the caller's nine host arrays, planned
for the whole call (launches of S, a taper, the last `depth` steps one by one), several steps in flight into one host
array.  Everything a caller can read -- the host arrays, the hand-over count, each batch's boards,
rewards and env-steps -- must be what one launch per step leaves (experiment connect_group=1, the test library), and the
last delivery into every host array must be the CPU oracle's."""

import functools

import numpy as np
import pytest

from tests.knobs import knobs
from oracle import oracle

pytestmark = pytest.mark.gpu

SEED = 0x0123456789ABCDEF
DEPTH, HOSTS = 3, 9   # bench.py's shape: three batches in flight, three host arrays a stream, RewardSink(slots=9)


def _batches(n, depth, first):
    import torch
    from simulator.batch import ConnectBatch

    out = []
    for _ in range(depth):
        with torch.cuda.stream(torch.cuda.Stream()):
            b = ConnectBatch(6, 7, 4, n, use_torch=True)
        b.set_first_game(first)
        out.append(b)
    return out


def _play(group, n, counts, first=77, depth=DEPTH, hosts_n=HOSTS, close_early=False):
    """Enqueue calls of `counts` steps with hand-over under connect_group=`group` (None: the library's default); returns
    what a caller can read afterwards."""
    from simulator.batch import RewardSink
    from simulator.pipeline import RolloutExecutor

    saved = {k: knobs.get(k) for k in ("connect_group",)}
    for k in saved:
        knobs.pop(k, None)
    if group is not None:
        knobs["connect_group"] = str(group)
    try:
        batches = _batches(n, depth, first)
        hosts = [np.full((n, 2), 9, dtype=np.int8) for _ in range(hosts_n)]
        sink = RewardSink(n, slots=hosts_n, threads=3)
        exe = RolloutExecutor(batches, sink=sink, host_arrays=hosts, seed0=SEED)
        for count in counts:
            exe.enqueue(count, True)
        handovers, steps = exe.handovers, exe.steps
        last = None
        if close_early:
            exe.close()   # destroy with launches in flight: it delivers them first
        else:
            exe.drain()
            last = next(k for k, h in enumerate(hosts) if h is exe.last_host_array())
            exe.close()
        out = {
            "hosts": [h.copy() for h in hosts],
            "handovers": handovers,
            "steps": steps,
            "last": last,
            "grid": [b.grid.copy() for b in batches],
            "reward": [b.reward.copy() for b in batches],
            "env_steps": [b.steps for b in batches],
        }
        sink.close()
        for b in batches:
            b.close()
        return out
    finally:
        for k, v in saved.items():
            knobs.pop(k, None)
            if v is not None:
                knobs[k] = v


@functools.lru_cache(maxsize=None)
def _per_step(n, counts, first=77, depth=DEPTH, hosts_n=HOSTS, close_early=False):
    """The reference: one launch per step.  Computed once per shape and shared."""
    return _play(1, n, counts, first, depth, hosts_n, close_early)


def _same(a, b):
    assert a["handovers"] == b["handovers"] and a["steps"] == b["steps"] and a["last"] == b["last"]
    for k, (x, y) in enumerate(zip(a["hosts"], b["hosts"])):
        np.testing.assert_array_equal(x, y, err_msg=f"host array {k}")
    for k in range(len(a["grid"])):
        np.testing.assert_array_equal(a["grid"][k], b["grid"][k], err_msg=f"batch {k} boards")
        np.testing.assert_array_equal(a["reward"][k], b["reward"][k], err_msg=f"batch {k} rewards")
    assert a["env_steps"] == b["env_steps"]


def _oracle_check(got, n, first, hosts_n=HOSTS):
    """The last step delivered into each host array is the oracle's for that step's seed."""
    for j in range(max(0, got["handovers"] - hosts_n), got["handovers"]):
        orc = oracle.ConnectOracle(6, 7, 4, n)
        orc.rollout(SEED + j, first_game=first)
        np.testing.assert_array_equal(got["hosts"][j % hosts_n], orc.reward, err_msg=f"hand-over {j}")


# 27 steps: 1 + 8 + 8, the taper 4 + 2 + 1, three single steps; 40: the tickets wrap the ring of 32; 100: three times
@pytest.mark.parametrize("group", [8, None])
@pytest.mark.parametrize("count", [27, 40, 100])
def test_deep_groups_equal_per_step(group, count):
    n = 6000   # from game 77 on: a ragged last wave and a ragged code byte
    got = _play(group, n, (count,))
    _same(got, _per_step(n, (count,)))
    if group == 8:
        _oracle_check(got, n, 77)


@pytest.mark.parametrize("n,first", [(65, 0), (1 << 16, 77)])   # two waves, the second with one game; 2^16
def test_deep_groups_sizes(n, first):
    got = _play(8, n, (40,), first)
    _same(got, _per_step(n, (40,), first))
    _oracle_check(got, n, first)


def test_a_launch_uses_every_host_array():
    """Eight host arrays at S = 8: a launch delivers into all of them, two steps in flight into one array are the rule."""
    got = _play(8, 6000, (40,), hosts_n=8)
    _same(got, _per_step(6000, (40,), hosts_n=8))
    _oracle_check(got, 6000, 77, 8)


def test_depth_two():
    got = _play(8, 6000, (40, 5, 27), depth=2)
    _same(got, _per_step(6000, (40, 5, 27), depth=2))
    _oracle_check(got, 6000, 77)


def test_destroy_with_deep_groups_in_flight():
    """Executor and sink destroyed with eight-step launches in flight: everything is delivered first, and the process
    goes on to play another call."""
    got = _play(8, 300_001, (9, 30), close_early=True)
    _same(got, _per_step(300_001, (9, 30), close_early=True))
    again = _play(8, 6000, (27,))
    _same(again, _per_step(6000, (27,)))
