"""GPU tests of the executor's grouped Connect launches (bgs_pipeline.hip, k_connect_rollout_opened_steps): consecutive
steps from the initial state share ONE launch, every wave carrying its lanes from one step's chunk into the next.
Grouped and one-launch-per-step runs (experiment connect_group=1, the test library) must leave the same host arrays,
hand-over order, batch boards, rewards and env-step counts; a sample is checked against the CPU oracle.  By default only
calls of at least kConnectGroupMinCall (48) steps are grouped; connect_group=N groups calls of any length."""

import numpy as np
import pytest

from tests.knobs import knobs
from oracle import oracle

pytestmark = pytest.mark.gpu

SEED = 0x0123456789ABCDEF


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


def _run(group, n, plan, depth=3, slots=9, first=77, close_early=False):
    """Enqueue `plan` -- a list of (count, handover) calls -- under connect_group=`group` (None: the library's default) and
    return what a caller can read: every host array, the hand-over count, the last host array's index and, per batch,
    its boards, rewards and env-steps."""
    from simulator.batch import RewardSink
    from simulator.pipeline import RolloutExecutor

    old = knobs.get("connect_group")
    if group is None:
        knobs.pop("connect_group", None)
    else:
        knobs["connect_group"] = str(group)
    try:
        batches = _batches(n, depth, first)
        hosts = [np.full((n, 2), 9, dtype=np.int8) for _ in range(slots)]
        sink = RewardSink(n, slots=slots, threads=3)
        exe = RolloutExecutor(batches, sink=sink, host_arrays=hosts, seed0=SEED)
        for count, handover in plan:
            exe.enqueue(count, handover)
        handovers, steps = exe.handovers, exe.steps
        if close_early:
            exe.close()   # destroy with the steps still in flight: it delivers them first
            last = None
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
        if old is None:
            knobs.pop("connect_group", None)
        else:
            knobs["connect_group"] = old


def _same(a, b):
    assert a["handovers"] == b["handovers"] and a["steps"] == b["steps"] and a["last"] == b["last"]
    for k, (x, y) in enumerate(zip(a["hosts"], b["hosts"])):
        np.testing.assert_array_equal(x, y, err_msg=f"host array {k}")
    for k in range(len(a["grid"])):
        np.testing.assert_array_equal(a["grid"][k], b["grid"][k], err_msg=f"batch {k} boards")
        np.testing.assert_array_equal(a["reward"][k], b["reward"][k], err_msg=f"batch {k} rewards")
    assert a["env_steps"] == b["env_steps"]


@pytest.mark.parametrize("group", [2, 3])
@pytest.mark.parametrize("n", [6000, 300_001])   # ragged: the last wave's chunk is short, n is no multiple of 4
def test_grouped_equals_per_step(group, n):
    """Counts that are no multiple of S (1, S - 1, S + 1, 2S + 1 for S = 2 and 3), steps without hand-over in between."""
    plan = [(1, True), (2, True), (3, True), (5, True), (4, False), (7, True)]
    _same(_run(group, n, plan), _run(1, n, plan))


@pytest.mark.parametrize("depth,slots", [(1, 2), (2, 4), (4, 8)])
def test_grouped_other_depths(depth, slots):
    plan = [(5, True), (3, False), (6, True)]
    _same(_run(2, 20_000, plan, depth, slots), _run(1, 20_000, plan, depth, slots))


def test_grouped_destroy_in_flight():
    plan = [(4, True), (9, True)]
    _same(_run(2, 300_001, plan, close_early=True), _run(1, 300_001, plan, close_early=True))


@pytest.mark.parametrize("plan", [[(47, True), (48, True)], [(60, True), (50, False), (49, True)]])
def test_default_groups_long_calls(plan):
    """The library's default: calls shorter than 48 steps launch per step, longer ones in groups of two."""
    _same(_run(None, 6000, plan), _run(1, 6000, plan))


def test_grouped_matches_the_oracle():
    """Every host array and every batch against the oracle: step s is batch s % depth, seed SEED + s."""
    n, first, depth, slots = 6000, 77, 3, 9
    got = _run(2, n, [(3, True), (8, True), (50, True)], depth, slots, first)
    for j in range(got["handovers"] - slots, got["handovers"]):
        orc = oracle.ConnectOracle(6, 7, 4, n)
        orc.rollout(SEED + j, first_game=first)
        np.testing.assert_array_equal(got["hosts"][j % slots], orc.reward, err_msg=f"hand-over {j}")
    for k in range(depth):
        s = max(s for s in range(got["steps"]) if s % depth == k)
        orc = oracle.ConnectOracle(6, 7, 4, n)
        orc.rollout(SEED + s, first_game=first)
        np.testing.assert_array_equal(got["reward"][k], orc.reward, err_msg=f"batch {k} (step {s})")
        np.testing.assert_array_equal(got["grid"][k], orc.grid, err_msg=f"batch {k} (step {s})")


def test_feeder_path_is_unchanged():
    """bgs_pipeline_feed enqueues one step at a time: the same host arrays with and without grouping switched off."""
    from simulator.batch import RewardSink
    from simulator.pipeline import RolloutExecutor

    n, slots = 20_000, 6
    seeds = np.arange(11, dtype=np.uint64) * np.uint64(1000003) + np.uint64(5)
    results = []
    for group in (None, 1):
        if group is None:
            knobs.pop("connect_group", None)
        else:
            knobs["connect_group"] = str(group)
        try:
            batches = _batches(n, 3, 0)
            hosts = [np.zeros((n, 2), dtype=np.int8) for _ in range(slots)]
            sink = RewardSink(n, slots=slots, threads=2)
            got = []
            with RolloutExecutor(batches, sink=sink, host_arrays=hosts, seed0=SEED) as exe:
                exe.feed(seeds)
                for j in range(len(seeds)):
                    exe.wait_handover(j)
                    got.append(hosts[j % slots].copy())
                    exe.release(j)
                exe.drain()
            sink.close()
            for b in batches:
                b.close()
            results.append(got)
        finally:
            knobs.pop("connect_group", None)
    for j, (x, y) in enumerate(zip(*results)):
        np.testing.assert_array_equal(x, y, err_msg=f"fed step {j}")
    orc = oracle.ConnectOracle(6, 7, 4, n)
    orc.rollout(int(seeds[-1]), first_game=0)
    np.testing.assert_array_equal(results[0][-1], orc.reward)
