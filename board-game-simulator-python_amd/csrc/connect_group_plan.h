// connect_group_plan.h -- how a call of `count` pipeline steps is cut into launches when the executor groups Connect
// steps (bgs_pipeline.hip, enqueue_steps; the kernel is k_connect_rollout_opened_steps).  Host code only, no HIP: the
// plan is a pure function of four integers and tests/test_connect_group_plan.py compiles it into a program of its own.
//
// A call is, front to back:
//   head    one launch of (head steps) % cap, when that is not 0, then launches of `cap` steps each;
//   taper   launches that halve, cap / 2, cap / 4, .., 1, and stay at 1 until the taper has at least `depth` launches;
//   last    `depth` one-step launches, each on its own batch's stream: the steps that leave the batches' boards.
// cap = min(steps per launch asked for, host arrays, code slots of the sink's ring): a launch delivers each of its steps
// into a host array and a ring slot of its own.  Launch g of the grouped ones goes to stream g % depth, so with the taper
// the `depth` streams run out of work within one short launch of each other; without it one stream would play a launch
// of `cap` steps alone at the end of every call.  What the plan guarantees (the test sweeps it):
//   * the launches cover the steps of the call once, in order;
//   * the last `depth` steps are launches of one;
//   * no launch is larger than cap;
//   * each of the `depth` launches in front of the last ones, and each of the last ones, is at most half the launch
//     before it, or is a launch of one.
// A call too short for a head (fewer than taper + cap steps in front of the last ones) is a taper alone that may start at
// cap: nothing runs before it that it would have to halve.
#pragma once

#include <stdint.h>

struct ConnectGroupPlan {
    int64_t grouped = 0;   // steps in front of the last `depth`
    int64_t head = 0;      // of those, the steps in front of the taper
    int64_t at = 0;        // steps handed out so far
    int64_t count = 0;
    int cap = 1;
    int prev = 0;          // the taper's previous launch (its first launch is at most prev / 2)
};

// steps of the canonical taper behind launches of `cap`: cap / 2, cap / 4, .., 1, then ones up to `depth` launches
constexpr int64_t connect_group_taper_steps(int cap, int depth) {
    int64_t sum = 0;
    int launches = 0;
    for (int k = cap / 2; k >= 1; k /= 2) {
        sum += k;
        ++launches;
    }
    return sum + (launches < depth ? depth - launches : 0);
}

constexpr ConnectGroupPlan connect_group_plan(int64_t count, int depth, int steps, int host_arrays, int ring) {
    ConnectGroupPlan p;
    p.count = count;
    int cap = steps;
    if (cap > host_arrays) cap = host_arrays;
    if (cap > ring) cap = ring;
    if (cap < 1) cap = 1;
    p.cap = cap;
    p.grouped = count > depth ? count - depth : 0;
    if (cap == 1) {   // one launch per step
        p.grouped = 0;
        return p;
    }
    const int64_t taper = connect_group_taper_steps(cap, depth);
    if (p.grouped >= taper + cap) {
        p.head = p.grouped - taper;
        p.prev = cap;
    } else {
        p.head = 0;
        p.prev = 2 * cap;
    }
    return p;
}

// the size of the next launch, 0 when the call is handed out
constexpr int connect_group_next(ConnectGroupPlan& p) {
    if (p.at >= p.count) return 0;
    int k = 1;
    if (p.at < p.head) {
        const int64_t odd = p.head % p.cap;
        k = p.at == 0 && odd != 0 ? (int)odd : p.cap;
    } else if (p.at < p.grouped) {
        k = p.prev / 2 > 1 ? p.prev / 2 : 1;
        if (k > p.grouped - p.at) k = (int)(p.grouped - p.at);
        p.prev = k;
    }
    p.at += k;
    return k;
}
