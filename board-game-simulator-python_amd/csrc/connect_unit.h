// connect_unit.h -- what the Connect kernels and their launchers are made of besides connect_kernels.hip itself: the
// geometry record the kernels take by value and the launch tuning.  The Makefile hashes THIS header (with bgs_common.h
// and the kernel source) into the Connect unit's id (bgs_kernel_unit_id(0)): counters under profiles/ are quoted as long
// as that id stands, and an edit to the Bounce unit does not move it.
#pragma once

#include <stdint.h>

struct ConnectGeom {
    int h, w, k, nw;   // nw = 64-bit words per plane
};

// Launch tuning of the fused rollouts.  These live here (a header the unit's id hashes) and not in bgs_capi.hip because
// they change what a launch executes: counters taken under one setting must not be quoted for another.
constexpr int kRolloutOpeningBlocks = 3;    // K2o: 4-ply blocks played in lock step before a board joins the refill loop
constexpr int kGamesPerLaneOneWord = 8;     // one-word Connect boards: games per lane a launch aims for (512 per wave at 2^20)
constexpr int kGamesPerLane = 4;            // every other rollout

// Where a four-in-a-row that is not vertical can start on a one-word board (bit(x, y) = x * (h + 1) + y): it spans four
// columns, so its lowest cell lies in a column <= w - 4 and a row <= h - 1.  When that last start bit is below 32 the
// rollouts' full ply tests the low word of the board only (four_in_a_row_at_low, connect_board.h): 6x7 (26), 5x8 (28),
// 7x6 (22) -- not 6x8 (33).  Compile time for a static geometry, a wave-uniform branch for a run-time one.
constexpr bool runs_start_low(int h, int w) { return (w - 4) * (h + 1) + h - 1 <= 31; }

// Multi-step form of the K2o rollout (k_connect_rollout_opened_steps): one launch plays the batches of up to
// kConnectGroupMax consecutive pipeline steps, every wave chunk w of each step in turn, its lanes carrying on from one
// step's chunk into the next instead of idling until the wave's longest game has ended.  The executor hands
// kConnectGroupSteps steps to a launch (S; bgs_pipeline.hip).
// Measured on one MI355X (bench.py, 2^20 boards, three batches, docs/EXPERIMENTS.md §17): S = 2 and 3 read the same
// (+8 % on 200-step regions); a call of 20 steps gains nothing -- its ramp and tail are most of it -- and its first
// region read 3-5 % lower, so a call groups its steps only from kConnectGroupMinCall steps on.
constexpr int kConnectGroupSteps = 2;
constexpr int kConnectGroupMax = 8;
constexpr int kConnectGroupMinCall = 48;

// one step of a grouped launch, by value in the kernel's arguments
struct ConnectGroupStep {
    uint64_t seed;
    uint64_t first_game;
    uint64_t* planes;            // the step's arena, or NULL: it leaves no boards, status or rewards (a later step of the same
    uint8_t* status;             // launch sequence overwrites that batch; its outcome codes and env-steps still go out)
    uint16_t* reward;
    uint32_t* codes;             // 2-bit outcome codes, (n + 15) / 16 dwords (the sink's page-locked slot), or NULL
    unsigned long long* steps;   // the batch's env-step counter
};
struct ConnectGroup {
    ConnectGroupStep step[kConnectGroupMax];
    int count;
};
