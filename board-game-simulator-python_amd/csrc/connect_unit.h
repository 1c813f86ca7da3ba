// connect_unit.h -- what the Connect kernels and their launchers are made of besides connect_kernels.hip itself: the
// geometry record the kernels take by value and the launch tuning.  The Makefile hashes THIS header (with bgs_common.h
// and the kernel source) into the Connect unit's id (bgs_kernel_unit_id(0)): counters under profiles/ are quoted as long
// as that id stands, and an edit to the Bounce unit does not move it.
#pragma once

#include <stddef.h>
#include <stdint.h>

struct ConnectGeom {
    int h, w, k, nw;   // nw = 64-bit words per plane
};

// Launch tuning of the fused rollouts.  These live here (a header the unit's id hashes) and not in bgs_capi.hip because
// they change what a launch executes: counters taken under one setting must not be quoted for another.
constexpr int kRolloutOpeningBlocks = 3;    // K2o: 4-ply blocks played in lock step before a board joins the refill loop
constexpr int kGamesPerLaneOneWord = 8;     // one-word Connect boards: games per lane a launch aims for (512 per wave at 2^20)
constexpr int kGamesPerLane = 4;            // every other rollout

// The launch shape of the fused rollouts, computed here once for every launcher.  Resident waves: CUs x 4 SIMDs x waves
// per SIMD (rollout_wps); every wave gets an equal contiguous chunk of games -- rollout_chunk when it is set -- a multiple
// of 64: whole dwords of outcome codes per wave, whole refill rounds.  The LDS a workgroup of four waves needs besides a
// kernel's static arrays: the wave-private slices of the fused 2-bit codes (K2a, the LDS-staged kernel), K2o's one outcome
// byte per game, and the grouped kernel's two outcome slices a wave.
constexpr int kRolloutWave = 64;             // lanes per wave (BGS_WAVE)
constexpr int kRolloutWavesPerBlock = 4;     // waves per workgroup (BGS_BLOCK / BGS_WAVE)
constexpr size_t kRolloutLdsLimit = 32u << 10;   // what a launch may ask for in dynamic LDS
struct ConnectLaunchShape {
    int64_t per_wave;        // games per wave
    int64_t waves;
    unsigned blocks;
    size_t code_lds;         // bytes: per_wave / 16 dwords of 2-bit codes per wave
    size_t outcome_lds;      // bytes: one outcome byte per game
    size_t outcome_lds2;     // bytes: two outcome slices per wave
};
constexpr ConnectLaunchShape connect_launch_shape(int64_t n, int num_cus, int rollout_wps, int rollout_chunk) {
    const int64_t resident = (int64_t)num_cus * 4 * rollout_wps;
    const int64_t asked = rollout_chunk > 0 ? rollout_chunk : (n + resident - 1) / resident;
    const int64_t per_wave = (asked + kRolloutWave - 1) / kRolloutWave * kRolloutWave;
    const int64_t waves = (n + per_wave - 1) / per_wave;
    return ConnectLaunchShape{per_wave,
                              waves,
                              (unsigned)((waves + kRolloutWavesPerBlock - 1) / kRolloutWavesPerBlock),
                              (size_t)kRolloutWavesPerBlock * (size_t)(per_wave / 16) * sizeof(uint32_t),
                              (size_t)kRolloutWavesPerBlock * (size_t)per_wave,
                              (size_t)kRolloutWavesPerBlock * 2 * (size_t)per_wave};
}

// Which boards the one-word nibble rollouts (K2a, K2o) take, and which calls on them go to K2o, the kernel with the
// lock-step opening stage: from the initial state, no ply cap that can bind, the opening not switched off
// (rollout_opening = 0), a geometry on which nobody can win and no column can fill within the first four plies (H >= 4,
// K >= 3, W >= 2), at most 48 cells (a game is at most 12 blocks of four plies, whose words three philox calls give), and a
// chunk whose outcome bytes fit in LDS.  connect_opened_blocks: how many blocks that opening plays in lock step -- plies
// 4 and 5 are cheap only with K >= 4 and H >= 6, else the opening is one block; a setting past 4 plays 4.
constexpr bool connect_nibble_ok(const ConnectGeom& cg) { return cg.nw == 1 && cg.w <= 8 && cg.h <= 8; }
constexpr bool connect_opened_ok(const ConnectGeom& cg, bool from_initial, bool capped, int rollout_opening,
                                 const ConnectLaunchShape& shape) {
    return connect_nibble_ok(cg) && from_initial && !capped && rollout_opening != 0 && cg.h >= 4 && cg.w >= 2 && cg.k >= 3 &&
           cg.h * cg.w <= 48 && shape.outcome_lds <= kRolloutLdsLimit;
}
constexpr int connect_opened_blocks(const ConnectGeom& cg, int rollout_opening) {
    const int blocks = cg.k >= 4 && cg.h >= 6 ? rollout_opening : 1;
    return blocks >= 1 && blocks <= 3 ? blocks : 4;
}

// Where a four-in-a-row that is not vertical can start on a one-word board (bit(x, y) = x * (h + 1) + y): it spans four
// columns, so its lowest cell lies in a column <= w - 4 and a row <= h - 1.  When that last start bit is below 32 the
// rollouts' full ply tests the low word of the board only (four_in_a_row_at_low, connect_board.h): 6x7 (26), 5x8 (28),
// 7x6 (22) -- not 6x8 (33).  Compile time for a static geometry, a wave-uniform branch for a run-time one.
constexpr bool runs_start_low(int h, int w) { return (w - 4) * (h + 1) + h - 1 <= 31; }

// The deferred opening of K2o and its grouped form (docs/EXPERIMENTS.md §27): blocks 1 .. 2 (and 3) of the lock-step
// opening are played with cheap plies only -- every column taken as open, no run test -- and ONE whole-board run test
// per player after the block stands for its per-ply tests (stones are only added: a run made at an earlier ply is still
// there, a column that closed stays closed).  A game the test or the closed-column check flags is parked at its state
// after ply 4 (or at the stage's checkpoint) and replayed exactly by the refill loop.  What a geometry must give:
//   * K = 4 on a one-word board whose runs start in the low word (the whole-board test is four_in_a_row_low_hits), at
//     most 7 columns (bit 28 of the column nibbles marks a replayed game) of at most 8 rows (a nibble holds h + 7);
//   * no win and no full column within plies 1 .. 4, what the parked state rests on: 2k - 1 > 4 and h > 4;
//   * the column nibbles (h + 7 less the column's stones) cannot borrow within the twelve plies every lane plays, run
//     or no run, closed column or not: h + 7 >= 12.  (Stage 2's four more plies are played on from boards whose columns
//     held at most h stones after ply 12; the lanes flagged before keep their shifts defined with pos & 63.);
//   * a game of at most 44 cells, blocks 0 .. 10: the eight words parked with a replayed game (blocks 1 .. 8) and the
//     three it fetches when they run out (blocks 8 .. 10) cover it.
constexpr bool deferred_opening_ok(int h, int w, int k) {
    return k == 4 && w >= 4 && w <= 7 && h <= 8 && w * (h + 1) <= 64 && runs_start_low(h, w) && 2 * k - 1 > 4 && h > 4 &&
           h + 7 >= 12 && h * w <= 44;
}
// speculative stages of the deferred opening: 1 = plies 5 .. 12 (blocks 1 and 2), 2 = block 3 as well, from the ply-12
// checkpoint; 0 = the opening as it was.  kRolloutOpeningBlocks stays 3 either way: it is what every other path plays.
constexpr int kDeferredOpeningStages = 2;

// The outcome byte of K2o and its grouped form (docs/EXPERIMENTS.md §29).  A game that ends leaves ONE byte in its wave's
// LDS slice: its stones (= its plies: 1 .. 48 on the boards these kernels take, 7 .. 42 on 6x7x4) with bit 6 set when
// somebody holds a run.  0 is "no game": the padding of a chunk's last dword, never a game's byte.  Everything a game
// leaves besides its board follows from that byte, and is derived where a chunk is flushed -- four games a dword, twice a
// wave and step -- not where the game ends, once an iteration of the refill loop:
//   * its status byte as it goes to memory: a run belongs to whoever placed the last stone, ((stones - 1) & 1) + 1; a
//     board that stopped without a run is full, BGS_ST_DRAW (3); 0 for no game;
//   * its reward pair (two int8 in a uint16, player 1's in the low byte): +1 / -1 for status 1, -1 / +1 for status 2;
//   * its 2-bit code for the hand-over: the status;
//   * its plies, for the env-step counter.
// connect_outcome4 is that mapping for the four bytes of a dword at once; connect_outcome is its one-byte case.
constexpr uint32_t kOutcomeRun = 64u;
constexpr uint32_t connect_outcome_byte(uint32_t stones, bool run) { return stones | (run ? kOutcomeRun : 0u); }
struct ConnectOutcome4 {
    uint32_t status;      // four status bytes, game 0 in the low byte
    uint32_t reward[2];   // the reward pairs of games 0, 1 and of games 2, 3
    uint32_t codes;       // the byte of four 2-bit codes, game 0 in the low bits
    uint32_t plies;       // the plies of the four games together (at most 4 * 63)
};
constexpr ConnectOutcome4 connect_outcome4(uint32_t four) {
    constexpr uint32_t L = 0x01010101u;
    const uint32_t run = (four >> 6) & L, odd = four & L;
    const uint32_t game = ((four + 0x7F7F7F7Fu) >> 7) & L;    // (a byte is at most 127: no carry into the next one)
    const uint32_t low = game & ~(run & ~odd);                // status bit 0: unless a run came with an even stone
    const uint32_t high = game & ~(run & odd);                // status bit 1: unless a run came with an odd stone
    const uint32_t status = low | (high << 1);
    const uint32_t won1 = low & ~high, won2 = high & ~low;    // bit 8 k: game k has status 1 / 2
    const uint32_t a = (won1 & 1u) | ((won1 & 0x100u) << 8), b = (won2 & 1u) | ((won2 & 0x100u) << 8);
    const uint32_t c = ((won1 >> 16) & 1u) | ((won1 >> 8) & 0x10000u), d = ((won2 >> 16) & 1u) | ((won2 >> 8) & 0x10000u);
    return ConnectOutcome4{status,
                           {a * 0xFF01u | b * 0x01FFu, c * 0xFF01u | d * 0x01FFu},
                           (status & 3u) | ((status >> 6) & 0xCu) | ((status >> 12) & 0x30u) | ((status >> 18) & 0xC0u),
                           ((four & 0x3F3F3F3Fu) * L) >> 24};
}
struct ConnectOutcome {
    uint32_t status, reward, code, plies;
};
constexpr ConnectOutcome connect_outcome(uint32_t byte) {
    const ConnectOutcome4 o = connect_outcome4(byte & 255u);
    return ConnectOutcome{o.status, o.reward[0], o.codes, o.plies};
}

// Multi-step form of the K2o rollout (k_connect_rollout_opened_steps): one launch plays the batches of up to
// kConnectGroupMax consecutive pipeline steps, every wave chunk w of each step in turn, its lanes carrying on from one
// step's chunk into the next instead of idling until the wave's longest game has ended.  The executor hands
// kConnectGroupSteps steps to a launch (S; bgs_pipeline.hip).
// Measured on one MI355X (bench.py, 2^20 boards, three batches).  docs/EXPERIMENTS.md §17 read S = 2 and 3 the same (+8 %
// on 200-step regions) and kept 2, but that S = 3 was starved: the sink had nine code slots, a launch's deliveries all
// complete at its end, and the executor waited at launch time for the previous delivery into each host array, so a
// stream's next launch could not be enqueued before its previous one had been expanded on the host.  With the sink's ring
// of 32 code slots, no launch-time wait and the call planned as a whole (connect_group_plan.h) the sweep of §32 reads
// S = 4, 6 and 8 alike and above 2 and 3, and 4 -- the smallest of them -- is kept: a launch of eight leaves the ring
// room for one launch ahead of the three in flight, and the host's expansion of eight deliveries at once (16 MiB) then
// holds the next launch back by 40-50 us a launch.  A call of 20 steps gains nothing -- its ramp and tail are most of it
// -- so a call groups its steps only from kConnectGroupMinCall steps on (§17; not lowered in §32).
constexpr int kConnectGroupSteps = 4;
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
