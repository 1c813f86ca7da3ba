// evaluate_kernels.hip -- flat Monte-Carlo evaluation of every column of a batch of packed Connect boards
// (bgs_connect_evaluate_actions), of every move of a batch of packed Bounce boards (bgs_bounce_evaluate_moves, the
// second half of this file), and the sequential halving of both (after each).  The tree searches that play the same
// playouts are search_kernels.hip, the exact solvers solve_kernels.hip; what they share with this file is playout.h.
// Connect: for board i and column c, `playouts` games that start with column c on board i and
// continue by the uniform random policy, reduced on the device to (wins, draws, losses) of the player to move at board i.
// bgs_connect_evaluate_actions_policy plays the same games by a playout policy (include/bgs.h: BGS_POLICY_DECISIVE takes a
// winning cell, else blocks the opponent's, else plays uniformly); the policy is a template parameter of the same kernel.
//
// Game ids (include/bgs.h): playout p of column c of board i is global game
// G = ((first_game + i) * width + c) * playouts + p (mod 2^64), drawn under the batch's RNG contract at the board's absolute
// ply -- exactly an oracle rollout(seed, first_game * width * playouts) over the boards replicated W * P times, in
// (i, c, p) order, and stepped by their column.
//
// A unit of its own (bgs_kernel_unit_id(3)).  The boards and their primitives are the Connect and Bounce units' own:
// connect_board.h and bounce_board.h.
//
// Shape.  A wave owns either several whole (board, column) segments -- P <= games per wave -- or one slice of one segment.
// Its lanes take the chunk's playouts in order (the refill loop of K2a: lanes take new games at 4-ply block boundaries,
// the block itself is straight-line code masked by `live`), so the lanes of a wave sit on the same segment wherever P
// allows, and a lane keeps the board after the segment's first move in registers for all the playouts of the segment it
// takes.  W/D/L are counted in registers, flushed to the wave's LDS tally when the lane moves to the next segment, and
// the wave writes its segments once at the end (sliced segments: one integer atomic per wave and counter into counts the
// launcher zeroed).
#include "bounce_root_moves.h"
#include "playout.h"

#ifndef BGS_TU_ID
#define BGS_TU_ID "unknown"
#endif
extern "C" const char bgs_tu_id_evaluate[] = BGS_TU_ID;

namespace bgs {
namespace {

constexpr int kEvalWavesPerBlock = BGS_BLOCK / BGS_WAVE;
constexpr uint32_t kEvalMaxSegments = 64;       // (board, column) segments a wave may own: its LDS tally is 64 x 3 words
constexpr uint32_t kEvalGamesOneWord = 512;     // playouts a wave aims for: 8 a lane (K2o's kGamesPerLaneOneWord)
constexpr uint32_t kEvalGamesWide = 256;        // multi-word boards: 4 a lane
constexpr uint32_t kIllegal = 0xFFu;            // child code of an illegal column / an ended board

template <int NW, bool PER_PLY, int POLICY = BGS_POLICY_UNIFORM>
__global__ void __launch_bounds__(BGS_BLOCK)
k_connect_evaluate(EvalGeom g, const uint64_t* __restrict__ planes, const uint8_t* __restrict__ status, int64_t n,
                   uint64_t seed, uint64_t game_base, uint32_t playouts, uint32_t max_plies, uint32_t segs_per_wave,
                   uint32_t slices, uint32_t slice_len, int64_t wave_base, int64_t waves, int32_t* __restrict__ counts,
                   unsigned long long* __restrict__ steps) {
    __shared__ uint32_t tally_lds[kEvalWavesPerBlock][kEvalMaxSegments * 3];
    const uint32_t lane = threadIdx.x & (BGS_WAVE - 1);
    uint32_t* const tally = tally_lds[threadIdx.x >> 6];
    for (uint32_t k = lane; k < kEvalMaxSegments * 3; k += BGS_WAVE) tally[k] = 0;
    __syncthreads();

    // ---- the wave's work: segments [seg0, seg0 + nseg), playouts [pbeg, pbeg + per_seg) of each
    const int64_t segments = n * g.w();
    const int64_t wave = wave_base + (int64_t)__builtin_amdgcn_readfirstlane(blockIdx.x * kEvalWavesPerBlock + (threadIdx.x >> 6));
    int64_t seg0 = 0;
    uint32_t nseg = 0, pbeg = 0, per_seg = playouts;
    if (wave < waves) {
        if (slices == 1u) {
            seg0 = wave * (int64_t)segs_per_wave;
            const int64_t left = segments - seg0;
            nseg = left < (int64_t)segs_per_wave ? (uint32_t)left : segs_per_wave;
        } else {
            seg0 = wave / slices;
            pbeg = (uint32_t)(wave % slices) * slice_len;
            per_seg = playouts - pbeg < slice_len ? playouts - pbeg : slice_len;
            nseg = 1;
        }
    }
    const uint32_t avail = nseg * per_seg;
    uint32_t taken = 0;

    const uint32_t stride = (uint32_t)g.h() + 1u;
    Bits<NW> p[2];                 // the lane's game: stones of player 0 / player 1
    Bits<NW> c0, c1;               // the board after the current segment's first move
    uint32_t child = kIllegal;       // its status (0 running, 1 / 2 winner, 3 draw) or kIllegal
    uint32_t child_ply = 0, root_mover = 0;
    int64_t cur_seg = -1;
    uint64_t game = 0;
    uint32_t blk = 0, skip = 0, live = 0, st = 0, fresh = 0;
    uint32_t wins = 0, draws = 0, losses = 0, stepped = 0;
    Philox4 ph;
#pragma unroll
    for (int j = 0; j < 4; ++j) ph.v[j] = 0;
#pragma unroll
    for (int j = 0; j < NW; ++j) p[0].w[j] = p[1].w[j] = c0.w[j] = c1.w[j] = 0;

    auto flush = [&]() {
        if (cur_seg >= 0 && (wins | draws | losses)) {
            uint32_t* t = tally + (uint32_t)(cur_seg - seg0) * 3u;
            if (wins) atomicAdd(t + 0, wins);
            if (draws) atomicAdd(t + 1, draws);
            if (losses) atomicAdd(t + 2, losses);
        }
        wins = draws = losses = 0;
    };

    while (taken < avail || __builtin_amdgcn_ballot_w64(live != 0)) {
        // ---- refill: idle lanes take the chunk's next playouts.  A playout whose game is decided by the first move (or
        // capped at once, or illegal) is counted here and its lane takes another one in the same pass.
        for (;;) {
            const uint64_t need = __builtin_amdgcn_ballot_w64(live == 0);
            if (need == 0 || taken >= avail) break;
            const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(need >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)need, 0u));
            if (live == 0 && taken + rank < avail) {
                const uint32_t local = taken + rank;
                const uint32_t ls = slices == 1u ? local / per_seg : 0u;
                const uint32_t po = pbeg + (slices == 1u ? local - ls * per_seg : local);
                const int64_t seg = seg0 + ls;
                if (seg != cur_seg) {
                    flush();
                    cur_seg = seg;
                    const int64_t i = seg / g.w();
                    const int col = (int)(seg - i * g.w());
                    Bits<NW> r0, r1;
#pragma unroll
                    for (int j = 0; j < NW; ++j) {
                        r0.w[j] = planes[(int64_t)j * n + i];
                        r1.w[j] = planes[(int64_t)(NW + j) * n + i];
                    }
                    uint32_t rply = 0;
#pragma unroll
                    for (int j = 0; j < NW; ++j) rply += (uint32_t)__popcll(r0.w[j]) + (uint32_t)__popcll(r1.w[j]);
                    root_mover = rply & 1u;
                    const uint32_t height = (uint32_t)__popcll(shr(r0 | r1, col * (int)stride).w[0] & ((1ull << g.h()) - 1ull));
                    child = kIllegal;
                    if (status[i] == BGS_ST_RUNNING && height < (uint32_t)g.h()) {
                        Bits<NW>& mine = root_mover ? r1 : r0;
                        const bool won = drop_and_test(g, mine, (uint32_t)col * stride + height, ~0u);
                        child_ply = rply + 1u;
                        child = won ? root_mover + 1u : (child_ply == g.cells_total ? BGS_ST_DRAW : BGS_ST_RUNNING);
                        c0 = r0;
                        c1 = r1;
                    }
                }
                if (child != kIllegal) {
                    stepped += 1u;   // the first move: a transition of the replicated board
                    if (child != BGS_ST_RUNNING) {
                        wdl_count(child, root_mover, wins, draws, losses);
                    } else if (child_ply < max_plies) {
                        p[0] = c0;
                        p[1] = c1;
                        game = game_base + (uint64_t)(seg * (int64_t)playouts + po);
                        blk = child_ply >> 2;
                        skip = child_ply & 3u;
                        live = ~0u;
                        fresh = 1u;
                        st = 0;
                    }
                }
            }
            const uint32_t wanted = (uint32_t)__popcll(need);
            taken = avail - taken < wanted ? avail : taken + wanted;
        }
        if (!__builtin_amdgcn_ballot_w64(live != 0)) continue;

        // ---- the 4-ply block: a copy of connect_playout_block (playout.h), which the tree searches call and which says
        // what the block is -- the same draws, the same ply code, kept equal by eye.  With the call in its place this
        // kernel's launches came out above the parent's range in both orders (docs/EXPERIMENTS.md §41), so it keeps its text
        if (PER_PLY) {
            ph = philox4x32_10(seed, game, blk);
        } else {
            const bool want = live && (fresh || (blk & 3u) == 0u);
            if (__builtin_amdgcn_ballot_w64(want)) {
                if (want) ph = philox4x32_10(seed, game, blk >> 2);
            }
        }
        fresh = 0;
        const uint32_t word = PER_PLY ? 0u : philox_word(ph, blk);
        const uint32_t was_live = live;
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j) {
            const uint32_t draw = PER_PLY ? ph.v[j] : sub_draw(word, j);
            const uint32_t act = j >= skip ? live : 0u;
            const uint32_t ply = 4u * blk + j;          // stones before this sub-step; its mover is player j & 1
            bool won;
            if constexpr (POLICY == BGS_POLICY_DECISIVE) {
                const uint32_t pos = decisive_position(g, p[j & 1u], p[(j & 1u) ^ 1u], draw, won);
                drop(p[j & 1u], pos, act);
                won = won && act;
            } else {
                const uint32_t pos = draw_position(g, p[0] | p[1], draw);
                won = drop_and_test(g, p[j & 1u], pos, act);
            }
            const bool full = ply + 1u == g.cells_total;
            if (act) {
                st = won ? (j & 1u) + 1u : (full ? BGS_ST_DRAW : BGS_ST_RUNNING);
                live = (won || full || ply + 1u >= max_plies) ? 0u : live;
                stepped += 1u;
            }
        }
        blk += 1u;
        skip = 0;
        if (was_live && !live) wdl_count(st, root_mover, wins, draws, losses);
    }
    flush();
    __syncthreads();

    // ---- the wave's segments go out once: whole segments by plain stores, a slice by one atomic per counter
    if (nseg) {
        if (slices == 1u) {
            for (uint32_t k = lane; k < nseg * 3u; k += BGS_WAVE) counts[seg0 * 3 + k] = (int32_t)tally[k];
        } else if (lane < 3u && tally[lane]) {
            atomicAdd(counts + seg0 * 3 + lane, (int32_t)tally[lane]);
        }
    }
    add_steps(steps, stepped);
}

template <int NW, bool PER_PLY, int POLICY = BGS_POLICY_UNIFORM>
void launch_evaluate(const bgs_batch* b, const EvalGeom& g, uint64_t seed, uint32_t playouts, uint32_t max_plies,
                     int32_t* d_counts) {
    const int64_t segments = b->n * g.w();
    const uint32_t per_wave = NW == 1 ? kEvalGamesOneWord : kEvalGamesWide;
    uint32_t segs_per_wave = 1, slices = 1, slice_len = playouts;
    if (playouts <= per_wave) {
        segs_per_wave = per_wave / playouts;
        if (segs_per_wave > kEvalMaxSegments) segs_per_wave = kEvalMaxSegments;
    } else {
        slices = (playouts + per_wave - 1) / per_wave;
        slice_len = (playouts + slices - 1) / slices;
        slices = (playouts + slice_len - 1) / slice_len;   // every slice holds playouts
        (void)hipMemsetAsync(d_counts, 0, (size_t)segments * 3 * sizeof(int32_t), b->stream);
    }
    const int64_t waves = slices == 1 ? (segments + segs_per_wave - 1) / segs_per_wave : segments * (int64_t)slices;
    // game ids: ((first_game + i) * W + c) * P + p = first_game * W * P + (i * W + c) * P + p, mod 2^64
    const uint64_t game_base = b->first_game * (uint64_t)g.w() * (uint64_t)playouts;
    constexpr int64_t kMaxBlocks = (int64_t)1 << 30;
    for (int64_t w0 = 0; w0 < waves; w0 += kMaxBlocks * kEvalWavesPerBlock) {
        int64_t blocks = (waves - w0 + kEvalWavesPerBlock - 1) / kEvalWavesPerBlock;
        if (blocks > kMaxBlocks) blocks = kMaxBlocks;
        hipLaunchKernelGGL((k_connect_evaluate<NW, PER_PLY, POLICY>), dim3((uint32_t)blocks), dim3(BGS_BLOCK), 0, b->stream, g,
                           (const uint64_t*)b->d_planes, (const uint8_t*)b->d_status, b->n, seed, game_base, playouts, max_plies,
                           segs_per_wave, slices, slice_len, w0, waves, d_counts, b->d_steps);
    }
}

// ================================================================================================================
// Sequential halving (bgs_connect_evaluate_actions_halving, include/bgs.h): a budget of playouts a root, spent in
// R = max(1, ceil(log2 A)) rounds over the A legal columns; after every round the worse half of the columns leaves.
//
// Shape.  One team of lanes -- a workgroup of one wave (64 lanes) or of four (256), the launcher's choice by the
// playouts of a round -- owns one root for the whole launch.  Lane c < W builds the board after column c and its status
// once, into LDS.  A round's items are |S_r| * q_r playouts in (column ascending, p) order: the waves of the team draw
// them from a counter in LDS and refill their idle lanes at 4-ply block boundaries (the refill loop and the block of
// k_connect_evaluate), so the result does not depend on the team's size.  A finished playout goes into the LDS tally
// [16][3] by one LDS atomic.  A barrier ends the round; lane c of every wave then ranks column c among the survivors
// (the count of survivors that beat it on (score descending, column ascending): no sort), the wave's ballot of "rank
// below ceil(|S_r| / 2)" is the next survivor mask, and a second barrier keeps the next round's tally updates behind
// every wave's selection.  Global memory is touched for the root, the three outputs and the step counter only.
//
// Known limit: a root has one team, so a launch of few roots and a large budget leaves most of the CUs idle.
// ================================================================================================================
constexpr uint32_t kHalvingMaxCols = 16;          // the widest packed board (the survivor mask is 16 bits)
constexpr uint32_t kHalvingWaveItems = 512;       // playouts of a round up to which the team is one wave (8 a lane)

// R(x) = max(1, ceil(log2 x))
__host__ __device__ __forceinline__ uint32_t halving_rounds(uint32_t x) {
    uint32_t r = 1;
    while ((1u << r) < x) ++r;
    return r;
}

template <int NW, bool PER_PLY, int POLICY>
__global__ void __launch_bounds__(BGS_BLOCK)
k_connect_evaluate_halving(EvalGeom g, const uint64_t* __restrict__ planes, const uint8_t* __restrict__ status, int64_t n,
                           uint64_t seed, uint64_t game_base, uint32_t budget, uint32_t max_plies, int64_t root_base,
                           int32_t* __restrict__ counts, int32_t* __restrict__ given, int32_t* __restrict__ best,
                           unsigned long long* __restrict__ steps) {
    __shared__ uint64_t child_lds[kHalvingMaxCols][2 * NW];   // the board after column c
    __shared__ uint32_t child_st[kHalvingMaxCols];            // its status (0 running, 1 / 2 winner, 3 draw) or kIllegal
    __shared__ uint32_t tally[kHalvingMaxCols * 3];           // cumulative W/D/L of column c
    __shared__ uint32_t next_item;                            // the round's next playout
    const uint32_t lane = threadIdx.x & (BGS_WAVE - 1);
    const uint32_t width = (uint32_t)g.w();
    const uint32_t stride = (uint32_t)g.h() + 1u;
    const int64_t i = root_base + (int64_t)blockIdx.x;        // (the grid holds exactly the roots of this launch)

    // ---- the root, once: every lane takes its ply count, lane c builds the board after column c
    if (threadIdx.x < kHalvingMaxCols * 3) tally[threadIdx.x] = 0;
    if (threadIdx.x == 0) next_item = 0;
    Bits<NW> r0, r1;
#pragma unroll
    for (int j = 0; j < NW; ++j) {
        r0.w[j] = planes[(int64_t)j * n + i];
        r1.w[j] = planes[(int64_t)(NW + j) * n + i];
    }
    const uint32_t rply = popcount(r0) + popcount(r1);
    const uint32_t root_mover = rply & 1u, child_ply = rply + 1u;
    if (threadIdx.x < width) {
        const uint32_t col = threadIdx.x;
        const uint32_t height = (uint32_t)__popcll(shr(r0 | r1, (int)(col * stride)).w[0] & ((1ull << g.h()) - 1ull));
        uint32_t cst = kIllegal;
        if (status[i] == BGS_ST_RUNNING && height < (uint32_t)g.h()) {
            Bits<NW>& mine = root_mover ? r1 : r0;
            const bool won = drop_and_test(g, mine, col * stride + height, ~0u);
            cst = won ? root_mover + 1u : (child_ply == g.cells_total ? BGS_ST_DRAW : BGS_ST_RUNNING);
        }
#pragma unroll
        for (int j = 0; j < NW; ++j) {
            child_lds[col][j] = r0.w[j];
            child_lds[col][NW + j] = r1.w[j];
        }
        child_st[col] = cst;
    }
    __syncthreads();
    uint32_t alive = 0;             // (team-uniform) the survivors S_r, bit c = column c
    for (uint32_t c = 0; c < width; ++c) alive |= (child_st[c] != kIllegal ? 1u : 0u) << c;
    alive = (uint32_t)__builtin_amdgcn_readfirstlane((int)alive);
    const uint32_t rounds = alive ? halving_rounds((uint32_t)__popc(alive)) : 0u;

    Bits<NW> p[2];                  // the lane's game: stones of player 0 / player 1
#pragma unroll
    for (int j = 0; j < NW; ++j) p[0].w[j] = p[1].w[j] = 0;
    uint64_t game = 0;
    uint32_t blk = 0, skip = 0, live = 0, st = 0, fresh = 0, cur_col = 0, stepped = 0;
    uint32_t first_p = 0;           // (team-uniform) P_r
    uint32_t my_given = 0;          // lane c of the team's first wave: playouts column c has been given
    Philox4 ph;
#pragma unroll
    for (int j = 0; j < 4; ++j) ph.v[j] = 0;

    auto count = [&](uint32_t col, uint32_t s) {   // s: status of a finished game (0: capped, counted nowhere)
        if (s != 0u) atomicAdd(tally + col * 3u + (s == BGS_ST_DRAW ? 1u : (s - 1u == root_mover ? 0u : 2u)), 1u);
    };

    for (uint32_t r = 0; r < rounds; ++r) {
        const uint32_t m = (uint32_t)__popc(alive);
        const uint32_t q = budget / (m * rounds);
        const uint32_t total = m * q;
        bool dry = false;           // (wave-uniform) the round's counter has nothing left for this wave
        while (!dry || __builtin_amdgcn_ballot_w64(live != 0)) {
            // ---- refill: the wave's idle lanes take the round's next playouts.  A playout whose game is decided by the
            // first move (or capped at once) is counted here and its lane takes another one in the same pass.
            for (;;) {
                const uint64_t need = __builtin_amdgcn_ballot_w64(live == 0);
                if (need == 0 || dry) break;
                const uint32_t wanted = (uint32_t)__popcll(need);
                uint32_t base = 0;
                if (lane == 0) base = atomicAdd(&next_item, wanted);
                base = (uint32_t)__builtin_amdgcn_readfirstlane((int)base);
                if (base + wanted >= total) dry = true;
                const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(need >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)need, 0u));
                if (live == 0 && base + rank < total) {
                    const uint32_t item = base + rank;
                    const uint32_t k = item / q;
                    const uint32_t po = first_p + (item - k * q);
                    const uint32_t col = select_bit64((uint64_t)alive, k);   // the k-th survivor, ascending
                    const uint32_t cst = child_st[col];
                    stepped += 1u;   // the first move: a transition of the replicated board
                    if (cst != BGS_ST_RUNNING) {
                        count(col, cst);
                    } else if (child_ply < max_plies) {
#pragma unroll
                        for (int j = 0; j < NW; ++j) {
                            p[0].w[j] = child_lds[col][j];
                            p[1].w[j] = child_lds[col][NW + j];
                        }
                        game = game_base + (uint64_t)((i * (int64_t)width + col) * (int64_t)budget + po);
                        blk = child_ply >> 2;
                        skip = child_ply & 3u;
                        live = ~0u;
                        fresh = 1u;
                        st = 0;
                        cur_col = col;
                    }
                }
            }
            if (!__builtin_amdgcn_ballot_w64(live != 0)) continue;

            // ---- the 4-ply block: a copy of connect_playout_block (playout.h): the same draws, the same ply code, kept
            // equal by eye.  As in k_connect_evaluate, the call in its place was slower than the parent (EXPERIMENTS §41)
            if (PER_PLY) {
                ph = philox4x32_10(seed, game, blk);
            } else {
                const bool want = live && (fresh || (blk & 3u) == 0u);
                if (__builtin_amdgcn_ballot_w64(want)) {
                    if (want) ph = philox4x32_10(seed, game, blk >> 2);
                }
            }
            fresh = 0;
            const uint32_t word = PER_PLY ? 0u : philox_word(ph, blk);
            const uint32_t was_live = live;
#pragma unroll
            for (uint32_t j = 0; j < 4; ++j) {
                const uint32_t draw = PER_PLY ? ph.v[j] : sub_draw(word, j);
                const uint32_t act = j >= skip ? live : 0u;
                const uint32_t ply = 4u * blk + j;          // stones before this sub-step; its mover is player j & 1
                bool won;
                if constexpr (POLICY == BGS_POLICY_DECISIVE) {
                    const uint32_t pos = decisive_position(g, p[j & 1u], p[(j & 1u) ^ 1u], draw, won);
                    drop(p[j & 1u], pos, act);
                    won = won && act;
                } else {
                    const uint32_t pos = draw_position(g, p[0] | p[1], draw);
                    won = drop_and_test(g, p[j & 1u], pos, act);
                }
                const bool full = ply + 1u == g.cells_total;
                if (act) {
                    st = won ? (j & 1u) + 1u : (full ? BGS_ST_DRAW : BGS_ST_RUNNING);
                    live = (won || full || ply + 1u >= max_plies) ? 0u : live;
                    stepped += 1u;
                }
            }
            blk += 1u;
            skip = 0;
            if (was_live && !live) count(cur_col, st);
        }
        __syncthreads();   // the round's tally is complete

        // ---- selection: lane c ranks column c among the survivors
        bool keep = false;
        if (lane < width && ((alive >> lane) & 1u)) {
            const uint32_t mine = 2u * tally[lane * 3u] + tally[lane * 3u + 1u];
            uint32_t rank = 0;
            for (uint32_t c = 0; c < width; ++c) {
                const uint32_t other = 2u * tally[c * 3u] + tally[c * 3u + 1u];
                rank += (((alive >> c) & 1u) && (other > mine || (other == mine && c < lane))) ? 1u : 0u;
            }
            keep = rank < (m + 1u) / 2u;
            my_given += q;
        }
        alive = (uint32_t)__builtin_amdgcn_ballot_w64(keep) & 0xFFFFu;
        first_p += q;
        if (threadIdx.x == 0) next_item = 0;
        __syncthreads();   // every wave has read the tally; the counter is back at 0
    }

    // ---- the outputs of the root (the tally of an illegal column and of an ended board is zero)
    if (threadIdx.x < width) {
        const uint32_t c = threadIdx.x;
#pragma unroll
        for (uint32_t k = 0; k < 3; ++k) counts[(i * (int64_t)width + c) * 3 + k] = (int32_t)tally[c * 3u + k];
        if (given) given[i * (int64_t)width + c] = (int32_t)my_given;
    }
    if (threadIdx.x == 0 && best) best[i] = rounds ? (int32_t)__builtin_ctz(alive) : -1;
    add_steps(steps, stepped);
}

template <int NW, bool PER_PLY, int POLICY>
void launch_evaluate_halving(const bgs_batch* b, const EvalGeom& g, uint64_t seed, uint32_t budget, uint32_t max_plies,
                             int32_t* d_counts, int32_t* d_given, int32_t* d_best) {
    // the team: by the playouts of a round of a root with every column legal (about budget / R, whatever the round)
    const uint32_t team = budget / halving_rounds((uint32_t)g.w()) <= kHalvingWaveItems ? BGS_WAVE : BGS_BLOCK;
    // game ids: ((first_game + i) * W + c) * B + p = first_game * W * B + (i * W + c) * B + p, mod 2^64
    const uint64_t game_base = b->first_game * (uint64_t)g.w() * (uint64_t)budget;
    constexpr int64_t kMaxBlocks = (int64_t)1 << 30;
    for (int64_t i0 = 0; i0 < b->n; i0 += kMaxBlocks) {
        const int64_t blocks = b->n - i0 < kMaxBlocks ? b->n - i0 : kMaxBlocks;
        hipLaunchKernelGGL((k_connect_evaluate_halving<NW, PER_PLY, POLICY>), dim3((uint32_t)blocks), dim3(team), 0, b->stream, g,
                           (const uint64_t*)b->d_planes, (const uint8_t*)b->d_status, b->n, seed, game_base, budget, max_plies, i0,
                           d_counts, d_given, d_best, b->d_steps);
    }
}

// ================================================================================================================
// Bounce (bgs_bounce_evaluate_moves): for root i and slot s = x * H * W + c -- the move of the piece in column x of the
// active row to cell c, bit c of the root's targets[x] -- `playouts` games that start with that move and continue by the
// uniform random policy, reduced to (wins, draws, losses) of the player to move at root i.  Playout p of slot s of root i
// is global game ((first_game + i) * S + s) * P + p, S = W * H * W, drawn under Bounce's contract (a philox word per ply,
// keyed by the board's absolute ply): an oracle rollout(seed, first_game * S * P) over the roots replicated S * P times
// and stepped by their slot's move, illegal slots dropped.
//
// The ply is K3f's one-lane-per-board ply (bounce_board.h: enumerate_flat / pick_flat, target masks in a per-lane dword
// column of LDS).  It reads boards from memory and never assumes they descend from the configured start position (K3p's
// piece list does).
//
// Shape.  A first pass counts the legal moves of every root and scans them (uint64 inclusive prefix `ends` in the
// staging region): the legal (root, slot) segments are numbered 0 .. ends[n-1] - 1 in (root, slot) order, their playouts
// 0 .. ends[n-1] * P - 1 in (segment, playout) order.  Persistent waves draw chunks of that sequence from a device-wide
// counter and refill their idle lanes from it at ply boundaries (K3f's refill loop): a lane plays one game at a time,
// keeps the stepped board of its current segment in registers for every playout of that segment it takes, and counts
// W/D/L in registers.  A lane flushes its counts when it changes segment: into the wave's LDS tally when the segment
// lies in the window of its current chunk (a chunk spans at most kBounceEvalWindow segments), by global atomics
// otherwise; the window goes out by one atomic per segment and counter when the wave takes its next chunk.  Counts are
// zeroed by the launcher.  Games that never end stay in the bulk kernel up to the cap: the dynamic queue keeps the other
// lanes of their wave busy until it runs dry (docs/EXPERIMENTS.md: the tail's share of a launch).
// ================================================================================================================
constexpr uint32_t kBounceEvalWindow = 64;        // segments of a wave's LDS tally = most segments a chunk spans
constexpr uint32_t kBounceEvalChunk = 512;        // playouts a wave draws at a time (fewer when P is small: <= 63 * P)
// persistent waves per SIMD (the kernel holds 5 by its registers).  Default board, max_plies 1024, 10^9 env-steps/s at
// 256 roots x 256 playouts / 4096 x 64: 1 wave 2.01 / 2.47, 2 waves 2.71 / 4.09, 4 waves 2.88 / 5.13 (docs/EXPERIMENTS.md §16)
constexpr int kBounceEvalWps = 4;

template <class GEO, int NC, int POLICY = BGS_POLICY_UNIFORM>
__global__ void __launch_bounds__(BGS_BLOCK)
k_bounce_evaluate(GEO g, const uint64_t* __restrict__ planes, const uint8_t* __restrict__ status, const uint16_t* __restrict__ plies_buf,
                  int64_t n, uint64_t seed, uint64_t game_base, uint32_t playouts, uint32_t max_plies, uint32_t slots,
                  const uint64_t* __restrict__ ends, unsigned long long* __restrict__ queue, uint32_t chunk,
                  int32_t* __restrict__ counts, unsigned long long* __restrict__ steps) {
    extern __shared__ uint32_t target_tile[];   // [2 * 8 * NC dwords][256 lanes]
    __shared__ uint32_t tally_lds[kEvalWavesPerBlock][kBounceEvalWindow * 3];
    __shared__ uint64_t where_lds[kEvalWavesPerBlock][kBounceEvalWindow];   // root * S + slot of a window segment
    uint32_t* const column = target_tile + threadIdx.x;
    const uint32_t lane = threadIdx.x & (BGS_WAVE - 1);
    uint32_t* const tally = tally_lds[threadIdx.x >> 6];
    uint64_t* const where = where_lds[threadIdx.x >> 6];
    for (uint32_t k = lane; k < kBounceEvalWindow * 3; k += BGS_WAVE) tally[k] = 0;

    const uint64_t total = ends[n - 1] * (uint64_t)playouts;   // playouts of the batch
    const uint32_t hw = (uint32_t)(g.h * g.w);
    uint64_t c_next = 0, c_end = 0;   // (wave-uniform) the wave's chunk: playouts [c_next, c_end) still to hand out
    uint64_t win_base = 0;            // (wave-uniform) first segment of the tally's window
    bool dry = false;

    Board b, cb;                     // the lane's game; the board after its segment's first move
#pragma unroll
    for (int j = 0; j < 4; ++j) b.v[j] = cb.v[j] = 0;
    FlatMoves<NC> mv = no_moves<NC>();
    uint32_t st = 0, plies = 0, child_st = 0, child_ply = 0, root_mover = 0, stepped = 0;
    uint32_t wins = 0, draws = 0, losses = 0;
    uint64_t cur_seg = ~0ull, cur_where = 0, game = 0;
    bool has = false, search = false, have_block = false;
    Philox4 blk;
    blk.v[0] = blk.v[1] = blk.v[2] = blk.v[3] = 0;

    auto flush = [&]() {   // this lane's counts of cur_seg -> the window, or global memory
        if (wins | draws | losses) {
            const uint64_t k = cur_seg - win_base;
            if (cur_seg >= win_base && k < kBounceEvalWindow) {
                where[k] = cur_where;
                if (wins) atomicAdd(tally + 3 * k + 0, wins);
                if (draws) atomicAdd(tally + 3 * k + 1, draws);
                if (losses) atomicAdd(tally + 3 * k + 2, losses);
            } else {
                int32_t* c = counts + cur_where * 3;
                if (wins) atomicAdd(c + 0, (int32_t)wins);
                if (draws) atomicAdd(c + 1, (int32_t)draws);
                if (losses) atomicAdd(c + 2, (int32_t)losses);
            }
        }
        wins = draws = losses = 0;
    };
    auto drain = [&]() {   // the window -> global memory (every lane has flushed into it)
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
        const uint32_t k = lane;   // (kBounceEvalWindow == BGS_WAVE)
        const uint32_t t0 = tally[3 * k], t1 = tally[3 * k + 1], t2 = tally[3 * k + 2];
        if (t0 | t1 | t2) {
            int32_t* c = counts + where[k] * 3;
            if (t0) atomicAdd(c + 0, (int32_t)t0);
            if (t1) atomicAdd(c + 1, (int32_t)t1);
            if (t2) atomicAdd(c + 2, (int32_t)t2);
            tally[3 * k] = tally[3 * k + 1] = tally[3 * k + 2] = 0;
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
    };

    [[maybe_unused]] bool can_win = false;   // (BGS_POLICY_DECISIVE) the list the lane holds has a target in the mover's goal row

    for (;;) {
        // ---- refill: idle lanes take the next playouts of the chunk; a spent chunk is replaced from the queue (the
        // window moves to the new chunk's segments once every lane's counts of the old one are in it)
        for (;;) {
            const uint64_t need = __builtin_amdgcn_ballot_w64(!has);
            if (!need || dry) break;
            if (c_next >= c_end) {
                unsigned long long start = 0;
                if (lane == 0) start = atomicAdd(queue, (unsigned long long)chunk);
                start = ((unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(start >> 32)) << 32) |
                        (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)start);
                if (start >= total) {
                    dry = true;
                    break;
                }
                flush();
                drain();
                c_next = start;
                c_end = total - start < chunk ? total : start + chunk;
                win_base = start / playouts;
            }
            const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(need >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)need, 0u));
            const uint64_t avail = c_end - c_next;
            if (!has && rank < avail) {
                const uint64_t t = c_next + rank;
                const uint64_t seg = t / playouts;
                const uint32_t p = (uint32_t)(t - seg * playouts);
                if (seg != cur_seg) {
                    flush();
                    cur_seg = seg;
                    // the root: the first i with ends[i] > seg
                    int64_t lo = 0, hi = n - 1;
                    while (lo < hi) {
                        const int64_t mid = (lo + hi) >> 1;
                        if (ends[mid] > seg) hi = mid;
                        else lo = mid + 1;
                    }
                    const int64_t i = lo;
                    uint32_t j = (uint32_t)(seg - (i ? ends[i - 1] : 0ull));   // the root's j-th legal move
                    const Board r = load_board(planes, n, i);
                    const uint32_t rply = plies_buf[i];
                    root_mover = rply & 1u;
                    const uint64_t occ = occupancy(r);
                    uint64_t src = movable(g, occ, root_mover);
                    int s_cell = 0, t_cell = 0;
                    while (src) {
                        const int s = __ffsll((unsigned long long)src) - 1;
                        src &= src - 1;
                        const uint64_t tm = reach(g, r, occ, root_mover, s);
                        const uint32_t cnt = (uint32_t)__popcll(tm);
                        if (j < cnt) {
                            s_cell = s;
                            t_cell = (int)select_bit64(tm, j);
                            break;
                        }
                        j -= cnt;
                    }
                    const uint32_t x = (uint32_t)s_cell - (uint32_t)(((uint32_t)s_cell * g.inv_w) >> 16) * (uint32_t)g.w;
                    cur_where = (uint64_t)i * slots + (uint64_t)x * hw + (uint32_t)t_cell;
                    cb = r;
                    move_piece(cb, s_cell, t_cell);
                    child_ply = rply + 1u;
                    child_st = ((1ull << t_cell) & (g.goal_top | g.goal_bottom)) ? root_mover + 1u : BGS_ST_RUNNING;
                }
                stepped += 1u;   // the first move: a transition of the replicated board
                game = game_base + cur_where * playouts + p;
                b = cb;
                plies = child_ply;
                st = child_st;
                has = true;
                search = st == BGS_ST_RUNNING;   // (a blocked side to move is settled by the search, also at the cap)
                have_block = false;
            }
            const uint32_t wanted = (uint32_t)__popcll(need);
            c_next = avail < wanted ? c_end : c_next + wanted;
        }
        if (!__builtin_amdgcn_ballot_w64(has)) break;

        if (bounce_playout_ply<NC, POLICY>(g, seed, max_plies, column, b, mv, st, plies, game, has, search, have_block, can_win, blk, stepped)) {
            wdl_count(st, root_mover, wins, draws, losses);
        }
    }
    flush();
    drain();
    add_steps(steps, stepped);
}

template <class GEO, int NC, int POLICY = BGS_POLICY_UNIFORM>
void launch_bounce_evaluate(const bgs_batch* b, const GEO& g, uint64_t seed, uint32_t playouts, uint32_t max_plies, int32_t* d_counts,
                            uint64_t* d_ends, uint64_t* d_totals) {
    const uint32_t slots = (uint32_t)(b->bg.w * b->bg.h * b->bg.w);
    launch_bounce_root_moves<true>(b, g, d_ends, d_totals);
    (void)hipMemsetAsync(d_counts, 0, (size_t)b->n * slots * 3 * sizeof(int32_t), b->stream);
    unsigned long long* queue = reinterpret_cast<unsigned long long*>(b->d_work_count);   // (8-byte aligned: a region start)
    (void)hipMemsetAsync(queue, 0, sizeof(unsigned long long), b->stream);
    // a chunk spans at most kBounceEvalWindow segments: chunk / P + 1 <= 64
    uint64_t chunk = (uint64_t)(kBounceEvalWindow - 1) * playouts;
    if (chunk > kBounceEvalChunk) chunk = kBounceEvalChunk;
    // ---- the game ids: ((first_game + i) * S + s) * P + p = first_game * S * P + (i * S + s) * P + p, mod 2^64
    const uint64_t game_base = b->first_game * (uint64_t)slots * (uint64_t)playouts;
    const int64_t waves = (int64_t)b->num_cus * 4 * (b->bounce_eval_wps > 0 ? b->bounce_eval_wps : kBounceEvalWps);
    const size_t tile = sizeof(uint32_t) * 2 * 8 * NC * BGS_BLOCK;
    hipLaunchKernelGGL((k_bounce_evaluate<GEO, NC, POLICY>), dim3((uint32_t)((waves + kEvalWavesPerBlock - 1) / kEvalWavesPerBlock)), dim3(BGS_BLOCK),
                       tile, b->stream, g, (const uint64_t*)b->d_planes, (const uint8_t*)b->d_status, (const uint16_t*)b->d_plies, b->n, seed,
                       game_base, playouts, max_plies, slots, (const uint64_t*)d_ends, queue, (uint32_t)chunk, d_counts, b->d_steps);
}

// ================================================================================================================
// Sequential halving for Bounce (bgs_bounce_evaluate_moves_halving, include/bgs.h): the schedule of
// k_connect_evaluate_halving with "column" read as "arm", an arm being one of the root's A legal moves in canonical order
// (sources by ascending x, targets by ascending cell: ascending slot).
//
// Shape.  One workgroup of BGS_BLOCK lanes owns one root for the whole launch.  The piece in column x of the active row is
// searched by lane x (reach), the masks go to LDS, and every lane of the team fills its share of the arm table (source
// cell, target cell).  The root board stays in registers: a lane that takes a playout applies its arm's move to it.  A
// round's items are |S_r| * q_r playouts in (arm ascending, p) order; the waves draw them from a counter in LDS and refill
// their idle lanes at ply boundaries; the ply is this kernel's own copy of bounce_playout_ply (the search into the lane's
// LDS column, the blocked-side settlement, the decisive short-cut, a philox call per four plies).  A finished playout is one LDS atomic
// into the tally [arm][3], so the result does not depend on which lane played what.  A barrier ends the round.  Selection
// is by rank: lanes take the survivors tid, tid + BGS_BLOCK, ... and count those that beat each one on (score descending,
// arm ascending); an arm that leaves -- in the last round every arm -- stores its counts and its playouts.  The kept arms
// are compacted in order into the other survivor list behind a second barrier, and a third one keeps the next round's
// tally updates behind the selection.  Global memory: the root, the three outputs (zeroed by the launcher: illegal slots
// are never stored) and the step counter.
//
// The team is always BGS_BLOCK lanes: the move tile's stride is BGS_BLOCK dwords whatever the team (bounce_board.h), so a
// smaller team would pay the whole tile for a fraction of its lanes.
//
// Known limit: a root has one team, so a launch of few roots and a large budget leaves most of the CUs idle.
// ================================================================================================================
template <class GEO, int NC, int POLICY>
__global__ void __launch_bounds__(BGS_BLOCK)
k_bounce_evaluate_halving(GEO g, const uint64_t* __restrict__ planes, const uint8_t* __restrict__ status,
                          const uint16_t* __restrict__ plies_buf, int64_t n, uint64_t seed, uint64_t game_base, uint32_t budget,
                          uint32_t max_plies, uint32_t slots, int64_t root_base, int32_t* __restrict__ counts,
                          int32_t* __restrict__ given, int32_t* __restrict__ best, unsigned long long* __restrict__ steps) {
    extern __shared__ uint32_t target_tile[];                      // [2 * 8 * NC dwords][256 lanes]
    __shared__ uint32_t tally[kBounceHalvingMaxArms * 3];          // cumulative W/D/L of an arm
    __shared__ uint16_t arm_move[kBounceHalvingMaxArms];           // source cell << 8 | target cell
    __shared__ uint16_t survivors[2][kBounceHalvingMaxArms];       // S_r in [r & 1], ascending
    __shared__ uint8_t kept[kBounceHalvingMaxArms];                // survivor k stays in S_{r+1}
    __shared__ uint64_t root_targets[8 * NC];                      // targets of the piece in column x of the active row
    __shared__ uint32_t next_item;                                 // the round's next playout
    uint32_t* const column = target_tile + threadIdx.x;
    const uint32_t tid = threadIdx.x, lane = threadIdx.x & (BGS_WAVE - 1);
    const uint32_t hw = (uint32_t)(g.h * g.w);
    const int64_t i = root_base + (int64_t)blockIdx.x;             // (the grid holds exactly the roots of this launch)

    // ---- the root, once: its legal moves, the arm table, S_0
    for (uint32_t k = tid; k < kBounceHalvingMaxArms * 3; k += BGS_BLOCK) tally[k] = 0;
    if (tid == 0) next_item = 0;
    const Board root = load_board(planes, n, i);
    const uint32_t rply = plies_buf[i];
    const uint32_t root_mover = rply & 1u, child_ply = rply + 1u;
    const uint64_t root_occ = occupancy(root);
    // (an ended root and one that holds the most plies a board can have no arms, as in k_bounce_eval_count)
    const uint64_t sources = status[i] == BGS_ST_RUNNING && rply < kBounceMaxPlies ? movable(g, root_occ, root_mover) : 0ull;
    const uint32_t first_source = sources ? (uint32_t)(__ffsll((unsigned long long)sources) - 1) : 0u;
    const uint32_t row_base = ((first_source * g.inv_w) >> 16) * (uint32_t)g.w;
    if (tid < 8 * NC) {
        const bool piece = tid < (uint32_t)g.w && ((sources >> ((row_base + tid) & 63u)) & 1ull);
        root_targets[tid] = piece ? reach(g, root, root_occ, root_mover, (int)(row_base + tid)) : 0ull;
    }
    __syncthreads();
    uint32_t arms = 0;
    for (uint32_t x = 0; x < 8 * NC; ++x) arms += (uint32_t)__popcll(root_targets[x]);
    arms = (uint32_t)__builtin_amdgcn_readfirstlane((int)arms);
    const uint32_t rounds = arms ? halving_rounds(arms) : 0u;
    if (arms == 0u || budget < arms * rounds) {   // nothing to play, or some q_r would be 0: the outputs stay zero
        if (tid == 0 && best) best[i] = arms ? BGS_HALVING_SHORT : -1;
        return;
    }
    for (uint32_t a = tid; a < arms; a += BGS_BLOCK) {
        uint32_t j = a, x = 0;
        for (; x < 8 * NC - 1; ++x) {
            const uint32_t cnt = (uint32_t)__popcll(root_targets[x]);
            if (j < cnt) break;
            j -= cnt;
        }
        arm_move[a] = (uint16_t)(((row_base + x) << 8) | select_bit64(root_targets[x], j));
        survivors[0][a] = (uint16_t)a;
    }
    __syncthreads();
    auto slot_of = [&](uint32_t arm) {            // x * H * W + target cell
        const uint32_t packed = arm_move[arm];
        return ((packed >> 8) - row_base) * hw + (packed & 255u);
    };

    Board b;                         // the lane's game
#pragma unroll
    for (int j = 0; j < 4; ++j) b.v[j] = 0;
    FlatMoves<NC> mv;
#pragma unroll
    for (int k = 0; k < NC; ++k) mv.counts[k] = 0;
    mv.n = 0;
    mv.row_base = 0;
    uint32_t st = 0, plies = 0, cur_arm = 0, stepped = 0;
    uint64_t game = 0;
    bool has = false, search = false, have_block = false;
    [[maybe_unused]] bool can_win = false;   // (BGS_POLICY_DECISIVE) the list the lane holds has a target in the mover's goal row
    Philox4 blk;
    blk.v[0] = blk.v[1] = blk.v[2] = blk.v[3] = 0;
    uint32_t m = arms;               // (team-uniform) |S_r|
    uint32_t first_p = 0;            // (team-uniform) P_r

    for (uint32_t r = 0; r < rounds; ++r) {
        const uint16_t* const cur = survivors[r & 1u];
        uint16_t* const nxt = survivors[(r & 1u) ^ 1u];
        const uint32_t q = budget / (m * rounds);
        const uint32_t total = m * q;
        bool dry = false;            // (wave-uniform) the round's counter has nothing left for this wave
        while (!dry || __builtin_amdgcn_ballot_w64(has)) {
            // ---- refill: the wave's idle lanes take the round's next playouts
            const uint64_t need = __builtin_amdgcn_ballot_w64(!has);
            if (need && !dry) {
                const uint32_t wanted = (uint32_t)__popcll(need);
                uint32_t base = 0;
                if (lane == 0) base = atomicAdd(&next_item, wanted);
                base = (uint32_t)__builtin_amdgcn_readfirstlane((int)base);
                if (base + wanted >= total) dry = true;
                const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(need >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)need, 0u));
                if (!has && base + rank < total) {
                    const uint32_t item = base + rank;
                    const uint32_t k = item / q;
                    const uint32_t po = first_p + (item - k * q);
                    cur_arm = cur[k];
                    const uint32_t move = arm_move[cur_arm];
                    const int s_cell = (int)(move >> 8), t_cell = (int)(move & 255u);
                    stepped += 1u;   // the first move: a transition of the replicated board
                    game = game_base + ((uint64_t)i * slots + slot_of(cur_arm)) * budget + po;
                    b = root;
                    move_piece(b, s_cell, t_cell);
                    plies = child_ply;
                    st = ((1ull << t_cell) & (g.goal_top | g.goal_bottom)) ? root_mover + 1u : BGS_ST_RUNNING;
                    has = true;
                    search = st == BGS_ST_RUNNING;   // (a blocked side to move is settled by the search, also at the cap)
                    have_block = false;
                }
            }
            if (!__builtin_amdgcn_ballot_w64(has)) continue;

            // ---- this kernel's own copy of bounce_playout_ply, kept equal by eye: the same draws, the same ply code.  With
            // the shared call its registers, LDS and waves were the same and its uniform launches some 4 % slower at 64 and 256
            // roots (docs/EXPERIMENTS.md §36)
            if (__builtin_amdgcn_ballot_w64(search)) {
                const uint64_t occ = occupancy(b);
                enumerate_flat<NC, true>(g, b, occ, plies & 1u, search, column, mv);
                const bool blocked = search && mv.n == 0u;
                if (__builtin_amdgcn_ballot_w64(blocked)) {
                    FlatMoves<NC> other;
#pragma unroll
                    for (int k = 0; k < NC; ++k) other.counts[k] = 0;
                    other.n = 0;
                    other.row_base = 0;
                    enumerate_flat<NC, true>(g, b, occ, 1u - (plies & 1u), blocked, column, other);
                    if (blocked) st = other.n ? (1u - (plies & 1u)) + 1u : BGS_ST_DRAW;
                }
                if constexpr (POLICY == BGS_POLICY_DECISIVE) {
                    if (search) can_win = st == BGS_ST_RUNNING && b_can_win<NC>(mv, column, (plies & 1u) ? g.goal_bottom : g.goal_top);
                }
                search = false;
            }
            const bool run = has && st == BGS_ST_RUNNING && plies < max_plies;
            if (has && !run) {       // finished: one LDS atomic (a capped game, st 0, is counted nowhere)
                if (st != 0u) atomicAdd(tally + cur_arm * 3u + (st == BGS_ST_DRAW ? 1u : (st - 1u == root_mover ? 0u : 2u)), 1u);
                has = false;
            }
            if constexpr (POLICY == BGS_POLICY_DECISIVE) {
                if (run && can_win) {   // every candidate ends the game for the mover: one transition, nothing drawn or moved
                    st = (plies & 1u) + 1u;
                    ++plies;
                    stepped += 1u;
                }
            }
            if (POLICY == BGS_POLICY_DECISIVE ? run && !can_win : run) {
                if (!have_block || (plies & 3u) == 0u) {
                    blk = philox4x32_10(seed, game, plies >> 2);
                    have_block = true;
                }
                const uint32_t mover = plies & 1u;
                int s, t;
                pick_flat<NC>(mv, column, sample_index(philox_word(blk, plies), mv.n), s, t);
                move_piece(b, s, t);
                ++plies;
                stepped += 1u;
                if ((1ull << t) & (g.goal_top | g.goal_bottom)) st = mover + 1u;
                else search = true;
            }
        }
        __syncthreads();   // the round's tally is complete

        // ---- selection: survivor k is ranked among the m survivors; the arms that leave store their outputs
        const uint32_t keep = (m + 1u) / 2u;
        const bool last = r + 1u == rounds;
        for (uint32_t k = tid; k < m; k += BGS_BLOCK) {
            const uint32_t arm = cur[k];
            const uint32_t mine = 2u * tally[arm * 3u] + tally[arm * 3u + 1u];
            uint32_t rank = 0;
            for (uint32_t j = 0; j < m; ++j) {   // (cur is ascending: survivor j is the lower arm when j < k)
                const uint32_t other = 2u * tally[cur[j] * 3u] + tally[cur[j] * 3u + 1u];
                rank += (other > mine || (other == mine && j < k)) ? 1u : 0u;
            }
            kept[k] = rank < keep ? 1u : 0u;
            if (rank >= keep || last) {
                const int64_t at = i * (int64_t)slots + slot_of(arm);
#pragma unroll
                for (uint32_t c = 0; c < 3; ++c) counts[at * 3 + c] = (int32_t)tally[arm * 3u + c];
                if (given) given[at] = (int32_t)(first_p + q);
            }
        }
        __syncthreads();   // every survivor's flag is written
        for (uint32_t k = tid; k < m; k += BGS_BLOCK) {
            if (kept[k]) {
                uint32_t pos = 0;
                for (uint32_t j = 0; j < k; ++j) pos += kept[j];
                nxt[pos] = cur[k];
            }
        }
        m = keep;
        first_p += q;
        if (tid == 0) next_item = 0;
        __syncthreads();   // S_{r+1} is complete, every wave has read the tally, the counter is back at 0
    }
    if (tid == 0 && best) best[i] = (int32_t)slot_of(survivors[rounds & 1u][0]);
    add_steps(steps, stepped);
}

template <class GEO, int NC, int POLICY>
void launch_bounce_evaluate_halving(const bgs_batch* b, const GEO& g, uint64_t seed, uint32_t budget, uint32_t max_plies,
                                    int32_t* d_counts, int32_t* d_given, int32_t* d_best) {
    const uint32_t slots = (uint32_t)(b->bg.w * b->bg.h * b->bg.w);
    (void)hipMemsetAsync(d_counts, 0, (size_t)b->n * slots * 3 * sizeof(int32_t), b->stream);
    if (d_given) (void)hipMemsetAsync(d_given, 0, (size_t)b->n * slots * sizeof(int32_t), b->stream);
    // game ids: ((first_game + i) * S + s) * B + p = first_game * S * B + (i * S + s) * B + p, mod 2^64
    const uint64_t game_base = b->first_game * (uint64_t)slots * (uint64_t)budget;
    const size_t tile = sizeof(uint32_t) * 2 * 8 * NC * BGS_BLOCK;
    constexpr int64_t kMaxBlocks = (int64_t)1 << 30;
    for (int64_t i0 = 0; i0 < b->n; i0 += kMaxBlocks) {
        const int64_t blocks = b->n - i0 < kMaxBlocks ? b->n - i0 : kMaxBlocks;
        hipLaunchKernelGGL((k_bounce_evaluate_halving<GEO, NC, POLICY>), dim3((uint32_t)blocks), dim3(BGS_BLOCK), tile, b->stream, g,
                           (const uint64_t*)b->d_planes, (const uint8_t*)b->d_status, (const uint16_t*)b->d_plies, b->n, seed, game_base,
                           budget, max_plies, slots, i0, d_counts, d_given, d_best, b->d_steps);
    }
}

}  // namespace

void bounce_evaluate(const bgs_batch* b, uint64_t seed, int32_t playouts, int32_t max_plies, int32_t* d_counts, uint64_t* d_ends,
                     uint64_t* d_totals, int policy) {
    uint32_t cap = (uint32_t)max_plies;
    if (cap > kBounceMaxPlies) cap = kBounceMaxPlies;   // plies are stored as uint16
    with_policy(policy, [&](auto pol) {
        with_bounce_geom(b, [&](const auto& g, auto nc) {
            launch_bounce_evaluate<std::decay_t<decltype(g)>, decltype(nc)::value, decltype(pol)::value>(b, g, seed, (uint32_t)playouts, cap, d_counts, d_ends, d_totals);
        });
    });
}

void bounce_evaluate_halving(const bgs_batch* b, uint64_t seed, int32_t budget, int32_t max_plies, int policy, int32_t* d_counts,
                             int32_t* d_given, int32_t* d_best) {
    uint32_t cap = (uint32_t)max_plies;
    if (cap > kBounceMaxPlies) cap = kBounceMaxPlies;   // plies are stored as uint16
    with_policy(policy, [&](auto pol) {
        with_bounce_geom(b, [&](const auto& g, auto nc) {
            launch_bounce_evaluate_halving<std::decay_t<decltype(g)>, decltype(nc)::value, decltype(pol)::value>(b, g, seed, (uint32_t)budget, cap, d_counts, d_given, d_best);
        });
    });
}

void connect_evaluate(const bgs_batch* b, uint64_t seed, int32_t playouts, int32_t max_plies, int32_t* d_counts, int policy) {
    const EvalGeom g = eval_geom(b);
    with_connect_form(b, policy, [&](auto nw, auto per_ply, auto pol) {
        launch_evaluate<decltype(nw)::value, decltype(per_ply)::value, decltype(pol)::value>(b, g, seed, (uint32_t)playouts, (uint32_t)max_plies, d_counts);
    });
}

int32_t connect_halving_min_budget(int width) { return (int32_t)((uint32_t)width * halving_rounds((uint32_t)width)); }

void connect_evaluate_halving(const bgs_batch* b, uint64_t seed, int32_t budget, int32_t max_plies, int policy, int32_t* d_counts,
                              int32_t* d_given, int32_t* d_best) {
    const EvalGeom g = eval_geom(b);
    with_connect_form(b, policy, [&](auto nw, auto per_ply, auto pol) {
        launch_evaluate_halving<decltype(nw)::value, decltype(per_ply)::value, decltype(pol)::value>(b, g, seed, (uint32_t)budget, (uint32_t)max_plies, d_counts, d_given, d_best);
    });
}

}  // namespace bgs
