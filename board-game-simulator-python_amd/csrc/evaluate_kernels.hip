// evaluate_kernels.hip -- flat Monte-Carlo evaluation of every column of a batch of packed Connect boards
// (bgs_connect_evaluate_actions), of every move of a batch of packed Bounce boards (bgs_bounce_evaluate_moves, the
// second half of this file), the exact Connect solver (bgs_connect_solve_actions, between the two) and the exact Bounce
// solver (bgs_bounce_solve_moves, at the end).  Connect: for board i and column c, `playouts` games that start with column c on board i and
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
#include <type_traits>

#include "../../include/bgs.h"
#include "bgs_common.h"
#include "bgs_internal.h"
#include "bounce_board.h"
#include "connect_board.h"

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

struct EvalGeom {
    int rh, rw, rk;
    __host__ __device__ __forceinline__ int h() const { return rh; }
    __host__ __device__ __forceinline__ int w() const { return rw; }
    __host__ __device__ __forceinline__ int k() const { return rk; }
    uint32_t cells_total;          // h * w: a board with this many stones is full
    uint64_t bottoms[BGS_CONNECT_MAX_WORDS];   // the bottom cell of every column
    uint64_t cells[BGS_CONNECT_MAX_WORDS];     // every real cell (no sentinels)
};

// the mover drops a stone on `pos` (act = all ones) or nothing (act = 0), untested
template <int NW>
__device__ __forceinline__ void drop(Bits<NW>& mine, uint32_t pos, uint32_t act) {
    if (NW == 1) {
        const uint64_t bit = 1ull << (pos & 63u);
        mine.w[0] = ((uint64_t)and_or((uint32_t)(bit >> 32), act, (uint32_t)(mine.w[0] >> 32)) << 32) |
                    and_or((uint32_t)bit, act, (uint32_t)mine.w[0]);
        return;
    }
#pragma unroll
    for (int j = 0; j < NW; ++j) mine.w[j] |= ((uint32_t)j == (pos >> 6) && act) ? 1ull << (pos & 63u) : 0ull;
}

// the mover of this ply drops a stone on `pos` (act = all ones) or nothing (act = 0); returns "the mover has won"
template <int NW>
__device__ __forceinline__ bool drop_and_test(const EvalGeom& g, Bits<NW>& mine, uint32_t pos, uint32_t act) {
    drop(mine, pos, act);
    if (NW == 1) {
        const bool won = g.k() == 4 ? four_in_a_row_at(mine.w[0], g.h(), pos) : has_run(g, mine);
        return won && act;
    }
    return act && has_run(g, mine);
}

// the idx-th cell of `set` in ascending order, idx drawn from `draw` over its cells.  `set` is a subset of the landing
// cells: at most one cell a column and never a sentinel, so ascending cells are ascending columns and the one-word
// field search (select_landing) serves any such subset
template <int NW>
__device__ __forceinline__ uint32_t draw_from_cells(const EvalGeom& g, const Bits<NW>& set, uint32_t draw) {
    if (NW == 1) {
        const uint32_t idx = sample_index(draw, (uint32_t)__popcll(set.w[0]));
        const bool by_fields = g.h() <= 15 && (uint32_t)g.w() <= (1u << g.h());   // (uniform)
        return by_fields ? select_landing(set.w[0], g.bottoms[0], g.bottoms[0] << g.h(), (uint32_t)g.h() + 1u, idx)
                         : select_bit64(set.w[0], idx);
    }
    uint32_t cnt = 0;
#pragma unroll
    for (int j = 0; j < NW; ++j) cnt += (uint32_t)__popcll(set.w[j]);
    uint32_t idx = sample_index(draw, cnt), pos = 0;
    bool found = false;
#pragma unroll
    for (int j = 0; j < NW; ++j) {
        const uint32_t c = (uint32_t)__popcll(set.w[j]);
        const bool here = !found && idx < c;
        pos = here ? 64u * j + select_bit64(set.w[j], idx) : pos;
        idx -= (!found && !here) ? c : 0u;
        found = found || here;
    }
    return pos;
}

// one uniformly drawn ply on a board with the stones `occ`: the position of the stone it drops
template <int NW>
__device__ __forceinline__ uint32_t draw_position(const EvalGeom& g, const Bits<NW>& occ, uint32_t draw) {
    return draw_from_cells(g, landing_of(g, occ), draw);
}

template <int NW>
__device__ __forceinline__ Bits<NW> threats(const EvalGeom& g, const Bits<NW>& me);   // (with the solver, below)

// one ply of BGS_POLICY_DECISIVE by the side with the stones `me` against `op`: the candidate cells are the landing
// cells that complete a run of `me` (W), else those that would complete one of `op` (B), else every landing cell; the
// ply's draw indexes them in ascending column order.  `wins`: the cell came from W -- the stone dropped there wins, and
// no other cell of this ply could, so the caller needs no win test of its own.
template <int NW>
__device__ __forceinline__ uint32_t decisive_position(const EvalGeom& g, const Bits<NW>& me, const Bits<NW>& op, uint32_t draw,
                                                      bool& wins) {
    const Bits<NW> landing = landing_of(g, me | op);
    const Bits<NW> w = threats(g, me) & landing;
    const Bits<NW> b = threats(g, op) & landing;
    wins = any(w);
    const bool block = any(b);
    Bits<NW> set;
#pragma unroll
    for (int j = 0; j < NW; ++j) set.w[j] = wins ? w.w[j] : (block ? b.w[j] : landing.w[j]);
    return draw_from_cells(g, set, draw);
}

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

    auto count = [&](uint32_t s) {   // s: status of a finished game (0: capped, counted nowhere)
        wins += (s != 0u && s != BGS_ST_DRAW && s - 1u == root_mover) ? 1u : 0u;
        losses += (s != 0u && s != BGS_ST_DRAW && s - 1u != root_mover) ? 1u : 0u;
        draws += s == BGS_ST_DRAW ? 1u : 0u;
    };
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
                        count(child);
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

        // ---- the block's draws: the strict contract's four words are one philox call a block; the default contract's
        // call serves four blocks, so a lane makes one at a 16-ply boundary or for a new game only
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
        if (was_live && !live) count(st);
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

            // ---- the 4-ply block of k_connect_evaluate: the same draws, the same ply code
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
// UCT tree search (bgs_connect_search_actions, include/bgs.h): `iterations` iterations of UCT a root, `leaf_playouts`
// playouts a leaf, integer arithmetic throughout.
//
// Shape: leaf-parallel MCTS.  One wave (a 64-lane workgroup) owns one root for the whole launch.  The descent is
// wave-uniform: the position is rebuilt from the root as the descent goes (nodes hold no boards), lane c holds n, s and
// the child of column c of the node at hand and computes U(c), and the arg-max is taken over the lanes.  The path goes
// into LDS as (node, column) pairs.  The 64 lanes then play the leaf's playouts (the refill loop and the 4-ply block of
// k_connect_evaluate: idle lanes take the leaf's next playouts at block boundaries), W/D/L are reduced by LDS atomics,
// and lane k updates edge k of the path.
//
// A node is 3 * width words: n[c], s[c], child[c] (0: no child yet).  A node is zeroed when it is made (the root at the
// start), so the caller's memory needs no preparation.  The tree is written by some lanes (lane k of the back-propagation,
// the lanes that zero a new node) and read by others (lane c of the next descent): a __syncthreads() of the one-wave
// workgroup stands between every such pair.
//
// One kernel, two places for the tree (the template parameter FOREST):
//   the plain search (bgs_connect_search_actions): the tree lives in the caller's workspace, iterations + 1 nodes a root,
//     starts empty and is forgotten after the launch;
//   the forest (bgs_connect_forest_search / bgs_connect_forest_advance): the trees are kept from launch to launch in the
//     caller's memory, `capacity` nodes a tree, and re-rooted between the launches.  A tree's share of the forest, in
//     32-bit words, rounded up to 256 bytes:
//       word 0         the nodes in use, the root counted (0: an emptied tree)
//       word 1         unused
//       words 2 ..     the position the root stands for: the 2 * NW plane words of the batch (player 0's, then player
//                      1's), 64 bits each, 8-byte aligned
//       words 16 ..    `capacity` nodes
//     The re-rooting needs a bit a node and a prefix count a 32 nodes; both live in LDS, which is what bounds `capacity`
//     (BGS_CONNECT_FOREST_MAX_CAPACITY), so the forest holds no scratch.
// FOREST changes four things and nothing else: where the tree is; the start (the carried check, or the emptying, where
// the plain search zeroes node 0); whether a new node fits (a node is made when the edge has no child AND the tree has
// room; an edge whose node did not fit plays its playouts from p' all the same and is tried again the next time -- the
// plain tree has room for a node an iteration, so there the question is settled when the kernel is compiled); and the
// header and `carried` written at the end.  The iteration -- descent, playout block, back-propagation -- is one text.
//
// The proving search (bgs_connect_search_actions_proving; the template parameter PROVE, the plain tree only) keeps
// game-end facts on the edges: bits 31:30 of an edge's child word hold its tag, seen from the player to move at the node
// (kTagOpen = 0, so a zeroed node is all OPEN and an OPEN edge's word is its child index as before).  PROVE changes five
// things and nothing else: a lane's column is a candidate of the selection only while its tag is OPEN; an edge that
// ends the game is tagged when it is played; the legal columns of every path node go to LDS beside the path; after an
// iteration that tagged its last edge the tags are backed up the path (lane c reads column c's tag, ballots give the
// node's value, lane 0 tags the parent's edge, a barrier follows every such write); and a root whose value is no longer
// OPEN stops iterating.  A tagged edge is never descended again, so the descent never meets a child word with tag bits.
//
// Known limit: a root has one wave, so a launch of few roots uses few CUs, and leaf_playouts < 64 leaves lanes idle
// (DESIGN.md §9).
// ================================================================================================================
constexpr uint32_t kTagOpen = 0u, kTagWin = 1u, kTagDraw = 2u, kTagLoss = 3u;   // bits 31:30 of a child word
constexpr uint32_t kTagShift = 30u;
static_assert(((uint64_t)1 << 29) + 1u < ((uint64_t)1 << kTagShift), "a child index (at most T <= 2^29, plus the root) stays below the tag bits");
constexpr uint32_t kSearchMaxPath = 64 * BGS_CONNECT_MAX_WORDS;   // a descent drops at most h * w stones
constexpr uint32_t kForestHeaderWords = 16;

// words of a root's tree in the workspace: iterations + 1 nodes, rounded up to 256 bytes
__host__ __device__ __forceinline__ uint64_t search_root_words(uint32_t width, uint32_t iterations) {
    return (((uint64_t)iterations + 1u) * width * 3u + 63u) & ~(uint64_t)63u;
}

// words of a tree's share of the forest: the header and `capacity` nodes, rounded up to 256 bytes
__host__ __device__ __forceinline__ uint64_t forest_tree_words(uint32_t width, uint32_t capacity) {
    return (kForestHeaderWords + (uint64_t)capacity * width * 3u + 63u) & ~(uint64_t)63u;
}

// floor(sqrt(x)), exact
__device__ __forceinline__ uint32_t search_isqrt(uint32_t x) {
    uint32_t r = (uint32_t)sqrtf((float)x);
    while ((uint64_t)r * r > x) --r;
    while ((uint64_t)(r + 1u) * (r + 1u) <= x) ++r;
    return r;
}

// Q = floor(s * 2048 / n), n >= 1, s <= 2 n < 2^31: the double quotient of two integers below 2^42 is within one of it
__device__ __forceinline__ uint32_t search_q(uint32_t s, uint32_t n) {
    const uint64_t num = (uint64_t)s << 11;
    uint32_t q = (uint32_t)((double)num / (double)n);
    while ((uint64_t)q * n > num) --q;
    while ((uint64_t)(q + 1u) * n <= num) ++q;
    return q;
}

// lg(N) = 256 e + ((256 N) >> e) - 256, e = floor(log2 N): a piecewise-linear log2 in Q8 (N >= 1)
__host__ __device__ __forceinline__ uint32_t search_lg(uint32_t total) {
    const uint32_t e = 31u - (uint32_t)__builtin_clz(total);
    return 256u * e + (uint32_t)(((uint64_t)total << 8) >> e) - 256u;
}

// (the plain launch passes capacity = iterations + 1, restart = 1 and carried = nullptr; its instantiation reads none of them)
template <int NW, bool PER_PLY, int POLICY, bool FOREST, bool PROVE = false>
__global__ void __launch_bounds__(BGS_WAVE)
k_connect_search(EvalGeom g, const uint64_t* __restrict__ planes, const uint8_t* __restrict__ status, int64_t n, uint64_t seed,
                 uint64_t game_base, uint32_t iterations, uint32_t leaf_playouts, uint32_t explore, uint32_t max_plies,
                 int64_t root_base, uint32_t capacity, uint32_t restart, uint32_t* trees, int32_t* __restrict__ counts,
                 int32_t* __restrict__ visits, int32_t* __restrict__ best, int32_t* __restrict__ nodes,
                 int32_t* __restrict__ carried, unsigned long long* __restrict__ steps, int8_t* __restrict__ proved = nullptr,
                 int32_t* __restrict__ done = nullptr) {
    static_assert(!(PROVE && FOREST), "the forest does not prove");
    __shared__ uint32_t path_node[kSearchMaxPath];   // the descent: edge k leaves node path_node[k] by column path_col[k]
    __shared__ uint32_t path_col[kSearchMaxPath];
    __shared__ uint32_t path_legal[PROVE ? kSearchMaxPath : 1u];   // PROVE: the legal columns of path_node[k], a bit a column
    __shared__ uint32_t tally[3];                    // W/D/L of the iteration's playouts, for the root's mover
    __shared__ unsigned long long step_sum;
    const uint32_t lane = threadIdx.x;
    const uint32_t width = (uint32_t)g.w();
    const uint32_t stride = (uint32_t)g.h() + 1u;
    const uint32_t node_words = width * 3u;
    const int64_t i = root_base + (int64_t)blockIdx.x;       // (the grid holds exactly the roots of this launch)
    // ---- where the tree is: behind the header of its share of the forest, or bare in the workspace
    uint32_t *head = nullptr, *tree;
    uint64_t* head_planes = nullptr;
    if constexpr (FOREST) {
        head = trees + (uint64_t)i * forest_tree_words(width, capacity);
        head_planes = reinterpret_cast<uint64_t*>(head + 2);
        tree = head + kForestHeaderWords;
    } else {
        tree = trees + (uint64_t)i * search_root_words(width, iterations);
    }

    Bits<NW> r0, r1;
#pragma unroll
    for (int j = 0; j < NW; ++j) {
        r0.w[j] = planes[(int64_t)j * n + i];
        r1.w[j] = planes[(int64_t)(NW + j) * n + i];
    }
    const uint32_t rply = popcount(r0) + popcount(r1);
    const uint32_t root_mover = rply & 1u;
    const bool running = status[i] == BGS_ST_RUNNING;
    uint32_t cw = 0, cd = 0, cl = 0;    // lane c: W/D/L of the playouts through root column c
    uint64_t stepped = 0;
    if (lane == 0) step_sum = 0;

    // ---- the start.  FOREST: the carried check (wave-uniform: every lane reads the same header); a tree that fails it
    // is emptied.  The plain tree starts empty.
    uint32_t used = 0;                  // (uniform) nodes in the tree, the root counted
    bool keep = false;
    if constexpr (FOREST) {
        used = head[0];
        keep = restart == 0u && running && used >= 1u && used <= capacity;
        if (keep) {
#pragma unroll
            for (int j = 0; j < NW; ++j) keep = keep && head_planes[j] == r0.w[j] && head_planes[NW + j] == r1.w[j];
        }
        if (keep) {                     // N + T * P < 2^31: the root's n[c] stay in int32
            const uint32_t nc = lane < width ? tree[lane] : 0u;
            uint64_t total = 0;
            for (uint32_t c = 0; c < width; ++c) total += (uint32_t)__builtin_amdgcn_readlane((int)nc, (int)c);
            keep = total + (uint64_t)iterations * leaf_playouts < (1ull << 31);
        }
        keep = __builtin_amdgcn_readfirstlane((int)keep) != 0;
    }
    if (!keep) {
        used = running ? 1u : 0u;
        if (running && lane < node_words) tree[lane] = 0;     // the root is node 0 (3 * width <= 48 words)
        if constexpr (FOREST) {
            if (running && lane == 0) {
#pragma unroll
                for (int j = 0; j < NW; ++j) {
                    head_planes[j] = r0.w[j];
                    head_planes[NW + j] = r1.w[j];
                }
            }
        }
    }
    used = (uint32_t)__builtin_amdgcn_readfirstlane((int)used);
    [[maybe_unused]] const uint32_t brought = used ? used - 1u : 0u;
    __syncthreads();

    Bits<NW> q[2];                      // the lane's playout: stones of player 0 / player 1
#pragma unroll
    for (int j = 0; j < NW; ++j) q[0].w[j] = q[1].w[j] = 0;
    Philox4 ph;
#pragma unroll
    for (int j = 0; j < 4; ++j) ph.v[j] = 0;

    [[maybe_unused]] uint32_t ran = 0;            // PROVE (uniform): the iterations run, and whether the root's value is proved
    [[maybe_unused]] bool decided = false;
    for (uint32_t t = 0; running && t < iterations; ++t) {
        if constexpr (PROVE) {
            if (decided) break;
            ran = t + 1u;
        }
        // ---- descent (wave-uniform): p is the position at node v
        Bits<NW> p[2] = {r0, r1};
        uint32_t ply = rply, v = 0, depth = 0, leaf = BGS_ST_RUNNING, col0 = 0;
        for (;;) {
            const Bits<NW> occ = p[0] | p[1];
            uint32_t height = (uint32_t)g.h();
            if (lane < width) height = (uint32_t)__popcll(shr(occ, (int)(lane * stride)).w[0] & ((1ull << g.h()) - 1ull));
            bool legal = height < (uint32_t)g.h();
            uint32_t* const node = tree + (uint64_t)v * node_words;
            uint32_t nc = 0, sc = 0, ch = 0;
            if (legal) {
                nc = node[lane];
                sc = node[width + lane];
                ch = node[2u * width + lane];
            }
            if constexpr (PROVE) {                                     // the candidates: legal and OPEN (nc counts in N for those alone)
                const uint32_t legal_columns = (uint32_t)__builtin_amdgcn_ballot_w64(legal);
                if (lane == 0) path_legal[depth] = legal_columns;
                legal = legal && (ch >> kTagShift) == kTagOpen;
                nc = legal ? nc : 0u;
            }
            const uint64_t unvisited = __builtin_amdgcn_ballot_w64(legal && nc == 0u);
            uint32_t col;
            if (unvisited) {
                col = (uint32_t)__builtin_ctzll(unvisited);            // the expansion: the lowest column never played
            } else {
                uint32_t total = 0;
                for (uint32_t c = 0; c < width; ++c) total += (uint32_t)__builtin_amdgcn_readlane((int)nc, (int)c);
                uint32_t key = 0;                                      // (U(c) << 4 | 15 - c) + 1: the largest U, then the lowest column
                if (legal) {
                    const uint32_t u = search_q(sc, nc) + search_isqrt(explore * search_lg(total) / nc);
                    key = ((u << 4) | (15u - lane)) + 1u;
                }
                uint32_t top = 0;
                for (uint32_t c = 0; c < width; ++c) {
                    const uint32_t other = (uint32_t)__builtin_amdgcn_readlane((int)key, (int)c);
                    top = other > top ? other : top;
                }
                col = 15u - ((top - 1u) & 15u);
            }
            col = (uint32_t)__builtin_amdgcn_readfirstlane((int)col);
            const uint32_t at = (uint32_t)__builtin_amdgcn_readlane((int)height, (int)col);
            const uint32_t child = (uint32_t)__builtin_amdgcn_readlane((int)ch, (int)col);
            if (lane == 0) {
                path_node[depth] = v;
                path_col[depth] = col;
            }
            col0 = depth == 0u ? col : col0;
            const uint32_t mover = ply & 1u;
            Bits<NW>& mine = mover ? p[1] : p[0];
            const bool won = drop_and_test(g, mine, col * stride + at, ~0u);
            ply += 1u;
            depth += 1u;
            leaf = won ? mover + 1u : (ply == g.cells_total ? (uint32_t)BGS_ST_DRAW : (uint32_t)BGS_ST_RUNNING);
            leaf = (uint32_t)__builtin_amdgcn_readfirstlane((int)leaf);
            if constexpr (PROVE) {                                     // an edge that ends the game is a fact (it had no child: ch = 0)
                if (leaf != BGS_ST_RUNNING && lane == col) node[2u * width + lane] = (won ? kTagWin : kTagDraw) << kTagShift;
            }
            if (leaf != BGS_ST_RUNNING) break;                         // a terminal edge: no node, no game
            if (child == 0u) {                                         // no node for p' yet: one is made if it fits
                bool fits = true;                                      // (the plain tree has iterations + 1 nodes: room for every iteration's)
                if constexpr (FOREST) fits = used < capacity;
                if (fits) {
                    if (lane < node_words) tree[(uint64_t)used * node_words + lane] = 0;
                    if (lane == col) node[2u * width + lane] = used;
                    used += 1u;
                }
                break;
            }
            v = child;
        }

        // ---- the leaf's playouts: the lanes take them in order, idle lanes refill at 4-ply block boundaries
        uint32_t wins = 0, draws = 0, losses = 0, played = 0;
        if (lane < 3u) tally[lane] = 0;
        if (leaf != BGS_ST_RUNNING) {
            if (lane == 0) {       // all playouts of the iteration have the edge's outcome
                wins = (leaf != BGS_ST_DRAW && leaf - 1u == root_mover) ? leaf_playouts : 0u;
                losses = (leaf != BGS_ST_DRAW && leaf - 1u != root_mover) ? leaf_playouts : 0u;
                draws = leaf == BGS_ST_DRAW ? leaf_playouts : 0u;
            }
        } else if (ply < max_plies) {
            // G = ((first_game + i) * T + t) * P + j
            const uint64_t game0 = game_base + ((uint64_t)i * iterations + t) * (uint64_t)leaf_playouts;
            uint64_t game = 0;
            uint32_t taken = 0, blk = 0, skip = 0, live = 0, st = 0, fresh = 0;
            while (taken < leaf_playouts || __builtin_amdgcn_ballot_w64(live != 0)) {
                const uint64_t need = __builtin_amdgcn_ballot_w64(live == 0);
                if (need != 0 && taken < leaf_playouts) {
                    const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(need >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)need, 0u));
                    if (live == 0 && rank < leaf_playouts - taken) {
                        q[0] = p[0];
                        q[1] = p[1];
                        game = game0 + (uint64_t)(taken + rank);
                        blk = ply >> 2;
                        skip = ply & 3u;
                        live = ~0u;
                        fresh = 1u;
                        st = 0;
                    }
                    const uint32_t wanted = (uint32_t)__popcll(need);
                    taken = leaf_playouts - taken < wanted ? leaf_playouts : taken + wanted;
                }

                // ---- the 4-ply block of k_connect_evaluate: the same draws, the same ply code
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
                    const uint32_t at = 4u * blk + j;          // stones before this sub-step; its mover is player j & 1
                    bool won;
                    if constexpr (POLICY == BGS_POLICY_DECISIVE) {
                        const uint32_t pos = decisive_position(g, q[j & 1u], q[(j & 1u) ^ 1u], draw, won);
                        drop(q[j & 1u], pos, act);
                        won = won && act;
                    } else {
                        const uint32_t pos = draw_position(g, q[0] | q[1], draw);
                        won = drop_and_test(g, q[j & 1u], pos, act);
                    }
                    const bool full = at + 1u == g.cells_total;
                    if (act) {
                        st = won ? (j & 1u) + 1u : (full ? BGS_ST_DRAW : BGS_ST_RUNNING);
                        live = (won || full || at + 1u >= max_plies) ? 0u : live;
                        played += 1u;
                    }
                }
                blk += 1u;
                skip = 0;
                if (was_live && !live) {      // (st == 0: capped, counted nowhere)
                    wins += (st != 0u && st != BGS_ST_DRAW && st - 1u == root_mover) ? 1u : 0u;
                    losses += (st != 0u && st != BGS_ST_DRAW && st - 1u != root_mover) ? 1u : 0u;
                    draws += st == BGS_ST_DRAW ? 1u : 0u;
                }
            }
        }
        stepped += played;
        __syncthreads();            // the tally is zero, the path and the new node are written
        if (wins) atomicAdd(tally + 0, wins);
        if (draws) atomicAdd(tally + 1, draws);
        if (losses) atomicAdd(tally + 2, losses);
        __syncthreads();
        const uint32_t tw = tally[0], td = tally[1], tl = tally[2];

        // ---- back-propagation: lane k takes edge k of the path; its mover is the root's at even k
        for (uint32_t k = lane; k < depth; k += BGS_WAVE) {
            uint32_t* const node = tree + (uint64_t)path_node[k] * node_words;
            const uint32_t c = path_col[k];
            node[c] += leaf_playouts;
            node[width + c] += td + 2u * ((k & 1u) ? tl : tw);
        }
        if (lane == col0) {
            cw += tw;
            cd += td;
            cl += tl;
        }
        if constexpr (PROVE) {
            // ---- the tags go up the path (wave-uniform), while the node at hand has a value: lane c reads column c's tag
            // (the last edge's was written during the descent, barriers ago; an upper one by lane 0, a barrier ago)
            if (leaf != BGS_ST_RUNNING) {
                for (uint32_t k = depth; k-- > 0u;) {
                    const uint32_t* const node = tree + (uint64_t)path_node[k] * node_words;
                    const bool legal = lane < width && ((path_legal[k] >> lane) & 1u) != 0u;
                    const uint32_t tag = legal ? node[2u * width + lane] >> kTagShift : kTagLoss;
                    const bool wins_here = __builtin_amdgcn_ballot_w64(legal && tag == kTagWin) != 0;
                    const bool open_here = __builtin_amdgcn_ballot_w64(legal && tag == kTagOpen) != 0;
                    const bool draw_here = __builtin_amdgcn_ballot_w64(legal && tag == kTagDraw) != 0;
                    if (!wins_here && open_here) break;                // the value is OPEN: nothing is known further up
                    if (k == 0u) {
                        decided = true;
                        break;
                    }
                    // the parent's edge, seen from the parent's mover: a won node is a lost move, a lost node a winning one
                    const uint32_t up = wins_here ? kTagLoss : (draw_here ? kTagDraw : kTagWin);
                    if (lane == 0) tree[(uint64_t)path_node[k - 1u] * node_words + 2u * width + path_col[k - 1u]] |= up << kTagShift;
                    __syncthreads();
                }
            }
        }
        __syncthreads();            // the tree is whole again before the next descent reads it; tally and path are free
    }

    // ---- the outputs of the root (an illegal column was never played: its words of the root are zero)
    uint32_t nv = 0, sv = 0;
    if (running && lane < width) {
        nv = tree[lane];
        sv = tree[width + lane];
    }
    if (lane < width) {
        counts[(i * (int64_t)width + lane) * 3 + 0] = (int32_t)cw;
        counts[(i * (int64_t)width + lane) * 3 + 1] = (int32_t)cd;
        counts[(i * (int64_t)width + lane) * 3 + 2] = (int32_t)cl;
        if (visits) visits[i * (int64_t)width + lane] = (int32_t)nv;
    }
    // PROVE: the root's tags; `among` = the columns `best` is taken over (those not proved lost, or all when all are)
    [[maybe_unused]] uint64_t among = ~0ull, won_columns = 0;
    if constexpr (PROVE) {
        uint32_t height = (uint32_t)g.h();
        if (lane < width) height = (uint32_t)__popcll(shr(r0 | r1, (int)(lane * stride)).w[0] & ((1ull << g.h()) - 1ull));
        const bool legal = running && height < (uint32_t)g.h();
        const uint32_t tag = legal ? tree[2u * width + lane] >> kTagShift : kTagOpen;
        if (lane < width && proved) {
            const int code = tag == kTagWin ? BGS_SOLVE_WIN : (tag == kTagDraw ? BGS_SOLVE_DRAW : (tag == kTagLoss ? BGS_SOLVE_LOSS : BGS_SOLVE_UNKNOWN));
            proved[i * (int64_t)width + lane] = (int8_t)(legal ? code : BGS_SOLVE_NONE);
        }
        if (lane == 0 && done) done[i] = (int32_t)ran;
        won_columns = __builtin_amdgcn_ballot_w64(legal && tag == kTagWin);
        among = __builtin_amdgcn_ballot_w64(legal && tag != kTagLoss);
        among = among ? among : ~0ull;
    }
    if (best) {
        // the most visits, then the larger 2 * wins + draws, then the lower column; an illegal column has no visits
        int32_t top = -1;
        uint32_t top_n = 0, top_s = 0;
        for (uint32_t c = 0; running && c < width; ++c) {
            const uint32_t cn = (uint32_t)__builtin_amdgcn_readlane((int)nv, (int)c);
            const uint32_t cs = (uint32_t)__builtin_amdgcn_readlane((int)sv, (int)c);
            if constexpr (PROVE) {
                if (!((among >> c) & 1ull)) continue;
            }
            if (cn > 0u && (top < 0 || cn > top_n || (cn == top_n && cs > top_s))) {
                top = (int32_t)c;
                top_n = cn;
                top_s = cs;
            }
        }
        if constexpr (PROVE) {      // a proved win is the move (there is one at most: the search stopped at the first)
            if (won_columns) top = (int32_t)__builtin_ctzll(won_columns);
        }
        if (lane == 0) best[i] = top;
    }
    if (lane == 0) {
        if constexpr (FOREST) {
            head[0] = used;         // the header: the planes were recorded when the tree was emptied, or carried with it
            if (carried) carried[i] = (int32_t)brought;
        }
        if (nodes) nodes[i] = (int32_t)(used ? used - 1u : 0u);
    }
    if (stepped) atomicAdd(&step_sum, (unsigned long long)stepped);
    __syncthreads();
    if (lane == 0 && step_sum) atomicAdd(steps + (size_t)(blockIdx.x % BGS_STEP_SHARDS) * BGS_STEP_STRIDE, step_sum);
}

// what a search launch is given beyond the batch (connect_search / connect_forest_search fill it)
struct ConnectSearchArgs {
    uint64_t seed;
    uint32_t iterations, leaf_playouts, explore, max_plies;
    uint32_t capacity, restart;             // the plain search: iterations + 1, 1
    int32_t *counts, *visits, *best, *nodes;
    int32_t* carried;                       // the plain search: nullptr
    void* trees;                            // the workspace, or the forest
    int8_t* proved = nullptr;               // the proving search alone: the root's tags and the iterations run
    int32_t* done = nullptr;
};

template <int NW, bool PER_PLY, int POLICY, bool FOREST, bool PROVE = false>
void launch_search(const bgs_batch* b, const EvalGeom& g, const ConnectSearchArgs& a) {
    // game ids: ((first_game + i) * T + t) * P + j = first_game * T * P + (i * T + t) * P + j, mod 2^64
    const uint64_t game_base = b->first_game * (uint64_t)a.iterations * (uint64_t)a.leaf_playouts;
    constexpr int64_t kMaxBlocks = (int64_t)1 << 30;
    for (int64_t i0 = 0; i0 < b->n; i0 += kMaxBlocks) {
        const int64_t blocks = b->n - i0 < kMaxBlocks ? b->n - i0 : kMaxBlocks;
        hipLaunchKernelGGL((k_connect_search<NW, PER_PLY, POLICY, FOREST, PROVE>), dim3((uint32_t)blocks), dim3(BGS_WAVE), 0, b->stream,
                           g, (const uint64_t*)b->d_planes, (const uint8_t*)b->d_status, b->n, a.seed, game_base, a.iterations,
                           a.leaf_playouts, a.explore, a.max_plies, i0, a.capacity, a.restart, static_cast<uint32_t*>(a.trees),
                           a.counts, a.visits, a.best, a.nodes, a.carried, b->d_steps, a.proved, a.done);
    }
}

// The re-rooting (bgs_connect_forest_advance): one wave a tree, in place, one launch.  Nodes are made in increasing index
// order, so a child's index is above its parent's, and a compaction that keeps the order keeps that property:
//   mark     the subtree of r = the root's child[c] in a bit mask (LDS), by an ascending sweep from r over chunks of 64
//            nodes: a chunk's words come in coalesced, lane l then marks the children of node base + l if that node is
//            marked, and the chunk is swept again while a lane finds its node newly marked (a chain inside the chunk);
//   number   new[v] = the marked nodes below v: a prefix popcount, one entry a mask word;
//   move     chunk by chunk in ascending order: the chunk is read into LDS, a barrier, then every marked node goes to
//            new[v] <= v with its child words mapped -- a slot of this chunk or an earlier one, never one still to be read;
//   header   one lane, last, behind a barrier: the count, and the stone of column c dropped on the recorded position.
// Chunks without a marked node are neither read nor written.  The work is that of the nodes in use, not of `capacity`.
__global__ void __launch_bounds__(BGS_WAVE)
k_connect_forest_advance(uint32_t height, uint32_t width, uint32_t nw, const int32_t* __restrict__ columns, uint32_t capacity,
                         uint32_t* forest, int32_t* __restrict__ kept, int64_t root_base) {
    extern __shared__ __attribute__((aligned(16))) uint32_t forest_lds[];
    const uint32_t lane = threadIdx.x;
    const uint32_t node_words = width * 3u;
    const uint32_t mask_room = (((capacity + 31u) >> 5) + 3u) & ~3u;
    uint32_t* const mask = forest_lds;              // bit v: node v stays
    uint32_t* const below = mask + mask_room;       // the marked nodes in the mask words before this one
    uint32_t* const chunk = below + mask_room;      // 64 nodes
    const int64_t i = root_base + (int64_t)blockIdx.x;
    uint32_t* const head = forest + (uint64_t)i * forest_tree_words(width, capacity);
    uint32_t* const tree = head + kForestHeaderWords;

    const int32_t c = columns[i];
    uint32_t used = head[0];
    used = (uint32_t)__builtin_amdgcn_readfirstlane((int)(used <= capacity ? used : 0u));
    if (c < 0) {                                    // untouched
        if (kept && lane == 0) kept[i] = (int32_t)(used ? used - 1u : 0u);
        return;
    }
    // the new root: the child of the root's edge c (0: never played, terminal, did not fit, a full column)
    uint32_t r = (used != 0u && (uint32_t)c < width) ? tree[2u * width + (uint32_t)c] : 0u;
    r = (uint32_t)__builtin_amdgcn_readfirstlane((int)(r < used ? r : 0u));
    // the cell the stone takes on the recorded position, and its mover: plane bits are counted in 32-bit words
    const uint32_t plane_words = 2u * nw;           // 32-bit words a player
    uint32_t stones = lane < 2u * plane_words ? (uint32_t)__popc(head[2u + lane]) : 0u;
    for (int d = 32; d >= 1; d >>= 1) stones += (uint32_t)__shfl_xor((int)stones, d);
    uint32_t at = 0;
    if ((uint32_t)c < width) {
        for (uint32_t y0 = 0; y0 < height; y0 += BGS_WAVE) {
            const uint32_t bit = (uint32_t)c * (height + 1u) + y0 + lane;
            const bool taken = y0 + lane < height &&
                               (((head[2u + (bit >> 5)] | head[2u + plane_words + (bit >> 5)]) >> (bit & 31u)) & 1u) != 0u;
            at += (uint32_t)__popcll(__builtin_amdgcn_ballot_w64(taken));
        }
    }
    if (r == 0u || at >= height) {                  // emptied: the next search starts anew from the batch's board
        if (lane == 0) {
            head[0] = 0;
            if (kept) kept[i] = 0;
        }
        return;
    }

    // ---- mark
    const uint32_t mask_words = (used + 31u) >> 5;
    for (uint32_t k = lane; k < mask_words; k += BGS_WAVE) mask[k] = 0;
    __syncthreads();
    if (lane == 0) mask[r >> 5] = 1u << (r & 31u);
    __syncthreads();
    for (uint32_t base = r & ~63u; base < used; base += 64u) {
        const uint32_t m0 = mask[base >> 5], m1 = (base >> 5) + 1u < mask_words ? mask[(base >> 5) + 1u] : 0u;
        if ((m0 | m1) == 0u) continue;              // (uniform) nothing of this chunk is in the subtree
        const uint32_t count = used - base < 64u ? used - base : 64u;
        for (uint32_t k = lane; k < count * node_words; k += BGS_WAVE) chunk[k] = tree[(uint64_t)base * node_words + k];
        __syncthreads();
        bool done = false;
        for (;;) {
            const uint32_t v = base + lane;
            const bool go = !done && lane < count && ((mask[v >> 5] >> (v & 31u)) & 1u) != 0u;
            if (__builtin_amdgcn_ballot_w64(go) == 0) break;
            if (go) {
                for (uint32_t x = 0; x < width; ++x) {
                    const uint32_t ch = chunk[lane * node_words + 2u * width + x];
                    if (ch > v && ch < used) atomicOr(mask + (ch >> 5), 1u << (ch & 31u));
                }
                done = true;
            }
            __syncthreads();
        }
        __syncthreads();                            // the chunk is free for the next one
    }

    // ---- number
    uint32_t total = 0;
    for (uint32_t k0 = 0; k0 < mask_words; k0 += BGS_WAVE) {
        const uint32_t k = k0 + lane;
        const uint32_t bits = k < mask_words ? (uint32_t)__popc(mask[k]) : 0u;
        uint32_t upto = bits;                       // the inclusive scan of the wave
        for (int d = 1; d < BGS_WAVE; d <<= 1) {
            const uint32_t other = (uint32_t)__shfl_up((int)upto, d);
            upto += lane >= (uint32_t)d ? other : 0u;
        }
        if (k < mask_words) below[k] = total + upto - bits;
        total += (uint32_t)__shfl((int)upto, BGS_WAVE - 1);
    }
    __syncthreads();

    // ---- move
    for (uint32_t base = r & ~63u; base < used; base += 64u) {
        const uint32_t m0 = mask[base >> 5], m1 = (base >> 5) + 1u < mask_words ? mask[(base >> 5) + 1u] : 0u;
        if ((m0 | m1) == 0u) continue;
        const uint32_t count = used - base < 64u ? used - base : 64u;
        for (uint32_t k = lane; k < count * node_words; k += BGS_WAVE) chunk[k] = tree[(uint64_t)base * node_words + k];
        __syncthreads();                            // every word of the chunk is read before one is written
        for (uint32_t l = 0; l < count; ++l) {
            const uint32_t v = base + l;
            const uint32_t word = mask[v >> 5];
            if (((word >> (v & 31u)) & 1u) == 0u) continue;
            const uint32_t to = below[v >> 5] + (uint32_t)__popc(word & ((1u << (v & 31u)) - 1u));
            if (lane < node_words) {
                uint32_t x = chunk[l * node_words + lane];
                if (lane >= 2u * width) {           // a child word: the child's new index (a kept node's children are kept)
                    x = (x > v && x < used) ? below[x >> 5] + (uint32_t)__popc(mask[x >> 5] & ((1u << (x & 31u)) - 1u)) : 0u;
                }
                tree[(uint64_t)to * node_words + lane] = x;
            }
        }
        __syncthreads();                            // the chunk is free for the next one
    }

    // ---- header (the tree's writes are issued; the count and the stone go last)
    __syncthreads();
    if (lane == 0) {
        const uint32_t bit = (uint32_t)c * (height + 1u) + at;
        head[0] = total;
        head[2u + ((stones & 1u) ? plane_words : 0u) + (bit >> 5)] |= 1u << (bit & 31u);
        if (kept) kept[i] = (int32_t)(total - 1u);
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
constexpr uint32_t kBounceMaxPlies = 65535u;      // plies are uint16 (the Bounce unit's kMaxPlies)
// persistent waves per SIMD (the kernel holds 5 by its registers).  Default board, max_plies 1024, 10^9 env-steps/s at
// 256 roots x 256 playouts / 4096 x 64: 1 wave 2.01 / 2.47, 2 waves 2.71 / 4.09, 4 waves 2.88 / 5.13 (docs/EXPERIMENTS.md §16)
constexpr int kBounceEvalWps = 4;

// legal moves of a root: 0 when it has ended or (CAPPED: the evaluation, which stores the plies its games hold) holds the
// most plies a board can
template <bool CAPPED, class GEO>
__device__ __forceinline__ uint32_t b_root_moves(const GEO& g, const uint64_t* __restrict__ planes, const uint8_t* __restrict__ status,
                                                 const uint16_t* __restrict__ plies_buf, int64_t n, int64_t i) {
    if (status[i] != BGS_ST_RUNNING || (CAPPED && plies_buf[i] >= kBounceMaxPlies)) return 0u;
    const Board b = load_board(planes, n, i);
    const uint64_t occ = occupancy(b);
    const uint32_t player = plies_buf[i] & 1u;
    uint64_t src = movable(g, occ, player);
    uint32_t cnt = 0;
    while (src) {
        const int s = __ffsll((unsigned long long)src) - 1;
        src &= src - 1;
        cnt += (uint32_t)__popcll(reach(g, b, occ, player, s));
    }
    return cnt;
}

// ---- the first pass: legal moves a root -> ends[i] (inclusive prefix over the batch), in three small kernels
// (each workgroup scans its 256 roots; one workgroup scans the workgroups' totals; the totals are added back)
__device__ __forceinline__ uint64_t block_inclusive_scan(uint64_t v, uint64_t* lds) {
    lds[threadIdx.x] = v;
    __syncthreads();
    for (uint32_t off = 1; off < BGS_BLOCK; off <<= 1) {
        const uint64_t add = threadIdx.x >= off ? lds[threadIdx.x - off] : 0ull;
        __syncthreads();
        lds[threadIdx.x] += add;
        __syncthreads();
    }
    return lds[threadIdx.x];
}

template <class GEO, bool CAPPED = true>
__global__ void __launch_bounds__(BGS_BLOCK)
k_bounce_eval_count(GEO g, const uint64_t* __restrict__ planes, const uint8_t* __restrict__ status, const uint16_t* __restrict__ plies_buf,
                    int64_t n, uint64_t* __restrict__ ends, uint64_t* __restrict__ totals) {
    __shared__ uint64_t lds[BGS_BLOCK];
    const int64_t i = (int64_t)blockIdx.x * BGS_BLOCK + threadIdx.x;
    const uint64_t mine = i < n ? b_root_moves<CAPPED>(g, planes, status, plies_buf, n, i) : 0ull;
    const uint64_t incl = block_inclusive_scan(mine, lds);
    if (i < n) ends[i] = incl;
    if (threadIdx.x == BGS_BLOCK - 1) totals[blockIdx.x] = incl;
}

// totals[0 .. blocks) -> exclusive prefix, in place (one workgroup, a contiguous run of entries a thread)
__global__ void __launch_bounds__(BGS_BLOCK) k_bounce_eval_scan_totals(uint64_t* __restrict__ totals, int64_t blocks) {
    __shared__ uint64_t lds[BGS_BLOCK];
    const int64_t per = (blocks + BGS_BLOCK - 1) / BGS_BLOCK;
    const int64_t lo = (int64_t)threadIdx.x * per, hi = lo + per < blocks ? lo + per : blocks;
    uint64_t sum = 0;
    for (int64_t k = lo; k < hi; ++k) sum += totals[k];
    uint64_t run = block_inclusive_scan(sum, lds) - sum;
    for (int64_t k = lo; k < hi; ++k) {
        const uint64_t t = totals[k];
        totals[k] = run;
        run += t;
    }
}

__global__ void __launch_bounds__(BGS_BLOCK)
k_bounce_eval_add_totals(uint64_t* __restrict__ ends, const uint64_t* __restrict__ totals, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * BGS_BLOCK + threadIdx.x;
    if (i < n && blockIdx.x) ends[i] += totals[blockIdx.x];
}

// one more finished game on a W/D/L triple, seen from the root's mover.  s is the game's status, 1 / 2 (the winner + 1)
// or BGS_ST_DRAW; a capped game (s = 0) is counted nowhere
__device__ __forceinline__ void wdl_count(uint32_t s, uint32_t root_mover, uint32_t& wins, uint32_t& draws, uint32_t& losses) {
    wins += (s != 0u && s != BGS_ST_DRAW && s - 1u == root_mover) ? 1u : 0u;
    losses += (s != 0u && s != BGS_ST_DRAW && s - 1u != root_mover) ? 1u : 0u;
    draws += s == BGS_ST_DRAW ? 1u : 0u;
}

// BGS_POLICY_DECISIVE for Bounce (include/bgs.h): the candidate list of a ply is W, the actions whose target lies in the
// mover's goal row, when W is not empty.  Every element of W ends the game for the mover and the outputs are counts and
// steps alone, so such a ply neither draws nor moves: the lanes that have just searched fold their sources' LDS masks
// with the goal row into a flag, and a flagged lane's ply is one transition and the mover's win.  Narrower than Connect's
// policy (no blocking step): the moves that leave the opponent without a win in one need a move search per candidate.
template <int NC>
__device__ __forceinline__ bool b_can_win(const FlatMoves<NC>& m, const uint32_t* column, uint64_t goal) {
    const uint32_t glo = (uint32_t)goal, ghi = (uint32_t)(goal >> 32);
    uint32_t hit = 0;
#pragma unroll
    for (int x = 0; x < 8 * NC; ++x) {   // (a column without targets was not written by this search: its dwords are stale)
        const uint32_t cnt = (uint32_t)(m.counts[x >> 3] >> (8 * (x & 7))) & 255u;
        const uint32_t lo = column[(2u * x) * BGS_BLOCK] & glo, hi = column[(2u * x + 1u) * BGS_BLOCK] & ghi;
        hit |= cnt ? (lo | hi) : 0u;
    }
    return hit != 0u;
}

template <int NC>
__device__ __forceinline__ FlatMoves<NC> no_moves() {
    FlatMoves<NC> m;
#pragma unroll
    for (int k = 0; k < NC; ++k) m.counts[k] = 0;
    m.n = 0;
    m.row_base = 0;
    return m;
}

// The Bounce playout step of the flat evaluation (k_bounce_evaluate) and of the tree searches (k_bounce_search: plain,
// forest, proving); k_bounce_evaluate_halving plays the same ply from a copy of its own, which says why.  The wave plays
// one ply of every lane's game.  A lane's game is its kernel's own locals, taken by reference:
// the board b with `plies` plies and the status st (BGS_ST_RUNNING, or how the game ended: 1 / 2 the winner + 1,
// BGS_ST_DRAW), the global game id, the mover's action list mv, and the flags `has` (the lane holds a
// game), `search` (b has just moved: its list is not made yet), have_block (blk holds the draws of the 4-ply block of
// `plies`) and, for BGS_POLICY_DECISIVE, can_win (the list has a target in the mover's goal row).  A lane that takes a new
// game sets has, search = "st is running" (a blocked side to move is settled by the search, also at the cap) and clears
// have_block.
//   * The action lists of the boards that have just moved, into the lane's LDS column.  A side to move without an action
//     settles the game: the other side wins if IT could move, else a draw.
//   * A game that has ended, or runs and holds the cap (st = BGS_ST_RUNNING = 0: counted nowhere), leaves the lane, and
//     the function returns true for it: nothing below touches its st, so the caller finds there how it ended.  What a
//     kernel does with a finished game is all the kernels differ in here, and stays in the kernel.
//   * One ply on every running board.  BGS_POLICY_DECISIVE: when the list has a target in the mover's goal row every
//     candidate ends the game for the mover, so the ply is one transition and the mover's win, nothing drawn or moved.
//     Else the draw of DESIGN.md §3 ("RNG contract") at the game's absolute ply -- word plies & 3 of
//     philox4x32_10(seed, game, plies >> 2), one call a four plies and for a new game -- indexes the list.
// `stepped` grows by the transitions the lane made.
template <int NC, int POLICY, class GEO>
__device__ __forceinline__ bool bounce_playout_ply(const GEO& g, uint64_t seed, uint32_t max_plies, uint32_t* column, Board& b,
                                                   FlatMoves<NC>& mv, uint32_t& st, uint32_t& plies, uint64_t game, bool& has,
                                                   bool& search, bool& have_block, bool& can_win, Philox4& blk, uint32_t& stepped) {
    if (__builtin_amdgcn_ballot_w64(search)) {
        const uint64_t occ = occupancy(b);
        enumerate_flat<NC, true>(g, b, occ, plies & 1u, search, column, mv);
        const bool blocked = search && mv.n == 0u;
        if (__builtin_amdgcn_ballot_w64(blocked)) {
            FlatMoves<NC> other = no_moves<NC>();
            enumerate_flat<NC, true>(g, b, occ, 1u - (plies & 1u), blocked, column, other);
            if (blocked) st = other.n ? (1u - (plies & 1u)) + 1u : BGS_ST_DRAW;
        }
        if constexpr (POLICY == BGS_POLICY_DECISIVE) {
            if (search) can_win = st == BGS_ST_RUNNING && b_can_win<NC>(mv, column, (plies & 1u) ? g.goal_bottom : g.goal_top);
        }
        search = false;
    }
    const bool run = has && st == BGS_ST_RUNNING && plies < max_plies;
    const bool finished = has && !run;
    has = has && run;
    if constexpr (POLICY == BGS_POLICY_DECISIVE) {
        if (run && can_win) {
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
    return finished;
}

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
    const int64_t blocks = (b->n + BGS_BLOCK - 1) / BGS_BLOCK;
    hipLaunchKernelGGL((k_bounce_eval_count<GEO>), dim3((uint32_t)blocks), dim3(BGS_BLOCK), 0, b->stream, g, (const uint64_t*)b->d_planes,
                       (const uint8_t*)b->d_status, (const uint16_t*)b->d_plies, b->n, d_ends, d_totals);
    if (blocks > 1) {
        hipLaunchKernelGGL(k_bounce_eval_scan_totals, dim3(1), dim3(BGS_BLOCK), 0, b->stream, d_totals, blocks);
        hipLaunchKernelGGL(k_bounce_eval_add_totals, dim3((uint32_t)blocks), dim3(BGS_BLOCK), 0, b->stream, d_ends,
                           (const uint64_t*)d_totals, b->n);
    }
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
// The most arms of a packed root.  The sources are the k <= W pieces of one interior row; a target is an empty interior
// cell or a cell of the mover's goal row: at most (H - 2) * W - k + W of them whatever else the board holds.  So
// A <= k * ((H - 1) * W - k), greatest over H * W <= 64 at 16 x 4 with k = 16 (boards of fewer than 3 rows have no
// interior and no move).
constexpr uint32_t bounce_most_arms() {
    uint32_t most = 0;
    for (uint32_t h = 3; h <= BGS_BOUNCE_MAX_CELLS; ++h)
        for (uint32_t w = 1; h * w <= BGS_BOUNCE_MAX_CELLS; ++w)
            for (uint32_t k = 1; k <= w; ++k) most = k * ((h - 1) * w - k) > most ? k * ((h - 1) * w - k) : most;
    return most;
}
constexpr uint32_t kBounceHalvingMaxArms = 512;
static_assert(bounce_most_arms() == kBounceHalvingMaxArms, "the arm table, the survivor lists and the tally hold every legal move of a root");
static_assert(kBounceHalvingMaxArms * 10u < (1u << 16), "arm indices and A * R(A) fit the tables' 16 bits and a uint32 with room");

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

// ================================================================================================================
// UCT tree search for Bounce (bgs_bounce_search_moves, include/bgs.h): k_connect_search's iteration with "column" read as
// "arm", for a game whose nodes have 1 .. 512 arms and whose descents have no h * w bound.
//
// Shape.  One workgroup of BGS_BLOCK lanes owns one root for the whole launch, as in k_bounce_evaluate_halving (the move
// tile's stride is BGS_BLOCK whatever the team).  The descent is team-uniform: every lane holds the position p and
// applies the same stored moves to it.
//
// The tree, per root: a pool of `edges` (E) edges of four words (n, s, child or outcome, source cell << 8 | target cell), a
// node table of C entries (first edge, arms) and the descent path (C edge indices: a descent leaves every node at most
// once).  A node's arms are the A consecutive edges from its first edge, in canonical order; they are written once, when
// the node is made (movable, and reach by lane x, as the halving kernel's root set-up), so a descent replays stored moves
// and never searches the moves of a node it has been through.  The third word of an edge is 0 (no child yet), a node
// index 1 .. C - 1, kEdgeEnded | the BGS_ST_* code of the game the edge ends (the outcome is kept absolute, not relative to
// the mover: nothing needs the relative form) or kEdgeCapped (p' is running and holds the cap: no node, now or later):
// revisiting an edge that ends the game or is capped costs no move search either.
//
// One kernel, two places for the tree (the template parameter FOREST):
//   the plain search (bgs_bounce_search_moves): the tree lives in the caller's workspace with C = iterations + 1 (iteration
//     t passes through the root and at most t made nodes), starts empty and is forgotten after the launch.  A root's
//     share: the pool, the node table, the path; rounded up to 256 bytes;
//   the forest (bgs_bounce_forest_search / bgs_bounce_forest_advance): the trees are kept from launch to launch in the
//     caller's memory, C = `capacity` nodes a tree, and re-rooted between the launches.  A tree's share of the forest, in
//     32-bit words, rounded up to 256 bytes:
//       word 0         the nodes in use, the root counted (0: an emptied tree)
//       word 1         the pool edges in use
//       word 2         the absolute ply count of the position the root stands for
//       word 3         the effective cap (min(max_plies, 65535)) the tree's kEdgeCapped sentinels were written under
//       words 4 .. 11  the position the root stands for: the four 64-bit planes of the batch, 8-byte aligned
//       words 16 ..    the E edges
//       then           the C node-table entries
//       then           the C words of descent path; they mean nothing between launches
//     With C <= 65536 and E <= BGS_BOUNCE_FOREST_MAX_EDGES = 2^29 a share has fewer than 2^32 words.
// FOREST changes these things and nothing else: where the share and its parts are; the exit of a root without arms (the
// forest's also empties the tree and writes `carried`); the start (the carried check, or the emptying, where the plain
// search makes node 0); "a node is made when the edge has no child, the tree holds fewer than C nodes AND the pool has
// room for its arms" (the plain tree has a node an iteration, so there only the pool is asked); and the header written
// back at the end, behind a barrier, with `carried`.  The iteration -- descent, refill loop, ply, back-propagation -- is
// one text.
//
// A descent step: the lanes read the node's edges strided (at most two a lane), reduce the lowest arm with n = 0 and
// N = sum n over the waves (shuffles) and the team (one LDS word a wave), and without an unplayed arm reduce the key
// (U << 9 | 511 - arm) + 1 the same way (U < 2^17).  The reduction words are double-buffered by the parity of the depth:
// every step has at least one barrier, so a wave cannot write a buffer that another wave still reads.
//
// The leaf's P playouts are the halving kernel's refill loop and bounce_playout_ply: the waves draw playouts
// from a counter in LDS, refill idle lanes at ply boundaries, count W/D/L of the root's mover in registers and add them
// to an LDS tally when the leaf is played out.  Lane k then updates edge k of the path.
//
// Ordering.  The tree, the node table and the path are written by some lanes and read by others, always of this
// workgroup: a __syncthreads() stands between every writer and its next reader (barriers A, B, C below, and the barriers
// of the descent).  Global memory beyond the workspace: the root, the outputs (counts and visits zeroed by the launcher:
// illegal slots are never stored; counts is accumulated by lane 0 alone) and the step counter, the only global atomic.
//
// The proving search (bgs_bounce_search_moves_proving; the template parameter PROVE, the plain tree only) keeps game-end
// facts on the edges, in the third word: kEdgeEnded | outcome is a fact as it stands, and a value backed up from the node
// below overwrites the child index with kEdgeProved | outcome (the outcome absolute in both, so the tag seen from a node
// is "outcome - 1 == its mover"; a decided node is never entered again, so its index is not missed).  kEdgeCapped and
// every word below kEdgeProved are OPEN.  PROVE changes five things and nothing else: a lane's arm is a candidate of the
// selection -- counts in N, can be the unplayed arm, has a key -- only while its tag is OPEN; after an iteration whose
// last edge ended the game the values go up the path (the node of path edge k is the child word of path edge k - 1,
// still intact while the walk goes upwards, so the path holds edges only, as before); a root whose value is no longer
// OPEN stops iterating; `proved` and `done` are written; and `best` looks at the root's tags.  The edge stays four words
// and the workspace is the plain search's.  A tagged edge is never selected, so the descent never reads an ended or a
// proved word as a child.
//
// Known limit: a root has one team, so a launch of few roots leaves most CUs idle, and leaf_playouts < BGS_BLOCK leaves
// lanes idle.
// ================================================================================================================
constexpr uint32_t kEdgeWords = 4;
constexpr uint32_t kEdgeEnded = 0xFFFFFFF0u;      // | BGS_ST_*: the edge ends the game (1, 2: the winner + 1; 3: a draw)
constexpr uint32_t kEdgeCapped = 0xFFFFFFFFu;     // the position behind the edge runs and holds the cap
constexpr uint32_t kEdgeProved = 0xFFFFFFE0u;     // | BGS_ST_*: (PROVE) a value backed up from below, the outcome absolute as in kEdgeEnded
constexpr uint32_t kNoArm = 0xFFFFu;
constexpr int kSearchTeamWaves = BGS_BLOCK / BGS_WAVE;
static_assert(((uint64_t)1 << 29) + 1u < kEdgeProved, "a child index (at most T <= 2^29) stays below the reserved ranges");

// (PROVE) the tag of an edge with third word `word`, seen from `mover`, the player to move at its node: every word of the
// two reserved ranges but kEdgeCapped is a fact (an edge that ends the game, or a value backed up), and its low bits are
// the absolute outcome
__device__ __forceinline__ uint32_t bounce_edge_tag(uint32_t word, uint32_t mover) {
    if (word < kEdgeProved || word == kEdgeCapped) return kTagOpen;
    const uint32_t outcome = word & 15u;
    return outcome == (uint32_t)BGS_ST_DRAW ? kTagDraw : (outcome - 1u == mover ? kTagWin : kTagLoss);
}
static_assert(kBounceHalvingMaxArms <= 2 * BGS_BLOCK, "a lane holds at most two arms of a node");
static_assert((uint32_t)BGS_ST_DRAW < 15u, "an outcome code fits the low bits of kEdgeEnded and stays below kEdgeCapped");

constexpr uint32_t kBounceForestHeaderWords = 16;

// words of a root's share of the workspace: the edge pool, the node table, the path; rounded up to 256 bytes
__host__ __device__ __forceinline__ uint64_t bounce_search_root_words(uint32_t iterations, uint32_t edges) {
    return ((uint64_t)edges * kEdgeWords + ((uint64_t)iterations + 1u) * 3u + 63u) & ~(uint64_t)63u;
}

// words of a tree's share of the forest: the header before the same three parts; rounded up to 256 bytes
__host__ __device__ __forceinline__ uint64_t bounce_forest_tree_words(uint32_t capacity, uint32_t edges) {
    return (kBounceForestHeaderWords + (uint64_t)edges * kEdgeWords + (uint64_t)capacity * 3u + 63u) & ~(uint64_t)63u;
}

__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += (uint32_t)__shfl_xor((int)v, off, BGS_WAVE);
    return v;
}
__device__ __forceinline__ uint32_t wave_min(uint32_t v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const uint32_t o = (uint32_t)__shfl_xor((int)v, off, BGS_WAVE);
        v = o < v ? o : v;
    }
    return v;
}
__device__ __forceinline__ uint32_t wave_max(uint32_t v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const uint32_t o = (uint32_t)__shfl_xor((int)v, off, BGS_WAVE);
        v = o > v ? o : v;
    }
    return v;
}

// what the forest's instantiation alone is given, last in the list; the plain one's is empty, so the plain kernel's
// arguments keep the offsets they have without the forest (these kernels sit at the SGPR ceiling, and the arguments are
// the first SGPRs loaded: docs/EXPERIMENTS.md §33)
template <bool FOREST>
struct BounceForestArgs {};
template <>
struct BounceForestArgs<true> {
    uint32_t capacity, restart;
    int32_t* carried;
};

// what the proving instantiation alone is given, in the forest's place (the forest does not prove, so the last argument is
// one or the other and the plain and the forest kernels keep the arguments they had): the root's tags and the
// iterations run (either may be nullptr)
struct BounceProveArgs {
    int8_t* proved;
    int32_t* done;
};
template <bool FOREST, bool PROVE>
using BounceExtraArgs = std::conditional_t<PROVE, BounceProveArgs, BounceForestArgs<FOREST>>;

template <class GEO, int NC, int POLICY, bool FOREST, bool PROVE = false>
__global__ void __launch_bounds__(BGS_BLOCK)
k_bounce_search(GEO g, const uint64_t* __restrict__ planes, const uint8_t* __restrict__ status, const uint16_t* __restrict__ plies_buf,
                int64_t n, uint64_t seed, uint64_t game_base, uint32_t iterations, uint32_t leaf_playouts, uint32_t explore,
                uint32_t max_plies, uint32_t edges, uint32_t slots, int64_t root_base, uint32_t* trees, int32_t* counts,
                int32_t* visits, int32_t* best, int32_t* nodes, int32_t* used_out, unsigned long long* __restrict__ steps,
                BounceExtraArgs<FOREST, PROVE> extra) {
    static_assert(!(PROVE && FOREST), "the forest does not prove");
    extern __shared__ uint32_t target_tile[];                      // [2 * 8 * NC dwords][256 lanes]
    __shared__ uint64_t node_targets[8 * NC];                      // targets of the piece in column x of the active row of p'
    __shared__ uint64_t other_targets[8 * NC];                     // ... of the side that has just moved, when p' is blocked
    __shared__ uint32_t red_min[2][kSearchTeamWaves], red_sum[2][kSearchTeamWaves], red_key[2][kSearchTeamWaves];
    __shared__ uint32_t tally[3];                                  // W/D/L of the iteration's playouts, for the root's mover
    __shared__ uint32_t next_item;                                 // the leaf's next playout
    uint32_t* const column = target_tile + threadIdx.x;
    const uint32_t tid = threadIdx.x, lane = threadIdx.x & (BGS_WAVE - 1), wave = threadIdx.x / BGS_WAVE;
    const uint32_t hw = (uint32_t)(g.h * g.w);
    const int64_t i = root_base + (int64_t)blockIdx.x;             // (the grid holds exactly the roots of this launch)
    // ---- where the tree is: behind the header of its share of the forest, or bare in the workspace
    uint32_t *head = nullptr, *pool;
    uint64_t* head_planes = nullptr;
    uint64_t table_room;                                                        // the node table's entries (C)
    if constexpr (FOREST) {
        head = trees + (uint64_t)i * bounce_forest_tree_words(extra.capacity, edges);
        head_planes = reinterpret_cast<uint64_t*>(head + 4);
        pool = head + kBounceForestHeaderWords;
        table_room = extra.capacity;
    } else {
        pool = trees + (uint64_t)i * bounce_search_root_words(iterations, edges);
        table_room = (uint64_t)iterations + 1u;
    }
    uint32_t* const node_tab = pool + (uint64_t)edges * kEdgeWords;             // node v: first edge, arms
    uint32_t* const path = node_tab + table_room * 2u;                          // edge k of the descent
    const auto uniform = [](uint32_t x) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)x); };

    // the targets of `player`'s pieces on `bd`, the piece in column x by lane x, into dst (complete behind the caller's
    // barrier); returns the cell of column 0 of the active row
    const auto spread = [&](const Board& bd, uint64_t occ, uint32_t player, bool live, uint64_t* dst) {
        const uint64_t sources = live ? movable(g, occ, player) : 0ull;
        const uint32_t first_source = sources ? (uint32_t)(__ffsll((unsigned long long)sources) - 1) : 0u;
        const uint32_t base = ((first_source * g.inv_w) >> 16) * (uint32_t)g.w;
        if (tid < 8 * NC) {
            const bool piece = tid < (uint32_t)g.w && ((sources >> ((base + tid) & 63u)) & 1ull);
            dst[tid] = piece ? reach(g, bd, occ, player, (int)(base + tid)) : 0ull;
        }
        return base;
    };
    const auto count_arms = [&](const uint64_t* t) {
        uint32_t arms = 0;
        for (uint32_t x = 0; x < 8 * NC; ++x) arms += (uint32_t)__popcll(t[x]);
        return uniform(arms);
    };
    // the arm table of a new node: `arms` fresh edges from edge `first`, in canonical order (first + arms <= edges)
    const auto make_arms = [&](uint32_t first, uint32_t arms, uint32_t base) {
        for (uint32_t a = tid; a < arms; a += BGS_BLOCK) {
            uint32_t j = a, x = 0;
            for (; x < 8 * NC - 1; ++x) {
                const uint32_t cnt = (uint32_t)__popcll(node_targets[x]);
                if (j < cnt) break;
                j -= cnt;
            }
            const uint32_t move = ((base + x) << 8) | select_bit64(node_targets[x], j);
            *reinterpret_cast<uint4*>(pool + (uint64_t)(first + a) * kEdgeWords) = make_uint4(0u, 0u, 0u, move);
        }
    };

    // ---- the root: its arms say whether there is anything to search
    const Board root = load_board(planes, n, i);
    const uint32_t rply = plies_buf[i];
    const uint32_t root_mover = rply & 1u;
    // (an ended root and one that holds the most plies a board can have no arms, as in k_bounce_eval_count)
    const uint32_t root_base_cell = spread(root, occupancy(root), root_mover, status[i] == BGS_ST_RUNNING && rply < kBounceMaxPlies, node_targets);
    __syncthreads();
    const uint32_t root_arms = count_arms(node_targets);
    if (root_arms == 0u) {   // nothing to search (FOREST: an emptied tree); counts and visits stay zero
        if (tid == 0) {
            if constexpr (FOREST) {
                head[0] = 0;
                head[1] = 0;
                if (extra.carried) extra.carried[i] = 0;
            }
            if (best) best[i] = -1;
            if (nodes) nodes[i] = 0;
            if (used_out) used_out[i] = 0;
            if constexpr (PROVE) {      // (every slot of `proved` stays BGS_SOLVE_NONE, as the launcher filled it)
                if (extra.done) extra.done[i] = 0;
            }
        }
        return;
    }

    // ---- the start.  The plain tree starts empty.  FOREST: the carried check; a tree that fails it is emptied.  Every wave
    // reads the header and decides for itself; the decision is the team's because the words it reads do not change while it
    // is made: nothing of the header, the table or the pool is written before barrier (H) below, which every wave passes
    // with its reads returned (readfirstlane needs them) whatever it decided.  Behind (H) the waves hold the same `keep`, so
    // the branches that follow -- and the barriers inside them -- are taken by all four waves or by none.
    uint32_t made = 0, used = 0;        // (team-uniform) nodes in the tree, the root not counted; pool edges in use
    bool keep = false;
    if constexpr (FOREST) {
        const uint32_t count = uniform(head[0]);                    // (the header counts the root)
        used = uniform(head[1]);
        keep = extra.restart == 0u && count >= 1u && count <= extra.capacity && used >= root_arms && used <= edges && head[2] == rply &&
               head[3] == max_plies;
        if (keep) {
#pragma unroll
            for (int j = 0; j < 4; ++j) keep = keep && head_planes[j] == root.v[j];
        }
        keep = uniform(keep ? 1u : 0u) != 0u;
        __syncthreads();                // (H) every wave has read the header before any wave rewrites it
        if (keep) {                     // N + T * P < 2^31: the root's n stay in int32 (the root's block starts at edge 0)
            uint32_t sum = 0;
            for (uint32_t a = tid; a < root_arms; a += BGS_BLOCK) sum += pool[(uint64_t)a * kEdgeWords];
            sum = wave_sum(sum);
            if (lane == 0) red_sum[0][wave] = sum;
            __syncthreads();
            uint64_t total = 0;
#pragma unroll
            for (int w = 0; w < kSearchTeamWaves; ++w) total += red_sum[0][w];
            keep = total + (uint64_t)iterations * leaf_playouts < (1ull << 31);
            keep = uniform(keep ? 1u : 0u) != 0u;
            __syncthreads();            // (red_sum[0] is free for the first descent step)
        }
        made = count - 1u;
    }
    if (!keep) {                        // node 0 and its arms; FOREST: board i recorded
        make_arms(0u, root_arms, root_base_cell);
        if (tid == 0) {
            node_tab[0] = 0u;
            node_tab[1] = root_arms;
            if constexpr (FOREST) {
                head[2] = rply;
                head[3] = max_plies;
#pragma unroll
                for (int j = 0; j < 4; ++j) head_planes[j] = root.v[j];
            }
        }
        made = 0u;
        used = root_arms;
    }
    [[maybe_unused]] const uint32_t brought = made;
    __syncthreads();
    const auto slot_of = [&](uint32_t move) { return ((move >> 8) - root_base_cell) * hw + (move & 255u); };

    Board b;                         // the lane's game
#pragma unroll
    for (int j = 0; j < 4; ++j) b.v[j] = 0;
    FlatMoves<NC> mv = no_moves<NC>();
    uint32_t st = 0, plies = 0, stepped = 0;
    uint64_t game = 0;
    bool has = false, search = false, have_block = false;
    [[maybe_unused]] bool can_win = false;   // (BGS_POLICY_DECISIVE) the list the lane holds has a target in the mover's goal row
    Philox4 blk;
    blk.v[0] = blk.v[1] = blk.v[2] = blk.v[3] = 0;

    [[maybe_unused]] uint32_t ran = 0;      // PROVE (team-uniform): the iterations run, and whether the root's value is proved
    [[maybe_unused]] bool decided = false;
    for (uint32_t t = 0; t < iterations; ++t) {
        if constexpr (PROVE) {
            if (decided) break;
            ran = t + 1u;
        }
        // ---- descent (team-uniform): p is the position at node v
        Board p = root;
        uint32_t ply = rply, v = 0, depth = 0, move0 = 0;
        uint32_t leaf = BGS_ST_RUNNING;     // the outcome of an edge that ends the game
        bool capped = false;                // p' runs and holds the cap
        for (;;) {
            const uint32_t first = uniform(node_tab[2u * v]), arms = uniform(node_tab[2u * v + 1u]);
            const uint32_t* const node = pool + (uint64_t)first * kEdgeWords;
            uint32_t na[2] = {0u, 0u}, sa[2] = {0u, 0u};
            uint32_t fresh = kNoArm, sum = 0;
            [[maybe_unused]] bool open[2] = {false, false};   // PROVE: the lane's arm is a candidate (its tag is OPEN)
#pragma unroll
            for (uint32_t k = 0; k < 2; ++k) {
                const uint32_t a = tid + k * BGS_BLOCK;
                if (a < arms) {
                    if constexpr (PROVE) {  // a tagged arm is in neither N, the unplayed arms nor the keys (the tag's sign is not needed)
                        const uint4 whole = *reinterpret_cast<const uint4*>(node + (uint64_t)a * kEdgeWords);
                        open[k] = whole.z < kEdgeProved || whole.z == kEdgeCapped;
                        na[k] = whole.x;
                        sa[k] = whole.y;
                        sum += open[k] ? whole.x : 0u;
                        fresh = (open[k] && whole.x == 0u && a < fresh) ? a : fresh;
                    } else {
                        const uint2 ns = *reinterpret_cast<const uint2*>(node + (uint64_t)a * kEdgeWords);
                        na[k] = ns.x;
                        sa[k] = ns.y;
                        sum += ns.x;
                        fresh = (ns.x == 0u && a < fresh) ? a : fresh;
                    }
                }
            }
            const uint32_t buf = depth & 1u;
            fresh = wave_min(fresh);
            sum = wave_sum(sum);
            if (lane == 0) {
                red_min[buf][wave] = fresh;
                red_sum[buf][wave] = sum;
            }
            __syncthreads();
            uint32_t arm = kNoArm, total = 0;
#pragma unroll
            for (int w = 0; w < kSearchTeamWaves; ++w) {
                arm = red_min[buf][w] < arm ? red_min[buf][w] : arm;
                total += red_sum[buf][w];
            }
            arm = uniform(arm);             // the expansion: the lowest arm never played
            if (arm == kNoArm) {
                const uint32_t scaled = explore * search_lg(uniform(total));
                uint32_t key = 0;           // (U(a) << 9 | 511 - a) + 1: the largest U, then the lowest arm
#pragma unroll
                for (uint32_t k = 0; k < 2; ++k) {
                    const uint32_t a = tid + k * BGS_BLOCK;
                    if (PROVE ? open[k] : a < arms) {
                        const uint32_t u = search_q(sa[k], na[k]) + search_isqrt(scaled / na[k]);
                        const uint32_t mine = ((u << 9) | (511u - a)) + 1u;
                        key = mine > key ? mine : key;
                    }
                }
                key = wave_max(key);
                if (lane == 0) red_key[buf][wave] = key;
                __syncthreads();
                uint32_t top = 0;
#pragma unroll
                for (int w = 0; w < kSearchTeamWaves; ++w) top = red_key[buf][w] > top ? red_key[buf][w] : top;
                arm = uniform(511u - ((top - 1u) & 511u));
            }
            const uint32_t e = first + arm;
            uint32_t* const edge = pool + (uint64_t)e * kEdgeWords;
            const uint32_t child = uniform(edge[2]), move = uniform(edge[3]);
            if (tid == 0) path[depth] = e;
            move0 = depth == 0u ? move : move0;
            const int s_cell = (int)(move >> 8), t_cell = (int)(move & 255u);
            const uint32_t mover = ply & 1u;
            move_piece(p, s_cell, t_cell);
            ply += 1u;
            depth += 1u;
            if (child == kEdgeCapped) {
                capped = true;
                break;
            }
            if (child >= kEdgeEnded) {
                leaf = child & 15u;
                break;
            }
            if (child != 0u) {
                v = child;
                continue;
            }
            // ---- the edge has no child: what p' is
            uint32_t code = 0;              // the edge's new third word, if any
            if ((1ull << t_cell) & (g.goal_top | g.goal_bottom)) {
                leaf = mover + 1u;
                code = kEdgeEnded | leaf;
            } else {
                const uint64_t occ = occupancy(p);
                const uint32_t base = spread(p, occ, ply & 1u, true, node_targets);
                __syncthreads();
                const uint32_t fan = count_arms(node_targets);
                if (fan == 0u) {            // the side to move is blocked: the mover wins if it could move, else a draw
                    spread(p, occ, mover, true, other_targets);
                    __syncthreads();
                    leaf = count_arms(other_targets) ? mover + 1u : (uint32_t)BGS_ST_DRAW;
                    code = kEdgeEnded | leaf;
                } else if (ply >= max_plies) {
                    capped = true;
                    code = kEdgeCapped;
                } else {
                    bool fits = used + fan <= edges;                 // (the plain table has iterations + 1 entries: room for every iteration's)
                    if constexpr (FOREST) fits = made + 1u < extra.capacity && fits;
                    if (fits) {             // a new node for p'; without room the edge is tried again next time
                        made += 1u;
                        make_arms(used, fan, base);
                        if (tid == 0) {
                            node_tab[2u * made] = used;
                            node_tab[2u * made + 1u] = fan;
                        }
                        code = made;
                        used += fan;
                    }
                }
            }
            if (tid == 0 && code) edge[2] = code;
            break;
        }

        // ---- the leaf's playouts: the halving kernel's refill loop, from p'
        const bool play = leaf == BGS_ST_RUNNING && !capped;
        if (tid < 3u) tally[tid] = 0;
        if (tid == 0) next_item = 0;
        __syncthreads();            // (A) the counter and the tally are zero; the path, the new node and the edge are written
        uint32_t wins = 0, draws = 0, losses = 0;
        if (play) {
            // G = ((first_game + i) * T + t) * P + j
            const uint64_t game0 = game_base + ((uint64_t)i * iterations + t) * (uint64_t)leaf_playouts;
            bool dry = false;        // (wave-uniform) the leaf's counter has nothing left for this wave
            while (!dry || __builtin_amdgcn_ballot_w64(has)) {
                const uint64_t need = __builtin_amdgcn_ballot_w64(!has);
                if (need && !dry) {
                    if (__builtin_amdgcn_ballot_w64(stepped >= (1u << 30))) {   // (a lane adds at most 65535 a playout)
                        add_steps(steps, stepped);
                        stepped = 0;
                    }
                    const uint32_t wanted = (uint32_t)__popcll(need);
                    uint32_t base = 0;
                    if (lane == 0) base = atomicAdd(&next_item, wanted);
                    base = uniform(base);
                    if (base + wanted >= leaf_playouts) dry = true;
                    const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(need >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)need, 0u));
                    if (!has && base + rank < leaf_playouts) {
                        game = game0 + (uint64_t)(base + rank);
                        b = p;
                        plies = ply;
                        st = BGS_ST_RUNNING;
                        has = true;
                        search = true;
                        have_block = false;
                    }
                }
                if (!__builtin_amdgcn_ballot_w64(has)) continue;

                if (bounce_playout_ply<NC, POLICY>(g, seed, max_plies, column, b, mv, st, plies, game, has, search, have_block, can_win, blk, stepped)) {
                    wdl_count(st, root_mover, wins, draws, losses);
                }
            }
            if (wins) atomicAdd(tally + 0, wins);
            if (draws) atomicAdd(tally + 1, draws);
            if (losses) atomicAdd(tally + 2, losses);
        }
        __syncthreads();            // (B) the tally is complete
        uint32_t tw = 0, td = 0, tl = 0;
        if (play) {
            tw = tally[0];
            td = tally[1];
            tl = tally[2];
        } else if (!capped) {       // all playouts of the iteration have the edge's outcome
            tw = (leaf != BGS_ST_DRAW && leaf - 1u == root_mover) ? leaf_playouts : 0u;
            tl = (leaf != BGS_ST_DRAW && leaf - 1u != root_mover) ? leaf_playouts : 0u;
            td = leaf == BGS_ST_DRAW ? leaf_playouts : 0u;
        }

        // ---- back-propagation: lane k takes edge k of the path; its mover is the root's at even k
        for (uint32_t k = tid; k < depth; k += BGS_BLOCK) {
            uint32_t* const edge = pool + (uint64_t)path[k] * kEdgeWords;
            edge[0] += leaf_playouts;
            edge[1] += td + 2u * ((k & 1u) ? tl : tw);
        }
        if (tid == 0) {
            int32_t* const c = counts + (i * (int64_t)slots + slot_of(move0)) * 3;
            c[0] += (int32_t)tw;
            c[1] += (int32_t)td;
            c[2] += (int32_t)tl;
        }
        if constexpr (PROVE) {
            // ---- the tags go up the path (team-uniform), while the node at hand has a value.  `leaf` is the team's (every
            // lane read the same words behind the descent's barriers), and only a fresh edge sets it here: a tagged edge is
            // never selected.  The last edge's word was written before barrier (A); an upper one by lane 0, behind barrier
            // (V) of the step below.  A step's flags -- 1: an arm is WIN, 2: an arm is OPEN, 4: an arm is DRAW -- go through
            // red_min[0], which is free from barrier (A) to the next descent: (U) stands between its writers and its readers,
            // (V) between its readers and the next step's writers.  Every lane reads the same four words behind (U), so the
            // break, the trip count and both barriers are the team's.
            if (leaf != BGS_ST_RUNNING) {
                for (uint32_t k = depth; k-- > 0u;) {
                    // the node edge k leaves: the root, or the child word of edge k - 1, which is tagged only further down
                    const uint32_t at = k ? uniform(pool[(uint64_t)path[k - 1u] * kEdgeWords + 2u]) : 0u;
                    const uint32_t first = uniform(node_tab[2u * at]), arms = uniform(node_tab[2u * at + 1u]);
                    const uint32_t mover = (rply + k) & 1u;
                    uint32_t flags = 0;
#pragma unroll
                    for (uint32_t j = 0; j < 2; ++j) {
                        const uint32_t a = tid + j * BGS_BLOCK;
                        if (a < arms) {
                            const uint32_t tag = bounce_edge_tag(pool[(uint64_t)(first + a) * kEdgeWords + 2u], mover);
                            flags |= tag == kTagWin ? 1u : (tag == kTagOpen ? 2u : (tag == kTagDraw ? 4u : 0u));
                        }
                    }
                    flags = (__builtin_amdgcn_ballot_w64((flags & 1u) != 0u) ? 1u : 0u) | (__builtin_amdgcn_ballot_w64((flags & 2u) != 0u) ? 2u : 0u) |
                            (__builtin_amdgcn_ballot_w64((flags & 4u) != 0u) ? 4u : 0u);
                    if (lane == 0) red_min[0][wave] = flags;
                    __syncthreads();        // (U)
                    uint32_t value = 0;
#pragma unroll
                    for (int w = 0; w < kSearchTeamWaves; ++w) value |= red_min[0][w];
                    value = uniform(value);
                    if (!(value & 1u) && (value & 2u)) break;      // the value is OPEN: nothing is known further up
                    if (k == 0u) {
                        decided = true;
                        break;
                    }
                    // the parent's edge takes the node's value as an absolute outcome: a won node is its mover's
                    const uint32_t outcome = (value & 1u) ? mover + 1u : ((value & 4u) ? (uint32_t)BGS_ST_DRAW : (1u - mover) + 1u);
                    if (tid == 0) pool[(uint64_t)path[k - 1u] * kEdgeWords + 2u] = kEdgeProved | outcome;
                    __syncthreads();        // (V)
                }
            }
        }
        __syncthreads();            // (C) the tree is whole again before the next descent reads it; tally and path are free
    }

    // ---- the outputs of the root (illegal slots are never stored: the launcher zeroed them)
    if (visits) {
        for (uint32_t a = tid; a < root_arms; a += BGS_BLOCK) {
            const uint32_t* const edge = pool + (uint64_t)a * kEdgeWords;
            visits[i * (int64_t)slots + slot_of(edge[3])] = (int32_t)edge[0];
        }
    }
    if constexpr (PROVE) {      // the root's tags in the solver's codes, by slot (every other slot stays BGS_SOLVE_NONE)
        if (extra.proved) {
            for (uint32_t a = tid; a < root_arms; a += BGS_BLOCK) {
                const uint32_t* const edge = pool + (uint64_t)a * kEdgeWords;
                const uint32_t tag = bounce_edge_tag(edge[2], root_mover);
                const int code = tag == kTagWin ? BGS_SOLVE_WIN : (tag == kTagDraw ? BGS_SOLVE_DRAW : (tag == kTagLoss ? BGS_SOLVE_LOSS : BGS_SOLVE_UNKNOWN));
                extra.proved[i * (int64_t)slots + slot_of(edge[3])] = (int8_t)code;
            }
        }
        if (tid == 0 && extra.done) extra.done[i] = (int32_t)ran;
    }
    if constexpr (FOREST) __syncthreads();   // the tree's last writes are issued by every wave before the header says what it holds
    if (tid == 0) {
        if (best) {   // the most visits, then the larger 2 * wins + draws, then the lower slot (the arms ascend by slot)
            int32_t top = -1;
            uint32_t top_n = 0, top_s = 0;
            // PROVE: a proved win is the move (at most one: the search stops at the first); otherwise the rule runs over the
            // arms not proved lost, or over all when all are
            [[maybe_unused]] int32_t won = -1;
            [[maybe_unused]] bool spare = false;
            if constexpr (PROVE) {
                for (uint32_t a = 0; a < root_arms; ++a) {
                    const uint32_t* const edge = pool + (uint64_t)a * kEdgeWords;
                    const uint32_t tag = bounce_edge_tag(edge[2], root_mover);
                    if (tag == kTagWin && won < 0) won = (int32_t)slot_of(edge[3]);
                    spare = spare || tag != kTagLoss;
                }
            }
            for (uint32_t a = 0; a < root_arms; ++a) {
                const uint32_t* const edge = pool + (uint64_t)a * kEdgeWords;
                const uint32_t cn = edge[0], cs = edge[1];
                if constexpr (PROVE) {
                    if (spare && bounce_edge_tag(edge[2], root_mover) == kTagLoss) continue;
                }
                if (cn > 0u && (top < 0 || cn > top_n || (cn == top_n && cs > top_s))) {
                    top = (int32_t)slot_of(edge[3]);
                    top_n = cn;
                    top_s = cs;
                }
            }
            if constexpr (PROVE) top = won >= 0 ? won : top;
            best[i] = top;
        }
        if constexpr (FOREST) {
            head[0] = made + 1u;    // the header: ply, cap and planes were recorded when the tree was emptied, or carried with it
            head[1] = used;
            if (extra.carried) extra.carried[i] = (int32_t)brought;
        }
        if (nodes) nodes[i] = (int32_t)made;
        if (used_out) used_out[i] = (int32_t)used;
    }
    add_steps(steps, stepped);
}

// what a search launch is given beyond the batch (bounce_search / bounce_forest_search fill it)
struct BounceSearchArgs {
    uint64_t seed;
    uint32_t iterations, leaf_playouts, explore, max_plies;
    uint32_t capacity, edges, restart;      // (the plain search reads neither capacity nor restart)
    int32_t *counts, *visits, *best, *nodes, *used;
    int32_t* carried;                       // (nor carried)
    void* trees;                            // the workspace, or the forest
    int8_t* proved = nullptr;               // the proving search alone: the root's tags and the iterations run
    int32_t* done = nullptr;
};

template <class GEO, int NC, int POLICY, bool FOREST, bool PROVE = false>
void launch_bounce_search(const bgs_batch* b, const GEO& g, const BounceSearchArgs& a) {
    const uint32_t slots = (uint32_t)(b->bg.w * b->bg.h * b->bg.w);
    (void)hipMemsetAsync(a.counts, 0, (size_t)b->n * slots * 3 * sizeof(int32_t), b->stream);
    if (a.visits) (void)hipMemsetAsync(a.visits, 0, (size_t)b->n * slots * sizeof(int32_t), b->stream);
    // game ids: ((first_game + i) * T + t) * P + j = first_game * T * P + (i * T + t) * P + j, mod 2^64
    const uint64_t game_base = b->first_game * (uint64_t)a.iterations * (uint64_t)a.leaf_playouts;
    const size_t tile = sizeof(uint32_t) * 2 * 8 * NC * BGS_BLOCK;
    BounceExtraArgs<FOREST, PROVE> extra;
    if constexpr (FOREST) extra = {a.capacity, a.restart, a.carried};
    if constexpr (PROVE) {      // every slot BGS_SOLVE_NONE; the kernel stores the legal ones
        static_assert((uint8_t)(int8_t)BGS_SOLVE_NONE == 0xFEu, "the fill byte is BGS_SOLVE_NONE");
        if (a.proved) (void)hipMemsetAsync(a.proved, 0xFE, (size_t)b->n * slots * sizeof(int8_t), b->stream);
        extra = {a.proved, a.done};
    }
    constexpr int64_t kMaxBlocks = (int64_t)1 << 30;
    for (int64_t i0 = 0; i0 < b->n; i0 += kMaxBlocks) {
        const int64_t blocks = b->n - i0 < kMaxBlocks ? b->n - i0 : kMaxBlocks;
        hipLaunchKernelGGL((k_bounce_search<GEO, NC, POLICY, FOREST, PROVE>), dim3((uint32_t)blocks), dim3(BGS_BLOCK), tile, b->stream, g,
                           (const uint64_t*)b->d_planes, (const uint8_t*)b->d_status, (const uint16_t*)b->d_plies, b->n, a.seed,
                           game_base, a.iterations, a.leaf_playouts, a.explore, a.max_plies, a.edges, slots, i0,
                           static_cast<uint32_t*>(a.trees), a.counts, a.visits, a.best, a.nodes, a.used, b->d_steps, extra);
    }
}

// The re-rooting (bgs_bounce_forest_advance): one wave a tree, in place, one launch.  Two arrays that refer to each other
// are compacted: the node table (first edge, arms) and the edge pool (whose third words are node indices).  Nodes are made
// in increasing index order and a node's edge block is allocated when it is made, so a child's index is above its parent's
// and the first-edge offsets ascend with the node index; a compaction that keeps the order keeps both properties:
//   mark     the subtree of r = the child word of the root's arm with the slot played, in a bit mask (LDS, a bit a node), by
//            an ascending sweep from r over chunks of 64 nodes: lane l walks the child words of node base + l if that node
//            is marked and has not been walked, and the chunk is swept again while some lane found its node newly marked
//            (a chain inside the chunk).  Marks only get set and a lane walks its node once, so a chunk takes at most 65
//            sweeps; a child index is above its parent's, so a mark never lands in a chunk that has been left.
//   number   new[v] = the marked nodes below v: a prefix popcount, one entry a mask word (LDS).
//   move     chunk by chunk in ascending order.  The table entries of the chunk's 64 nodes are read, then -- behind a
//            barrier -- written to new[v] <= v with the new first-edge offsets: a running sum of the kept nodes' arms,
//            carried from chunk to chunk (a scan inside the chunk).  The chunk's kept edges are one contiguous range of
//            destinations; it is moved in batches of 256 edges, each lane four: all reads of a batch, a barrier, all of its
//            writes, a barrier.  A destination never exceeds its source and sources ascend with destinations, so a batch
//            writes below everything that later batches read.  Child words are mapped to new[child]; 0 and the ended /
//            capped sentinels stay.
//   header   one lane, last, behind a barrier: the counts, the ply + 1, the move applied to the recorded planes.
// Chunks without a marked node are neither read nor written: the work is that of the nodes and edges in use.
// One wave, not a workgroup of four: the phases are separated by barriers (free in one wave), the sweep is serial along a
// chain of parents and children whatever the team, and a batch of boards brings a tree a CU's SIMD anyway; what a tree's
// move phase needs is loads in flight, which the four edges a lane give.
// Rubbish: every count, offset and index read from the forest is checked against the share's bounds before it is used as
// one, so memory that never held a tree is emptied or shuffled inside its own share, never indexed out of it.
constexpr uint32_t kAdvanceBatch = 4;      // edges a lane moves between two barriers

__global__ void __launch_bounds__(BGS_WAVE)
k_bounce_forest_advance(uint32_t height, uint32_t width, const int32_t* __restrict__ slot_in, uint32_t capacity, uint32_t edges,
                        uint32_t* forest, int32_t* __restrict__ kept, int64_t root_base) {
    extern __shared__ __attribute__((aligned(16))) uint32_t forest_lds[];
    const uint32_t lane = threadIdx.x;
    const uint32_t mask_room = (((capacity + 31u) >> 5) + 3u) & ~3u;
    uint32_t* const mask = forest_lds;              // bit v: node v stays
    uint32_t* const below = mask + mask_room;       // the marked nodes in the mask words before this one
    uint32_t* const cum = below + mask_room;        // [65] the kept edges of the chunk before node l (cum[64]: all of them)
    uint32_t* const from = cum + 68;                // [64] the old first edge of node l of the chunk
    uint32_t* const self = from + 64;               // [64] 1: node l of the chunk stays
    const int64_t i = root_base + (int64_t)blockIdx.x;
    uint32_t* const head = forest + (uint64_t)i * bounce_forest_tree_words(capacity, edges);
    uint32_t* const pool = head + kBounceForestHeaderWords;
    uint32_t* const node_tab = pool + (uint64_t)edges * kEdgeWords;
    const auto uniform = [](uint32_t x) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)x); };

    const int32_t slot = slot_in[i];
    uint32_t count = uniform(head[0]), used = uniform(head[1]);
    if (count > capacity || used > edges) count = used = 0u;        // a header out of range: none
    if (slot < 0) {                                 // untouched
        if (kept && lane == 0) kept[i] = (int32_t)(count ? count - 1u : 0u);
        return;
    }
    // a node's block, checked: (first, arms) with first + arms <= used, else no arms
    const auto block_of = [&](uint32_t v, uint32_t& first, uint32_t& arms) {
        const uint2 fa = *reinterpret_cast<const uint2*>(node_tab + 2u * (uint64_t)v);
        const bool fits = fa.x <= used && fa.y <= used - fa.x;
        first = fits ? fa.x : 0u;
        arms = fits ? fa.y : 0u;
    };

    // ---- the new root: the child of the root's arm whose move is that of the slot (source column, target cell)
    const uint32_t hw = height * width;
    uint32_t r = 0, played = 0;                     // 0: none (never expanded, ended, capped, did not fit, no such arm)
    if (count != 0u && (uint32_t)slot < width * hw) {
        const uint32_t x = (uint32_t)slot / hw, cell = (uint32_t)slot % hw;
        uint32_t first0, arms0;
        block_of(0u, first0, arms0);
        first0 = uniform(first0);
        arms0 = uniform(arms0);
        for (uint32_t a0 = 0; a0 < arms0 && r == 0u; a0 += BGS_WAVE) {
            const uint32_t a = a0 + lane;
            uint32_t child = 0, move = 0;
            bool hit = false;
            if (a < arms0) {
                const uint32_t* const edge = pool + (uint64_t)(first0 + a) * kEdgeWords;
                child = edge[2];
                move = edge[3];
                hit = (move & 255u) == cell && (move >> 8) < hw && (move >> 8) % width == x;
            }
            const uint64_t hits = __builtin_amdgcn_ballot_w64(hit);
            if (hits) {
                const int at = __builtin_ctzll(hits);
                const uint32_t ch = (uint32_t)__builtin_amdgcn_readlane((int)child, at);
                played = (uint32_t)__builtin_amdgcn_readlane((int)move, at);
                r = (ch > 0u && ch < count) ? ch : 0u;
                break;
            }
        }
    }
    r = uniform(r);
    if (r == 0u) {                                  // emptied: the next search starts anew from the batch's board
        if (lane == 0) {
            head[0] = 0;
            head[1] = 0;
            if (kept) kept[i] = 0;
        }
        return;
    }

    // ---- mark
    const uint32_t mask_words = (count + 31u) >> 5;
    for (uint32_t k = lane; k < mask_words; k += BGS_WAVE) mask[k] = 0;
    __syncthreads();
    if (lane == 0) mask[r >> 5] = 1u << (r & 31u);
    __syncthreads();
    for (uint32_t base = r & ~63u; base < count; base += 64u) {
        const uint32_t m0 = mask[base >> 5], m1 = (base >> 5) + 1u < mask_words ? mask[(base >> 5) + 1u] : 0u;
        if ((m0 | m1) == 0u) continue;              // (uniform) nothing of this chunk is in the subtree
        const uint32_t v = base + lane;
        bool done = false;
        for (;;) {
            const bool go = !done && v < count && ((mask[v >> 5] >> (v & 31u)) & 1u) != 0u;
            if (__builtin_amdgcn_ballot_w64(go) == 0) break;
            if (go) {
                uint32_t first, arms;
                block_of(v, first, arms);
                for (uint32_t a = 0; a < arms; ++a) {
                    const uint32_t ch = pool[(uint64_t)(first + a) * kEdgeWords + 2u];
                    if (ch > v && ch < count) atomicOr(mask + (ch >> 5), 1u << (ch & 31u));
                }
                done = true;
            }
            __syncthreads();
        }
    }
    __syncthreads();

    // ---- number
    uint32_t total = 0;
    for (uint32_t k0 = 0; k0 < mask_words; k0 += BGS_WAVE) {
        const uint32_t k = k0 + lane;
        const uint32_t bits = k < mask_words ? (uint32_t)__popc(mask[k]) : 0u;
        uint32_t upto = bits;                       // the inclusive scan of the wave
        for (int d = 1; d < BGS_WAVE; d <<= 1) {
            const uint32_t other = (uint32_t)__shfl_up((int)upto, d);
            upto += lane >= (uint32_t)d ? other : 0u;
        }
        if (k < mask_words) below[k] = total + upto - bits;
        total += (uint32_t)__shfl((int)upto, BGS_WAVE - 1);
    }
    __syncthreads();
    // the new index of a marked node
    const auto renumber = [&](uint32_t v) { return below[v >> 5] + (uint32_t)__popc(mask[v >> 5] & ((1u << (v & 31u)) - 1u)); };

    // ---- move
    uint32_t run = 0;                               // (uniform) the edges of the kept nodes before this chunk
    bool bad = false;
    for (uint32_t base = r & ~63u; base < count; base += 64u) {
        const uint32_t m0 = mask[base >> 5], m1 = (base >> 5) + 1u < mask_words ? mask[(base >> 5) + 1u] : 0u;
        if ((m0 | m1) == 0u) continue;
        const uint32_t v = base + lane;
        const bool stays = v < count && ((mask[v >> 5] >> (v & 31u)) & 1u) != 0u;
        uint32_t first = 0, arms = 0;
        if (stays) block_of(v, first, arms);
        uint32_t upto = arms;                       // the inclusive scan of the wave, saturating: rubbish cannot wrap it
        for (int d = 1; d < BGS_WAVE; d <<= 1) {
            const uint32_t other = (uint32_t)__shfl_up((int)upto, d);
            const uint32_t sum = upto + (lane >= (uint32_t)d ? other : 0u);          // (both below 2^31)
            upto = sum < 0x7FFFFFFFu ? sum : 0x7FFFFFFFu;
        }
        const uint32_t moved = (uint32_t)__shfl((int)upto, BGS_WAVE - 1);
        if ((uint64_t)run + moved > used) {         // (uniform; rubbish only: the blocks of a tree are disjoint) none
            bad = true;
            break;
        }
        cum[lane] = upto - arms;
        from[lane] = first;
        self[lane] = stays ? v : 0u;
        if (lane == 0) cum[64] = moved;
        __syncthreads();                            // every table entry of the chunk is read before one is written
        if (stays) *reinterpret_cast<uint2*>(node_tab + 2u * (uint64_t)renumber(v)) = make_uint2(run + upto - arms, arms);
        for (uint32_t k0 = 0; k0 < moved; k0 += kAdvanceBatch * BGS_WAVE) {
            uint4 e[kAdvanceBatch];
#pragma unroll
            for (uint32_t j = 0; j < kAdvanceBatch; ++j) {
                const uint32_t k = k0 + j * BGS_WAVE + lane;       // the k-th kept edge of the chunk
                e[j] = make_uint4(0u, 0u, 0u, 0u);
                if (k < moved) {
                    uint32_t l = 0;                 // its node: the last l with cum[l] <= k (so node l has arms)
#pragma unroll
                    for (uint32_t step = 32; step > 0; step >>= 1) l += cum[l + step] <= k ? step : 0u;
                    e[j] = *reinterpret_cast<const uint4*>(pool + (uint64_t)(from[l] + (k - cum[l])) * kEdgeWords);
                    const uint32_t ch = e[j].z, parent = self[l];
                    if (ch != 0u && ch < kEdgeEnded) {              // a node index: a kept node's children are kept
                        const bool marked = ch > parent && ch < count && ((mask[ch >> 5] >> (ch & 31u)) & 1u) != 0u;
                        e[j].z = marked ? renumber(ch) : 0u;
                    }
                }
            }
            __syncthreads();                        // every edge of the batch is read before one is written
#pragma unroll
            for (uint32_t j = 0; j < kAdvanceBatch; ++j) {
                const uint32_t k = k0 + j * BGS_WAVE + lane;
                const uint64_t to = (uint64_t)run + k;
                if (k < moved) *reinterpret_cast<uint4*>(pool + to * kEdgeWords) = e[j];     // (to < run + moved <= used <= E)
            }
            __syncthreads();
        }
        run += moved;
        __syncthreads();                            // cum, from and self are free for the next chunk
    }

    // ---- header (the tree's writes are issued; the counts and the move go last)
    __syncthreads();
    if (lane == 0) {
        if (bad) {
            head[0] = 0;
            head[1] = 0;
            if (kept) kept[i] = 0;
        } else {
            Board p;
            uint64_t* const head_planes = reinterpret_cast<uint64_t*>(head + 4);
#pragma unroll
            for (int j = 0; j < 4; ++j) p.v[j] = head_planes[j];
            move_piece(p, (int)((played >> 8) & 63u), (int)(played & 63u));
#pragma unroll
            for (int j = 0; j < 4; ++j) head_planes[j] = p.v[j];
            head[0] = total;
            head[1] = run;
            head[2] += 1u;
            if (kept) kept[i] = (int32_t)(total - 1u);
        }
    }
}

EvalGeom eval_geom(const bgs_batch* b) {
    EvalGeom g{};
    g.rh = b->cg.h;
    g.rw = b->cg.w;
    g.rk = b->cg.k;
    g.cells_total = (uint32_t)(g.h() * g.w());
    for (int x = 0; x < g.w(); ++x) {
        const int bit = x * (g.h() + 1);
        g.bottoms[bit >> 6] |= 1ull << (bit & 63);
        for (int y = 0; y < g.h(); ++y) g.cells[(bit + y) >> 6] |= 1ull << ((bit + y) & 63);
    }
    return g;
}

// ================================================================================================================
// Exact Connect solver (bgs_connect_solve_actions): for board i and column c, a depth-first alpha-beta search of the
// position after c, with a horizon of `depth` plies counted from board i (column c is ply 1).  Scores are seen from the
// side to move at a node and are absolute in the ply: a win that ends T plies after board i scores kSolveK - T for the
// winner and -(kSolveK - T) for the loser, a draw or a line the horizon cuts scores 0 -- so a plain negamax gives the
// fastest win and the slowest loss, and a window passes from parent to child by negation alone.
//
// Shape.  A task is one (board, column); one lane runs one task.  Persistent one-wave workgroups draw tasks from a
// device-wide counter: the wave's idle lanes take the next ones together (one atomic per refill), and a task that
// settles without a search (an ended board, a full column, an immediate win or draw, depth 1) frees its lane in the same
// refill pass.  The search is one uniform loop; in an iteration a lane may return from a child (pop), choose and play
// its next move (push), and evaluate the node it has just entered -- so most iterations visit one node a lane.
//
// Node evaluation, in this order: a full board or an exhausted horizon scores 0; a landing cell that completes k in a
// row for the mover is an immediate win; with one ply of horizon left nothing else can end inside it (0); two winning
// landing cells of the opponent lose in two plies; one is the only move searched (any other loses in two plies, and
// the block never scores below that); otherwise every legal column, centre first.
//
// Stack.  Moves are undone by XOR, so a level holds one 32-bit word in LDS, [level][lane] (no bank conflicts):
// bits 0-7 the cell played (or the forced block), 8-12 the next column index in centre-first order, 13 "forced",
// 16-31 alpha (int16).  Beta is not stored: a level's beta is minus its parent's alpha.
// ================================================================================================================
constexpr int kSolveK = 1024;             // |score| of a win or loss that ends T plies after the root: kSolveK - T
constexpr int kSolveWavesPerCU = 16;      // persistent waves a CU (fewer when the stack does not fit the LDS)
constexpr uint32_t kSolveLdsPerCU = 160u * 1024u;
enum : uint32_t { kSolveIdle = 0, kSolveEnter = 1, kSolveCont = 2, kSolveRet = 3 };

// the cells where a stone of `me` would complete k in a row (occupied cells and sentinels included: the caller masks).
// The sentinel row between columns is never a stone, so no run wraps from one column into the next.  k = 4: the runs
// before (B_m) and after (A_m) a cell are built once per direction and joined, A3 | A2 B1 | A1 B2 | B3; any other k
// tests every split of the k - 1 other stones.
template <int NW>
__device__ __forceinline__ Bits<NW> threats(const EvalGeom& g, const Bits<NW>& me) {
    const int dirs[3] = {g.h() + 1, g.h() + 2, g.h()};
    Bits<NW> t;
    if (g.k() == 4) {
        t = shl(me, 1);
        t = t & shl(me, 2);
        t = t & shl(me, 3);
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            Bits<NW> a1 = shr(me, dirs[d]), b1 = shl(me, dirs[d]);
            Bits<NW> a2 = a1, b2 = b1;
            a2 = a2 & shr(me, 2 * dirs[d]);
            b2 = b2 & shl(me, 2 * dirs[d]);
            Bits<NW> a3 = a2, b3 = b2;
            a3 = a3 & shr(me, 3 * dirs[d]);
            b3 = b3 & shl(me, 3 * dirs[d]);
            a2 = a2 & b1;
            a1 = a1 & b2;
            t = t | a3;
            t = t | b3;
            t = t | a2;
            t = t | a1;
        }
        return t;
    }
#pragma unroll
    for (int j = 0; j < NW; ++j) t.w[j] = ~0ull;
    for (int m = 1; m < g.k(); ++m) t = t & shl(me, m);   // vertical: the k - 1 cells below
    for (int d = 0; d < 3; ++d) {
        for (int split = 0; split < g.k(); ++split) {       // `split` stones after the cell, k - 1 - split before it
            Bits<NW> m;
#pragma unroll
            for (int j = 0; j < NW; ++j) m.w[j] = ~0ull;
            for (int i = 1; i <= split; ++i) m = m & shr(me, i * dirs[d]);
            for (int i = 1; i < g.k() - split; ++i) m = m & shl(me, i * dirs[d]);
            t = t | m;
        }
    }
    return t;
}

template <int NW>
__global__ void __launch_bounds__(BGS_WAVE)
k_connect_solve(EvalGeom g, const uint64_t* __restrict__ planes, const uint8_t* __restrict__ status, int64_t n, int32_t depth,
                uint64_t max_nodes, unsigned long long* __restrict__ queue, int8_t* __restrict__ codes, int16_t* __restrict__ plies_out,
                unsigned long long* __restrict__ nodes_out) {
    extern __shared__ uint32_t solve_stack[];   // [levels][64 lanes]
    uint32_t* const stk = solve_stack + threadIdx.x;
    const uint32_t lane = threadIdx.x;
    const uint64_t tasks = (uint64_t)n * (uint64_t)g.w();
    const uint32_t stride = (uint32_t)g.h() + 1u;
    const uint64_t colmask = (1ull << g.h()) - 1ull;
    const uint32_t half = (uint32_t)g.w() >> 1;

    Bits<NW> me, op;   // stones of the side to move at the current node, and of the other side
#pragma unroll
    for (int j = 0; j < NW; ++j) me.w[j] = op.w[j] = 0;
    uint32_t mode = kSolveIdle, empty = 0;
    int l = 0, val = 0;
    uint64_t task = 0, visited = 0, total = 0;
    bool dry = false;

    auto finish = [&](int code, int plies) {
        codes[task] = (int8_t)code;
        if (plies_out) plies_out[task] = (int16_t)plies;
        total += visited;
        mode = kSolveIdle;
    };

    for (;;) {
        // ---- refill: idle lanes take the next tasks; a task settled before any search frees its lane at once
        for (;;) {
            const uint64_t need = __builtin_amdgcn_ballot_w64(mode == kSolveIdle);
            if (!need || dry) break;
            const uint32_t wanted = (uint32_t)__popcll(need);
            unsigned long long base = 0;
            if (lane == 0) base = atomicAdd(queue, (unsigned long long)wanted);
            base = ((unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(base >> 32)) << 32) |
                   (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)base);
            if (base + wanted >= tasks) dry = true;
            const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(need >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)need, 0u));
            if (mode == kSolveIdle && base + rank < tasks) {
                task = base + rank;
                visited = 0;
                const int64_t i = (int64_t)(task / (uint32_t)g.w());
                const uint32_t col = (uint32_t)(task - (uint64_t)i * (uint32_t)g.w());
                Bits<NW> r0, r1;
#pragma unroll
                for (int j = 0; j < NW; ++j) {
                    r0.w[j] = planes[(int64_t)j * n + i];
                    r1.w[j] = planes[(int64_t)(NW + j) * n + i];
                }
                const uint32_t stones = popcount(r0) + popcount(r1);
                empty = g.cells_total - stones;
                const uint32_t mover = stones & 1u;
                const uint64_t cell = shr(landing_of(g, r0 | r1), (int)(col * stride)).w[0] & colmask;
                if (status[i] != BGS_ST_RUNNING || cell == 0ull) {
                    finish(BGS_SOLVE_NONE, 0);
                } else {
                    const uint32_t pos = col * stride + (uint32_t)(__ffsll((unsigned long long)cell) - 1);
                    me = mover ? r1 : r0;   // the root's mover, then the opponent moves at level 0
                    op = mover ? r0 : r1;
                    if (drop_and_test(g, me, pos, ~0u)) {
                        finish(BGS_SOLVE_WIN, 1);
                    } else if (empty == 1u) {
                        finish(BGS_SOLVE_DRAW, (int)empty);
                    } else if (depth == 1) {
                        finish(BGS_SOLVE_UNKNOWN, 0);
                    } else {
                        const Bits<NW> t = me;
                        me = op;
                        op = t;
                        l = 0;
                        mode = kSolveEnter;
                    }
                }
            }
        }
        if (!__builtin_amdgcn_ballot_w64(mode != kSolveIdle)) break;

        // ---- return from a child: undo the parent's move, raise its alpha, cut off at its beta
        if (mode == kSolveRet) {
            if (l == 0) {
                const int s = -val;
                if (s > 0) finish(BGS_SOLVE_WIN, kSolveK - s);
                else if (s < 0) finish(BGS_SOLVE_LOSS, kSolveK + s);
                else if (empty <= (uint32_t)depth) finish(BGS_SOLVE_DRAW, (int)empty);
                else finish(BGS_SOLVE_UNKNOWN, 0);
            } else {
                --l;
                const uint32_t word = stk[l * BGS_WAVE];
                const Bits<NW> t = me;
                me = op;
                op = t;
                flip(me, word & 255u);
                int alpha = (int)(int16_t)(word >> 16);
                const int beta = l == 0 ? kSolveK : -(int)(int16_t)(stk[(l - 1) * BGS_WAVE] >> 16);
                alpha = -val > alpha ? -val : alpha;
                if (alpha >= beta) {
                    val = alpha;
                } else {
                    stk[l * BGS_WAVE] = (word & 0xFFFFu) | ((uint32_t)alpha << 16);
                    mode = kSolveCont;
                }
            }
        }
        // ---- the node's next move: push it, or return alpha
        if (mode == kSolveCont) {
            const uint32_t word = stk[l * BGS_WAVE];
            uint32_t next = (word >> 8) & 31u, pos = 0;
            bool found = false;
            if (word & (1u << 13)) {
                found = next == 0u;
                pos = word & 255u;
                next = (uint32_t)g.w();
            } else {
                const Bits<NW> land = landing_of(g, me | op);
                for (; next < (uint32_t)g.w() && !found; ++next) {
                    const uint32_t col = (next & 1u) ? half - ((next + 1u) >> 1) : half + (next >> 1);
                    const uint64_t cell = shr(land, (int)(col * stride)).w[0] & colmask;
                    found = cell != 0ull;
                    pos = found ? col * stride + (uint32_t)(__ffsll((unsigned long long)cell) - 1) : pos;
                }
            }
            if (!found) {
                val = (int)(int16_t)(word >> 16);
                mode = kSolveRet;
            } else {
                stk[l * BGS_WAVE] = (word & 0xFFFF2000u) | (next << 8) | pos;
                flip(me, pos);
                const Bits<NW> t = me;
                me = op;
                op = t;
                ++l;
                mode = kSolveEnter;
            }
        }
        // ---- a node entered: settle it, or open its level
        if (mode == kSolveEnter) {
            ++visited;
            const Bits<NW> land = landing_of(g, me | op);
            const int r = depth - 1 - l;   // plies the horizon leaves from this node
            if (visited > max_nodes) {
                finish(BGS_SOLVE_BUDGET, 0);
            } else if (!any(land) || r <= 0) {
                val = 0;
                mode = kSolveRet;
            } else {
                Bits<NW> wins = threats(g, me);
                wins = wins & land;
                if (any(wins)) {
                    val = kSolveK - (l + 2);
                    mode = kSolveRet;
                } else if (r == 1) {
                    val = 0;
                    mode = kSolveRet;
                } else {
                    Bits<NW> lose = threats(g, op);
                    lose = lose & land;
                    const uint32_t cnt = popcount(lose);
                    if (cnt >= 2u) {
                        val = -(kSolveK - (l + 3));
                        mode = kSolveRet;
                    } else {
                        const int alpha = l <= 1 ? -kSolveK : (int)(int16_t)(stk[(l - 2) * BGS_WAVE] >> 16);
                        stk[l * BGS_WAVE] = (cnt ? lowest(lose) | (1u << 13) : 0u) | ((uint32_t)alpha << 16);
                        mode = kSolveCont;
                    }
                }
            }
        }
    }
    // ---- positions visited: one atomic per wave
    for (int off = 32; off >= 1; off >>= 1) total += __shfl_xor(total, off);
    if (lane == 0 && total) atomicAdd(nodes_out, (unsigned long long)total);
}

template <int NW>
void launch_solve(const bgs_batch* b, const EvalGeom& g, int32_t depth, int64_t max_nodes, int8_t* d_codes, int16_t* d_plies,
                  unsigned long long* d_nodes) {
    // No line is longer than the board has cells, so a deeper horizon cuts nothing: depth > cells is the same full solve
    // (and DRAW, empty <= depth, stays exact).  The clamp also bounds the stack.  Level l is opened only by a node with
    // r = depth - 1 - l >= 2 plies of horizon, so l <= depth - 3 = levels - 1.  Unclamped, a node of an empty root with
    // one empty cell left (level cells - 2) could open a level past the allocation.
    if (depth > (int32_t)g.cells_total) depth = (int32_t)g.cells_total;
    int64_t levels = depth - 2;
    if (levels < 1) levels = 1;
    const size_t lds = (size_t)levels * BGS_WAVE * sizeof(uint32_t);
    int64_t per_cu = (int64_t)(kSolveLdsPerCU / lds);
    if (per_cu > kSolveWavesPerCU) per_cu = kSolveWavesPerCU;
    if (per_cu < 1) per_cu = 1;
    const int64_t tasks = b->n * g.w();
    int64_t waves = (int64_t)b->num_cus * per_cu;
    if (waves > (tasks + BGS_WAVE - 1) / BGS_WAVE) waves = (tasks + BGS_WAVE - 1) / BGS_WAVE;
    unsigned long long* queue = reinterpret_cast<unsigned long long*>(b->d_work_count);   // (8-byte aligned: a region start)
    (void)hipMemsetAsync(queue, 0, sizeof(unsigned long long), b->stream);
    (void)hipMemsetAsync(d_nodes, 0, sizeof(unsigned long long), b->stream);
    hipLaunchKernelGGL((k_connect_solve<NW>), dim3((uint32_t)waves), dim3(BGS_WAVE), lds, b->stream, g, (const uint64_t*)b->d_planes,
                       (const uint8_t*)b->d_status, b->n, depth, (uint64_t)max_nodes, queue, d_codes, d_plies, d_nodes);
}


// ================================================================================================================
// Exact Bounce solver (bgs_bounce_solve_moves): for board i and every legal move m of its side to move, a depth-first
// alpha-beta search of the position after m with a horizon of `depth` plies counted from board i (m is ply 1).  Bounce
// games can cycle, so this is a horizon search and nothing else: there is no full solve.  Scores are the Connect
// solver's: seen from the side to move at a node and absolute in the ply -- a win that ends T plies after board i scores
// kSolveK - T for the winner and -(kSolveK - T) for the loser, a drawn end or a line the horizon cuts scores 0.
//
// Shape.  The counting pass of the evaluation (k_bounce_eval_count, here without the ply cap) numbers the LEGAL (board,
// move) pairs 0 .. ends[n-1] - 1 in (board, source, target) order; illegal slots keep the NONE the launcher filled in.
// Searches are split at the second ply: a task is one (board, move, reply).  Persistent one-wave workgroups draw moves
// from a device-wide counter in rounds (up to 64 a round, fewer when the batch would leave waves without work): a lane
// owns one move, settles it if the move itself ends the game or a reply lands in the opponent's goal row (a loss in
// two), else counts the opponent's replies; a prefix over the
// wave numbers the round's reply tasks, and the lanes take them from that list as they fall idle (the owner's position
// comes over by lane shuffles, the reply is found by its index).  Every reply is searched with a full window; the
// move's value is the least of its replies' values (LDS atomic min a reply, the budget hit as a sticky sentinel), the
// positions visited below a move are counted in LDS and checked against max_nodes, and the owner writes the entry when
// the round is done.
//
// Node evaluation, in this order: the moves of the side to move S are searched source by source; a target in S's goal
// row settles the node as a win in one (with a ply of horizon left); a node where S has no move at all is an ended game,
// won by the side that moved into it if that side can still move, else drawn -- also at the last ply of the horizon,
// where the search needs nothing but "has S a move" (any_move: the walk of reach(), left at the first target); with no
// horizon left the node scores 0; otherwise its level is opened.
//
// Stack.  A move relocates a 4-bit value and is undone by moving it back (a searched move never lands in a goal row, so
// its target was empty).  A level holds four 32-bit words in LDS, [level][word][lane] (the bank is the lane): words 0-1
// the targets of the current source still to search, word 2 alpha (int16) << 16 | current source cell << 6 | the target
// cell played, word 3 the sources still to search, as columns of the active row.  Sources behind a cut-off are never
// searched.  Beta is minus the parent's alpha.  The position after a reply is level 1, the first the stack holds; level l is
// opened only with depth - 1 - l >= 1 plies left: depth - 2 levels (depth - 1 are allocated).
// ================================================================================================================
constexpr uint32_t kBounceSolveWords = 4;
static_assert((BGS_BOUNCE_SOLVE_MAX_DEPTH - 1) * kBounceSolveWords * BGS_WAVE * sizeof(uint32_t) <= 64u * 1024u,
              "the deepest stack fits a workgroup's LDS");

// has `player` a legal move at all: reach()'s walk over every movable piece, left at the first landing cell
template <class GEO>
__device__ __forceinline__ bool any_move(const GEO& g, const Board& b, uint64_t occ, uint32_t player) {
    const uint64_t empty_interior = ~occ & g.interior;
    const uint64_t landing = empty_interior | (player ? g.goal_bottom : g.goal_top);
    const uint64_t bounce_on = occ & g.interior;
    const uint32_t up = player ? 0u : (uint32_t)g.w, down = player ? (uint32_t)g.w : 0u;
    uint64_t src = movable(g, occ, player);
    bool found = false;
    while (src && !found) {
        uint64_t pending = src & (0ull - src), done = 0;
        src &= src - 1;
        while (pending && !found) {
            const int c = __ffsll((unsigned long long)pending) - 1;
            pending &= pending - 1;
            done |= 1ull << c;
            const uint32_t v = value_at(b, c);
            uint64_t a0 = 1ull << c, al = 0, ar = 0, land = 0;
            for (uint32_t s = 1; s <= v; ++s) {
                const uint64_t via_left = a0 | al, via_right = a0 | ar;
                const uint64_t nf = ((via_left | ar) << up) >> down;
                const uint64_t nl = (via_left & g.not_col0) >> 1;
                const uint64_t nr = (via_right & g.not_collast) << 1;
                if (s < v) {
                    a0 = nf & empty_interior;
                    al = nl & empty_interior;
                    ar = nr & empty_interior;
                    if (!(a0 | al | ar)) break;
                } else {
                    land = nf | nl | nr;
                }
            }
            found = (land & landing) != 0ull;
            pending |= land & bounce_on & ~done;
        }
    }
    return found;
}

// the j-th move of `player` in canonical order (sources by ascending cell, targets by ascending cell); false: fewer moves
template <class GEO>
__device__ __forceinline__ bool nth_move(const GEO& g, const Board& b, uint64_t occ, uint32_t player, uint32_t j, int& s_cell, int& t_cell) {
    uint64_t src = movable(g, occ, player);
    bool found = false;
    while (src && !found) {
        const int s = __ffsll((unsigned long long)src) - 1;
        src &= src - 1;
        const uint64_t tm = reach(g, b, occ, player, s);
        const uint32_t cnt = (uint32_t)__popcll(tm);
        if (j < cnt) {
            s_cell = s;
            t_cell = (int)select_bit64(tm, j);
            found = true;
        } else {
            j -= cnt;
        }
    }
    return found;
}

__device__ __forceinline__ uint64_t shfl64(uint64_t v, uint32_t src_lane) {
    const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)v, (int)src_lane), hi = (uint32_t)__shfl((int)(uint32_t)(v >> 32), (int)src_lane);
    return ((uint64_t)hi << 32) | lo;
}

__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}

template <class GEO>
__global__ void __launch_bounds__(BGS_WAVE)
k_bounce_solve(GEO g, const uint64_t* __restrict__ planes, const uint16_t* __restrict__ plies_buf, int64_t n, int32_t depth,
               uint64_t max_nodes, uint32_t slots, const uint64_t* __restrict__ ends, unsigned long long* __restrict__ queue,
               int8_t* __restrict__ codes, int16_t* __restrict__ plies_out, unsigned long long* __restrict__ nodes_out) {
    extern __shared__ uint32_t bounce_solve_stack[];   // [levels][4 words][64 lanes]
    __shared__ uint32_t first_reply[BGS_WAVE];          // owner lane -> the first reply task of its move (exclusive prefix)
    __shared__ int best[BGS_WAVE];                      // owner lane -> the least value (for the root's mover) over its replies
    __shared__ unsigned long long seen[BGS_WAVE];       // owner lane -> positions visited below its move
    const uint32_t lane = threadIdx.x;
    uint32_t* const stk = bounce_solve_stack + lane;
    const uint64_t moves = ends[n - 1];
    const uint32_t hw = (uint32_t)(g.h * g.w);
    // moves a wave takes a round: all its lanes when the batch is large, fewer when that leaves waves without work
    uint64_t per = moves / gridDim.x;
    per = per < 1 ? 1 : (per > BGS_WAVE ? BGS_WAVE : per);
    const uint32_t group = (uint32_t)per;
    constexpr int kBudgetHit = -0x40000000;

    Board b, mb;   // the position of the current node; (owner) the position after the lane's move
#pragma unroll
    for (int j = 0; j < 4; ++j) b.v[j] = mb.v[j] = 0;
    uint32_t mode = kSolveIdle, root_p = 0, owner = 0, own_p = 0;
    int l = 0, val = 0;
    uint64_t where = 0, total = 0;
    auto word = [&](int level, uint32_t k) -> uint32_t& { return stk[((uint32_t)(level - 1) * kBounceSolveWords + k) * BGS_WAVE]; };
    auto settle = [&](int code, int plies) {
        codes[where] = (int8_t)code;
        if (plies_out) plies_out[where] = (int16_t)plies;
    };

    for (;;) {
        // ---- a round: the wave takes `group` moves, a lane a move (its owner)
        unsigned long long base = 0;
        if (lane == 0) base = atomicAdd(queue, (unsigned long long)group);
        base = ((unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(base >> 32)) << 32) |
               (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)base);
        if (base >= moves) break;
        uint32_t replies = 0;   // reply tasks of this lane's move (0: none, or the move settled the entry)
        if (lane < group && base + lane < moves) {
            const uint64_t seg = base + lane;
            int64_t lo = 0, hi = n - 1;   // the board: the first i with ends[i] > seg
            while (lo < hi) {
                const int64_t mid = (lo + hi) >> 1;
                if (ends[mid] > seg) hi = mid;
                else lo = mid + 1;
            }
            const int64_t i = lo;
            const uint32_t j = (uint32_t)(seg - (i ? ends[i - 1] : 0ull));   // the board's j-th legal move
            mb = load_board(planes, n, i);
            own_p = plies_buf[i] & 1u;
            uint64_t occ = occupancy(mb);
            int s_cell = 0, t_cell = 0;
            (void)nth_move(g, mb, occ, own_p, j, s_cell, t_cell);
            const uint32_t x = (uint32_t)s_cell - (uint32_t)(((uint32_t)s_cell * g.inv_w) >> 16) * (uint32_t)g.w;
            where = (uint64_t)i * slots + (uint64_t)x * hw + (uint32_t)t_cell;
            if ((1ull << t_cell) & (g.goal_top | g.goal_bottom)) {
                settle(BGS_SOLVE_WIN, 1);
            } else {
                move_piece(mb, s_cell, t_cell);
                occ = occupancy(mb);
                // the opponent's replies; one that lands in its goal row loses the move in two plies, nothing to search
                const uint64_t goal = own_p ? g.goal_top : g.goal_bottom;
                uint64_t src = movable(g, occ, 1u - own_p);
                bool lost = false;
                while (src) {
                    const int s = __ffsll((unsigned long long)src) - 1;
                    src &= src - 1;
                    const uint64_t tm = reach(g, mb, occ, 1u - own_p, s);
                    lost = lost || (tm & goal) != 0ull;
                    replies += (uint32_t)__popcll(tm);
                }
                if (replies == 0u) settle(any_move(g, mb, occ, own_p) ? BGS_SOLVE_WIN : BGS_SOLVE_DRAW, 1);
                else if (depth == 1 || lost) {
                    settle(lost && depth > 1 ? BGS_SOLVE_LOSS : BGS_SOLVE_UNKNOWN, lost && depth > 1 ? 2 : 0);
                    replies = 0;
                }
            }
        }
        // exclusive prefix of the reply counts over the wave
        uint32_t incl = replies;
        for (int off = 1; off < BGS_WAVE; off <<= 1) {
            const uint32_t up = (uint32_t)__shfl_up((int)incl, off);
            incl += lane >= (uint32_t)off ? up : 0u;
        }
        const uint32_t tasks = (uint32_t)__shfl((int)incl, BGS_WAVE - 1);
        first_reply[lane] = incl - replies;
        best[lane] = kSolveK;
        seen[lane] = replies ? 1ull : 0ull;   // the position after the move
        wave_lds_sync();

        // ---- the round's reply tasks, a lane a task, idle lanes refilled from the wave's own list
        uint32_t next = 0;
        for (;;) {
            for (;;) {
                const uint64_t need = __builtin_amdgcn_ballot_w64(mode == kSolveIdle);
                if (!need || next >= tasks) break;
                const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(need >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)need, 0u));
                const uint32_t t = next + rank;
                const bool take = mode == kSolveIdle && t < tasks;
                uint32_t o = 0;   // the owner: the last lane whose first reply is <= t (it has replies: the next lane starts behind t)
                if (take) {
                    uint32_t lo = 0, hi = BGS_WAVE - 1;
                    while (lo < hi) {
                        const uint32_t mid = (lo + hi + 1) >> 1;
                        if (first_reply[mid] <= t) lo = mid;
                        else hi = mid - 1;
                    }
                    o = lo;   // (a later lane starts behind t; an empty lane before the owner starts at or before the owner)
                }
                Board ob;
#pragma unroll
                for (int j = 0; j < 4; ++j) ob.v[j] = shfl64(mb.v[j], o);
                const uint32_t op = (uint32_t)__shfl((int)own_p, (int)o);
                if (take) {
                    owner = o;
                    root_p = op;
                    b = ob;
                    const uint32_t me = 1u - root_p;   // the replying side
                    int s_cell = 0, t_cell = 0;
                    (void)nth_move(g, b, occupancy(b), me, t - first_reply[o], s_cell, t_cell);
                    if ((1ull << t_cell) & (g.goal_top | g.goal_bottom)) {
                        atomicMin(&best[owner], -(kSolveK - 2));
                    } else {
                        move_piece(b, s_cell, t_cell);
                        l = 1;
                        mode = kSolveEnter;
                    }
                }
                const uint32_t wanted = (uint32_t)__popcll(need);
                next = tasks - next < wanted ? tasks : next + wanted;
            }
            if (!__builtin_amdgcn_ballot_w64(mode != kSolveIdle)) break;

            // ---- return from a child: take the parent's move back, raise its alpha, cut off at its beta
            if (mode == kSolveRet) {
                if (l == 1) {   // the position after the reply is valued for the root's mover
                    atomicMin(&best[owner], val);
                    mode = kSolveIdle;
                } else {
                    --l;
                    const uint32_t w2 = word(l, 2);
                    move_piece(b, (int)(w2 & 63u), (int)((w2 >> 6) & 63u));
                    int alpha = (int)(int16_t)(w2 >> 16);
                    const int beta = l == 1 ? kSolveK : -(int)(int16_t)(word(l - 1, 2) >> 16);
                    alpha = -val > alpha ? -val : alpha;
                    if (alpha >= beta) {
                        val = alpha;
                    } else {
                        word(l, 2) = (w2 & 0xFFFFu) | ((uint32_t)alpha << 16);
                        mode = kSolveCont;
                    }
                }
            }
            // ---- the node's next move: play it, or return alpha
            if (mode == kSolveCont) {
                const uint32_t w2 = word(l, 2);
                uint64_t t = ((uint64_t)word(l, 1) << 32) | word(l, 0);
                uint32_t cur = (w2 >> 6) & 63u;
                if (t == 0ull) {   // the next source that has a target (none of them is a goal cell: the node was entered)
                    uint32_t rem = word(l, 3);
                    const uint32_t row_base = (uint32_t)(((cur * g.inv_w) >> 16) * (uint32_t)g.w);
                    const uint32_t p = (root_p + 1u + (uint32_t)l) & 1u;
                    const uint64_t occ = occupancy(b);
                    while (rem && t == 0ull) {
                        cur = row_base + (uint32_t)(__ffs((int)rem) - 1);
                        rem &= rem - 1u;
                        t = reach(g, b, occ, p, (int)cur);
                    }
                    word(l, 3) = rem;
                }
                if (t == 0ull) {
                    val = (int)(int16_t)(w2 >> 16);
                    mode = kSolveRet;
                } else {
                    const uint32_t d = (uint32_t)(__ffsll((unsigned long long)t) - 1);
                    t &= t - 1;
                    word(l, 0) = (uint32_t)t;
                    word(l, 1) = (uint32_t)(t >> 32);
                    word(l, 2) = (w2 & 0xFFFF0000u) | (cur << 6) | d;
                    move_piece(b, (int)cur, (int)d);
                    ++l;
                    mode = kSolveEnter;
                }
            }
            // ---- a node entered: settle it, or open its level
            if (mode == kSolveEnter) {
                const unsigned long long visited = atomicAdd(&seen[owner], 1ull) + 1ull;
                if (visited > max_nodes) {
                    atomicMin(&best[owner], kBudgetHit);
                    mode = kSolveIdle;
                } else {
                    const int r = depth - 1 - l;   // plies the horizon leaves from this node
                    const uint32_t p = (root_p + 1u + (uint32_t)l) & 1u;
                    const uint64_t occ = occupancy(b);
                    bool any = false, win = false;
                    uint32_t first = 0;
                    uint64_t first_t = 0, behind = 0;
                    if (r <= 0) {
                        any = any_move(g, b, occ, p);
                    } else {
                        const uint64_t goal = p ? g.goal_bottom : g.goal_top;
                        uint64_t src = movable(g, occ, p);
                        while (src && !win) {
                            const int s = __ffsll((unsigned long long)src) - 1;
                            src &= src - 1;
                            const uint64_t tm = reach(g, b, occ, p, s);
                            win = (tm & goal) != 0ull;
                            if (tm && !any) {
                                any = true;
                                first = (uint32_t)s;
                                first_t = tm;
                                behind = src;
                            }
                        }
                    }
                    if (win) {
                        val = kSolveK - (l + 2);
                        mode = kSolveRet;
                    } else if (!any) {   // the move into this node ended the game
                        val = any_move(g, b, occ, 1u - p) ? -(kSolveK - (l + 1)) : 0;
                        mode = kSolveRet;
                    } else if (r <= 0) {
                        val = 0;
                        mode = kSolveRet;
                    } else {
                        const int alpha = l <= 2 ? -kSolveK : (int)(int16_t)(word(l - 2, 2) >> 16);
                        const uint32_t row_base = (uint32_t)(((first * g.inv_w) >> 16) * (uint32_t)g.w);
                        word(l, 0) = (uint32_t)first_t;
                        word(l, 1) = (uint32_t)(first_t >> 32);
                        word(l, 2) = ((uint32_t)alpha << 16) | (first << 6);
                        word(l, 3) = (uint32_t)(behind >> row_base);
                        mode = kSolveCont;
                    }
                }
            }
        }
        // ---- the round's moves: the least value over the replies is the move's value for the root's mover
        wave_lds_sync();
        if (replies) {
            const int s = best[lane];
            if (s <= kBudgetHit) settle(BGS_SOLVE_BUDGET, 0);
            else if (s > 0) settle(BGS_SOLVE_WIN, kSolveK - s);
            else if (s < 0) settle(BGS_SOLVE_LOSS, kSolveK + s);
            else settle(BGS_SOLVE_UNKNOWN, 0);
            total += seen[lane] - 1ull;   // (positions searched: the replies' trees)
        }
        wave_lds_sync();
    }
    // ---- positions visited: one atomic per wave
    for (int off = 32; off >= 1; off >>= 1) total += __shfl_xor(total, off);
    if (lane == 0 && total) atomicAdd(nodes_out, (unsigned long long)total);
}

template <class GEO>
void launch_bounce_solve(const bgs_batch* b, const GEO& g, int32_t depth, int64_t max_nodes, int8_t* d_codes, int16_t* d_plies,
                         unsigned long long* d_nodes, uint64_t* d_ends, uint64_t* d_totals) {
    const uint32_t slots = (uint32_t)(b->bg.w * b->bg.h * b->bg.w);
    const int64_t blocks = (b->n + BGS_BLOCK - 1) / BGS_BLOCK;
    hipLaunchKernelGGL((k_bounce_eval_count<GEO, false>), dim3((uint32_t)blocks), dim3(BGS_BLOCK), 0, b->stream, g,
                       (const uint64_t*)b->d_planes, (const uint8_t*)b->d_status, (const uint16_t*)b->d_plies, b->n, d_ends, d_totals);
    if (blocks > 1) {
        hipLaunchKernelGGL(k_bounce_eval_scan_totals, dim3(1), dim3(BGS_BLOCK), 0, b->stream, d_totals, blocks);
        hipLaunchKernelGGL(k_bounce_eval_add_totals, dim3((uint32_t)blocks), dim3(BGS_BLOCK), 0, b->stream, d_ends,
                           (const uint64_t*)d_totals, b->n);
    }
    // every slot starts as NONE / 0: the kernel writes the legal ones
    const size_t cells = (size_t)b->n * slots;
    (void)hipMemsetAsync(d_codes, (uint8_t)BGS_SOLVE_NONE, cells, b->stream);
    if (d_plies) (void)hipMemsetAsync(d_plies, 0, cells * sizeof(int16_t), b->stream);
    unsigned long long* queue = reinterpret_cast<unsigned long long*>(b->d_work_count);   // (8-byte aligned: a region start)
    (void)hipMemsetAsync(queue, 0, sizeof(unsigned long long), b->stream);
    (void)hipMemsetAsync(d_nodes, 0, sizeof(unsigned long long), b->stream);
    const int64_t levels = depth > 1 ? depth - 1 : 1;
    const size_t lds = (size_t)levels * kBounceSolveWords * BGS_WAVE * sizeof(uint32_t);
    int64_t per_cu = (int64_t)(kSolveLdsPerCU / (lds + 1024));   // (+ the round's static tables)
    if (per_cu > kSolveWavesPerCU) per_cu = kSolveWavesPerCU;
    int64_t waves = (int64_t)b->num_cus * per_cu;
    const int64_t most = ((int64_t)cells + BGS_WAVE - 1) / BGS_WAVE;   // (the legal moves are counted on the device)
    if (waves > most) waves = most;
    hipLaunchKernelGGL((k_bounce_solve<GEO>), dim3((uint32_t)waves), dim3(BGS_WAVE), lds, b->stream, g, (const uint64_t*)b->d_planes,
                       (const uint16_t*)b->d_plies, b->n, depth, (uint64_t)max_nodes, slots, (const uint64_t*)d_ends, queue, d_codes,
                       d_plies, d_nodes);
}

}  // namespace

void bounce_solve(const bgs_batch* b, int32_t depth, int64_t max_nodes, int8_t* d_codes, int16_t* d_plies, unsigned long long* d_nodes,
                  uint64_t* d_ends, uint64_t* d_totals) {
    if (b->bounce_static_geom && bounce_is_default(b->bg))
        launch_bounce_solve<DefaultBounceGeom>(b, DefaultBounceGeom{}, depth, max_nodes, d_codes, d_plies, d_nodes, d_ends, d_totals);
    else
        launch_bounce_solve<BounceGeom>(b, b->bg, depth, max_nodes, d_codes, d_plies, d_nodes, d_ends, d_totals);
}

void bounce_evaluate(const bgs_batch* b, uint64_t seed, int32_t playouts, int32_t max_plies, int32_t* d_counts, uint64_t* d_ends,
                     uint64_t* d_totals, int policy) {
    uint32_t cap = (uint32_t)max_plies;
    if (cap > kBounceMaxPlies) cap = kBounceMaxPlies;   // plies are stored as uint16
    const uint32_t p = (uint32_t)playouts;
    if (policy == BGS_POLICY_DECISIVE) {
        constexpr int D = BGS_POLICY_DECISIVE;
        if (b->bounce_static_geom && bounce_is_default(b->bg))
            launch_bounce_evaluate<DefaultBounceGeom, 1, D>(b, DefaultBounceGeom{}, seed, p, cap, d_counts, d_ends, d_totals);
        else if (b->bg.w <= 8)
            launch_bounce_evaluate<BounceGeom, 1, D>(b, b->bg, seed, p, cap, d_counts, d_ends, d_totals);
        else
            launch_bounce_evaluate<BounceGeom, 3, D>(b, b->bg, seed, p, cap, d_counts, d_ends, d_totals);
        return;
    }
    if (b->bounce_static_geom && bounce_is_default(b->bg))
        launch_bounce_evaluate<DefaultBounceGeom, 1>(b, DefaultBounceGeom{}, seed, p, cap, d_counts, d_ends, d_totals);
    else if (b->bg.w <= 8)
        launch_bounce_evaluate<BounceGeom, 1>(b, b->bg, seed, p, cap, d_counts, d_ends, d_totals);
    else
        launch_bounce_evaluate<BounceGeom, 3>(b, b->bg, seed, p, cap, d_counts, d_ends, d_totals);
}

template <int POLICY>
static void bounce_evaluate_halving_policy(const bgs_batch* b, uint64_t seed, uint32_t budget, uint32_t cap, int32_t* d_counts,
                                           int32_t* d_given, int32_t* d_best) {
    if (b->bounce_static_geom && bounce_is_default(b->bg))
        launch_bounce_evaluate_halving<DefaultBounceGeom, 1, POLICY>(b, DefaultBounceGeom{}, seed, budget, cap, d_counts, d_given, d_best);
    else if (b->bg.w <= 8)
        launch_bounce_evaluate_halving<BounceGeom, 1, POLICY>(b, b->bg, seed, budget, cap, d_counts, d_given, d_best);
    else
        launch_bounce_evaluate_halving<BounceGeom, 3, POLICY>(b, b->bg, seed, budget, cap, d_counts, d_given, d_best);
}

void bounce_evaluate_halving(const bgs_batch* b, uint64_t seed, int32_t budget, int32_t max_plies, int policy, int32_t* d_counts,
                             int32_t* d_given, int32_t* d_best) {
    uint32_t cap = (uint32_t)max_plies;
    if (cap > kBounceMaxPlies) cap = kBounceMaxPlies;   // plies are stored as uint16
    if (policy == BGS_POLICY_DECISIVE)
        bounce_evaluate_halving_policy<BGS_POLICY_DECISIVE>(b, seed, (uint32_t)budget, cap, d_counts, d_given, d_best);
    else
        bounce_evaluate_halving_policy<BGS_POLICY_UNIFORM>(b, seed, (uint32_t)budget, cap, d_counts, d_given, d_best);
}

uint64_t bounce_search_root_bytes(int32_t iterations, int32_t edges) {
    return bounce_search_root_words((uint32_t)iterations, (uint32_t)edges) * sizeof(uint32_t);
}

template <int POLICY, bool FOREST, bool PROVE>
static void bounce_search_policy(const bgs_batch* b, const BounceSearchArgs& a) {
    if (b->bounce_static_geom && bounce_is_default(b->bg))
        launch_bounce_search<DefaultBounceGeom, 1, POLICY, FOREST, PROVE>(b, DefaultBounceGeom{}, a);
    else if (b->bg.w <= 8)
        launch_bounce_search<BounceGeom, 1, POLICY, FOREST, PROVE>(b, b->bg, a);
    else
        launch_bounce_search<BounceGeom, 3, POLICY, FOREST, PROVE>(b, b->bg, a);
}

template <bool FOREST, bool PROVE = false>
static void bounce_search_any(const bgs_batch* b, int policy, BounceSearchArgs a) {
    if (a.max_plies > kBounceMaxPlies) a.max_plies = kBounceMaxPlies;   // plies are stored as uint16
    if (policy == BGS_POLICY_DECISIVE)
        bounce_search_policy<BGS_POLICY_DECISIVE, FOREST, PROVE>(b, a);
    else
        bounce_search_policy<BGS_POLICY_UNIFORM, FOREST, PROVE>(b, a);
}

void bounce_search(const bgs_batch* b, uint64_t seed, int32_t iterations, int32_t leaf_playouts, int32_t explore, int32_t max_plies,
                   int policy, int32_t edges, int32_t* d_counts, int32_t* d_visits, int32_t* d_best, int32_t* d_nodes, int32_t* d_used,
                   void* d_workspace) {
    bounce_search_any<false>(b, policy, {seed, (uint32_t)iterations, (uint32_t)leaf_playouts, (uint32_t)explore, (uint32_t)max_plies,
                                         (uint32_t)iterations + 1u, (uint32_t)edges, 1u, d_counts, d_visits, d_best, d_nodes, d_used,
                                         nullptr, d_workspace});
}

void bounce_search_proving(const bgs_batch* b, uint64_t seed, int32_t iterations, int32_t leaf_playouts, int32_t explore,
                           int32_t max_plies, int policy, int32_t edges, int32_t* d_counts, int32_t* d_visits, int32_t* d_best,
                           int32_t* d_nodes, int32_t* d_used, int8_t* d_proved, int32_t* d_done, void* d_workspace) {
    bounce_search_any<false, true>(b, policy, {seed, (uint32_t)iterations, (uint32_t)leaf_playouts, (uint32_t)explore,
                                               (uint32_t)max_plies, (uint32_t)iterations + 1u, (uint32_t)edges, 1u, d_counts, d_visits,
                                               d_best, d_nodes, d_used, nullptr, d_workspace, d_proved, d_done});
}

uint64_t bounce_forest_tree_bytes(int32_t capacity, int32_t edges) {
    return bounce_forest_tree_words((uint32_t)capacity, (uint32_t)edges) * sizeof(uint32_t);
}

void bounce_forest_search(const bgs_batch* b, uint64_t seed, int32_t iterations, int32_t leaf_playouts, int32_t explore,
                          int32_t max_plies, int policy, int32_t capacity, int32_t edges, int restart, int32_t* d_counts,
                          int32_t* d_visits, int32_t* d_best, int32_t* d_nodes, int32_t* d_used, int32_t* d_carried, void* d_forest) {
    bounce_search_any<true>(b, policy, {seed, (uint32_t)iterations, (uint32_t)leaf_playouts, (uint32_t)explore, (uint32_t)max_plies,
                                        (uint32_t)capacity, (uint32_t)edges, restart ? 1u : 0u, d_counts, d_visits, d_best, d_nodes,
                                        d_used, d_carried, d_forest});
}

void bounce_forest_advance(const bgs_batch* b, const int32_t* d_slots, int32_t capacity, int32_t edges, int32_t* d_kept, void* d_forest) {
    const uint32_t room = (uint32_t)capacity;
    // LDS: the mask and the prefix counts (a bit and a 32nd of a word a node, each rounded up to 16 bytes), the chunk's scan
    // (65 words, rounded), old offsets and node indices (64 words each)
    const uint32_t mask_room = (((room + 31u) >> 5) + 3u) & ~3u;
    const size_t lds = ((size_t)2 * mask_room + 68u + 64u + 64u) * sizeof(uint32_t);
    constexpr int64_t kMaxBlocks = (int64_t)1 << 30;
    for (int64_t i0 = 0; i0 < b->n; i0 += kMaxBlocks) {
        const int64_t blocks = b->n - i0 < kMaxBlocks ? b->n - i0 : kMaxBlocks;
        hipLaunchKernelGGL(k_bounce_forest_advance, dim3((uint32_t)blocks), dim3(BGS_WAVE), lds, b->stream, (uint32_t)b->bg.h,
                           (uint32_t)b->bg.w, d_slots, room, (uint32_t)edges, static_cast<uint32_t*>(d_forest), d_kept, i0);
    }
}

void connect_solve(const bgs_batch* b, int32_t depth, int64_t max_nodes, int8_t* d_codes, int16_t* d_plies,
                   unsigned long long* d_nodes) {
    const EvalGeom g = eval_geom(b);
    switch (b->cg.nw) {
        case 1: launch_solve<1>(b, g, depth, max_nodes, d_codes, d_plies, d_nodes); break;
        case 2: launch_solve<2>(b, g, depth, max_nodes, d_codes, d_plies, d_nodes); break;
        default: launch_solve<3>(b, g, depth, max_nodes, d_codes, d_plies, d_nodes); break;
    }
}

void connect_evaluate(const bgs_batch* b, uint64_t seed, int32_t playouts, int32_t max_plies, int32_t* d_counts, int policy) {
    const EvalGeom g = eval_geom(b);
    const uint32_t p = (uint32_t)playouts, cap = (uint32_t)max_plies;
    const bool per_ply = b->rng_per_ply != 0;
    if (policy == BGS_POLICY_DECISIVE) {
        constexpr int D = BGS_POLICY_DECISIVE;
        switch (b->cg.nw) {
            case 1: per_ply ? launch_evaluate<1, true, D>(b, g, seed, p, cap, d_counts) : launch_evaluate<1, false, D>(b, g, seed, p, cap, d_counts); break;
            case 2: per_ply ? launch_evaluate<2, true, D>(b, g, seed, p, cap, d_counts) : launch_evaluate<2, false, D>(b, g, seed, p, cap, d_counts); break;
            default: per_ply ? launch_evaluate<3, true, D>(b, g, seed, p, cap, d_counts) : launch_evaluate<3, false, D>(b, g, seed, p, cap, d_counts); break;
        }
        return;
    }
    switch (b->cg.nw) {
        case 1: per_ply ? launch_evaluate<1, true>(b, g, seed, p, cap, d_counts) : launch_evaluate<1, false>(b, g, seed, p, cap, d_counts); break;
        case 2: per_ply ? launch_evaluate<2, true>(b, g, seed, p, cap, d_counts) : launch_evaluate<2, false>(b, g, seed, p, cap, d_counts); break;
        default: per_ply ? launch_evaluate<3, true>(b, g, seed, p, cap, d_counts) : launch_evaluate<3, false>(b, g, seed, p, cap, d_counts); break;
    }
}

int32_t connect_halving_min_budget(int width) { return (int32_t)((uint32_t)width * halving_rounds((uint32_t)width)); }

template <int NW>
static void evaluate_halving_nw(const bgs_batch* b, const EvalGeom& g, uint64_t seed, uint32_t budget, uint32_t cap, int policy,
                                int32_t* d_counts, int32_t* d_given, int32_t* d_best) {
    constexpr int U = BGS_POLICY_UNIFORM, D = BGS_POLICY_DECISIVE;
    const bool per_ply = b->rng_per_ply != 0;
    if (policy == D) {
        per_ply ? launch_evaluate_halving<NW, true, D>(b, g, seed, budget, cap, d_counts, d_given, d_best)
                : launch_evaluate_halving<NW, false, D>(b, g, seed, budget, cap, d_counts, d_given, d_best);
    } else {
        per_ply ? launch_evaluate_halving<NW, true, U>(b, g, seed, budget, cap, d_counts, d_given, d_best)
                : launch_evaluate_halving<NW, false, U>(b, g, seed, budget, cap, d_counts, d_given, d_best);
    }
}

void connect_evaluate_halving(const bgs_batch* b, uint64_t seed, int32_t budget, int32_t max_plies, int policy, int32_t* d_counts,
                              int32_t* d_given, int32_t* d_best) {
    const EvalGeom g = eval_geom(b);
    const uint32_t p = (uint32_t)budget, cap = (uint32_t)max_plies;
    switch (b->cg.nw) {
        case 1: evaluate_halving_nw<1>(b, g, seed, p, cap, policy, d_counts, d_given, d_best); break;
        case 2: evaluate_halving_nw<2>(b, g, seed, p, cap, policy, d_counts, d_given, d_best); break;
        default: evaluate_halving_nw<3>(b, g, seed, p, cap, policy, d_counts, d_given, d_best); break;
    }
}

uint64_t connect_search_root_bytes(int width, int32_t iterations) {
    return search_root_words((uint32_t)width, (uint32_t)iterations) * sizeof(uint32_t);
}

template <int NW, bool FOREST, bool PROVE = false>
static void search_nw(const bgs_batch* b, const EvalGeom& g, int policy, const ConnectSearchArgs& a) {
    constexpr int U = BGS_POLICY_UNIFORM, D = BGS_POLICY_DECISIVE;
    const bool per_ply = b->rng_per_ply != 0;
    if (policy == D) {
        per_ply ? launch_search<NW, true, D, FOREST, PROVE>(b, g, a) : launch_search<NW, false, D, FOREST, PROVE>(b, g, a);
    } else {
        per_ply ? launch_search<NW, true, U, FOREST, PROVE>(b, g, a) : launch_search<NW, false, U, FOREST, PROVE>(b, g, a);
    }
}

template <bool FOREST, bool PROVE = false>
static void search_any(const bgs_batch* b, int policy, const ConnectSearchArgs& a) {
    const EvalGeom g = eval_geom(b);
    switch (b->cg.nw) {
        case 1: search_nw<1, FOREST, PROVE>(b, g, policy, a); break;
        case 2: search_nw<2, FOREST, PROVE>(b, g, policy, a); break;
        default: search_nw<3, FOREST, PROVE>(b, g, policy, a); break;
    }
}

void connect_search(const bgs_batch* b, uint64_t seed, int32_t iterations, int32_t leaf_playouts, int32_t explore, int32_t max_plies,
                    int policy, int32_t* d_counts, int32_t* d_visits, int32_t* d_best, int32_t* d_nodes, void* d_workspace) {
    search_any<false>(b, policy, {seed, (uint32_t)iterations, (uint32_t)leaf_playouts, (uint32_t)explore, (uint32_t)max_plies,
                                  (uint32_t)iterations + 1u, 1u, d_counts, d_visits, d_best, d_nodes, nullptr, d_workspace});
}

void connect_search_proving(const bgs_batch* b, uint64_t seed, int32_t iterations, int32_t leaf_playouts, int32_t explore,
                            int32_t max_plies, int policy, int32_t* d_counts, int32_t* d_visits, int32_t* d_best, int32_t* d_nodes,
                            int8_t* d_proved, int32_t* d_done, void* d_workspace) {
    search_any<false, true>(b, policy, {seed, (uint32_t)iterations, (uint32_t)leaf_playouts, (uint32_t)explore, (uint32_t)max_plies,
                                        (uint32_t)iterations + 1u, 1u, d_counts, d_visits, d_best, d_nodes, nullptr, d_workspace,
                                        d_proved, d_done});
}

uint64_t connect_forest_tree_bytes(int width, int32_t capacity) {
    return forest_tree_words((uint32_t)width, (uint32_t)capacity) * sizeof(uint32_t);
}

void connect_forest_search(const bgs_batch* b, uint64_t seed, int32_t iterations, int32_t leaf_playouts, int32_t explore,
                           int32_t max_plies, int policy, int32_t capacity, int restart, int32_t* d_counts, int32_t* d_visits,
                           int32_t* d_best, int32_t* d_nodes, int32_t* d_carried, void* d_forest) {
    search_any<true>(b, policy, {seed, (uint32_t)iterations, (uint32_t)leaf_playouts, (uint32_t)explore, (uint32_t)max_plies,
                                 (uint32_t)capacity, restart ? 1u : 0u, d_counts, d_visits, d_best, d_nodes, d_carried, d_forest});
}

void connect_forest_advance(const bgs_batch* b, const int32_t* d_columns, int32_t capacity, int32_t* d_kept, void* d_forest) {
    const uint32_t width = (uint32_t)b->cg.w, room = (uint32_t)capacity;
    // LDS: the mask and the prefix counts (a bit and a 32nd of a word a node, each rounded up to 16 bytes), a chunk of 64 nodes
    const uint32_t mask_room = (((room + 31u) >> 5) + 3u) & ~3u;
    const size_t lds = ((size_t)2 * mask_room + (size_t)64 * width * 3u) * sizeof(uint32_t);
    constexpr int64_t kMaxBlocks = (int64_t)1 << 30;
    for (int64_t i0 = 0; i0 < b->n; i0 += kMaxBlocks) {
        const int64_t blocks = b->n - i0 < kMaxBlocks ? b->n - i0 : kMaxBlocks;
        hipLaunchKernelGGL(k_connect_forest_advance, dim3((uint32_t)blocks), dim3(BGS_WAVE), lds, b->stream, (uint32_t)b->cg.h, width,
                           (uint32_t)b->cg.nw, d_columns, room, static_cast<uint32_t*>(d_forest), d_kept, i0);
    }
}

}  // namespace bgs
