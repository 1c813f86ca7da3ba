// evaluate_kernels.hip -- flat Monte-Carlo evaluation of every column of a batch of packed Connect boards
// (bgs_connect_evaluate_actions): for board i and column c, `playouts` games that start with column c on board i and
// continue by the uniform random policy, reduced on the device to (wins, draws, losses) of the player to move at board i.
//
// Game ids (include/bgs.h): playout p of column c of board i is global game
// G = ((first_game + i) * width + c) * playouts + p (mod 2^64), drawn under the batch's RNG contract at the board's absolute
// ply -- exactly an oracle rollout(seed, first_game * width * playouts) over the boards replicated W * P times, in
// (i, c, p) order, and stepped by their column.
//
// A unit of its own (bgs_kernel_unit_id(3)): the Connect unit and its id stay as they are.  The ply below restates, on
// the same board packing (connect_kernels.hip: two bit-planes, column-major, a sentinel bit on top of every column), what
// the Connect unit's `play_plies` / `select_landing` / `select_bit64` (one-word boards), `four_in_a_row_at` and
// `has_run` / `drop_stone` (any board) do.
//
// Shape.  A wave owns either several whole (board, column) segments -- P <= games per wave -- or one slice of one segment.
// Its lanes take the chunk's playouts in order (the refill loop of K2a: lanes take new games at 4-ply block boundaries,
// the block itself is straight-line code masked by `live`), so the lanes of a wave sit on the same segment wherever P
// allows, and a lane keeps the board after the segment's first move in registers for all the playouts of the segment it
// takes.  W/D/L are counted in registers, flushed to the wave's LDS tally when the lane moves to the next segment, and
// the wave writes its segments once at the end (sliced segments: one integer atomic per wave and counter into counts the
// launcher zeroed).
#include "bgs_common.h"
#include "bgs_internal.h"

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
    int h, w, k;
    uint32_t cells_total;          // h * w: a board with this many stones is full
    uint64_t bottoms[BGS_CONNECT_MAX_WORDS];   // the bottom cell of every column
    uint64_t cells[BGS_CONNECT_MAX_WORDS];     // every real cell (no sentinels)
};

template <int NW>
struct Planes {
    uint64_t w[NW];
};

template <int NW>
__device__ __forceinline__ Planes<NW> por(const Planes<NW>& a, const Planes<NW>& b) {
    Planes<NW> r;
#pragma unroll
    for (int j = 0; j < NW; ++j) r.w[j] = a.w[j] | b.w[j];
    return r;
}

// 64 bits of `a` starting at bit `s` (>= 0; bits beyond the plane read as 0) -- the Connect unit's word_at / shr
template <int NW>
__device__ __forceinline__ uint64_t bits_at(const Planes<NW>& a, int s) {
    const int q = s >> 6, r = s & 63;
    uint64_t lo = 0, hi = 0;
#pragma unroll
    for (int j = 0; j < NW; ++j) {
        lo = (j == q) ? a.w[j] : lo;
        hi = (j == q + 1) ? a.w[j] : hi;
    }
    return r ? (lo >> r) | (hi << (64 - r)) : lo;
}

template <int NW>
__device__ __forceinline__ Planes<NW> shr(const Planes<NW>& a, int s) {
    Planes<NW> r;
#pragma unroll
    for (int j = 0; j < NW; ++j) r.w[j] = bits_at(a, 64 * j + s);
    return r;
}

// k stones in a row anywhere on the plane (the Connect unit's has_run): shift-and-AND with run doubling over the four
// directions vertical 1, horizontal H+1, rising H+2, falling H
template <int NW>
__device__ __forceinline__ bool has_run(const EvalGeom& g, const Planes<NW>& b) {
    const int dirs[4] = {1, g.h + 1, g.h + 2, g.h};
    uint64_t hit = 0;
#pragma unroll
    for (int d = 0; d < 4; ++d) {
        Planes<NW> m = b;
        int len = 1;
        while (2 * len <= g.k) {
            const Planes<NW> s = shr(m, len * dirs[d]);
#pragma unroll
            for (int j = 0; j < NW; ++j) m.w[j] &= s.w[j];
            len *= 2;
        }
        if (len < g.k) {
            const Planes<NW> s = shr(m, (g.k - len) * dirs[d]);
#pragma unroll
            for (int j = 0; j < NW; ++j) m.w[j] &= s.w[j];
        }
#pragma unroll
        for (int j = 0; j < NW; ++j) hit |= m.w[j];
    }
    return hit != 0;
}

// (a & b) | c in one VALU instruction (v_bitop3_b32, truth table 0xEA)
__device__ __forceinline__ uint32_t and_or(uint32_t a, uint32_t b, uint32_t c) {
    uint32_t r;
    asm("v_bitop3_b32 %0, %1, %2, %3 bitop3:0xea" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}

// four in a row through the stone just dropped on `pos` of a one-word plane (the Connect unit's four_in_a_row_at): the
// vertical run is the four cells ending at pos, the three other directions are tested on the whole plane
__device__ __forceinline__ bool four_in_a_row_at(uint64_t b, int h, uint32_t pos) {
    const int dirs[3] = {h + 1, h + 2, h};
    uint32_t acc_lo = 0, acc_hi = 0;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        const uint64_t s1 = b >> dirs[d];
        const uint32_t pl = (uint32_t)b & (uint32_t)s1, ph = (uint32_t)(b >> 32) & (uint32_t)(s1 >> 32);
        const uint64_t pairs = ((uint64_t)ph << 32) | pl;
        uint64_t s2;
        asm("v_lshrrev_b64 %0, %1, %2" : "=v"(s2) : "s"(2 * dirs[d]), "v"(pairs));
        if (d == 0) {
            acc_lo = pl & (uint32_t)s2;
            acc_hi = ph & (uint32_t)(s2 >> 32);
        } else {
            acc_lo = and_or(pl, (uint32_t)s2, acc_lo);
            acc_hi = and_or(ph, (uint32_t)(s2 >> 32), acc_hi);
        }
    }
    uint32_t column = (uint32_t)(b >> ((pos - 3u) & 63u));
    asm("" : "+v"(column));
    return ((acc_lo | acc_hi) != 0u) | ((column & 15u) == 15u);
}

// position of the k-th set bit of m (k < popcount(m)): the Connect unit's select_bit64
__device__ __forceinline__ uint32_t select_bit64(uint64_t m, uint32_t k) {
    const uint32_t lo = (uint32_t)m, hi = (uint32_t)(m >> 32);
    const uint32_t below = (uint32_t)__popc(lo);
    const bool upper = k >= below;
    uint32_t word = upper ? hi : lo, pos = upper ? 32u : 0u;
    k -= upper ? below : 0u;
#pragma unroll
    for (uint32_t half = 16u; half >= 1u; half >>= 1) {
        const uint32_t cnt = (uint32_t)__popc(word & ((1u << half) - 1u));
        const bool up = k >= cnt;
        word = up ? word >> half : word;
        pos += up ? half : 0u;
        k -= up ? cnt : 0u;
    }
    return pos;
}

// the idx-th set bit of a one-word `landing` (at most one bit per column field, never a field's top bit) by arithmetic
// on the fields: the Connect unit's select_landing.  Needs w <= 2^h.
__device__ __forceinline__ uint32_t select_landing(uint64_t landing, uint64_t bottoms, uint64_t tops, uint32_t stride, uint32_t idx) {
    const uint64_t flags = ((landing + (tops - bottoms)) & tops) >> (stride - 1u);
    const uint64_t cmp = ((uint64_t)idx - flags) * bottoms + tops;
    const uint32_t col = (uint32_t)__popcll(cmp & tops);
    const uint64_t low = (1ull << stride) - 1ull;
    return (uint32_t)__ffsll((unsigned long long)(landing & (low << (col * stride)))) - 1u;
}

// the cells the next stone of every open column would take: (stones + column bottoms) carries through each column's
// stones and stops under its sentinel; a carry may cross a word boundary with the column
template <int NW>
__device__ __forceinline__ Planes<NW> landing_of(const EvalGeom& g, const Planes<NW>& occ) {
    Planes<NW> r;
    uint64_t carry = 0;
#pragma unroll
    for (int j = 0; j < NW; ++j) {
        const uint64_t s = occ.w[j] + g.bottoms[j];
        const uint64_t t = s + carry;
        carry = (uint64_t)(s < occ.w[j]) + (uint64_t)(t < s);
        r.w[j] = t & g.cells[j];
    }
    return r;
}

// the mover of this ply drops a stone on `pos` (act = all ones) or nothing (act = 0); returns "the mover has won"
template <int NW>
__device__ __forceinline__ bool drop_and_test(const EvalGeom& g, Planes<NW>& mine, uint32_t pos, uint32_t act) {
    if (NW == 1) {
        const uint64_t bit = 1ull << (pos & 63u);
        mine.w[0] = ((uint64_t)and_or((uint32_t)(bit >> 32), act, (uint32_t)(mine.w[0] >> 32)) << 32) |
                    and_or((uint32_t)bit, act, (uint32_t)mine.w[0]);
        const bool won = g.k == 4 ? four_in_a_row_at(mine.w[0], g.h, pos) : has_run(g, mine);
        return won && act;
    }
#pragma unroll
    for (int j = 0; j < NW; ++j) mine.w[j] |= ((uint32_t)j == (pos >> 6) && act) ? 1ull << (pos & 63u) : 0ull;
    return act && has_run(g, mine);
}

// one uniformly drawn ply on the board (p0, p1) by the side `mover`: the position of the stone it drops
template <int NW>
__device__ __forceinline__ uint32_t draw_position(const EvalGeom& g, const Planes<NW>& occ, uint32_t draw) {
    const Planes<NW> landing = landing_of(g, occ);
    if (NW == 1) {
        const uint32_t idx = sample_index(draw, (uint32_t)__popcll(landing.w[0]));
        const bool by_fields = g.h <= 15 && (uint32_t)g.w <= (1u << g.h);   // (uniform)
        return by_fields ? select_landing(landing.w[0], g.bottoms[0], g.bottoms[0] << g.h, (uint32_t)g.h + 1u, idx)
                         : select_bit64(landing.w[0], idx);
    }
    uint32_t cnt = 0;
#pragma unroll
    for (int j = 0; j < NW; ++j) cnt += (uint32_t)__popcll(landing.w[j]);
    uint32_t idx = sample_index(draw, cnt), pos = 0;
    bool found = false;
#pragma unroll
    for (int j = 0; j < NW; ++j) {
        const uint32_t c = (uint32_t)__popcll(landing.w[j]);
        const bool here = !found && idx < c;
        pos = here ? 64u * j + select_bit64(landing.w[j], idx) : pos;
        idx -= (!found && !here) ? c : 0u;
        found = found || here;
    }
    return pos;
}

template <int NW, bool PER_PLY>
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
    const int64_t segments = n * g.w;
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

    const uint32_t stride = (uint32_t)g.h + 1u;
    Planes<NW> p[2];                 // the lane's game: stones of player 0 / player 1
    Planes<NW> c0, c1;               // the board after the current segment's first move
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
                    const int64_t i = seg / g.w;
                    const int col = (int)(seg - i * g.w);
                    Planes<NW> r0, r1;
#pragma unroll
                    for (int j = 0; j < NW; ++j) {
                        r0.w[j] = planes[(int64_t)j * n + i];
                        r1.w[j] = planes[(int64_t)(NW + j) * n + i];
                    }
                    uint32_t rply = 0;
#pragma unroll
                    for (int j = 0; j < NW; ++j) rply += (uint32_t)__popcll(r0.w[j]) + (uint32_t)__popcll(r1.w[j]);
                    root_mover = rply & 1u;
                    const uint32_t height = (uint32_t)__popcll(bits_at(por(r0, r1), col * (int)stride) & ((1ull << g.h) - 1ull));
                    child = kIllegal;
                    if (status[i] == BGS_ST_RUNNING && height < (uint32_t)g.h) {
                        Planes<NW>& mine = root_mover ? r1 : r0;
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
            const uint32_t pos = draw_position(g, por(p[0], p[1]), draw);
            const bool won = drop_and_test(g, p[j & 1u], pos, act);
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

template <int NW, bool PER_PLY>
void launch_evaluate(const bgs_batch* b, const EvalGeom& g, uint64_t seed, uint32_t playouts, uint32_t max_plies,
                     int32_t* d_counts) {
    const int64_t segments = b->n * g.w;
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
    const uint64_t game_base = b->first_game * (uint64_t)g.w * (uint64_t)playouts;
    constexpr int64_t kMaxBlocks = (int64_t)1 << 30;
    for (int64_t w0 = 0; w0 < waves; w0 += kMaxBlocks * kEvalWavesPerBlock) {
        int64_t blocks = (waves - w0 + kEvalWavesPerBlock - 1) / kEvalWavesPerBlock;
        if (blocks > kMaxBlocks) blocks = kMaxBlocks;
        hipLaunchKernelGGL((k_connect_evaluate<NW, PER_PLY>), dim3((uint32_t)blocks), dim3(BGS_BLOCK), 0, b->stream, g,
                           (const uint64_t*)b->d_planes, (const uint8_t*)b->d_status, b->n, seed, game_base, playouts, max_plies,
                           segs_per_wave, slices, slice_len, w0, waves, d_counts, b->d_steps);
    }
}

}  // namespace

void connect_evaluate(const bgs_batch* b, uint64_t seed, int32_t playouts, int32_t max_plies, int32_t* d_counts) {
    EvalGeom g{};
    g.h = b->cg.h;
    g.w = b->cg.w;
    g.k = b->cg.k;
    g.cells_total = (uint32_t)(g.h * g.w);
    for (int x = 0; x < g.w; ++x) {
        const int bit = x * (g.h + 1);
        g.bottoms[bit >> 6] |= 1ull << (bit & 63);
        for (int y = 0; y < g.h; ++y) g.cells[(bit + y) >> 6] |= 1ull << ((bit + y) & 63);
    }
    const uint32_t p = (uint32_t)playouts, cap = (uint32_t)max_plies;
    const bool per_ply = b->rng_per_ply != 0;
    switch (b->cg.nw) {
        case 1: per_ply ? launch_evaluate<1, true>(b, g, seed, p, cap, d_counts) : launch_evaluate<1, false>(b, g, seed, p, cap, d_counts); break;
        case 2: per_ply ? launch_evaluate<2, true>(b, g, seed, p, cap, d_counts) : launch_evaluate<2, false>(b, g, seed, p, cap, d_counts); break;
        default: per_ply ? launch_evaluate<3, true>(b, g, seed, p, cap, d_counts) : launch_evaluate<3, false>(b, g, seed, p, cap, d_counts); break;
    }
}

}  // namespace bgs
