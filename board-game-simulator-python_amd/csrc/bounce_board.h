// bounce_board.h -- the packed Bounce board and its move search, shared by the Bounce unit (bounce_kernels.hip) and the
// evaluation unit (evaluate_kernels.hip).  The Makefile hashes this header into the ids of both units.
//
// Board packing.  height * width <= 64 cells, cell index c = y * width + x (y = 0 bottom row).  Piece values (1..15) are
// bit-sliced into four uint64 planes: plane j holds bit j of every cell's value; occupancy is the OR of the planes.
//
// GEO is the run-time BounceGeom or the compile-time DefaultBounceGeom (bounce_unit.h).
#pragma once

#include "bgs_common.h"

namespace bgs {
namespace {

struct Board {
    uint64_t v[4];
};

__device__ __forceinline__ uint64_t occupancy(const Board& b) { return b.v[0] | b.v[1] | b.v[2] | b.v[3]; }

__device__ __forceinline__ uint32_t value_at(const Board& b, int c) {
    return (uint32_t)((b.v[0] >> c) & 1ull) | ((uint32_t)((b.v[1] >> c) & 1ull) << 1) |
           ((uint32_t)((b.v[2] >> c) & 1ull) << 2) | ((uint32_t)((b.v[3] >> c) & 1ull) << 3);
}

// every legal landing cell of the piece on cell `src` for `player` (SURVEY Appendix B rules 4-5).  Every queued cell is
// walked once: a segment of value(cell) steps.  Walkers only ever stand on interior cells (the start piece, empty interior
// cells), so a forward step never leaves the board and needs no mask; forward is "<< w" for player 0 and ">> w" for
// player 1, written as two shifts (up, down) one of which is by 0, so there is no per-lane select in the step.
// The walk is written out here and in enumerate_flat: as a function of its own, inlined, it changes the instructions of
// every Bounce kernel that searches moves.
template <class GEO>
__device__ __forceinline__ uint64_t reach(const GEO& g, const Board& b, uint64_t occ, uint32_t player, int src) {
    const uint64_t empty_interior = ~occ & g.interior;
    const uint64_t landing = empty_interior | (player ? g.goal_bottom : g.goal_top);
    const uint64_t bounce_on = occ & g.interior;
    const uint32_t up = player ? 0u : (uint32_t)g.w, down = player ? (uint32_t)g.w : 0u;
    uint64_t pending = 1ull << src, done = 0, targets = 0;
    while (pending) {
        const int c = __ffsll((unsigned long long)pending) - 1;
        pending &= pending - 1;
        done |= 1ull << c;
        const uint32_t v = value_at(b, c);
        uint64_t a0 = 1ull << c, al = 0, ar = 0, land = 0;
        for (uint32_t s = 1; s <= v; ++s) {
            const uint64_t via_left = a0 | al, via_right = a0 | ar;  // who may go on left / right (no reversal)
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
        targets |= land & landing;
        pending |= land & bounce_on & ~done;
    }
    return targets;
}

// pieces the side to move may pick: those in the occupied non-goal row nearest its own side (Appendix B rule 3)
template <class GEO>
__device__ __forceinline__ uint64_t movable(const GEO& g, uint64_t occ, uint32_t player) {
    const uint64_t oi = occ & g.interior;
    if (!oi) return 0;
    const int cell = player ? 63 - __clzll((long long)oi) : __ffsll((unsigned long long)oi) - 1;
    const int row = (int)(((uint32_t)cell * g.inv_w) >> 16);
    return oi & (((1ull << g.w) - 1ull) << (row * g.w));
}

__device__ __forceinline__ void move_piece(Board& b, int src_cell, int dst_cell) {
    const uint32_t v = value_at(b, src_cell);
    const uint64_t keep = ~(1ull << src_cell);
#pragma unroll
    for (int j = 0; j < 4; ++j) b.v[j] = (b.v[j] & keep) | ((uint64_t)((v >> j) & 1u) << dst_cell);
}

__device__ __forceinline__ Board load_board(const uint64_t* __restrict__ planes, int64_t n, int64_t i) {
    Board b;
#pragma unroll
    for (int j = 0; j < 4; ++j) b.v[j] = planes[(int64_t)j * n + i];
    return b;
}

__device__ __forceinline__ void store_board(uint64_t* __restrict__ planes, int64_t n, int64_t i, const Board& b) {
#pragma unroll
    for (int j = 0; j < 4; ++j) planes[(int64_t)j * n + i] = b.v[j];
}

// ------------------------------------------------------------------------------------------------
// The flat move list (K3f, and the Bounce evaluation): the move search of a ply is not run as nested loops (for every
// column: while cells are pending: for every step), whose trip counts differ from lane to lane so that a wave executes
// the SUM over columns of the per-column maxima.  It is ONE loop per wave in which every lane expands one cell of its own
// work queue per iteration -- the queue runs through the lane's sources one after the other and through each source's
// pending bounce cells -- so a wave executes the maximum over its lanes of the number of cells.
// Per-source target masks go to a per-lane dword column of LDS ([dword][lane]: the bank is the lane, dynamic indices
// never conflict); per-source counts are packed 8 bits each (a source has at most 64 targets: 0..64 needs 7 bits).
// NC words of counts: boards up to 8 * NC columns.
// ------------------------------------------------------------------------------------------------
template <int NC>
struct FlatMoves {
    uint64_t counts[NC];   // byte x = number of targets of the piece in column x of the active row
    uint32_t n;            // number of actions
    uint32_t row_base;     // cell index of column 0 of the active row
};

// the action list of `player` for the lanes with `want` set; the other lanes idle through the loop.  KEEP_IDLE: those
// lanes keep the list they hold (the evaluation plays from it); otherwise every lane's list is reset
template <int NC, bool KEEP_IDLE, class GEO>
__device__ __forceinline__ void enumerate_flat(const GEO& g, const Board& b, uint64_t occ, uint32_t player, bool want,
                                               uint32_t* column, FlatMoves<NC>& m) {
    const uint64_t empty_interior = ~occ & g.interior;
    const uint64_t landing = empty_interior | (player ? g.goal_bottom : g.goal_top);
    const uint64_t bounce_on = occ & g.interior;
    const uint32_t up = player ? 0u : (uint32_t)g.w, down = player ? (uint32_t)g.w : 0u;
    uint64_t rem = want ? movable(g, occ, player) : 0ull;   // sources still to search
    if (!KEEP_IDLE || want) {
        const int first = rem ? __ffsll((unsigned long long)rem) - 1 : 0;
        m.row_base = (uint32_t)((int)(((uint32_t)first * g.inv_w) >> 16) * g.w);
#pragma unroll
        for (int k = 0; k < NC; ++k) m.counts[k] = 0;
        m.n = 0;
    }
    uint64_t pending = 0, done = 0, targets = 0;
    uint32_t x = 0;
    bool open_source = false;  // a source is being searched and has not been booked yet
    while (__builtin_amdgcn_ballot_w64(rem != 0 || pending != 0 || open_source)) {
        if (pending == 0) {
            if (open_source) {  // the source's closure is complete: book it
                const uint32_t cnt = (uint32_t)__popcll(targets);
                if (NC == 1) {
                    m.counts[0] |= (uint64_t)cnt << (8u * x);
                } else {
#pragma unroll
                    for (int k = 0; k < NC; ++k) m.counts[k] |= (x >> 3) == (uint32_t)k ? (uint64_t)cnt << (8u * (x & 7u)) : 0ull;
                }
                m.n += cnt;
                column[(2u * x) * BGS_BLOCK] = (uint32_t)targets;
                column[(2u * x + 1u) * BGS_BLOCK] = (uint32_t)(targets >> 32);
                open_source = false;
            }
            if (rem) {  // next source
                const int cell = __ffsll((unsigned long long)rem) - 1;
                rem &= rem - 1;
                x = (uint32_t)cell - m.row_base;
                pending = 1ull << cell;
                done = 0;
                targets = 0;
                open_source = true;
            }
        }
        if (pending) {  // expand one cell: a segment of value(cell) steps (reach's walk)
            const int c = __ffsll((unsigned long long)pending) - 1;
            pending &= pending - 1;
            done |= 1ull << c;
            const uint32_t v = value_at(b, c);
            uint64_t a0 = 1ull << c, al = 0, ar = 0, land = 0;
            for (uint32_t s = 1; s <= v; ++s) {
                const uint64_t via_left = a0 | al, via_right = a0 | ar;  // who may go on left / right (no reversal)
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
            targets |= land & landing;
            pending |= land & bounce_on & ~done;
        }
    }
}

// the idx-th action of the canonical list (sources by ascending x, targets by ascending cell) from the packed counts and
// the LDS column
template <int NC>
__device__ __forceinline__ void pick_flat(const FlatMoves<NC>& m, const uint32_t* column, uint32_t idx, int& src_cell, int& dst_cell) {
    uint32_t col = 0;
    bool found = false;
#pragma unroll
    for (int x = 0; x < 8 * NC; ++x) {
        const uint32_t cnt = (uint32_t)(m.counts[x >> 3] >> (8 * (x & 7))) & 255u;
        const bool here = !found && idx < cnt;
        col = here ? (uint32_t)x : col;
        idx = (found || here) ? idx : idx - cnt;
        found = found || here;
    }
    const uint64_t chosen = ((uint64_t)column[(2u * col + 1u) * BGS_BLOCK] << 32) | column[(2u * col) * BGS_BLOCK];
    src_cell = (int)(m.row_base + col);
    dst_cell = (int)select_bit64(chosen, idx);
}

}  // namespace
}  // namespace bgs
