// connect_board.h -- the packed Connect board and its win tests, shared by the Connect unit (connect_kernels.hip) and
// the evaluation unit (evaluate_kernels.hip).  The Makefile hashes this header into the ids of both units.
//
// Board packing (connect_kernels.hip): two bit-planes, column-major, one always-empty sentinel bit on top of every
// column: bit(x, y) = x * (H + 1) + y.  A plane is NW = ceil(W * (H + 1) / 64) uint64 words.
#pragma once

#include "bgs_common.h"

namespace bgs {
namespace {

// ------------------------------------------------------------------------------------------------
// multi-word bitboards
// ------------------------------------------------------------------------------------------------
template <int NW>
struct Bits {
    uint64_t w[NW];
};

template <int NW>
__device__ __forceinline__ Bits<NW> zero_bits() {
    Bits<NW> r;
#pragma unroll
    for (int i = 0; i < NW; ++i) r.w[i] = 0;
    return r;
}

template <int NW>
__device__ __forceinline__ Bits<NW> operator&(const Bits<NW>& a, const Bits<NW>& b) {
    Bits<NW> r;
#pragma unroll
    for (int i = 0; i < NW; ++i) r.w[i] = a.w[i] & b.w[i];
    return r;
}

template <int NW>
__device__ __forceinline__ Bits<NW> operator|(const Bits<NW>& a, const Bits<NW>& b) {
    Bits<NW> r;
#pragma unroll
    for (int i = 0; i < NW; ++i) r.w[i] = a.w[i] | b.w[i];
    return r;
}

template <int NW>
__device__ __forceinline__ bool any(const Bits<NW>& a) {
    uint64_t acc = 0;
#pragma unroll
    for (int i = 0; i < NW; ++i) acc |= a.w[i];
    return acc != 0;
}

template <int NW>
__device__ __forceinline__ uint32_t popcount(const Bits<NW>& a) {
    uint32_t c = 0;
#pragma unroll
    for (int i = 0; i < NW; ++i) c += (uint32_t)__popcll(a.w[i]);
    return c;
}

// word `idx` of a (0 beyond the top); idx may be a run-time value: resolved with selects, never with
// dynamically indexed registers
template <int NW>
__device__ __forceinline__ uint64_t word_at(const Bits<NW>& a, int idx) {
    uint64_t r = 0;
#pragma unroll
    for (int i = 0; i < NW; ++i) r = (idx == i) ? a.w[i] : r;
    return r;
}

// logical shift right by s >= 0 bits, bits beyond the plane read as 0 (folds to constants when s is known at compile time)
template <int NW>
__device__ __forceinline__ Bits<NW> shr(const Bits<NW>& a, int s) {
    Bits<NW> r;
    if (NW == 1) {
        r.w[0] = s < 64 ? (a.w[0] >> s) : 0ull;
        return r;
    }
    const int ws = s >> 6, bs = s & 63;
#pragma unroll
    for (int i = 0; i < NW; ++i) {
        const uint64_t lo = word_at(a, i + ws);
        const uint64_t hi = word_at(a, i + ws + 1);
        r.w[i] = bs ? ((lo >> bs) | (hi << (64 - bs))) : lo;
    }
    return r;
}

template <int NW>
__device__ __forceinline__ void set_bit(Bits<NW>& a, int t) {
    if (NW == 1) {
        a.w[0] |= 1ull << t;
        return;
    }
    const int ws = t >> 6;
    const uint64_t m = 1ull << (t & 63);
#pragma unroll
    for (int i = 0; i < NW; ++i) a.w[i] |= (ws == i) ? m : 0ull;
}

template <int NW>
__device__ __forceinline__ bool test_bit(const Bits<NW>& a, int t) {
    return (word_at(a, t >> 6) >> (t & 63)) & 1ull;
}

// bit x of the result is bit x - s of `a` (s >= 0; bits below the plane read as 0)
template <int NW>
__device__ __forceinline__ Bits<NW> shl(const Bits<NW>& a, int s) {
    Bits<NW> r;
    if (NW == 1) {
        r.w[0] = s < 64 ? a.w[0] << s : 0ull;
        return r;
    }
    const int q = s >> 6, rr = s & 63;
#pragma unroll
    for (int j = 0; j < NW; ++j) {
        uint64_t x = 0, y = 0;
#pragma unroll
        for (int k = 0; k < NW; ++k) {
            x = (k == j - q) ? a.w[k] : x;
            y = (k == j - q - 1) ? a.w[k] : y;
        }
        r.w[j] = rr ? (x << rr) | (y >> (64 - rr)) : x;
    }
    return r;
}

template <int NW>
__device__ __forceinline__ void flip(Bits<NW>& a, uint32_t pos) {
#pragma unroll
    for (int j = 0; j < NW; ++j) a.w[j] ^= ((uint32_t)j == (pos >> 6)) ? 1ull << (pos & 63u) : 0ull;
}

template <int NW>
__device__ __forceinline__ uint32_t lowest(const Bits<NW>& a) {   // position of the lowest set bit (a != 0)
    uint32_t pos = 0;
    bool found = false;
#pragma unroll
    for (int j = 0; j < NW; ++j) {
        const bool here = !found && a.w[j] != 0ull;
        pos = here ? 64u * j + (uint32_t)(__ffsll((unsigned long long)a.w[j]) - 1) : pos;
        found = found || here;
    }
    return pos;
}

// k stones in a row anywhere on bitboard b: shift-and-AND with run doubling.
// directions: vertical 1, horizontal H+1, rising diagonal H+2, falling diagonal H.  G: anything with h() and k() (the
// Connect unit's Geo, the evaluation unit's EvalGeom).
template <class G, int NW>
__device__ __forceinline__ bool has_run(const G& g, const Bits<NW>& b) {
    const int k = g.k();
    const int dirs[4] = {1, g.h() + 1, g.h() + 2, g.h()};
    Bits<NW> hit = zero_bits<NW>();
#pragma unroll
    for (int d = 0; d < 4; ++d) {
        Bits<NW> m = b;
        int len = 1;
        while (2 * len <= k) {
            m = m & shr(m, len * dirs[d]);
            len *= 2;
        }
        if (len < k) m = m & shr(m, (k - len) * dirs[d]);
        hit = hit | m;
    }
    return any(hit);
}

// the cells the next stone of every open column would take: (stones + column bottoms) carries through each column's
// stones and stops under its sentinel; a carry may cross a word boundary with the column.  G: a geometry with the
// multi-word masks bottoms[] (the bottom cell of every column) and cells[] (every real cell), the evaluation unit's EvalGeom
template <class G, int NW>
__device__ __forceinline__ Bits<NW> landing_of(const G& g, const Bits<NW>& occ) {
    Bits<NW> r;
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

// (a & b) | c in one VALU instruction (v_bitop3_b32, truth table 0xEA)
__device__ __forceinline__ uint32_t and_or(uint32_t a, uint32_t b, uint32_t c) {
    uint32_t r;
    asm("v_bitop3_b32 %0, %1, %2, %3 bitop3:0xea" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}

// four in a row on a one-word board, written for instruction count (every VALU instruction costs about one issue
// quad here, whatever its width): per direction two 64-bit shifts, two ANDs for the pairs, and the quads are
// accumulated with the fused (pairs & shifted pairs) | acc
__device__ __forceinline__ bool four_in_a_row(uint64_t b, int h) {
    const int dirs[4] = {1, h + 1, h + 2, h};
    uint32_t acc_lo = 0, acc_hi = 0;
#pragma unroll
    for (int d = 0; d < 4; ++d) {
        const uint64_t s1 = b >> dirs[d];
        const uint32_t pl = (uint32_t)b & (uint32_t)s1, ph = (uint32_t)(b >> 32) & (uint32_t)(s1 >> 32);
        const uint64_t pairs = ((uint64_t)ph << 32) | pl;
        uint64_t s2;  // one v_lshrrev_b64 (hipcc would split this shift of two halves into alignbit + shift)
        asm("v_lshrrev_b64 %0, %1, %2" : "=v"(s2) : "s"(2 * dirs[d]), "v"(pairs));
        if (d == 0) {
            acc_lo = pl & (uint32_t)s2;
            acc_hi = ph & (uint32_t)(s2 >> 32);
        } else {
            acc_lo = and_or(pl, (uint32_t)s2, acc_lo);
            acc_hi = and_or(ph, (uint32_t)(s2 >> 32), acc_hi);
        }
    }
    return (acc_lo | acc_hi) != 0u;
}

// The same test split the way the rollout uses it: a run that the stone just dropped on `pos` completes is either
// vertical -- then it is the four cells ending at pos, one shift and one compare (a shift amount below zero wraps to
// 61..63 and leaves at most three bits, and a stone lower than row 3 has the previous column's always-empty sentinel in
// its window) -- or lies in one of the three other directions, tested on the whole board as above.
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
    uint32_t column = (uint32_t)(b >> ((pos - 3u) & 63u));  // the stone and the three cells below it
    asm("" : "+v"(column));  // (keeps the compare 32 bits wide: hipcc would otherwise widen it and add a move)
    return ((acc_lo | acc_hi) != 0u) | ((column & 15u) == 15u);
}

// four_in_a_row_at for geometries where runs_start_low(h, w) holds (connect_unit.h): bit s of the quads is set iff cells
// s, s + d, s + 2d and s + 3d are the mover's, a non-vertical run spans four columns, so s <= (w - 4)(h + 1) + h - 1 <= 31
// and the high word of the quads is always zero.  Only the low word of the second shift is needed then -- one
// v_alignbit_b32 of (ph, pl); 2d <= 2(h + 2) <= 20 < 32 for the h <= 8 of one-word rollouts -- and one accumulator:
// per direction five VALU instead of six, and no OR of the halves (four VALU a ply less).  The vertical test is
// four_in_a_row_at's.  (Folding the vertical hit into the accumulator as (column + 1) & 16 was not kept: see
// docs/EXPERIMENTS.md §26 -- it is wrong on a lane that is not playing.)
__device__ __forceinline__ bool four_in_a_row_at_low(uint64_t b, int h, uint32_t pos) {
    const int dirs[3] = {h + 1, h + 2, h};
    uint32_t acc = 0;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        const uint64_t s1 = b >> dirs[d];
        const uint32_t pl = (uint32_t)b & (uint32_t)s1, ph = (uint32_t)(b >> 32) & (uint32_t)(s1 >> 32);
        uint32_t s2;  // the low word of pairs >> 2d (hipcc would rebuild the 64-bit shift from the two halves)
        asm("v_alignbit_b32 %0, %1, %2, %3" : "=v"(s2) : "v"(ph), "v"(pl), "s"(2 * dirs[d]));
        acc = d == 0 ? (pl & s2) : and_or(pl, s2, acc);
    }
    uint32_t column = (uint32_t)(b >> ((pos - 3u) & 63u));
    asm("" : "+v"(column));
    return (acc != 0u) | ((column & 15u) == 15u);
}

// The idx-th set bit of `landing` (K1s): `landing` holds at most ONE bit per column field of S = h + 1 bits and never a field's
// top bit, so the search is arithmetic on the fields instead of the general popcount-guided search (forty instructions of
// the ply's hundred and fifty; round 5): a field is non-empty iff adding 2^(S-1) - 1 carries into its top bit; the number
// of non-empty fields up to field x is field x of (flags * bottoms) -- no carries between fields: a count is at most w --
// and field x of (idx - flags) * bottoms + tops keeps its top bit iff fewer than idx + 1 non-empty fields lie at or below x,
// i.e. iff the column sought lies above x: their number is that column.  K2a's nibble search, on fields of S bits.
// Needs w <= 2^(S-1) = 2^h (the counts must fit under a field's top bit): play_plies asks.
__device__ __forceinline__ uint32_t select_landing(uint64_t landing, uint64_t bottoms, uint64_t tops, uint32_t stride, uint32_t idx) {
    const uint64_t flags = ((landing + (tops - bottoms)) & tops) >> (stride - 1u);
    const uint64_t cmp = ((uint64_t)idx - flags) * bottoms + tops;
    const uint32_t col = (uint32_t)__popcll(cmp & tops);
    const uint64_t low = (1ull << stride) - 1ull;   // (uniform: a field's bits)
    return (uint32_t)__ffsll((unsigned long long)(landing & (low << (col * stride)))) - 1u;
}

}  // namespace
}  // namespace bgs
