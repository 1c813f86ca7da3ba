// bounce_root_moves.h -- the first pass of the two launches that number the legal (root, move) pairs of a Bounce batch: the
// flat evaluation (evaluate_kernels.hip) and the exact solver (solve_kernels.hip).  Three small kernels count the legal
// moves of every root and scan the counts over the batch.  They live in an anonymous namespace, so each of the two units
// holds its own copies; the search unit (search_kernels.hip) numbers nothing and does not include this header.  The
// Makefile hashes it into the ids of the two units that do.
#pragma once

#include "playout.h"

namespace bgs {
namespace {

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


// the pass on the batch's stream: ends[i] = the legal moves of roots 0 .. i, totals = a word a workgroup of scratch
template <bool CAPPED, class GEO>
void launch_bounce_root_moves(const bgs_batch* b, const GEO& g, uint64_t* d_ends, uint64_t* d_totals) {
    const int64_t blocks = (b->n + BGS_BLOCK - 1) / BGS_BLOCK;
    hipLaunchKernelGGL((k_bounce_eval_count<GEO, CAPPED>), dim3((uint32_t)blocks), dim3(BGS_BLOCK), 0, b->stream, g, (const uint64_t*)b->d_planes,
                       (const uint8_t*)b->d_status, (const uint16_t*)b->d_plies, b->n, d_ends, d_totals);
    if (blocks > 1) {
        hipLaunchKernelGGL(k_bounce_eval_scan_totals, dim3(1), dim3(BGS_BLOCK), 0, b->stream, d_totals, blocks);
        hipLaunchKernelGGL(k_bounce_eval_add_totals, dim3((uint32_t)blocks), dim3(BGS_BLOCK), 0, b->stream, d_ends,
                           (const uint64_t*)d_totals, b->n);
    }
}

}  // namespace
}  // namespace bgs
