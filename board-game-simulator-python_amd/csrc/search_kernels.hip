// search_kernels.hip -- the batched UCT tree searches: Connect (bgs_connect_search_actions, the forest
// bgs_connect_forest_search / bgs_connect_forest_advance, the proving search bgs_connect_search_actions_proving) in the
// first half of this file, Bounce (bgs_bounce_search_moves and its forest and proving forms) in the second.  A search is
// one kernel a game, k_connect_search / k_bounce_search; the forest and the proving search are template parameters of it
// (FOREST, PROVE), and the re-rooting of a forest is a kernel of its own.  The PUCT search whose leaves the caller
// evaluates (bgs_connect_guided_step, k_connect_search_guided) follows the Connect forest, and its Bounce sibling
// (bgs_bounce_guided_step, k_bounce_search_guided) the Bounce forest.  The section comments below describe each.
//
// A unit of its own (bgs_kernel_unit_id(4)).  The leaves' playouts are the evaluation unit's (evaluate_kernels.hip): the
// Connect 4-ply block is written out in k_connect_search, the Bounce ply is bounce_playout_ply of playout.h, which also
// holds the board and policy primitives the three analysis units share.
#include "playout.h"

#ifndef BGS_TU_ID
#define BGS_TU_ID "unknown"
#endif
extern "C" const char bgs_tu_id_search[] = BGS_TU_ID;

namespace bgs {
namespace {

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

                const bool ended = connect_playout_block<NW, PER_PLY, POLICY>(g, seed, max_plies, q, game, blk, skip, live, st, fresh, ph, played);
                if (ended) wdl_count(st, root_mover, wins, draws, losses);
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
// PUCT tree search with caller-evaluated leaves (bgs_connect_guided_step, include/bgs.h): one launch is one simulation
// of every tree -- the caller's (priors, value) of the pending leaf go into the tree, the root's statistics come out,
// and a descent finds the next leaf, whose position goes out for the caller's evaluator.  No playouts, no RNG.
//
// Shape: k_connect_search's.  One wave owns one tree; the descent is wave-uniform and rebuilds the position from the
// root; lane c holds n, s, the child and P of column c of the node at hand and computes U(c); N and the arg-max key
// are reduced over the lanes with readlane.  What differs is where the state between two simulations lives: the
// launch ends at the leaf, so the path and the leaf's kind are in the tree's share, not in LDS.
//
// A node is 4 * width words: n[c], s[c], child[c] (0: none), P[c].  A tree's share, in 32-bit words, rounded up to 256
// bytes:
//     word 0         the nodes in use, the root counted (0: an emptied tree)
//     word 1         the pending leaf: bits 7:0 its kind (kGuidedNone, kGuidedEvaluate, kGuidedWon, kGuidedFull), bits
//                    31:16 the legal columns of an EVALUATE leaf, a bit a column (the priors are read for those alone)
//     word 2         the edges of the pending path
//     word 3         1 once the root has its P
//     words 4 ..     the position the root stands for: the 2 * NW plane words of the batch, 64 bits each
//     words 16 ..    the path: h * w words, edge k leaves node (word >> 4) by column (word & 15)
//     then           `capacity` nodes
// Every word read back from the share is used only within its bounds (a path no longer than h * w, a node below the
// count, a column below the width): memory that passes the check by accident gives a wrong tree, never a wild store.
//
// Ordering: the tree is written by some lanes (lane k of the back-propagation, the lanes that fill a new node, lane 0
// for the path) and read by others; a __syncthreads() of the one-wave workgroup stands between the application and
// the report, the only such pair of a launch (the descent reads nodes the application wrote, behind the same barrier,
// and the path it writes is read by the next launch).
// ================================================================================================================
constexpr uint32_t kGuidedHeaderWords = 16;
constexpr uint32_t kGuidedNone = 0u, kGuidedEvaluate = 1u, kGuidedWon = 2u, kGuidedFull = 3u;
static_assert(BGS_GUIDED_MAX_CAPACITY <= (1 << 28), "a path word holds node << 4 | column");
static_assert(((uint64_t)BGS_GUIDED_MAX_VISITS + 1u) << 12 < ((uint64_t)1 << 32), "(N + 1) << 12 fits 32 bits");

// words of a tree's share: the header, the path and `capacity` nodes, rounded up to 256 bytes (below 2^32)
__host__ __device__ __forceinline__ uint64_t guided_tree_words(uint32_t height, uint32_t width, uint32_t capacity) {
    return (kGuidedHeaderWords + (uint64_t)height * width + (uint64_t)capacity * width * 4u + 63u) & ~(uint64_t)63u;
}

// floor(num / den), den >= 1, num < 2^34: the double quotient of two such integers is within one of it
__device__ __forceinline__ uint32_t guided_quotient(uint64_t num, uint32_t den) {
    uint32_t q = (uint32_t)((double)num / (double)den);
    while ((uint64_t)q * den > num) --q;
    while ((uint64_t)(q + 1u) * den <= num) ++q;
    return q;
}

template <int NW>
__global__ void __launch_bounds__(BGS_WAVE)
k_connect_search_guided(EvalGeom g, const uint64_t* __restrict__ planes, const uint8_t* __restrict__ status, int64_t n,
                        int64_t root_base, uint32_t capacity, uint32_t cpuct, uint32_t flags, const float* __restrict__ priors,
                        const float* __restrict__ values, int8_t* __restrict__ leaf_grid, int8_t* __restrict__ leaf_player,
                        int32_t* __restrict__ leaf_kind, int32_t* __restrict__ visits, int32_t* __restrict__ scores,
                        int32_t* __restrict__ best, int32_t* __restrict__ nodes, uint32_t* trees) {
    const uint32_t lane = threadIdx.x;
    const uint32_t width = (uint32_t)g.w();
    const uint32_t stride = (uint32_t)g.h() + 1u;
    const uint32_t node_words = width * 4u;
    const int64_t i = root_base + (int64_t)blockIdx.x;       // (the grid holds exactly the trees of this launch)
    uint32_t* const head = trees + (uint64_t)i * guided_tree_words((uint32_t)g.h(), width, capacity);
    uint64_t* const head_planes = reinterpret_cast<uint64_t*>(head + 4);
    uint32_t* const path = head + kGuidedHeaderWords;
    uint32_t* const tree = path + g.cells_total;

    Bits<NW> r0, r1;
#pragma unroll
    for (int j = 0; j < NW; ++j) {
        r0.w[j] = planes[(int64_t)j * n + i];
        r1.w[j] = planes[(int64_t)(NW + j) * n + i];
    }
    const uint32_t rply = popcount(r0) + popcount(r1);
    const bool running = status[i] == BGS_ST_RUNNING;
    // lane c: the stones in column c of a position (h for a lane without a column: never legal)
    const auto heights = [&](const Bits<NW>& occ) {
        uint32_t height = (uint32_t)g.h();
        if (lane < width) height = (uint32_t)__popcll(shr(occ, (int)(lane * stride)).w[0] & ((1ull << g.h()) - 1ull));
        return height;
    };

    // ---- 1. the check (wave-uniform: every lane reads the same header); a tree that fails it is emptied
    uint32_t used = head[0], pending = head[1], depth = head[2], expanded = head[3];
    bool live = (flags & BGS_GUIDED_RESTART) == 0u && running && used >= 1u && used <= capacity;
    if (live) {
#pragma unroll
        for (int j = 0; j < NW; ++j) live = live && head_planes[j] == r0.w[j] && head_planes[NW + j] == r1.w[j];
    }
    live = __builtin_amdgcn_readfirstlane((int)live) != 0;
    if (!live) {
        used = running ? 1u : 0u;
        pending = kGuidedNone;
        depth = 0;
        expanded = 0;
        if (running && lane < node_words) tree[lane] = 0;     // the root is node 0 (4 * width <= 64 words)
        if (running && lane == 0) {
#pragma unroll
            for (int j = 0; j < NW; ++j) {
                head_planes[j] = r0.w[j];
                head_planes[NW + j] = r1.w[j];
            }
        }
    }
    used = (uint32_t)__builtin_amdgcn_readfirstlane((int)used);
    pending = (uint32_t)__builtin_amdgcn_readfirstlane((int)pending);
    depth = (uint32_t)__builtin_amdgcn_readfirstlane((int)depth);
    depth = depth < g.cells_total ? depth : g.cells_total;
    expanded = (uint32_t)__builtin_amdgcn_readfirstlane((int)expanded);

    // ---- 2. the application of the pending evaluation
    const uint32_t kind = pending & 255u;
    if (kind != kGuidedNone) {
        uint32_t sigma = kind == kGuidedWon ? 0u : 1024u;     // the leaf's value for its mover, 0 .. 2048
        if (kind == kGuidedEvaluate) {
            const float x = values[i];
            int32_t v = 0;
            if (x == x) v = (int32_t)(fminf(fmaxf(x, -1.0f), 1.0f) * 1024.0f);
            sigma = (uint32_t)(1024 + v);
            // the priors of the leaf's legal columns, lane c column c: 16-bit weights, then 16-bit shares
            const uint32_t columns = pending >> 16;
            const bool legal = lane < width && ((columns >> lane) & 1u) != 0u;
            uint32_t weight = 0;
            if (legal) {
                const float pr = priors[i * (int64_t)width + lane];
                if (pr > 0.0f) weight = (uint32_t)(fminf(pr, 1.0f) * 65536.0f);
            }
            uint32_t sum = 0;
            for (uint32_t c = 0; c < width; ++c) sum += (uint32_t)__builtin_amdgcn_readlane((int)weight, (int)c);
            if (sum == 0u) {
                weight = legal ? 1u : 0u;
                sum = (uint32_t)__popcll(__builtin_amdgcn_ballot_w64(legal));
            }
            const uint32_t share = legal ? guided_quotient((uint64_t)weight << 16, sum) : 0u;
            if (depth == 0u) {                                // the root is the leaf: it only receives P
                if (lane < width) tree[3u * width + lane] = share;
                expanded = 1u;
            } else {                                          // a node is made if the edge has no child and the tree has room
                const uint32_t edge = path[depth - 1u];
                const uint32_t pv = edge >> 4, pc = edge & 15u;
                const bool known = pv < used && pc < width;
                const uint32_t child = known ? tree[(uint64_t)pv * node_words + 2u * width + pc] : 1u;
                if (__builtin_amdgcn_readfirstlane((int)child) == 0 && used < capacity) {
                    uint32_t* const made = tree + (uint64_t)used * node_words;
                    if (lane < 3u * width) made[lane] = 0;
                    if (lane < width) made[3u * width + lane] = share;
                    if (lane == 0) tree[(uint64_t)pv * node_words + 2u * width + pc] = used;
                    used += 1u;
                }
            }
        }
        // lane k takes edge k of the path: node k's mover is the leaf's when depth - k is even
        for (uint32_t k = lane; k < depth; k += BGS_WAVE) {
            const uint32_t edge = path[k];
            const uint32_t pv = edge >> 4, pc = edge & 15u;
            if (pv < used && pc < width) {
                uint32_t* const node = tree + (uint64_t)pv * node_words;
                node[pc] += 1u;
                node[width + pc] += ((depth - k) & 1u) ? 2048u - sigma : sigma;
            }
        }
        pending = kGuidedNone;
        depth = 0;
    }
    __syncthreads();                // the tree is whole: the report and the descent read what other lanes wrote

    // ---- 3. the report (an illegal column was never played: its words of the root are zero)
    uint32_t nv = 0, sv = 0;
    if (used != 0u && lane < width) {
        nv = tree[lane];
        sv = tree[width + lane];
    }
    if (lane < width) {
        if (visits) visits[i * (int64_t)width + lane] = (int32_t)nv;
        if (scores) scores[i * (int64_t)width + lane] = (int32_t)sv;
    }
    uint32_t root_total = 0;
    {
        // the most visits, then the larger s, then the lower column
        int32_t top = -1;
        uint32_t top_n = 0, top_s = 0;
        for (uint32_t c = 0; c < width; ++c) {
            const uint32_t cn = (uint32_t)__builtin_amdgcn_readlane((int)nv, (int)c);
            const uint32_t cs = (uint32_t)__builtin_amdgcn_readlane((int)sv, (int)c);
            root_total += cn;
            if (cn > 0u && (top < 0 || cn > top_n || (cn == top_n && cs > top_s))) {
                top = (int32_t)c;
                top_n = cn;
                top_s = cs;
            }
        }
        if (lane == 0) {
            if (best) best[i] = top;
            if (nodes) nodes[i] = (int32_t)(used ? used - 1u : 0u);
        }
    }

    // ---- 4. the selection (wave-uniform): p is the position at node v, and the leaf's at the end
    Bits<NW> p[2] = {r0, r1};
    uint32_t ply = rply, out_kind = (uint32_t)BGS_GUIDED_IDLE;
    if (used != 0u && (flags & BGS_GUIDED_FINISH) == 0u && root_total < (uint32_t)BGS_GUIDED_MAX_VISITS) {
        if (expanded == 0u) {                                          // an unexpanded root is itself the leaf
            const uint64_t columns = __builtin_amdgcn_ballot_w64(heights(p[0] | p[1]) < (uint32_t)g.h());
            pending = kGuidedEvaluate | ((uint32_t)columns << 16);
            out_kind = (uint32_t)BGS_GUIDED_EVALUATE;
        } else {
            uint32_t v = 0;
            for (;;) {
                const uint32_t height = heights(p[0] | p[1]);
                const bool legal = height < (uint32_t)g.h();
                if (__builtin_amdgcn_ballot_w64(legal) == 0) break;    // (a running position always has a column)
                const uint32_t* const node = tree + (uint64_t)v * node_words;
                uint32_t nc = 0, sc = 0, ch = 0, pc = 0;
                if (legal) {
                    nc = node[lane];
                    sc = node[width + lane];
                    ch = node[2u * width + lane];
                    pc = node[3u * width + lane];
                }
                uint32_t total = 0;
                for (uint32_t c = 0; c < width; ++c) total += (uint32_t)__builtin_amdgcn_readlane((int)nc, (int)c);
                // (a node's N is at most the root's, which the selection bounds: the clamp changes no tree and keeps (N + 1) << 12
                // in 32 bits whatever the memory held)
                total = total < (uint32_t)BGS_GUIDED_MAX_VISITS ? total : (uint32_t)BGS_GUIDED_MAX_VISITS;
                const uint32_t root = search_isqrt((total + 1u) << 12);
                uint32_t key = 0;                                      // (U(c) << 4 | 15 - c) + 1: the largest U, then the lowest column
                if (legal) {
                    const uint32_t q = nc ? (2u * sc) / nc : 2048u;
                    const uint32_t e = (uint32_t)(((uint64_t)(cpuct * pc) * root) >> 19) / (1u + nc);
                    key = (((q + e) << 4) | (15u - lane)) + 1u;
                }
                uint32_t top = 0;
                for (uint32_t c = 0; c < width; ++c) {
                    const uint32_t other = (uint32_t)__builtin_amdgcn_readlane((int)key, (int)c);
                    top = other > top ? other : top;
                }
                const uint32_t col = 15u - ((top - 1u) & 15u);
                const uint32_t at = (uint32_t)__builtin_amdgcn_readlane((int)height, (int)col);
                const uint32_t child = (uint32_t)__builtin_amdgcn_readlane((int)ch, (int)col);
                if (lane == 0 && depth < g.cells_total) path[depth] = (v << 4) | col;   // (always: the position had room for a stone)
                const uint32_t mover = ply & 1u;
                Bits<NW>& mine = mover ? p[1] : p[0];
                const bool won = __builtin_amdgcn_readfirstlane((int)drop_and_test(g, mine, col * stride + at, ~0u)) != 0;
                ply += 1u;
                depth += 1u;
                if (won || ply >= g.cells_total) {                     // the leaf ended the game: its value is known
                    pending = won ? kGuidedWon : kGuidedFull;
                    out_kind = (uint32_t)BGS_GUIDED_TERMINAL;
                    break;
                }
                if (child == 0u || child >= used) {                    // no node for p' yet: the caller evaluates it
                    const uint64_t columns = __builtin_amdgcn_ballot_w64(heights(p[0] | p[1]) < (uint32_t)g.h());
                    pending = kGuidedEvaluate | ((uint32_t)columns << 16);
                    out_kind = (uint32_t)BGS_GUIDED_EVALUATE;
                    break;
                }
                v = child;
            }
            if (out_kind == (uint32_t)BGS_GUIDED_IDLE) {               // (the descent found no column: nothing is pending)
                p[0] = r0;
                p[1] = r1;
                ply = rply;
                depth = 0;
            }
        }
    }

    // ---- the leaf goes out (an idle tree shows its root), in the encoding of bgs_read_grid: row 0 is the bottom
    int8_t* const cells = leaf_grid + i * (int64_t)g.cells_total;
    for (uint32_t j = lane; j < g.cells_total; j += BGS_WAVE) {
        const uint32_t y = j / width, x = j - y * width;
        const int bit = (int)(x * stride + y);
        cells[j] = (int8_t)((int)test_bit(p[0], bit) + 2 * (int)test_bit(p[1], bit) - 1);
    }
    if (lane == 0) {
        leaf_player[i] = (int8_t)(ply & 1u);
        leaf_kind[i] = (int32_t)out_kind;
        head[0] = used;             // the header: the planes were recorded when the tree was emptied
        head[1] = pending;
        head[2] = depth;
        head[3] = expanded;
    }
}

// The re-rooting of the guided trees (bgs_connect_guided_advance): k_connect_forest_advance on the guided share -- one
// wave a tree, in place, one launch over exactly the trees of the launch, with that kernel's mark, number, move and header
// passes on nodes of 4 * width words, of which words 2 * width .. 3 * width - 1 are the child words.  The three passes are a
// second text: one `__device__` function for both kernels changed the forest kernel's instruction order (same size, same
// registers, other bytes), and that kernel stays byte for byte what it was (docs/EXPERIMENTS.md).  What differs is the
// header: the planes stand at word 4, and a tree that was advanced has nothing pending (words 1 and 2 cleared: the
// pending path named nodes by their old indices) and a root that has its P (word 3: the new root was made by an
// application, which gave it P).  An emptied tree has words 0 .. 3 zero, as the step's check leaves it.  c < 0 touches
// nothing, a pending leaf included.
// Bounds: the count is used only up to `capacity`, the child word of the root's edge only below the count, the column only
// below the width, the stone's cell only below the height, a child word only above its node and below the count (so a
// store goes to a slot at or below the node it moves): memory that passes the step's check by accident gives a wrong
// tree, never a wild store.
// LDS: the two mask arrays (`capacity` bits and a 32nd of a word a node, each rounded up to 16 bytes) and a chunk of 64
// nodes: 2 * 8 KB + 16 KB = 32 KB at capacity 65536 and width 16 (BGS_GUIDED_ADVANCE_MAX_CAPACITY).
static_assert(BGS_GUIDED_ADVANCE_MAX_CAPACITY <= BGS_GUIDED_MAX_CAPACITY, "an advanced tree is a guided tree");
static_assert((2u * ((BGS_GUIDED_ADVANCE_MAX_CAPACITY + 31u) / 32u + 3u) + 64u * 16u * 4u) * sizeof(uint32_t) <= 64u * 1024u,
              "the masks and a chunk of 64 nodes of 64 words fit the LDS of a workgroup");
__global__ void __launch_bounds__(BGS_WAVE)
k_connect_guided_advance(uint32_t height, uint32_t width, uint32_t nw, const int32_t* __restrict__ columns, uint32_t capacity,
                         uint32_t* trees, int32_t* __restrict__ kept, int64_t root_base) {
    extern __shared__ __attribute__((aligned(16))) uint32_t guided_lds[];
    const uint32_t lane = threadIdx.x;
    const uint32_t node_words = width * 4u;
    const uint32_t mask_room = (((capacity + 31u) >> 5) + 3u) & ~3u;
    uint32_t* const mask = guided_lds;              // bit v: node v stays
    uint32_t* const below = mask + mask_room;       // the marked nodes in the mask words before this one
    uint32_t* const chunk = below + mask_room;      // 64 nodes
    const int64_t i = root_base + (int64_t)blockIdx.x;
    uint32_t* const head = trees + (uint64_t)i * guided_tree_words(height, width, capacity);
    uint32_t* const planes = head + 4;              // the recorded position, counted in 32-bit words
    uint32_t* const tree = head + kGuidedHeaderWords + height * width;

    const int32_t c = columns[i];
    uint32_t used = head[0];
    used = (uint32_t)__builtin_amdgcn_readfirstlane((int)(used <= capacity ? used : 0u));
    if (c < 0) {                                    // untouched, a pending leaf included
        if (kept && lane == 0) kept[i] = (int32_t)(used ? used - 1u : 0u);
        return;
    }
    // the new root: the child of the root's edge c (0: never played, terminal, did not fit, a full column)
    uint32_t r = (used != 0u && (uint32_t)c < width) ? tree[2u * width + (uint32_t)c] : 0u;
    r = (uint32_t)__builtin_amdgcn_readfirstlane((int)(r < used ? r : 0u));
    // the cell the stone takes on the recorded position, and its mover
    const uint32_t plane_words = 2u * nw;           // 32-bit words a player
    uint32_t stones = lane < 2u * plane_words ? (uint32_t)__popc(planes[lane]) : 0u;
    for (int d = 32; d >= 1; d >>= 1) stones += (uint32_t)__shfl_xor((int)stones, d);
    uint32_t at = 0;
    if ((uint32_t)c < width) {
        for (uint32_t y0 = 0; y0 < height; y0 += BGS_WAVE) {
            const uint32_t bit = (uint32_t)c * (height + 1u) + y0 + lane;
            const bool taken = y0 + lane < height &&
                               (((planes[bit >> 5] | planes[plane_words + (bit >> 5)]) >> (bit & 31u)) & 1u) != 0u;
            at += (uint32_t)__popcll(__builtin_amdgcn_ballot_w64(taken));
        }
    }
    if (r == 0u || at >= height) {                  // emptied: the next step starts the tree anew from the batch's board
        if (lane < 4u) head[lane] = 0;
        if (kept && lane == 0) kept[i] = 0;
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
                if (lane - 2u * width < width) {    // a child word: the child's new index (a kept node's children are kept)
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
        head[1] = kGuidedNone;                      // the pending leaf is dropped
        head[2] = 0;
        head[3] = 1u;                               // the new root was made with its P
        planes[((stones & 1u) ? plane_words : 0u) + (bit >> 5)] |= 1u << (bit & 31u);
        if (kept) kept[i] = (int32_t)(total - 1u);
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

// ================================================================================================================
// PUCT tree search for Bounce with caller-evaluated leaves (bgs_bounce_guided_step, include/bgs.h): one launch is one
// simulation of every tree, as k_connect_search_guided -- the caller's (priors, value) of the pending leaf go into the
// tree, the root's statistics come out, a descent finds the next leaf -- over k_bounce_search's tree: an edge pool, a node
// table, arms that are generated once (movable, reach) and replayed, the ended and capped sentinels.
//
// Shape: one wave a tree.  Lanes stride a node's arms, at most kGuidedLaneArms = 8 a lane; N and the selection key go
// through wave_sum and wave_max64 (the key is (U << 9 | 511 - arm) + 1 with U < 2^25 + 4097: 64 bits).  A step is a short
// chain of dependent loads a level, and a launch has thousands of trees: a wave a tree keeps four times the trees of a
// 256-lane team resident on a CU (docs/EXPERIMENTS.md §42).  LDS holds the 8 * NC target words of the position whose arms
// are being numbered, and nothing else.
//
// A tree's share, in 32-bit words, rounded up to 256 bytes:
//     word 0         the nodes in use, the root counted (0: an emptied tree)
//     word 1         the pool edges in use
//     word 2         the absolute ply count of the position the root stands for
//     word 3         the effective cap (min(max_plies, 65535)) the tree's kEdgeCapped sentinels were written under
//     words 4 .. 11  the position the root stands for: the four 64-bit planes of the batch
//     word 12        the pending leaf's kind (kGuidedNone, kGuidedEvaluate, kGuidedWon, kGuidedFull: sigma 1024, a draw or the cap)
//     word 13        the edges of the pending path
//     word 14        1 once the root's arms have their P
//     word 15        the ply count of an EVALUATE leaf
//     words 16 .. 23 the four planes of an EVALUATE leaf: the application makes its arms again from them
//     words 32 ..    the E edges, four words each: n, s, child or sentinel (k_bounce_search's), P << 14 | source cell << 8 |
//                    target cell (P <= 65536 takes 17 bits, the move 14)
//     then           the C node-table entries (first edge, arms)
//     then           the C words of the pending path, edge indices: a descent leaves every node at most once
// Every word read back from the share is used only within its bounds: a path no longer than C, an edge below the edges
// in use, a child below the nodes in use, a node's block inside the edges in use, a slot below S.  Memory that passes the
// check by accident gives a wrong tree, never a store outside its own share or its own output rows.
//
// Ordering, all inside the one-wave workgroup.  Writers and readers of the tree:
//   the emptying (strided lanes write the root's arms, lane 0 the table entry) and the application (strided lanes write a
//   new node's arms or the root's P, lane 0 the table entry and the parent's child word, lane k edge k of the path)
//     -- barrier (T) --
//   the report (strided lanes read the root's arms) and the descent (strided lanes read a node's arms, every lane the
//   table entry and the chosen edge).  The descent writes only an edge's sentinel and the path, which nothing of this
//   launch reads afterwards; the header goes last, by lane 0, and is read by the next launch.
// Writers of a row of visits and scores: the lanes zero every slot, strided, and behind barrier (Z) the lanes that hold
// the root's arms store theirs.  (A memset by the entry point in front of the launch was two more enqueues a step: with
// them a step of 64 trees took 22.9 us, docs/EXPERIMENTS.md §42.)
// Writers and readers of node_targets: lane x writes word x, every lane reads every word; put() has a barrier on either
// side of its store.
// ================================================================================================================
constexpr uint32_t kBounceGuidedHeaderWords = 32;
constexpr uint32_t kGuidedMoveBits = 14, kGuidedMoveMask = (1u << kGuidedMoveBits) - 1u;
constexpr uint32_t kGuidedLaneArms = kBounceHalvingMaxArms / BGS_WAVE;
static_assert(kGuidedLaneArms * BGS_WAVE == kBounceHalvingMaxArms, "the lanes of a wave hold every arm of a node");
static_assert((65536ull << kGuidedMoveBits) + kGuidedMoveMask < (1ull << 32), "P and the move share a word");
static_assert((((uint64_t)BGS_GUIDED_MAX_VISITS + 1u) << 41) < (1ull << 63), "the key of `best` holds n above s above the arm");

// words of a tree's share: the header, the pool, the node table and the path, rounded up to 256 bytes (below 2^32)
__host__ __device__ __forceinline__ uint64_t bounce_guided_tree_words(uint32_t capacity, uint32_t edges) {
    return (kBounceGuidedHeaderWords + (uint64_t)edges * kEdgeWords + (uint64_t)capacity * 3u + 63u) & ~(uint64_t)63u;
}

__device__ __forceinline__ uint64_t wave_max64(uint64_t v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const uint64_t o = (uint64_t)__shfl_xor((unsigned long long)v, off, BGS_WAVE);
        v = o > v ? o : v;
    }
    return v;
}

template <class GEO, int NC>
__global__ void __launch_bounds__(BGS_WAVE)
k_bounce_search_guided(GEO g, const uint64_t* __restrict__ planes, const uint8_t* __restrict__ status, const uint16_t* __restrict__ plies_buf,
                       int64_t n, int64_t root_base, uint32_t capacity, uint32_t edges, uint32_t cpuct, uint32_t cap, uint32_t flags,
                       const float* __restrict__ priors, const float* __restrict__ values, int8_t* __restrict__ leaf_grid,
                       int8_t* __restrict__ leaf_player, int32_t* __restrict__ leaf_kind, uint64_t* __restrict__ leaf_targets,
                       int32_t* __restrict__ visits, int32_t* __restrict__ scores, int32_t* __restrict__ best, int32_t* __restrict__ nodes,
                       int32_t* __restrict__ used_out, uint32_t* trees) {
    __shared__ uint64_t node_targets[8 * NC];                      // targets of the piece in column x of the active row
    const uint32_t lane = threadIdx.x;
    const uint32_t width = (uint32_t)g.w, hw = (uint32_t)(g.h * g.w), slots = width * hw;
    const int64_t i = root_base + (int64_t)blockIdx.x;             // (the grid holds exactly the trees of this launch)
    uint32_t* const head = trees + (uint64_t)i * bounce_guided_tree_words(capacity, edges);
    uint64_t* const head_planes = reinterpret_cast<uint64_t*>(head + 4);
    uint64_t* const leaf_planes = reinterpret_cast<uint64_t*>(head + 16);
    uint32_t* const pool = head + kBounceGuidedHeaderWords;
    uint32_t* const node_tab = pool + (uint64_t)edges * kEdgeWords;             // node v: first edge, arms
    uint32_t* const path = node_tab + (uint64_t)capacity * 2u;                  // edge k of the pending descent
    const auto uniform = [](uint32_t x) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)x); };

    // lane x: the targets of `player`'s piece in column x of its active row on `bd`; base: the cell of column 0 of that row
    const auto spread = [&](const Board& bd, uint64_t occ, uint32_t player, bool live, uint32_t& base) {
        const uint64_t sources = live ? movable(g, occ, player) : 0ull;
        const uint32_t first_source = sources ? (uint32_t)(__ffsll((unsigned long long)sources) - 1) : 0u;
        base = ((first_source * g.inv_w) >> 16) * (uint32_t)g.w;
        const bool piece = lane < width && ((sources >> ((base + lane) & 63u)) & 1ull);
        return piece ? reach(g, bd, occ, player, (int)(base + lane)) : 0ull;
    };
    // the lanes' masks into node_targets, for arm_move; returns the arms (uniform)
    const auto put = [&](uint64_t mask) {
        __syncthreads();
        if (lane < 8 * NC) node_targets[lane] = mask;
        __syncthreads();
        return uniform(wave_sum((uint32_t)__popcll(mask)));
    };
    // arm a (canonical order, a < the arms put) of the position in node_targets: its move word and its slot
    const auto arm_move = [&](uint32_t a, uint32_t base, uint32_t& slot) {
        uint32_t j = a, x = 0;
        for (; x < 8 * NC - 1; ++x) {
            const uint32_t cnt = (uint32_t)__popcll(node_targets[x]);
            if (j < cnt) break;
            j -= cnt;
        }
        const uint32_t cell = select_bit64(node_targets[x], j);
        slot = x * hw + cell;
        return ((base + x) << 8) | cell;
    };

    // ---- the root: its arms say whether there is anything to search (an ended root and one that holds the most plies a
    // board can have none, as in k_bounce_search)
    const Board root = load_board(planes, n, i);
    const uint32_t rply = plies_buf[i];
    uint32_t root_cell = 0;
    const uint64_t root_mask = spread(root, occupancy(root), rply & 1u, status[i] == BGS_ST_RUNNING && rply < kBounceMaxPlies, root_cell);
    uint32_t root_arms = put(root_mask);
    root_arms = root_arms <= edges ? root_arms : 0u;               // (never: E >= BGS_BOUNCE_SEARCH_MIN_EDGES)

    // ---- 1. the check (wave-uniform: every lane reads the same header); a tree that fails it is emptied
    uint32_t count = uniform(head[0]), used = uniform(head[1]), kind = uniform(head[12]), depth = uniform(head[13]);
    uint32_t expanded = uniform(head[14]);
    bool live = (flags & BGS_GUIDED_RESTART) == 0u && root_arms != 0u && count >= 1u && count <= capacity && used >= root_arms &&
                used <= edges && head[2] == rply && head[3] == cap;
    if (live) {
#pragma unroll
        for (int j = 0; j < 4; ++j) live = live && head_planes[j] == root.v[j];
    }
    live = uniform(live ? 1u : 0u) != 0u;
    if (!live) {                        // node 0 and its arms, no P yet; board i recorded
        kind = kGuidedNone;
        depth = 0;
        expanded = 0;
        count = root_arms ? 1u : 0u;
        used = root_arms;
        for (uint32_t a = lane; a < root_arms; a += BGS_WAVE) {
            uint32_t slot;
            const uint32_t move = arm_move(a, root_cell, slot);
            *reinterpret_cast<uint4*>(pool + (uint64_t)a * kEdgeWords) = make_uint4(0u, 0u, 0u, move);
        }
        if (root_arms != 0u && lane == 0) {
            node_tab[0] = 0u;
            node_tab[1] = root_arms;
            head[2] = rply;
            head[3] = cap;
#pragma unroll
            for (int j = 0; j < 4; ++j) head_planes[j] = root.v[j];
        }
    }
    depth = depth < capacity ? depth : capacity;

    // ---- 2. the application of the pending evaluation
    if (kind != kGuidedNone) {
        uint32_t sigma = kind == kGuidedWon ? 0u : 1024u;         // the leaf's value for its mover, 0 .. 2048
        if (kind == kGuidedEvaluate) {
            const float x = values[i];
            int32_t v = 0;
            if (x == x) v = (int32_t)(fminf(fmaxf(x, -1.0f), 1.0f) * 1024.0f);
            sigma = (uint32_t)(1024 + v);
            // the leaf's arms again: the root's are in node_targets, any other leaf's come from its recorded planes
            uint32_t arms = root_arms, base = root_cell;
            if (depth != 0u) {
                Board lp;
#pragma unroll
                for (int j = 0; j < 4; ++j) lp.v[j] = leaf_planes[j];
                arms = put(spread(lp, occupancy(lp), head[15] & 1u, true, base));
                arms = arms < kBounceHalvingMaxArms ? arms : kBounceHalvingMaxArms;
            }
            // the priors of the leaf's arms, arm lane + 64 k by lane: 16-bit weights, then 16-bit shares
            uint32_t move[kGuidedLaneArms], weight[kGuidedLaneArms], sum = 0;
#pragma unroll
            for (uint32_t k = 0; k < kGuidedLaneArms; ++k) {
                const uint32_t a = lane + k * BGS_WAVE;
                move[k] = weight[k] = 0;
                if (k * BGS_WAVE < arms && a < arms) {
                    uint32_t slot;
                    move[k] = arm_move(a, base, slot);
                    const float pr = priors[i * (int64_t)slots + slot];
                    if (pr > 0.0f) weight[k] = (uint32_t)(fminf(pr, 1.0f) * 65536.0f);
                    sum += weight[k];
                }
            }
            sum = uniform(wave_sum(sum));
            const bool flat = sum == 0u;                           // no weight on a legal slot: equal shares
            sum = flat ? arms : sum;
            uint32_t first = 0;
            bool place = false, fresh = false;
            if (depth == 0u) {                                     // the root is the leaf: it only receives P
                place = true;
                expanded = 1u;
            } else {            // a node is made if the edge has no child, the table has room and the pool has the arms
                const uint32_t e = uniform(path[depth - 1u]);
                const uint32_t child = e < used ? uniform(pool[(uint64_t)e * kEdgeWords + 2u]) : 1u;
                if (child == 0u && arms != 0u && count < capacity && used + arms <= edges) {
                    place = fresh = true;
                    first = used;
                    if (lane == 0) {
                        node_tab[2u * count] = used;
                        node_tab[2u * count + 1u] = arms;
                        pool[(uint64_t)e * kEdgeWords + 2u] = count;
                    }
                    count += 1u;
                    used += arms;
                }
            }
            if (place) {
#pragma unroll
                for (uint32_t k = 0; k < kGuidedLaneArms; ++k) {
                    const uint32_t a = lane + k * BGS_WAVE;
                    if (k * BGS_WAVE < arms && a < arms) {
                        const uint32_t share = guided_quotient((uint64_t)(flat ? 1u : weight[k]) << 16, sum);
                        const uint32_t word = (share << kGuidedMoveBits) | move[k];
                        uint32_t* const edge = pool + (uint64_t)(first + a) * kEdgeWords;
                        if (fresh) *reinterpret_cast<uint4*>(edge) = make_uint4(0u, 0u, 0u, word);
                        else edge[3] = word;
                    }
                }
            }
        }
        // lane k takes edge k of the path: node k's mover is the leaf's when depth - k is even
        for (uint32_t k = lane; k < depth; k += BGS_WAVE) {
            const uint32_t e = path[k];
            if (e < used) {
                uint32_t* const edge = pool + (uint64_t)e * kEdgeWords;
                edge[0] += 1u;
                edge[1] += ((depth - k) & 1u) ? 2048u - sigma : sigma;
            }
        }
        kind = kGuidedNone;
        depth = 0;
    }
    __syncthreads();                // (T) the tree is whole: the report and the descent read what other lanes wrote

    // ---- 3. the report: every slot of the row is zeroed, coalesced, and behind barrier (Z) the lanes that hold the root's
    // arms store theirs -- a slot has two writers, and the barrier stands between them; the root's block starts at edge 0
    const auto slot_of = [&](uint32_t word) { return (((word & kGuidedMoveMask) >> 8) - root_cell) * hw + (word & 255u); };
    for (uint32_t s = lane; s < slots; s += BGS_WAVE) {
        if (visits) visits[i * (int64_t)slots + s] = 0;
        if (scores) scores[i * (int64_t)slots + s] = 0;
    }
    __syncthreads();                // (Z)
    uint32_t root_total = 0;
    {
        uint64_t key = 0;           // n << 41 | s << 9 | 511 - arm: the most visits, then the larger s, then the lower slot
        if (count != 0u) {
            for (uint32_t a = lane; a < root_arms; a += BGS_WAVE) {
                const uint4 edge = *reinterpret_cast<const uint4*>(pool + (uint64_t)a * kEdgeWords);
                const uint32_t slot = slot_of(edge.w);
                if (slot < slots) {
                    if (visits) visits[i * (int64_t)slots + slot] = (int32_t)edge.x;
                    if (scores) scores[i * (int64_t)slots + slot] = (int32_t)edge.y;
                }
                root_total += edge.x;
                const uint64_t mine = ((uint64_t)edge.x << 41) | ((uint64_t)edge.y << 9) | (uint64_t)(511u - a);
                key = (edge.x != 0u && mine > key) ? mine : key;
            }
        }
        key = wave_max64(key);
        root_total = uniform(wave_sum(root_total));
        if (lane == 0) {
            if (best) best[i] = key ? (int32_t)slot_of(pool[(uint64_t)(511u - ((uint32_t)key & 511u)) * kEdgeWords + 3u]) : -1;
            if (nodes) nodes[i] = (int32_t)(count ? count - 1u : 0u);
            if (used_out) used_out[i] = (int32_t)used;
        }
    }

    // ---- 4. the selection (wave-uniform): p is the position at node v, and the leaf's at the end
    Board p = root;
    uint32_t ply = rply, out_kind = (uint32_t)BGS_GUIDED_IDLE;
    uint64_t leaf_mask = 0;             // lane x: the targets of the piece in column x of an EVALUATE leaf's active row
    if (count != 0u && (flags & BGS_GUIDED_FINISH) == 0u && root_total < (uint32_t)BGS_GUIDED_MAX_VISITS) {
        if (expanded == 0u) {                                          // an unexpanded root is itself the leaf
            leaf_mask = root_mask;
            kind = kGuidedEvaluate;
            out_kind = (uint32_t)BGS_GUIDED_EVALUATE;
        } else {
            uint32_t v = 0;
            while (depth < capacity) {                                 // (always: a descent leaves every node at most once)
                const uint32_t first = uniform(node_tab[2u * v]);
                uint32_t arms = uniform(node_tab[2u * v + 1u]);
                if (first > used || arms > used - first || arms == 0u) break;   // (never: a node's block lies inside the edges in use)
                arms = arms < kBounceHalvingMaxArms ? arms : kBounceHalvingMaxArms;
                const uint32_t* const node = pool + (uint64_t)first * kEdgeWords;
                uint32_t na[kGuidedLaneArms], sa[kGuidedLaneArms], pa[kGuidedLaneArms], total = 0;
#pragma unroll
                for (uint32_t k = 0; k < kGuidedLaneArms; ++k) {
                    const uint32_t a = lane + k * BGS_WAVE;
                    na[k] = sa[k] = pa[k] = 0;
                    if (k * BGS_WAVE < arms && a < arms) {
                        const uint4 edge = *reinterpret_cast<const uint4*>(node + (uint64_t)a * kEdgeWords);
                        na[k] = edge.x;
                        sa[k] = edge.y;
                        pa[k] = edge.w >> kGuidedMoveBits;
                        total += edge.x;
                    }
                }
                total = uniform(wave_sum(total));
                // (a node's N is at most the root's, which the selection bounds: the clamp changes no tree and keeps (N + 1) << 12
                // in 32 bits whatever the memory held)
                total = total < (uint32_t)BGS_GUIDED_MAX_VISITS ? total : (uint32_t)BGS_GUIDED_MAX_VISITS;
                const uint32_t sqrt_n = search_isqrt((total + 1u) << 12);
                uint64_t key = 0;                                      // (U(a) << 9 | 511 - a) + 1: the largest U, then the lowest arm
#pragma unroll
                for (uint32_t k = 0; k < kGuidedLaneArms; ++k) {
                    const uint32_t a = lane + k * BGS_WAVE;
                    if (k * BGS_WAVE < arms && a < arms) {
                        const uint32_t q = na[k] ? (2u * sa[k]) / na[k] : 2048u;
                        const uint32_t e = (uint32_t)(((uint64_t)(cpuct * pa[k]) * sqrt_n) >> 19) / (1u + na[k]);
                        const uint64_t mine = (((uint64_t)q + e) << 9 | (uint64_t)(511u - a)) + 1u;
                        key = mine > key ? mine : key;
                    }
                }
                key = wave_max64(key);
                const uint32_t arm = uniform(511u - ((uint32_t)(key - 1u) & 511u));
                const uint32_t e = first + arm;                        // (arm < arms: below the edges in use)
                uint32_t* const edge = pool + (uint64_t)e * kEdgeWords;
                const uint32_t child = uniform(edge[2]), word = uniform(edge[3]);
                if (lane == 0) path[depth] = e;
                const int s_cell = (int)((word >> 8) & 63u), t_cell = (int)(word & 63u);
                const uint32_t mover = ply & 1u;
                move_piece(p, s_cell, t_cell);
                ply += 1u;
                depth += 1u;
                out_kind = (uint32_t)BGS_GUIDED_TERMINAL;
                if (child == kEdgeCapped) {                            // p' runs and holds the cap
                    kind = kGuidedFull;
                    break;
                }
                if (child >= kEdgeEnded) {                             // the edge ends the game: its mover won, or a draw
                    kind = (child & 15u) == (uint32_t)BGS_ST_DRAW ? kGuidedFull : kGuidedWon;
                    break;
                }
                if (child != 0u && child < count) {
                    out_kind = (uint32_t)BGS_GUIDED_IDLE;
                    v = child;
                    continue;
                }
                // ---- the edge has no child: what p' is
                uint32_t code = 0;                                     // the edge's new third word, if any
                if ((1ull << t_cell) & (g.goal_top | g.goal_bottom)) {
                    kind = kGuidedWon;
                    code = kEdgeEnded | (mover + 1u);
                } else {
                    const uint64_t occ = occupancy(p);
                    uint32_t base;
                    leaf_mask = spread(p, occ, ply & 1u, true, base);
                    if (__builtin_amdgcn_ballot_w64(leaf_mask != 0ull) == 0) {   // the side to move is blocked: the mover wins if it could move
                        const bool could = __builtin_amdgcn_ballot_w64(spread(p, occ, mover, true, base) != 0ull) != 0;
                        kind = could ? kGuidedWon : kGuidedFull;
                        code = kEdgeEnded | (could ? mover + 1u : (uint32_t)BGS_ST_DRAW);
                    } else if (ply >= cap) {                           // no node, now or later
                        kind = kGuidedFull;
                        code = kEdgeCapped;
                    } else {                                           // the caller evaluates p'
                        kind = kGuidedEvaluate;
                        out_kind = (uint32_t)BGS_GUIDED_EVALUATE;
                    }
                }
                if (lane == 0 && code) edge[2] = code;
                break;
            }
            if (out_kind == (uint32_t)BGS_GUIDED_IDLE) {               // (never: the descent left the tree's bounds; nothing is pending)
                p = root;
                ply = rply;
                depth = 0;
                kind = kGuidedNone;
            }
        }
    }

    // ---- the leaf goes out (an idle tree shows its root), in the encoding of bgs_read_grid: the piece values by cell
    int8_t* const cells = leaf_grid + i * (int64_t)hw;
    for (uint32_t j = lane; j < hw; j += BGS_WAVE) cells[j] = (int8_t)value_at(p, (int)j);
    if (leaf_targets && lane < width) leaf_targets[i * (int64_t)width + lane] = out_kind == (uint32_t)BGS_GUIDED_EVALUATE ? leaf_mask : 0ull;
    if (lane == 0) {
        leaf_player[i] = (int8_t)(ply & 1u);
        leaf_kind[i] = (int32_t)out_kind;
        head[0] = count;            // the header: ply, cap and planes were recorded when the tree was emptied
        head[1] = used;
        head[12] = kind;
        head[13] = depth;
        head[14] = expanded;
        head[15] = ply;
#pragma unroll
        for (int j = 0; j < 4; ++j) leaf_planes[j] = p.v[j];
    }
}

}  // namespace

uint64_t bounce_guided_tree_bytes(int32_t capacity, int32_t edges) {
    return bounce_guided_tree_words((uint32_t)capacity, (uint32_t)edges) * sizeof(uint32_t);
}

void bounce_guided_step(const bgs_batch* b, int32_t capacity, int32_t edges, int32_t cpuct, int32_t max_plies, uint32_t flags,
                        const float* d_priors, const float* d_values, int8_t* d_leaf_grid, int8_t* d_leaf_player, int32_t* d_leaf_kind,
                        uint64_t* d_leaf_targets, int32_t* d_visits, int32_t* d_scores, int32_t* d_best, int32_t* d_nodes, int32_t* d_used,
                        void* d_trees) {
    const uint32_t cap = (uint32_t)max_plies > kBounceMaxPlies ? kBounceMaxPlies : (uint32_t)max_plies;   // plies are stored as uint16
    // (the kernel zeroes the rows of visits and scores itself: one enqueue a step, not three)
    with_bounce_geom(b, [&](const auto& g, auto nc) {
        constexpr int64_t kMaxBlocks = (int64_t)1 << 30;
        for (int64_t i0 = 0; i0 < b->n; i0 += kMaxBlocks) {
            const int64_t blocks = b->n - i0 < kMaxBlocks ? b->n - i0 : kMaxBlocks;
            hipLaunchKernelGGL((k_bounce_search_guided<std::decay_t<decltype(g)>, decltype(nc)::value>), dim3((uint32_t)blocks),
                               dim3(BGS_WAVE), 0, b->stream, g, (const uint64_t*)b->d_planes, (const uint8_t*)b->d_status,
                               (const uint16_t*)b->d_plies, b->n, i0, (uint32_t)capacity, (uint32_t)edges, (uint32_t)cpuct, cap, flags,
                               d_priors, d_values, d_leaf_grid, d_leaf_player, d_leaf_kind, d_leaf_targets, d_visits, d_scores, d_best,
                               d_nodes, d_used, static_cast<uint32_t*>(d_trees));
        }
    });
}

uint64_t bounce_search_root_bytes(int32_t iterations, int32_t edges) {
    return bounce_search_root_words((uint32_t)iterations, (uint32_t)edges) * sizeof(uint32_t);
}

template <bool FOREST, bool PROVE = false>
static void bounce_search_any(const bgs_batch* b, int policy, BounceSearchArgs a) {
    if (a.max_plies > kBounceMaxPlies) a.max_plies = kBounceMaxPlies;   // plies are stored as uint16
    with_policy(policy, [&](auto pol) {
        with_bounce_geom(b, [&](const auto& g, auto nc) {
            launch_bounce_search<std::decay_t<decltype(g)>, decltype(nc)::value, decltype(pol)::value, FOREST, PROVE>(b, g, a);
        });
    });
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

uint64_t connect_search_root_bytes(int width, int32_t iterations) {
    return search_root_words((uint32_t)width, (uint32_t)iterations) * sizeof(uint32_t);
}

template <bool FOREST, bool PROVE = false>
static void search_any(const bgs_batch* b, int policy, const ConnectSearchArgs& a) {
    const EvalGeom g = eval_geom(b);
    with_connect_form(b, policy, [&](auto nw, auto per_ply, auto pol) {
        launch_search<decltype(nw)::value, decltype(per_ply)::value, decltype(pol)::value, FOREST, PROVE>(b, g, a);
    });
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

uint64_t connect_guided_tree_bytes(int height, int width, int32_t capacity) {
    return guided_tree_words((uint32_t)height, (uint32_t)width, (uint32_t)capacity) * sizeof(uint32_t);
}

template <int NW>
static void launch_guided(const bgs_batch* b, const EvalGeom& g, int32_t capacity, int32_t cpuct, uint32_t flags, const float* d_priors,
                          const float* d_values, int8_t* d_leaf_grid, int8_t* d_leaf_player, int32_t* d_leaf_kind, int32_t* d_visits,
                          int32_t* d_scores, int32_t* d_best, int32_t* d_nodes, void* d_trees) {
    constexpr int64_t kMaxBlocks = (int64_t)1 << 30;
    for (int64_t i0 = 0; i0 < b->n; i0 += kMaxBlocks) {
        const int64_t blocks = b->n - i0 < kMaxBlocks ? b->n - i0 : kMaxBlocks;
        hipLaunchKernelGGL((k_connect_search_guided<NW>), dim3((uint32_t)blocks), dim3(BGS_WAVE), 0, b->stream, g,
                           (const uint64_t*)b->d_planes, (const uint8_t*)b->d_status, b->n, i0, (uint32_t)capacity, (uint32_t)cpuct,
                           flags, d_priors, d_values, d_leaf_grid, d_leaf_player, d_leaf_kind, d_visits, d_scores, d_best, d_nodes,
                           static_cast<uint32_t*>(d_trees));
    }
}

void connect_guided_step(const bgs_batch* b, int32_t capacity, int32_t cpuct, uint32_t flags, const float* d_priors,
                         const float* d_values, int8_t* d_leaf_grid, int8_t* d_leaf_player, int32_t* d_leaf_kind, int32_t* d_visits,
                         int32_t* d_scores, int32_t* d_best, int32_t* d_nodes, void* d_trees) {
    const EvalGeom g = eval_geom(b);
    const auto launch = [&](auto nw) {
        launch_guided<decltype(nw)::value>(b, g, capacity, cpuct, flags, d_priors, d_values, d_leaf_grid, d_leaf_player, d_leaf_kind,
                                           d_visits, d_scores, d_best, d_nodes, d_trees);
    };
    switch (b->cg.nw) {             // the words of a plane, as with_connect_form: no RNG contract and no policy here
        case 1: launch(std::integral_constant<int, 1>{}); break;
        case 2: launch(std::integral_constant<int, 2>{}); break;
        default: launch(std::integral_constant<int, 3>{}); break;
    }
}

void connect_guided_advance(const bgs_batch* b, const int32_t* d_columns, int32_t capacity, int32_t* d_kept, void* d_trees) {
    const uint32_t width = (uint32_t)b->cg.w, room = (uint32_t)capacity;
    // LDS: as connect_forest_advance, with nodes of 4 * width words
    const uint32_t mask_room = (((room + 31u) >> 5) + 3u) & ~3u;
    const size_t lds = ((size_t)2 * mask_room + (size_t)64 * width * 4u) * sizeof(uint32_t);
    constexpr int64_t kMaxBlocks = (int64_t)1 << 30;
    for (int64_t i0 = 0; i0 < b->n; i0 += kMaxBlocks) {
        const int64_t blocks = b->n - i0 < kMaxBlocks ? b->n - i0 : kMaxBlocks;
        hipLaunchKernelGGL(k_connect_guided_advance, dim3((uint32_t)blocks), dim3(BGS_WAVE), lds, b->stream, (uint32_t)b->cg.h, width,
                           (uint32_t)b->cg.nw, d_columns, room, static_cast<uint32_t*>(d_trees), d_kept, i0);
    }
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
