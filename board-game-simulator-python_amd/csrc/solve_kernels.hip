// solve_kernels.hip -- the exact solvers: Connect (bgs_connect_solve_actions: per-column win / draw / loss by a
// depth-first alpha-beta search, k_connect_solve) in the first half of this file, Bounce (bgs_bounce_solve_moves: the
// horizon search per move, k_bounce_solve) in the second.  The section comments below describe each.
//
// A unit of its own (bgs_kernel_unit_id(5)).  The Connect solver's threat map is playout.h's, shared with the evaluation and the
// search units; the count and scan of the Bounce roots' legal moves are bounce_root_moves.h's, shared with the evaluation.
#include "bounce_root_moves.h"
#include "playout.h"

#ifndef BGS_TU_ID
#define BGS_TU_ID "unknown"
#endif
extern "C" const char bgs_tu_id_solve[] = BGS_TU_ID;

namespace bgs {
namespace {

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
// Shape.  The counting pass of the evaluation (k_bounce_eval_count of bounce_root_moves.h, here without the ply cap) numbers the LEGAL (board,
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
    launch_bounce_root_moves<false>(b, g, d_ends, d_totals);
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

void connect_solve(const bgs_batch* b, int32_t depth, int64_t max_nodes, int8_t* d_codes, int16_t* d_plies,
                   unsigned long long* d_nodes) {
    const EvalGeom g = eval_geom(b);
    switch (b->cg.nw) {
        case 1: launch_solve<1>(b, g, depth, max_nodes, d_codes, d_plies, d_nodes); break;
        case 2: launch_solve<2>(b, g, depth, max_nodes, d_codes, d_plies, d_nodes); break;
        default: launch_solve<3>(b, g, depth, max_nodes, d_codes, d_plies, d_nodes); break;
    }
}

}  // namespace bgs
