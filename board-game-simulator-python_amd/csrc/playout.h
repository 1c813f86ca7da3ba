// playout.h -- what more than one of the three analysis units uses: the evaluation unit (evaluate_kernels.hip: flat
// Monte-Carlo evaluation and sequential halving), the search unit (search_kernels.hip: the UCT tree searches) and the
// solve unit (solve_kernels.hip: the exact solvers).  The Makefile hashes this header into the ids of all three.
//
// Connect: the geometry record the kernels take by value (EvalGeom), the stone drop with and without its win test, the
// draw of a landing cell, the threat map, the ply of BGS_POLICY_DECISIVE and the 4-ply playout block of the tree searches.
// Bounce: the W/D/L count (Connect's kernels count with it too), the playout ply of the flat evaluation and the tree
// searches, and the most arms a root can have.  Last, the host's
// choice of instantiation, once a game.  Everything else lives with its only user (the first pass of the Bounce
// evaluation and solver, which the search does not need: bounce_root_moves.h).
#pragma once
#include <type_traits>

#include "../../include/bgs.h"
#include "bgs_common.h"
#include "bgs_internal.h"
#include "bounce_board.h"
#include "connect_board.h"

namespace bgs {
namespace {

// ---- Connect
struct EvalGeom {
    int rh, rw, rk;
    __host__ __device__ __forceinline__ int h() const { return rh; }
    __host__ __device__ __forceinline__ int w() const { return rw; }
    __host__ __device__ __forceinline__ int k() const { return rk; }
    uint32_t cells_total;          // h * w: a board with this many stones is full
    uint64_t bottoms[BGS_CONNECT_MAX_WORDS];   // the bottom cell of every column
    uint64_t cells[BGS_CONNECT_MAX_WORDS];     // every real cell (no sentinels)
};

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

// The Connect playout step of the tree searches (k_connect_search: plain, forest, proving); k_connect_evaluate and
// k_connect_evaluate_halving play the same block from copies of their own, which say why.  The wave plays one 4-ply
// block of every lane's game.  A lane's game is its kernel's own locals, taken by reference: the stones p[0] / p[1] of
// player 0 / 1, the global game id, the block `blk` the game stands in, the plies of that block already on
// the board (`skip`), the flags `live` (all ones: the lane holds a running game) and `fresh` (the game is new: ph holds
// nothing of it), and the status st.  A lane that takes a new game at `ply` stones sets blk = ply >> 2, skip = ply & 3,
// live = ~0u, fresh = 1 and st = 0.
//   * The block's draws, DESIGN.md §3 ("RNG contract") at the game's absolute ply 4 * blk + j.  PER_PLY (the strict
//     contract): word j of philox4x32_10(seed, game, blk), one call a block.  The default contract: sub-draw j of word
//     blk & 3 of philox4x32_10(seed, game, blk >> 2) -- the call serves four blocks, so a lane makes one at a 16-ply
//     boundary or for a new game only.
//   * Four plies, player j & 1 to move at sub-step j; the first `skip` of a new game's block are on the board already and
//     drop nothing.  BGS_POLICY_UNIFORM: a uniformly drawn landing cell and the win test.  BGS_POLICY_DECISIVE:
//     decisive_position, which says itself whether its stone wins.
//   * A game ends by a win, on the full board or at the cap of max_plies stones; `live` is then 0 and st says how (1 / 2
//     the winner + 1, BGS_ST_DRAW, or 0 = BGS_ST_RUNNING at the cap: counted nowhere).
// Returns "this lane's game has just finished".  What a kernel does with a finished game is all the kernels differ in
// here, and stays in the kernel.  `stepped` grows by the plies the lane played.
template <int NW, bool PER_PLY, int POLICY>
__device__ __forceinline__ bool connect_playout_block(const EvalGeom& g, uint64_t seed, uint32_t max_plies, Bits<NW> (&p)[2],
                                                      uint64_t game, uint32_t& blk, uint32_t& skip, uint32_t& live, uint32_t& st,
                                                      uint32_t& fresh, Philox4& ph, uint32_t& stepped) {
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
    return was_live && !live;
}

// ---- Bounce
constexpr uint32_t kBounceMaxPlies = 65535u;      // plies are uint16 (the Bounce unit's kMaxPlies)

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

// ---- the host's choice of instantiation.  `f` is a generic lambda; a choice reaches it as a std::integral_constant or a
// std::bool_constant, so `decltype(nw)::value` and the like are constant expressions in its body.
template <class F>
void with_policy(int policy, F&& f) {
    if (policy == BGS_POLICY_DECISIVE) f(std::integral_constant<int, BGS_POLICY_DECISIVE>{});
    else f(std::integral_constant<int, BGS_POLICY_UNIFORM>{});
}

// Connect: f(nw, per_ply, policy) -- the words of a plane (1, 2, else 3), the batch's RNG contract, the playout policy
template <class F>
void with_connect_form(const bgs_batch* b, int policy, F&& f) {
    auto by_rng = [&](auto nw) {
        with_policy(policy, [&](auto pol) {
            if (b->rng_per_ply) f(nw, std::true_type{}, pol);
            else f(nw, std::false_type{}, pol);
        });
    };
    switch (b->cg.nw) {
        case 1: by_rng(std::integral_constant<int, 1>{}); break;
        case 2: by_rng(std::integral_constant<int, 2>{}); break;
        default: by_rng(std::integral_constant<int, 3>{}); break;
    }
}

// Bounce: f(g, nc) -- the compile-time geometry of the default grid, else the batch's own; nc = the NC of the move lists
// (FlatMoves<NC>, bounce_board.h: 1 up to 8 columns, else 3)
template <class F>
void with_bounce_geom(const bgs_batch* b, F&& f) {
    if (b->bounce_static_geom && bounce_is_default(b->bg)) f(DefaultBounceGeom{}, std::integral_constant<int, 1>{});
    else if (b->bg.w <= 8) f(b->bg, std::integral_constant<int, 1>{});
    else f(b->bg, std::integral_constant<int, 3>{});
}

}  // namespace
}  // namespace bgs
