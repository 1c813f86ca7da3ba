/*
 * bgs.h -- C ABI of libbgs.so, the MI355X (gfx950) batched board-game rollout engine.
 *
 * This is the drop-in boundary for the ONE hot path of jojolebarjos/board-game-simulator-python:
 *   legal-move enumeration -> uniform action sampling -> sample_next_state transition -> terminal + reward,
 * for N independent boards per launch.  Every entry point names the reference binding it replaces
 * (paths relative to the reference tree, src/simulator/game/...).  The reference itself has no batched API,
 * no RNG and no device; "batch", "seed" and "device" are this library's concepts.
 *
 * Conventions
 *   - plain C types only; no C++ or torch types cross this boundary;
 *   - every function returns BGS_OK (0) or a negative bgs_status; bgs_last_error() gives a thread-local
 *     message.  The reference raises C++ exceptions that nanobind turns into RuntimeError
 *     (textual/connect.py:115-118, textual/bounce.py:119-128): the Python shim maps BGS_ERR_ILLEGAL and
 *     BGS_ERR_RUNTIME to RuntimeError and BGS_ERR_ARG to TypeError/ValueError;
 *   - host arrays are C-contiguous, reference layout: grid int8[n][height][width], row 0 = bottom row
 *     (tensor.hpp:29-34; tests/test_connect.py:24-25); the caller owns every buffer it passes
 *     (the reference copies both ways too: tensor.hpp:63,80-84);
 *   - a batch lives on ONE device; all work is enqueued on the batch's HIP stream (default: the null
 *     stream); functions that fill host memory synchronise that stream before returning;
 *   - winner codes: -1 running, 0 / 1 that player won, 2 draw.  reward = +1 / -1 per player, 0 / 0 otherwise.
 *
 * RNG contract (build-defined: the reference has no RNG, its callers use random.choice, README.md:62).  A draw is a
 * 32-bit value, the sampled action is index (draw * n_actions) >> 32 of the canonical action list (Connect: legal columns
 * ascending; Bounce: sources by ascending x, targets by ascending (y, x)); philox = philox4x32-10 with key = seed.
 *   Bounce : draw(seed, game, ply) = philox(counter = (game lo, game hi, ply >> 2, 0))[ply & 3] -- a word per ply.
 *   Connect: word(seed, game, ply) = philox(counter = (game lo, game hi, ply >> 4, 0))[(ply >> 2) & 3] -- a word per block
 *            of four plies -- and draw = word * A^(ply & 3) mod 2^32, A = 747796405: the four draws of a block are four
 *            consecutive states of the multiplicative congruential generator x -> A x mod 2^32 started at the word.  Every
 *            one of them is a bijection of the word, so each ply's index is distributed exactly as a word of its own would
 *            make it (bias <= n / 2^32); the four plies of a block share 32 bits of entropy, and counted over ALL 2^32 words
 *            every four-move sequence of a 7-column board comes within 4.2 x 10^-5 (relative) of 1 / 7^4 and every pair of
 *            plies within 4 x 10^-7 of 1 / 49 (13 columns: 2.9 x 10^-4, 16 columns: 4.3 x 10^-4; tools/subdraw_lattice.c).
 *            Different blocks use different philox words.  (Round 5; until then Connect drew a word per ply too.  One philox
 *            call now serves sixteen plies, and the bench kernel's ply loop holds none: DESIGN.md section 3.)
 *   Connect, strict contract (round 6; bgs_set_rng_contract(b, BGS_RNG_PER_PLY) or BGS_ROLLOUT_DRAW_PER_PLY): exactly
 *            Bounce's rule -- a philox word per ply.  The word-per-block contract stays the default; both are pinned by the
 *            oracle (oracle/bgs_oracle.h: ORC_RNG_PER_BLOCK / ORC_RNG_PER_PLY) and by the -m gpu parity tests.
 * `game` = first_game + index in batch, so results do not depend on sharding, launch geometry or kernel family.
 */
#ifndef BGS_H
#define BGS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* libbgs.so is built with -fvisibility=hidden and a linker version script (csrc/bgs.map): the functions this header
 * declares are the whole dynamic symbol table of the library (tests/test_abi_and_host.py compares `nm -D` with it). */
#if defined(__GNUC__) || defined(__clang__)
#define BGS_API __attribute__((visibility("default")))
#else
#define BGS_API
#endif

typedef struct bgs_batch bgs_batch; /* opaque: N boards of one game configuration on one device */

typedef enum bgs_status {
    BGS_OK = 0,
    BGS_ERR_ARG = -1,         /* bad argument / unsupported geometry */
    BGS_ERR_ILLEGAL = -2,     /* illegal move (per-board code in status arrays) */
    BGS_ERR_RUNTIME = -3,     /* HIP runtime error */
    BGS_ERR_NO_DEVICE = -4    /* no usable GPU: the product path has no CPU fallback */
} bgs_status;

typedef enum bgs_buffer_id {
    BGS_BUF_PLANES = 0,  /* uint64 [planes][n]  bit-packed boards, one plane contiguous over the batch */
    BGS_BUF_STATUS = 1,  /* uint8  [n]          0 running, 1 / 2 player 0 / 1 won, 3 draw */
    BGS_BUF_PLIES = 2,   /* uint16 [n]          plies played (Bounce only; Connect derives it from the planes) */
    BGS_BUF_REWARD = 3,  /* int8   [n][2]       reward per player, valid after a board ended (else 0) */
    BGS_BUF_STEPS = 4,   /* uint64 [2048]       sharded env-step counter: the SUM of all words is the count */
    BGS_BUF_STAGING = 5  /* scratch the read/write entry points unpack through */
} bgs_buffer_id;

/* rollout flags */
#define BGS_ROLLOUT_DEFAULT 0u
#define BGS_ROLLOUT_FROM_INITIAL 1u /* ignore the stored boards: every game starts from Config.sample_initial_state() */
#define BGS_ROLLOUT_DRAW_PER_PLY 4u /* Connect: this call draws under the strict RNG contract (BGS_RNG_PER_PLY below) */

/* RNG contracts of a Connect batch (bgs_set_rng_contract; Bounce draws a word per ply under either) */
#define BGS_RNG_PER_BLOCK 0 /* default: a philox word per block of four plies, the plies' draws its sub-draws (see above) */
#define BGS_RNG_PER_PLY 1   /* strict: a philox word per ply -- draw(seed, game, ply) = philox(counter = (game lo, game hi,
                             * ply >> 2, 0))[ply & 3], exactly Bounce's: one independent uniform choice per ply, what a
                             * caller of the reference gets from random.choice (README.md:62).  Costs the rollout kernels a
                             * philox call per four plies instead of per sixteen (bench.py --rng per-ply prints both rates). */

/* ---- library ------------------------------------------------------------------------------------ */
BGS_API int bgs_version(void);
BGS_API const char* bgs_last_error(void);
BGS_API int bgs_device_count(int* count);
/* identity of the kernels this library was LINKED with (16 hex digits): every kernel translation unit embeds the hash of
 * its own source, the kernel headers and the compile flags when it is compiled, and this folds the six.  Measurement
 * files under profiles/ carry the id of the build they were taken on, and bench.py refuses to quote instruction counts
 * of another build.  `make -C csrc print-id` gives the id the sources in the tree would produce. */
BGS_API const char* bgs_build_id(void);
/* the id one kernel unit was compiled with: 0 connect_kernels, 1 bounce_kernels, 2 generic_kernels, 3 evaluate_kernels,
 * 4 search_kernels, 5 solve_kernels; NULL otherwise */
BGS_API const char* bgs_kernel_unit_id(int unit);

/* ---- configuration + batch lifetime ------------------------------------------------------------- */
/* replaces connect::Config(height, width, count) + Config::sample_initial_state (connect.cpp:26,32), N at a time.
 * arena: optional caller-owned device memory of at least bgs_connect_arena_bytes() bytes (256-byte aligned),
 * e.g. a torch uint8 tensor; NULL lets the library hipMalloc its own. */
BGS_API int bgs_connect_arena_bytes(int height, int width, int count, int64_t n, size_t* bytes);
BGS_API int bgs_connect_create(int height, int width, int count, int64_t n, int device, void* arena, size_t arena_bytes,
                       bgs_batch** out);
/* replaces bounce::Config(grid) + Config::sample_initial_state (bounce.cpp:26,29); cfg_grid int8[height][width] host.
 * Batches of 32768 boards and more (bit-packed boards, at most 16 pieces) also get the OPENING BOOK of their start position:
 * every path of up to four plies from it, enumerated once per start position and device by the library's own move search
 * and shared by the batches that have that start position -- the fused rollout's lanes start four plies in, with the
 * game's own draws (results are those of searching every ply, bit for bit).  Device memory OUTSIDE the arena: 21.7 MB for
 * the default 9x6 board, freed with the last batch that uses it.  BGS_BOUNCE_BOOK=0 switches it off. */
BGS_API int bgs_bounce_arena_bytes(int height, int width, int64_t n, size_t* bytes);
BGS_API int bgs_bounce_create(const int8_t* cfg_grid, int height, int width, int64_t n, int device, void* arena,
                      size_t arena_bytes, bgs_batch** out);
BGS_API int bgs_destroy(bgs_batch* b);

/* hipStream_t; NULL = null stream.  Work already enqueued for the batch on its previous stream is ordered before
 * anything enqueued on the new one (event + stream wait), so a batch may be created under one stream and used on
 * another without a host synchronisation. */
BGS_API int bgs_set_stream(bgs_batch* b, void* hip_stream);
/* a HIP stream of the library's own (non-blocking), for hosts without torch: batches that should overlap -- one per
 * host thread, say -- each get one.  Destroy it after the batches bound to it. */
BGS_API int bgs_stream_create(int device, void** hip_stream);
BGS_API int bgs_stream_destroy(int device, void* hip_stream);
BGS_API int bgs_set_first_game(bgs_batch* b, uint64_t first_game); /* global id of board 0 (sharding across GPUs) */
/* The RNG contract every later random step / rollout of this (Connect) batch draws under: BGS_RNG_PER_BLOCK (default) or
 * BGS_RNG_PER_PLY.  Build-defined like the RNG itself (the reference has none: its callers use random.choice,
 * README.md:62); a single rollout call can ask for the strict contract with BGS_ROLLOUT_DRAW_PER_PLY instead. */
BGS_API int bgs_set_rng_contract(bgs_batch* b, int contract);
/* A hint, not a rule of the game: how many rollout launches the caller keeps in flight on this batch's device (its own
 * included; 1 = one launch at a time, the default).  Results never depend on it.  The Bounce rollout shapes its launch
 * by it -- alone on the chip: a short bulk pass on many waves (shortest time to the last reward); among 16: few
 * long-lived waves (fewest instructions per ply).  bgs_pipeline_create passes its depth to its batches.  The reference
 * has no counterpart (one board per call: bounce.cpp:51). */
BGS_API int bgs_set_launches_in_flight(bgs_batch* b, int32_t launches);
BGS_API int bgs_synchronize(bgs_batch* b);
BGS_API int bgs_info(const bgs_batch* b, int* game, int* height, int* width, int* count, int64_t* n, int* planes);
/* Geometries beyond the bit-packed kernels' limits (Connect: height > 15, width > 16 or width * (height + 1) > 192;
 * Bounce: more than 64 cells or piece values above 15) are served by the generic kernels: same entry points, same
 * results, the board held as int8[n][h][w] (BGS_BUF_PLANES is then that grid).  Limits of the generic path: Connect
 * height, width <= 64; Bounce height, width <= 64, height * width <= 1024, values <= 127.
 * bgs_legal_bytes: bytes per board of the legal-move record of bgs_transition, and whether the batch is generic:
 *   Connect           uint8[width] mask;
 *   Bounce (packed)   uint64[width + 1]: target masks per column of the active row, then the active row's y;
 *   Bounce (generic)  int32 active row (-1 = none), then uint8 flags[width][height * width] (1 = legal target cell
 *                     of the piece in that column of the active row), padded to a multiple of 8 bytes. */
BGS_API int bgs_legal_bytes(const bgs_batch* b, size_t* bytes, int* generic);
/* device pointer + size of one of the batch's buffers (zero-copy hand-over to torch / RCCL) */
BGS_API int bgs_buffer(const bgs_batch* b, int buffer_id, void** device_ptr, size_t* bytes);

/* ---- the hot path --------------------------------------------------------------------------------- */
/* all boards back to Config::sample_initial_state() (connect.cpp:32, bounce.cpp:29); zeroes the step counter */
BGS_API int bgs_reset(bgs_batch* b);
/* ONE ply on every running board: State::get_actions (connect.cpp:43, bounce.cpp:40) -> uniform choice
 * (README.md:62 random.choice) -> Action::sample_next_state (connect.cpp:52, bounce.cpp:51) -> has_ended / reward */
BGS_API int bgs_step_random(bgs_batch* b, uint64_t seed);
/* `plies` such plies on every board that is (still) running, boards held in registers in between where the kernel
 * allows it (Connect boards of one 64-bit word: the per-ply memory traffic divides by `plies`); the result is the one
 * of `plies` calls of bgs_step_random */
BGS_API int bgs_step_random_n(bgs_batch* b, uint64_t seed, int32_t plies);
/* ONE caller-chosen ply: State::get_action_at (connect.cpp:44 / bounce.cpp:42) + Action::sample_next_state.
 * Connect: actions int32[n] = column; Bounce: int32[n][4] = source x, y, target x, y.  A negative first entry
 * skips the board.  actions_on_device != 0: `actions` is a device pointer.  status (host int32[n], may be
 * NULL): BGS_OK or BGS_ERR_ILLEGAL per board; illegal moves leave the board untouched. */
BGS_API int bgs_step_actions(bgs_batch* b, const int32_t* actions, int actions_on_device, int32_t* status);
/* plies until every board ended or holds max_plies plies (README.md:52 `while not state.has_ended`), fused in
 * one launch with the board in registers */
BGS_API int bgs_rollout(bgs_batch* b, uint64_t seed, int32_t max_plies, uint32_t flags);
/* Flat Monte-Carlo evaluation of every legal column of every board (Connect, bit-packed boards only).
 * counts int32[n][width][3] = (wins, draws, losses) of the player to move at board i, over `playouts` games that
 * start with column c and then continue by the batch's uniform random policy and RNG contract until they end or
 * hold max_plies plies; a capped game is counted in none of the three.  Illegal columns and ended boards: 0, 0, 0.
 * The batch's boards are not modified; the transitions played are added to bgs_steps.  counts_on_device != 0: a
 * device pointer (16-byte aligned), enqueued on the batch's stream, no synchronisation, no allocation; otherwise a
 * host buffer and the call returns when it is filled.
 * RNG: playout p of column c of board i is the game with global id G = ((first_game + i) * width + c) * playouts + p
 * (mod 2^64), played from board i after column c, its draws keyed by (seed, G, ply) under the batch's contract, ply the
 * board's absolute ply count: the playouts of board i in (c, p) order are a bgs_rollout(seed) with first_game =
 * first_game * width * playouts over the boards replicated width * playouts times and stepped by their column. */
BGS_API int bgs_connect_evaluate_actions(bgs_batch* b, uint64_t seed, int32_t playouts, int32_t max_plies,
                                         int32_t* counts, int counts_on_device);
/* bgs_connect_evaluate_actions with a playout policy.  Game ids, the first column, the cap, the bgs_steps accounting,
 * the counts layout and the refusals are those of bgs_connect_evaluate_actions; the batch is not modified.
 *   BGS_POLICY_UNIFORM   bgs_connect_evaluate_actions itself: the same launch, byte-identical counts and steps.
 *   BGS_POLICY_DECISIVE  decisive and anti-decisive moves.  The policy is defined by the build, as the RNG contract is.
 *                        At every ply of a playout after its forced first column:
 *                          1. L = the legal columns, ascending;
 *                          2. W = the columns of L whose landing cell completes `count` in a row for the side to move;
 *                          3. B = the columns of L whose landing cell would complete `count` in a row for the opponent,
 *                             if the opponent dropped there now;
 *                          4. the candidate list S = W if W is not empty, else B if B is not empty, else L;
 *                          5. the ply draws exactly the word it draws under BGS_POLICY_UNIFORM: the batch's contract
 *                             (per-block sub-draw or per-ply), keyed by (seed, G, absolute ply);
 *                          6. it plays element (draw * |S|) >> 32 of S.
 *                        No ply draws an extra or a different word: only the list the index is taken from changes.
 * Refused (BGS_ERR_ARG, with a message that says why): an unknown policy, a Bounce batch, a generic batch, and what
 * bgs_connect_evaluate_actions refuses. */
#define BGS_POLICY_UNIFORM 0
#define BGS_POLICY_DECISIVE 1
BGS_API int bgs_connect_evaluate_actions_policy(bgs_batch* b, uint64_t seed, int32_t playouts, int32_t max_plies, int policy,
                                                int32_t* counts, int counts_on_device);
/* Sequential-halving Monte-Carlo evaluation of every board (Karnin, Koren and Somekh 2013; Connect, bit-packed boards
 * only), one launch: a fixed `budget` of playouts a board is spent in rounds, and the worse half of the columns leaves
 * after every round.  For a running board i with A legal columns, R(x) = max(1, ceil(log2 x)):
 *   start      S_0 = the legal columns, R = R(A), P_0 = 0;
 *   round r    (r = 0 .. R-1) every column of S_r plays q_r = floor(budget / (|S_r| * R)) further playouts, those with
 *              the playout indices [P_r, P_r + q_r); P_{r+1} = P_r + q_r;
 *   selection  a column's score is 2 * wins + draws over all rounds so far (a capped playout scores 0); S_{r+1} = the
 *              ceil(|S_r| / 2) columns of S_r ranked highest, by score descending, then by column ascending.
 * best int32[n] = the one column of S_R; given int32[n][width] = the playouts a column was given; counts
 * int32[n][width][3] = its cumulative (wins, draws, losses) for the player to move at board i.  Illegal columns: all
 * zeros.  An ended board: all zeros and best = -1.
 * Playout p of column c of board i is the game G = ((first_game + i) * width + c) * budget + p (mod 2^64), played exactly
 * as bgs_connect_evaluate_actions_policy plays it (forced first column, policy, the batch's RNG contract keyed by the
 * absolute ply, the cap): a column's counts are those of the first given[i][c] playouts of the flat evaluation with
 * playouts = budget, so sharding by first_game holds.  The q_r of a board sum to at most `budget`.
 * The transitions of the playouts played are added to bgs_steps, first moves included; the boards are not modified.
 * given and best may be NULL.  on_device != 0: device pointers (16-byte aligned), enqueued on the batch's stream, no
 * synchronisation, no allocation; otherwise host buffers, filled when the call returns.
 * Refused (BGS_ERR_ARG, with a message that says why): budget < width * R(width) (the least budget that keeps every
 * q_r >= 1), max_plies < 1, an unknown policy, a Bounce batch, a generic batch, NULL counts, a misaligned device pointer,
 * n * width * budget beyond int64. */
BGS_API int bgs_connect_evaluate_actions_halving(bgs_batch* b, uint64_t seed, int32_t budget, int32_t max_plies, int policy,
                                                 int32_t* counts, int32_t* given, int32_t* best, int on_device);
/* Batched UCT tree search (Connect, bit-packed boards only), one launch: for every running board i (the root),
 * `iterations` (T) iterations of UCT with `leaf_playouts` (P) playouts a leaf.  Everything is integer arithmetic: the
 * result is defined bit for bit.  The batch's boards are not modified.
 * Tree.  A node is a position; for every column c it holds n[c] (the playouts that went through edge c), s[c] (the sum of
 * 2 * wins + draws of those playouts, seen from the player to move at the node) and the child node, if any.  The root is
 * node 0.
 * Iteration t (t = 0 .. T-1), from the root, at node v with position p:
 *   1. L = the legal columns of p, ascending;
 *   2. if some column of L has n[c] = 0, take the lowest such column (the expansion);
 *   3. otherwise take the column of L with the largest U(c) = Q(c) + E(c), ties to the lowest column, where
 *        N    = the sum of n[c] over L,
 *        Q(c) = floor(s[c] * 2048 / n[c])                     (0 .. 4096; a 64-bit intermediate),
 *        E(c) = isqrt(floor(explore * lg(N) / n[c]))          (isqrt: the exact floor square root),
 *        lg(N) = 256 * e + ((N * 256) >> e) - 256, e = floor(log2 N)   (a piecewise-linear log2 in Q8);
 *      with explore <= 2^18 and N < 2^31, explore * lg(N) fits 32 bits.  explore is about 45426 * C * C for a UCB1
 *      constant C on rewards in [0, 1];
 *   4. play c, giving p'.  p' has ended (c won, or filled the board): no node is made and no game is played, all P
 *      playouts of the iteration have that outcome.  p' is running and n[c] was 0: a new node is made for p' and the
 *      iteration's playouts start from p'.  p' is running and n[c] > 0: v becomes child[c], back to step 1;
 *   5. playout j (0 <= j < P) of iteration t of board i is the game G = ((first_game + i) * T + t) * P + j (mod 2^64),
 *      played from p' exactly as bgs_connect_evaluate_actions_policy plays a game after its forced first column: the
 *      policy, the batch's RNG contract keyed by (seed, G, absolute ply), the cap max_plies.  If p' already holds
 *      >= max_plies plies the P playouts are capped at once.  A capped playout scores 0 but counts in n;
 *   6. every edge (v, c) of the path gets n[c] += P and s[c] += 2 * (playouts won by the player to move at v) + draws.
 * Outputs.  visits int32[n][width] (may be NULL) = the root's n[c]; counts int32[n][width][3] = (wins, draws, losses) of
 * the root's mover over the playouts through root column c, capped playouts in none of the three; best int32[n] (may be
 * NULL) = the root column with the most visits, ties to the larger 2 * wins + draws, then to the lower column; nodes
 * int32[n] (may be NULL) = the nodes made, the root not counted (at most T).  An ended board: all zeros and best = -1.
 * Illegal columns: zeros.
 * bgs_steps gets the transitions of the playouts played, from p' on: the moves of the descent are not counted and a
 * terminal leaf adds nothing.  A root's results depend on (board, first_game + i) only, so sharding by first_game holds.
 * Workspace.  The tree lives in caller-owned device memory; bgs_connect_search_workspace_bytes says how much this batch
 * needs for T iterations (n roots of T + 1 nodes of 3 * width 32-bit words, a root's share rounded up to 256 bytes).  Its
 * contents need no preparation and mean nothing afterwards.  on_device != 0: workspace is a 256-byte aligned device
 * pointer of at least that size, the outputs are 16-byte aligned device pointers, and the call is an enqueue on the
 * batch's stream with no synchronisation and no allocation.  on_device == 0: the outputs are host buffers, filled when the
 * call returns; workspace may be NULL (the library then allocates and frees it around the call) or a device pointer as
 * above.
 * Refused (BGS_ERR_ARG, with a message that says why): a Bounce batch, a generic batch, T < 1, P < 1, T * P > 2^29
 * (scores stay in int32), explore < 0 or > 2^18, max_plies < 1, an unknown policy, NULL counts, a misaligned pointer, a
 * workspace that is too small (or NULL with on_device), n * T * P beyond int64. */
BGS_API int bgs_connect_search_workspace_bytes(const bgs_batch* b, int32_t iterations, size_t* bytes);
BGS_API int bgs_connect_search_actions(bgs_batch* b, uint64_t seed, int32_t iterations, int32_t leaf_playouts, int32_t explore,
                                       int32_t max_plies, int policy, int32_t* counts, int32_t* visits, int32_t* best,
                                       int32_t* nodes, void* workspace, size_t workspace_bytes, int on_device);
/* The same search, proving wins, draws and losses in its tree (MCTS-Solver: Winands, Bjornsson and Saito 2008; Connect,
 * bit-packed boards only), one launch.  What stays as in bgs_connect_search_actions: the workspace and its size
 * (bgs_connect_search_workspace_bytes serves both entry points), the argument checks and refusals, the on_device rules,
 * the game ids G = ((first_game + i) * T + t) * P + j with the T that was asked for, the RNG contracts, the policies,
 * bgs_steps, and sharding by first_game.  proved and done may be NULL, like visits, best and nodes.
 * Tags.  Every edge (v, c) has a tag, seen from the player to move at v: OPEN (the initial state), WIN, DRAW or LOSS.
 * The value of a node is WIN if a legal column is tagged WIN; otherwise OPEN if a legal column is OPEN (a legal column
 * that has never been visited is OPEN); otherwise DRAW if a legal column is tagged DRAW; otherwise LOSS.
 * Iteration t (t = 0 .. T-1):
 *   0. if the root's value is not OPEN, this root's search is over: done[i] = t, and the remaining iterations and their
 *      game ids are not used;
 *   1.-3. the selection of bgs_connect_search_actions, word for word, with L read as "the legal columns of p whose tag
 *      is OPEN, ascending"; N is the sum of n[c] over those columns.  A node the descent stands on always has such a
 *      column: that is the invariant of step 7;
 *   4. as there.  In addition, an edge that ends the game is tagged WIN if c won and DRAW if c filled the board; all P
 *      playouts of the iteration still carry that outcome.  A position at or beyond max_plies is not an end and tags
 *      nothing;
 *   5.-6. as there;
 *   7. only after an iteration whose last edge was tagged in step 4: go up the path, for k = depth-1 down to 0 (edge k
 *      leaves path_node[k]).  If the value of path_node[k] is OPEN, stop.  If k = 0, the root is decided.  Otherwise
 *      edge k-1 of the path is tagged with the negation of that value: a WIN node makes its parent's edge LOSS, a LOSS
 *      node makes it WIN, DRAW stays DRAW.  A decided node is therefore never entered again.
 * Outputs.  counts, visits and nodes mean what they mean there.  proved int8[n][width] (may be NULL) = the root's tags in
 * the solver's codes: BGS_SOLVE_WIN, BGS_SOLVE_DRAW or BGS_SOLVE_LOSS for a tagged column, BGS_SOLVE_UNKNOWN for a legal
 * OPEN column, BGS_SOLVE_NONE for an illegal column or an ended board.  done int32[n] (may be NULL) = the iterations
 * run: T for an undecided root, 0 for an ended board.  best: if a root column is tagged WIN, that column (there is at
 * most one: the search stops at the first); otherwise the rule of bgs_connect_search_actions (the most visits, then the
 * larger s, then the lower column) over the legal columns not tagged LOSS; if every legal column is tagged LOSS, that
 * rule over all legal columns.
 * Equal to the plain search.  While no edge of a root's tree has been tagged, that root's state is the plain search's,
 * bit for bit: a root whose search tags nothing returns the outputs of bgs_connect_search_actions, and done = T.
 * Known weakness: a column proved DRAW stops collecting visits, so an undecided root can prefer an OPEN column whose Q
 * is below a draw's.  The forests (bgs_connect_forest_search, bgs_bounce_forest_search) do not prove; Bounce proves
 * with bgs_bounce_search_moves_proving. */
BGS_API int bgs_connect_search_actions_proving(bgs_batch* b, uint64_t seed, int32_t iterations, int32_t leaf_playouts,
                                               int32_t explore, int32_t max_plies, int policy, int32_t* counts,
                                               int32_t* visits, int32_t* best, int32_t* nodes, int8_t* proved, int32_t* done,
                                               void* workspace, size_t workspace_bytes, int on_device);
/* The same search on trees that outlive a launch (Connect, bit-packed boards only): a FOREST is caller-owned device
 * memory that holds one tree per board of the batch, each with room for `capacity` (C) nodes, the root included, and
 * persists from launch to launch.  An agent that plays a game searches, plays, advances the trees by the columns played
 * and searches again: the subtree under the move played is carried into the next search.
 * Layout.  Opaque; bgs_connect_forest_bytes says how large (per tree: a header -- the nodes in use and the position the
 * root stands for, as the planes of the batch --, C nodes of 3 * width 32-bit words, a tree's share rounded up to 256
 * bytes).  The re-rooting keeps its scratch on the chip, which bounds C: 2 <= C <= BGS_CONNECT_FOREST_MAX_CAPACITY.
 * bgs_connect_forest_search.  For board i, at the start of the launch, tree i is CARRIED if restart == 0, the board is
 * running, the header's node count is in [1, C], the recorded root position equals board i's planes, and the root's N
 * (the sum of its n[c]) plus T * P is below 2^31.  Otherwise the tree is emptied: a running board is left with one zeroed
 * root node and board i recorded as the root position; an ended board gets an emptied tree, all-zero outputs and
 * best = -1.  THE FIRST LAUNCH ON FRESH MEMORY MUST PASS restart != 0: memory that was never written may pass the check by
 * accident.  Then T iterations of bgs_connect_search_actions, word for word, with step 4 read as
 * bgs_bounce_search_moves reads it: p' has ended: no node and no game; p' runs and the edge has a child: descend; p' runs
 * and the edge has no child: a node is made if and only if the tree holds fewer than C nodes, and either way the P
 * playouts start from p' (an edge whose node did not fit is tried again the next time it is taken).  Node 0 is the root
 * and never a child, so a child word of 0 means "none".  Playout j of iteration t is the game
 * G = ((first_game + i) * T + t) * P + j with this launch's T, played as bgs_connect_search_actions plays it: the caller
 * varies `seed` from launch to launch.  Selection, Q, E, lg(N), isqrt, the back-propagation, bgs_steps and sharding by
 * first_game are unchanged.
 * Outputs: counts int32[n][width][3] = W/D/L through each root column of THIS launch's playouts; visits int32[n][width] =
 * the root's n[c], carried visits included; best int32[n] by the rule of bgs_connect_search_actions over those visits and
 * s; nodes int32[n] = the nodes in the tree at the end, the root not counted (<= C - 1); carried int32[n] = the nodes in
 * the tree at the start after the check, the root not counted (0 for a tree that was emptied).  visits, best, nodes and
 * carried may be NULL.  With restart != 0 and C >= T + 1 the outputs and bgs_steps are those of
 * bgs_connect_search_actions, bit for bit, and carried is all zeros.
 * `forest` is always a 256-byte aligned device pointer.  on_device != 0: the outputs are 16-byte aligned device pointers
 * and the call is an enqueue on the batch's stream with no synchronisation and no allocation; otherwise they are host
 * buffers, filled when the call returns.
 * bgs_connect_forest_advance re-roots every tree: columns int32[n], for tree i with c = columns[i]: c < 0: the tree is
 * untouched.  The root's edge c has a child r: the subtree of r becomes the tree and r becomes node 0; n, s and the
 * parent/child relations of every kept node are unchanged, and the recorded position becomes the position after c (a plain
 * drop, no win test).  Anything else -- an edge never played, a terminal edge, a node that did not fit, a full column,
 * c >= width, a tree that is already empty --: the tree is emptied, and the next search starts it anew from the batch's
 * board.  kept int32[n] (may be NULL) = the nodes after the call, the root not counted.  The call neither reads nor
 * modifies the batch's boards: the caller plays the same columns with bgs_step_actions, before or after.  Two plies (the
 * own move, then the reply) are two calls.  on_device: where columns and kept live, as above.
 * Refused (BGS_ERR_ARG, with a message that says why; the outputs and the forest are untouched): a Bounce batch, a generic
 * batch, C < 2 or C > BGS_CONNECT_FOREST_MAX_CAPACITY, what bgs_connect_search_actions refuses for T, P, explore,
 * max_plies, the policy and the pointers, a NULL or misaligned forest, forest_bytes too small, NULL columns. */
#define BGS_CONNECT_FOREST_MAX_CAPACITY 65536
BGS_API int bgs_connect_forest_bytes(const bgs_batch* b, int32_t capacity, size_t* bytes);
BGS_API int bgs_connect_forest_search(bgs_batch* b, uint64_t seed, int32_t iterations, int32_t leaf_playouts, int32_t explore,
                                      int32_t max_plies, int policy, int32_t capacity, int restart, int32_t* counts, int32_t* visits,
                                      int32_t* best, int32_t* nodes, int32_t* carried, void* forest, size_t forest_bytes,
                                      int on_device);
BGS_API int bgs_connect_forest_advance(bgs_batch* b, const int32_t* columns, int32_t capacity, int32_t* kept, void* forest,
                                       size_t forest_bytes, int on_device);
/* PUCT tree search whose leaves the CALLER evaluates (Connect, bit-packed boards only): the search of a policy/value
 * network.  One call is one simulation of every tree: it applies the caller's (priors, value) to the pending leaf of
 * every tree, reports the root's statistics and descends to the next leaf, whose position it writes out; the caller runs
 * its evaluator on that device tensor and calls again.  Integer arithmetic throughout, no RNG anywhere: the result is
 * defined bit for bit.  The boards and bgs_steps are untouched.
 * EVERY POINTER IS A DEVICE POINTER: `trees` 256-byte aligned, the rest 16-byte aligned; the call is an enqueue on the
 * batch's stream with no synchronisation and no allocation, so the loop can sit in a stream or in a captured graph with
 * the network.  There is no host variant, because the evaluator lives on the device.  visits, scores, best and nodes may
 * be NULL; priors and values may be NULL only with BGS_GUIDED_RESTART.
 * Tree and node.  One tree per board, in caller-owned opaque memory (bgs_connect_guided_bytes says how large), with room
 * for `capacity` (C) nodes, the root included.  A node holds four values per column c: n[c], s[c], the child and P[c].
 * The position is rebuilt during the descent.  Each tree's share also holds, between calls: the nodes in use; the root
 * position, as the batch's planes; the pending leaf: its kind and its path of (node, column) pairs, at most h * w of
 * them.  The share is rounded up to 256 bytes.
 * One step, for board i, in this order:
 *   1. Check.  The tree is LIVE if BGS_GUIDED_RESTART is not set, the board is running, the nodes in use are in [1, C]
 *      and the recorded planes equal board i's.  Otherwise the tree is emptied and any pending evaluation is dropped; a
 *      running board gets one unexpanded root and has board i recorded.  So a board that the caller stepped or reset
 *      between two calls restarts on its own.  THE FIRST CALL ON FRESH MEMORY MUST PASS BGS_GUIDED_RESTART.
 *   2. Apply, if an evaluation is pending.  A leaf of kind EVALUATE reads priors[i][0..w) and values[i]; kind TERMINAL
 *      reads neither.
 *      Priors.  For a legal column c of the leaf with x = priors[i][c]: w[c] = 0 unless x > 0 (NaN, zero and negatives
 *      give 0), otherwise w[c] = floor(min(x, 1.0f) * 65536.0f), exact in float32.  Illegal columns are ignored.
 *      W = the sum of w[c]; if W = 0, every legal w[c] = 1 (and W their number).  P[c] = floor(w[c] * 65536 / W).
 *      Value, seen from the player to move at the leaf: NaN gives v = 0; otherwise x is clamped to [-1, 1] and
 *      v = (int32)(x * 1024.0f), truncated toward zero.  sigma = 1024 + v.  A TERMINAL leaf has sigma = 0 if the last
 *      edge won and sigma = 1024 if it filled the board.
 *      The leaf is made a node -- n, s and child zeroed, its P set, the parent's child word linking it -- if and only
 *      if the leaf is EVALUATE, is not the root, its edge has no child and the tree holds fewer than C nodes.  An edge
 *      whose node did not fit is tried again later (the forest's rule).  An EVALUATE leaf that IS the root only
 *      receives P.  Every edge k of the path gets n += 1, and s += sigma if node k's mover is the leaf's mover, else
 *      s += 2048 - sigma.
 *   3. Report, through the outputs that are not NULL: visits[i][c] = the root's n[c]; scores[i][c] = the root's s[c];
 *      nodes[i] = the nodes in use, the root not counted; best[i] = the column with the most visits, then the larger s,
 *      then the lower column; best[i] = -1 for an ended board or a root with no visit.  Illegal columns read as zeros.
 *   4. Select, unless BGS_GUIDED_FINISH is set, the board has ended, or the sum of the root's n[c] has reached
 *      BGS_GUIDED_MAX_VISITS: each of those three gives kind IDLE.  An unexpanded root is itself the leaf: EVALUATE,
 *      with an empty path.  Otherwise, at node v with N = the sum of n[c] over the legal columns, take the legal column
 *      with the largest U(c) = Q(c) + E(c), ties to the lowest column, where
 *        Q(c) = floor(2 * s[c] / n[c]), or 2048 for n[c] = 0,
 *        E(c) = floor(((cpuct * P[c] * isqrt((N + 1) << 12)) >> 19) / (1 + n[c])), computed in 64 bits (isqrt: the exact
 *               floor square root); `cpuct` is c_puct in Q8, 0 .. 4096, and E stays below 2^25.
 *      Play the column.  The game ended: the leaf is TERMINAL.  There is no child: the leaf is EVALUATE.  Otherwise
 *      descend.  The path and the kind are recorded, and leaf_grid[i] (int8[h][w], in bgs_read_grid's encoding),
 *      leaf_player[i] (the leaf's ply & 1) and leaf_kind[i] are written.  IDLE rows carry the root's grid and player.
 * A tree's result depends only on its board and the rows it was fed, so any split of the batch gives the same trees.
 * A call with flags 0 on a tree with nothing pending -- one that BGS_GUIDED_FINISH or bgs_connect_guided_advance left --
 * applies nothing and reads neither that tree's priors row nor its values entry: it reports and selects.  That is how a
 * search RESUMES on trees that were carried; it needs no flag of its own (priors and values must still be device
 * pointers).
 * Refused (BGS_ERR_ARG, with a message; the outputs and the trees are untouched): a Bounce batch, a generic batch, C < 2
 * or C > BGS_GUIDED_MAX_CAPACITY, cpuct outside [0, 4096], unknown flag bits, BGS_GUIDED_RESTART together with
 * BGS_GUIDED_FINISH, NULL trees, leaf_grid, leaf_player or leaf_kind, NULL priors or values without BGS_GUIDED_RESTART, a
 * misaligned pointer, trees_bytes too small.
 * bgs_connect_guided_advance re-roots every tree, so that a loop that searches, plays and searches again keeps the
 * evaluations under the move it played: columns int32[n], for tree i with c = columns[i]:
 *   c < 0: the share is untouched, a pending leaf included; kept[i] = the nodes in use, the root not counted (0 for an
 *     emptied tree).
 *   The root's edge c has a child r, c < width, and column c of the recorded position has room: the subtree of r becomes
 *     the tree and r becomes node 0; the kept nodes stay in the order they were made; n, s, P and the parent/child
 *     relations of every kept node are unchanged; the recorded position gets the stone of column c (a plain drop by the
 *     side to move, no win test); the pending leaf is dropped (kind none, a path of no edge) and the root counts as one
 *     that has its P.  kept[i] = the nodes after the call, the root not counted.
 *   Anything else -- an edge never played, a terminal edge, a node that did not fit, a full column, c >= width, a tree
 *     that is already empty, a node count above C --: the tree is emptied (no node, nothing pending, a root without P),
 *     kept[i] = 0, and the next step starts the tree anew from the batch's board, by its check.
 * The call neither reads nor modifies the boards or bgs_steps: the caller plays the same columns with bgs_step_actions
 * before the next bgs_connect_guided_step; if it does not, that step's check finds other planes and empties the tree.
 * Two plies (the own move, then the reply) are two calls.
 * Every pointer is a device pointer, as in the step: `trees` 256-byte aligned, columns and kept 16-byte aligned, kept may
 * be NULL; an enqueue on the batch's stream with no synchronisation and no allocation, so it can sit in a captured graph;
 * there is no host variant.  trees, capacity and trees_bytes are those of bgs_connect_guided_step and
 * bgs_connect_guided_bytes.  The re-rooting keeps its scratch on the chip, as the forest's does, which bounds C here:
 * C <= BGS_GUIDED_ADVANCE_MAX_CAPACITY; larger trees can be searched, not advanced.
 * Refused (BGS_ERR_ARG, with a message; kept and the trees are untouched): what bgs_connect_guided_bytes refuses,
 * C > BGS_GUIDED_ADVANCE_MAX_CAPACITY, NULL columns, NULL trees, a misaligned pointer, trees_bytes too small. */
#define BGS_GUIDED_RESTART 1u      /* empty every tree first; nothing is pending; priors/values are not read */
#define BGS_GUIDED_FINISH  2u      /* apply the pending evaluation, select nothing */
#define BGS_GUIDED_EVALUATE 0      /* leaf_kind: the caller's priors[i] / values[i] are wanted for this leaf */
#define BGS_GUIDED_TERMINAL 1      /* the leaf ended the game: its value is known, the caller's row is ignored */
#define BGS_GUIDED_IDLE     2      /* no simulation: ended board, FINISH, or the root at BGS_GUIDED_MAX_VISITS */
#define BGS_GUIDED_MAX_CAPACITY (1 << 20)
#define BGS_GUIDED_MAX_VISITS   (1 << 19)
BGS_API int bgs_connect_guided_bytes(const bgs_batch* b, int32_t capacity, size_t* bytes);
BGS_API int bgs_connect_guided_step(bgs_batch* b, int32_t capacity, int32_t cpuct, uint32_t flags,
                                    const float* priors, const float* values,
                                    int8_t* leaf_grid, int8_t* leaf_player, int32_t* leaf_kind,
                                    int32_t* visits, int32_t* scores, int32_t* best, int32_t* nodes,
                                    void* trees, size_t trees_bytes);
#define BGS_GUIDED_ADVANCE_MAX_CAPACITY 65536/* = BGS_CONNECT_FOREST_MAX_CAPACITY: the same scratch on the chip */
BGS_API int bgs_connect_guided_advance(bgs_batch* b, const int32_t* columns, int32_t capacity,
                                       int32_t* kept, void* trees, size_t trees_bytes);
/* Flat Monte-Carlo evaluation of every legal move of every board (Bounce, bit-packed boards only: at most 64 cells,
 * piece values <= 15).  counts int32[n][width][height * width][3]: entry [i][x][c] = (wins, draws, losses) of the
 * player to move at board i over `playouts` games that start with the move of the piece in column x of the active row
 * to cell c = ty * width + tx (bit c of targets[i][x], bgs_bounce_read_targets), then continue by the uniform random
 * policy until they end or hold max_plies plies (clamped to 65535: plies are 16-bit); a capped game is counted in none
 * of the three.  Illegal slots and ended boards (boards without a legal move among them): 0, 0, 0.  The batch's boards
 * are not modified; the transitions played, first moves included, are added to bgs_steps.  counts_on_device: as
 * bgs_connect_evaluate_actions (a 16-byte aligned device pointer, enqueued on the batch's stream, no synchronisation, no
 * allocation; otherwise a host buffer, filled when the call returns).
 * RNG: with S = width * height * width, playout p of slot s = x * height * width + c of board i is the game with global
 * id G = ((first_game + i) * S + s) * playouts + p (mod 2^64), its draws keyed by (seed, G, ply), a philox word per ply,
 * ply the board's absolute ply count: the playouts of board i in (s, p) order are a bgs_rollout(seed) with first_game =
 * first_game * S * playouts over the boards replicated S * playouts times and stepped by their slot's move, the
 * illegal slots dropped.  Refused (BGS_ERR_ARG): Connect and generic batches, playouts < 1, max_plies < 1, a misaligned
 * device pointer, n * S * playouts beyond int64. */
BGS_API int bgs_bounce_evaluate_moves(bgs_batch* b, uint64_t seed, int32_t playouts, int32_t max_plies, int32_t* counts,
                                      int counts_on_device);
/* bgs_bounce_evaluate_moves with a playout policy (BGS_POLICY_*, above).  Game ids, slots, the counts layout, the cap
 * (clamped to 65535), the bgs_steps accounting (first moves included), the device and host variants and the refusals are
 * those of bgs_bounce_evaluate_moves; the batch is not modified.
 *   BGS_POLICY_UNIFORM   bgs_bounce_evaluate_moves itself: the same launch, byte-identical counts and steps.
 *   BGS_POLICY_DECISIVE  a win in one is taken.  The policy is defined by the build, as the RNG contract is.  At every
 *                        ply of a playout after its forced first move (a ply is played only if the game is running and
 *                        holds fewer than max_plies plies):
 *                          1. L = the canonical action list of the side to move: sources by ascending x, targets by
 *                             ascending (y, x).  An empty L is settled as under the uniform policy, before the policy
 *                             and also at the cap: the other side wins if it could move, else a draw;
 *                          2. W = the actions of L whose target lies in the mover's goal row (the top row for player 0,
 *                             the bottom row for player 1);
 *                          3. the candidate list S = W if W is not empty, else L;
 *                          4. the ply draws exactly the word it draws under BGS_POLICY_UNIFORM: philox keyed by
 *                             (seed, G, absolute ply), a word per ply;
 *                          5. it plays element (draw * |S|) >> 32 of S, in L's order.
 *                        No ply draws an extra or a different word.  Every element of W ends the game for the mover, and
 *                        counts and bgs_steps, the only outputs, do not depend on which one is played: the kernel ends
 *                        the game at such a ply without picking or moving (one transition, the mover wins).  Step 5
 *                        stays in the definition so that a later observer of the final board has one answer.
 *                        There is no blocking step, which makes this policy narrower than Connect's: finding the moves
 *                        that leave the opponent without a win in one needs a move search per candidate, about 12
 *                        searches a ply on the default board.
 * Refused (BGS_ERR_ARG, with a message that says why): an unknown policy, a Connect batch, a generic batch, and what
 * bgs_bounce_evaluate_moves refuses. */
BGS_API int bgs_bounce_evaluate_moves_policy(bgs_batch* b, uint64_t seed, int32_t playouts, int32_t max_plies, int policy,
                                             int32_t* counts, int counts_on_device);
/* Sequential-halving Monte-Carlo evaluation of every board (Bounce, bit-packed boards only), one launch: the schedule of
 * bgs_connect_evaluate_actions_halving with "column" read as "arm".  Slots are those of bgs_bounce_evaluate_moves:
 * S = width * height * width, slot s = x * height * width + c is the move of the piece in column x of the active row to
 * cell c.  The arms of a running board i are its A legal moves in canonical order (sources by ascending x, targets by
 * ascending (y, x)): ascending slot order.  With R(x) = max(1, ceil(log2 x)):
 *   start      S_0 = the legal moves, R = R(A), P_0 = 0;
 *   round r    (r = 0 .. R-1) every arm of S_r plays q_r = floor(budget / (|S_r| * R)) further playouts, those with the
 *              playout indices [P_r, P_r + q_r); P_{r+1} = P_r + q_r;
 *   selection  an arm's score is 2 * wins + draws over all rounds so far (a capped playout scores 0); S_{r+1} = the
 *              ceil(|S_r| / 2) arms of S_r ranked highest, by score descending, then by slot ascending.
 * best int32[n] = the slot of the one arm of S_R; given int32[n][width][height * width] = the playouts a slot was given;
 * counts int32[n][width][height * width][3] = its cumulative (wins, draws, losses) for the player to move at board i.
 * An illegal slot: all zeros.  A board that has ended, has no legal move or holds 65535 plies (the boards
 * bgs_bounce_evaluate_moves gives no playouts): all zeros and best = -1.
 * Playout p of slot s of board i is the game G = ((first_game + i) * S + s) * budget + p (mod 2^64), played exactly as
 * bgs_bounce_evaluate_moves_policy plays it (forced first move, policy, a philox word per absolute ply, the cap clamped
 * to 65535, the settlement of a side without a move): an arm's counts are those of the first given[i][s] playouts of the
 * flat evaluation with playouts = budget, so sharding by first_game holds.  The q_r of a board sum to at most `budget`.
 * A budget too small for a board: the number of arms differs from board to board, so the least budget is a matter of the
 * board and not of the call.  A running board with budget < A * R(A) -- some q_r would be 0 -- is not evaluated: its
 * counts and given are all zeros and best = BGS_HALVING_SHORT; every other board of the batch is evaluated as usual.
 * The transitions of the playouts played are added to bgs_steps, first moves included; the boards are not modified.
 * given and best may be NULL.  on_device != 0: device pointers (16-byte aligned), enqueued on the batch's stream, no
 * synchronisation, no allocation; otherwise host buffers, filled when the call returns.
 * Refused (BGS_ERR_ARG, with a message that says why): a Connect batch, a generic batch, budget < 1, max_plies < 1, an
 * unknown policy, NULL counts, a misaligned device pointer, n * S * budget beyond int64. */
#define BGS_HALVING_SHORT (-2)
BGS_API int bgs_bounce_evaluate_moves_halving(bgs_batch* b, uint64_t seed, int32_t budget, int32_t max_plies, int policy,
                                              int32_t* counts, int32_t* given, int32_t* best, int on_device);
/* Batched UCT tree search (Bounce, bit-packed boards only), one launch: bgs_connect_search_actions with "column" read as
 * "arm".  For every running board i (the root), `iterations` (T) iterations of UCT with `leaf_playouts` (P) playouts a
 * leaf; everything is integer arithmetic and the result is defined bit for bit.  The batch's boards are not modified.
 * Arms and slots.  The arms of a position are its legal moves in canonical order (sources by ascending x, targets by
 * ascending (y, x)), numbered 0 .. A-1.  Slots are those of bgs_bounce_evaluate_moves: S = width * height * width, slot
 * s = x * height * width + c is the move of the piece in column x of the active row to cell c; the arms of a position
 * are in ascending slot order.
 * Tree.  A node is a position with A >= 1 arms; for every arm a it holds n[a] (the playouts that went through the edge),
 * s[a] (the sum of 2 * wins + draws of those playouts, seen from the player to move at the node) and the child node, if
 * any.  The root is node 0.  Every root has a pool of `edges` (E) edges: a node with A arms takes A of them when it is
 * made, the root its own first.  BGS_BOUNCE_SEARCH_MIN_EDGES(height, width) is the most arms a position of the geometry
 * can have (the k <= width pieces of the active row reach at most (height - 1) * width - k cells each); a call with E
 * below it is refused, so a root always fits and no board is ever "short".
 * Iteration t (t = 0 .. T-1), from the root, at node v with position p:
 *   1.-3. the selection of bgs_connect_search_actions over the arms of p: the lowest arm with n[a] = 0 if there is one,
 *      otherwise the arm with the largest U(a) = Q(a) + E(a), ties to the lowest arm, with N the sum of n[a] over the
 *      arms of v and Q, E, lg and isqrt exactly as defined there;
 *   4. play arm a, giving p'.
 *      p' has ended -- the target lies in the mover's goal row, or the side to move at p' has no move and the game is
 *      settled as bgs_step_actions settles it (the mover wins if it could move, else a draw): no node is made and no
 *      game is played, all P playouts of the iteration have that outcome.
 *      p' is running and holds >= min(max_plies, 65535) plies: no node is made, now or later, and the P playouts are
 *      capped at once (they score 0 and count in n).
 *      p' is running and the edge has a child: v becomes the child, back to step 1.
 *      p' is running and the edge has no child: a node is made for p' if and only if (edges in use) + A(p') <= E, and
 *      either way the iteration's P playouts start from p'.  An edge whose node could not be made is tried again the
 *      next time it is taken: the pool only grows, but a position with fewer arms elsewhere may still fit later.
 *      THIS DIFFERS from bgs_connect_search_actions, which makes the node when n[c] was 0: here the test is "the edge
 *      has no child", because an edge can have been played without getting its node;
 *   5. playout j (0 <= j < P) of iteration t of board i is the game G = ((first_game + i) * T + t) * P + j (mod 2^64),
 *      played from p' exactly as bgs_bounce_evaluate_moves_policy plays a game after its forced first move: the policy
 *      (BGS_POLICY_UNIFORM or BGS_POLICY_DECISIVE), a philox word per absolute ply keyed by (seed, G, ply), the cap
 *      clamped to 65535, the settlement of a side without a move.  A capped playout scores 0 but counts in n;
 *   6. every edge (v, a) of the path gets n[a] += P and s[a] += 2 * (playouts won by the player to move at v) + draws.
 * Outputs.  counts int32[n][width][height * width][3] = (wins, draws, losses) of the root's mover over the playouts
 * through the root arm of that slot, capped playouts in none of the three; visits int32[n][width][height * width] (may
 * be NULL) = the root's n by slot; best int32[n] (may be NULL) = the slot of the root arm with the most visits, ties to
 * the larger s, then to the lower slot, or -1; nodes int32[n] (may be NULL) = the nodes made, the root not counted (at
 * most T); used int32[n] (may be NULL) = the pool edges in use at the end, the root's included: used + (the arms of some
 * position) > E is how a caller sees that the pool ran dry.  Illegal slots: zeros.  A board that has ended, has no move
 * or already holds 65535 plies: all zeros, best = -1, used = 0.
 * bgs_steps gets the transitions of the playouts played, from p' on: the moves of the descent are not counted and a
 * terminal leaf adds nothing.  A root's results depend on (board, first_game + i) only, so sharding by first_game holds.
 * Workspace.  Caller-owned device memory; bgs_bounce_search_workspace_bytes says how much this batch needs for T
 * iterations and E edges: n roots of 16 * E bytes (the edge pool: n, s, child, move), 8 * (T + 1) bytes (the node
 * table) and 4 * (T + 1) bytes (the descent path, which can be T + 1 edges long and therefore lives here), a root's share
 * rounded up to 256 bytes.  Its contents need no preparation and mean nothing afterwards.  on_device != 0: workspace is a
 * 256-byte aligned device pointer of at least that size, the outputs are 16-byte aligned device pointers, and the call is
 * an enqueue on the batch's stream with no synchronisation and no allocation.  on_device == 0: the outputs are host
 * buffers, filled when the call returns; workspace may be NULL (the library then allocates and frees it around the
 * call) or a device pointer as above.
 * Refused (BGS_ERR_ARG, with a message that names the argument; every output is left untouched): a Connect batch, a
 * generic batch, T < 1, P < 1, T * P > 2^29, explore < 0 or > 2^18, max_plies < 1, an unknown policy, E below
 * BGS_BOUNCE_SEARCH_MIN_EDGES, NULL counts, a misaligned pointer, a workspace that is too small (or NULL with
 * on_device), n * T * P beyond int64. */
#define BGS_BOUNCE_SEARCH_MIN_EDGES(h, w) ((h) >= 3 ? (w) * (w) * ((h) - 2) : 1)
BGS_API int bgs_bounce_search_workspace_bytes(const bgs_batch* b, int32_t iterations, int32_t edges, size_t* bytes);
BGS_API int bgs_bounce_search_moves(bgs_batch* b, uint64_t seed, int32_t iterations, int32_t leaf_playouts, int32_t explore,
                                    int32_t max_plies, int policy, int32_t edges, int32_t* counts, int32_t* visits,
                                    int32_t* best, int32_t* nodes, int32_t* used, void* workspace, size_t workspace_bytes,
                                    int on_device);
/* The same search, proving wins, draws and losses in its tree (MCTS-Solver: Winands, Bjornsson and Saito 2008; Bounce,
 * bit-packed boards only), one launch: the sibling of bgs_connect_search_actions_proving.  What stays as in
 * bgs_bounce_search_moves: the workspace and its size (bgs_bounce_search_workspace_bytes serves both entry points), the
 * pool of E edges and the rule that an edge whose node did not fit is tried again, the cap rule, the game ids G =
 * ((first_game + i) * T + t) * P + j with the T that was asked for, the policies, bgs_steps, sharding by first_game, the
 * refusals, and the on_device rules (proved and done are 16-byte aligned device pointers then).  proved and done may be
 * NULL, like visits, best, nodes and used.
 * Tags.  Every edge (v, a) has a tag, seen from the player to move at v: OPEN, WIN, DRAW or LOSS.  An arm that was never
 * played is OPEN.  An arm whose position runs and holds the cap is OPEN and stays OPEN: it is selectable and its
 * playouts score 0, exactly as in bgs_bounce_search_moves.  An edge whose node did not fit the pool is OPEN.  The value
 * of a node is WIN if an arm is tagged WIN; otherwise OPEN if an arm is OPEN; otherwise DRAW if an arm is tagged DRAW;
 * otherwise LOSS.
 * Iteration t (t = 0 .. T-1):
 *   0. if the root's value is not OPEN, this root's search is over: done[i] = t, and the remaining iterations and their
 *      game ids are not used;
 *   1.-3. the selection of bgs_bounce_search_moves, word for word, over the arms of p whose tag is OPEN: the lowest such
 *      arm with n[a] = 0 if there is one, otherwise the largest U(a), ties to the lowest arm; N is the sum of n[a] over
 *      the OPEN arms alone.  (A tagged arm has n[a] > 0.)  A node the descent stands on always has an OPEN arm: that is
 *      the invariant of step 7;
 *   4. as there.  In addition, an edge that ends the game is tagged: WIN if the mover won -- the target lies in its goal
 *      row, or the side to move at p' has no move while the mover has one -- and DRAW if neither side has a move.  All P
 *      playouts of the iteration still carry that outcome.  A position that runs and holds the cap is not an end and
 *      tags nothing;
 *   5.-6. as there;
 *   7. only after an iteration whose last edge was tagged in step 4: go up the path, for k = depth-1 down to 0 (edge k
 *      leaves path_node[k]; path_node[0] is the root).  If the value of path_node[k] is OPEN, stop.  If k = 0, the root
 *      is decided.  Otherwise edge k-1 of the path is tagged with the negation of that value: a WIN node makes its
 *      parent's edge LOSS, a LOSS node makes it WIN, DRAW stays DRAW.  A decided node is therefore never entered again.
 * Outputs.  counts, visits, nodes and used mean what they mean there; the nodes under a tagged edge stay counted and keep
 * their pool edges.  proved int8[n][width][height * width] (may be NULL), by slot: BGS_SOLVE_WIN, BGS_SOLVE_DRAW or
 * BGS_SOLVE_LOSS for a tagged root arm, BGS_SOLVE_UNKNOWN for a legal OPEN arm, BGS_SOLVE_NONE for an illegal slot and
 * for every slot of a board that has ended, has no move or holds 65535 plies.  done int32[n] (may be NULL) = the
 * iterations run: T for a root still OPEN after T iterations and for one decided by the T-th, 0 for a board without arms.
 * best: if a root arm is tagged WIN, its slot (there is at most one: the search stops at the first); otherwise the rule
 * of bgs_bounce_search_moves (the most visits, then the larger s, then the lower slot, n > 0) over the arms not tagged
 * LOSS; if every arm is tagged LOSS, that rule over all arms; -1 for a board without arms.
 * Equal to the plain search.  While no edge of a root's tree has been tagged, that root's state is the plain search's,
 * bit for bit: a root whose search plays no edge that ends the game returns the outputs of bgs_bounce_search_moves,
 * done = T and proved = BGS_SOLVE_UNKNOWN on its legal slots.
 * Soundness.  The tree is a tree of lines, and every tagged line ends in a true end of the game below the cap, so a tag
 * is a statement about the game without the cap and needs no repetition rule.
 * Known weakness: as for Connect, an arm proved DRAW stops collecting visits, so an undecided root can prefer an OPEN arm
 * whose Q is below a draw's.  The forest (bgs_bounce_forest_search) does not prove. */
BGS_API int bgs_bounce_search_moves_proving(bgs_batch* b, uint64_t seed, int32_t iterations, int32_t leaf_playouts,
                                            int32_t explore, int32_t max_plies, int policy, int32_t edges, int32_t* counts,
                                            int32_t* visits, int32_t* best, int32_t* nodes, int32_t* used, int8_t* proved,
                                            int32_t* done, void* workspace, size_t workspace_bytes, int on_device);
/* The same search on trees that outlive a launch (Bounce, bit-packed boards only), the sibling of
 * bgs_connect_forest_*: a FOREST is caller-owned device memory that holds one tree per board of the batch, each with room
 * for `nodes_cap` (C) nodes, the root included, and `edges` (E) pool edges, and persists from launch to launch.  An agent
 * that plays a game searches, plays, advances the trees by the moves played and searches again: the subtree under the
 * move played is carried into the next search.
 * Layout.  Opaque, 256-byte aligned; bgs_bounce_forest_bytes says how large.  Per tree: a 64-byte header (the nodes in
 * use, 0 for an emptied tree; the edges in use; the absolute ply count of the position the root stands for; the effective
 * cap min(max_plies, 65535) under which the tree's "capped" edges were written; that position as the batch's four 64-bit
 * planes), E edges of four 32-bit words (n, s, child, move), C node-table entries (first edge, arms) and C words of
 * descent path (a descent leaves every node at most once; the words mean nothing between launches), a tree's share
 * rounded up to 256 bytes.  2 <= C <= BGS_BOUNCE_FOREST_MAX_NODES (the re-rooting keeps a bit a node on the chip) and
 * BGS_BOUNCE_SEARCH_MIN_EDGES(height, width) <= E <= BGS_BOUNCE_FOREST_MAX_EDGES (every word index of a share fits 32
 * bits).
 * bgs_bounce_forest_search.  For board i, at the start of the launch, tree i is CARRIED if restart == 0, board i is
 * running and has arms, the nodes in use are in [1, C], the edges in use are in [the arms of the root, E], the recorded
 * planes and the recorded ply count equal board i's (the ply keys the draws and decides the cap, so it is part of the
 * position), the recorded cap equals min(max_plies, 65535) of this launch (a carried "capped" edge is only true under
 * the cap it was written with), and the root's N (the sum of its n[a]) plus T * P is below 2^31.  Otherwise the tree is
 * emptied: a running board with arms is left with its root node and the root's arms, and board i is recorded; a board
 * without arms (ended, no move, 65535 plies) gets an emptied tree, all-zero outputs, best = -1 and used = 0.  THE FIRST
 * LAUNCH ON FRESH MEMORY MUST PASS restart != 0: memory that was never written may pass the check by accident.  Then T
 * iterations of bgs_bounce_search_moves, word for word, with one change in step 4: a node is made for p' if and only if
 * the edge has no child, the tree holds fewer than C nodes and (edges in use) + A(p') <= E; either way the P playouts
 * start from p', and an edge whose node did not fit is tried again the next time it is taken.  Playout j of iteration t
 * is the game G = ((first_game + i) * T + t) * P + j with this launch's T: the caller varies `seed` from launch to
 * launch.  Selection, Q, E, lg, isqrt, the sentinels of ended and capped edges, the back-propagation, bgs_steps and
 * sharding by first_game are unchanged.
 * Outputs: counts int32[n][width][height * width][3] = W/D/L through each root slot of THIS launch's playouts; visits
 * int32[n][width][height * width] = the root's n by slot, carried visits included; best int32[n] by the rule of
 * bgs_bounce_search_moves over those visits and s; nodes int32[n] = the nodes in the tree at the end, the root not counted
 * (<= C - 1); used int32[n] = the pool edges in use at the end; carried int32[n] = the nodes in the tree at the start
 * after the check, the root not counted (0 for a tree that was emptied).  All but counts may be NULL.  With restart != 0,
 * C >= T + 1 and the same E the outputs and bgs_steps are those of bgs_bounce_search_moves, bit for bit, and carried is
 * all zeros.
 * `forest` is always a 256-byte aligned device pointer.  on_device != 0: the outputs are 16-byte aligned device pointers
 * and the call is an enqueue on the batch's stream with no synchronisation and no allocation; otherwise they are host
 * buffers, filled when the call returns.
 * bgs_bounce_forest_advance re-roots every tree: slots int32[n] in the encoding of `best`, slot x * height * width + c of
 * the position the tree's root stands for.  For tree i with s = slots[i]: s < 0: the tree is untouched.  The root has an
 * arm of that slot (its stored move's target cell is c and its source cell lies in column x) whose child word is a node
 * r in (0, nodes in use): the subtree of r becomes the tree and r becomes node 0; every kept node keeps its arms, n, s,
 * moves and ended / capped sentinels, child words are renumbered, kept nodes stay in their relative order and their edge
 * blocks are packed from edge 0 in that order; the header gets the new counts, the move is applied to the recorded planes
 * and the recorded ply count goes up by 1.  Anything else -- a slot out of range, no such arm, an arm never expanded, an
 * edge that ends the game or is capped, a node that did not fit, a tree that is already empty --: the tree is emptied,
 * and the next search starts it anew from the batch's board.  kept int32[n] (may be NULL) = the nodes after the call, the
 * root not counted.  The call neither reads nor modifies the batch's boards: the caller plays the same moves with
 * bgs_step_actions, before or after, and a tree whose board went another way fails the next search's check.  Two plies
 * (the own move, then the reply) are two calls.  A header that is out of range, or a child index at or beyond the nodes
 * in use, is read as "none": memory that never held a tree is never indexed out of its own share.  The work is that of
 * the nodes and edges in use, one launch, in place.  on_device: where slots and kept live, as above.
 * Refused (BGS_ERR_ARG, with a message that names the argument; the outputs and the forest are untouched): a Connect
 * batch, a generic batch, C < 2 or C > BGS_BOUNCE_FOREST_MAX_NODES, E below BGS_BOUNCE_SEARCH_MIN_EDGES or above
 * BGS_BOUNCE_FOREST_MAX_EDGES, what bgs_bounce_search_moves refuses for T, P, explore, max_plies, the policy and the
 * pointers, a NULL or misaligned forest, forest_bytes too small, NULL slots. */
#define BGS_BOUNCE_FOREST_MAX_NODES 65536
#define BGS_BOUNCE_FOREST_MAX_EDGES (1 << 29)
BGS_API int bgs_bounce_forest_bytes(const bgs_batch* b, int32_t nodes, int32_t edges, size_t* bytes);
BGS_API int bgs_bounce_forest_search(bgs_batch* b, uint64_t seed, int32_t iterations, int32_t leaf_playouts, int32_t explore,
                                     int32_t max_plies, int policy, int32_t nodes_cap, int32_t edges, int restart,
                                     int32_t* counts, int32_t* visits, int32_t* best, int32_t* nodes, int32_t* used,
                                     int32_t* carried, void* forest, size_t forest_bytes, int on_device);
BGS_API int bgs_bounce_forest_advance(bgs_batch* b, const int32_t* slots, int32_t nodes_cap, int32_t edges, int32_t* kept,
                                      void* forest, size_t forest_bytes, int on_device);
/* PUCT tree search whose leaves the CALLER evaluates (Bounce, bit-packed boards only), the sibling of
 * bgs_connect_guided_step: what that text says holds here unless restated -- one call is one simulation of every tree,
 * EVERY POINTER IS A DEVICE POINTER (`trees` 256-byte aligned, the rest 16-byte aligned), the call is one enqueue on the
 * batch's stream with no synchronisation, no allocation and no RNG, there is no host variant, the boards and bgs_steps
 * are untouched, the flags and kinds are the BGS_GUIDED_* values and BGS_GUIDED_MAX_VISITS bounds the root's N.
 * Slots and arms are those of bgs_bounce_search_moves.  With S = width * height * width, slot x * height * width + c is
 * the piece in column x of the active row moving to cell c, and a position's arms are its legal moves in ascending slot
 * order.  priors float32[n][S], values float32[n].
 * Tree.  `nodes_cap` (C) nodes, the root included, 2 <= C <= BGS_BOUNCE_FOREST_MAX_NODES, and a pool of `edges` (E)
 * edges, BGS_BOUNCE_SEARCH_MIN_EDGES(height, width) <= E <= BGS_BOUNCE_FOREST_MAX_EDGES; a node with A arms takes A pool
 * edges when it is made, the root its own first.  An edge holds n, s, the child (or the sentinel of an edge that ends the
 * game, or of one whose position holds the cap), its move and P.  Opaque; bgs_bounce_guided_bytes says how large; a
 * tree's share is rounded up to 256 bytes and holds, between calls: the nodes and the edges in use; the root position
 * (four planes), its ply count and the effective cap min(max_plies, 65535); whether the root has its P; the pending
 * leaf: its kind, its path of edge indices (at most C) and, for an EVALUATE leaf, its four planes and its ply count.
 * One step, for board i, in this order:
 *   1. Check.  The tree is LIVE if BGS_GUIDED_RESTART is not set, the board is running, has arms and holds fewer than
 *      65535 plies, the nodes in use are in [1, C], the edges in use are in [the arms of the root, E], and the recorded
 *      planes, ply count and cap equal board i's and this call's.  Otherwise the tree is emptied and the pending leaf is
 *      dropped; a running board with arms gets node 0 with its arms (P = 0, not expanded) and is recorded.  THE FIRST
 *      CALL ON FRESH MEMORY MUST PASS BGS_GUIDED_RESTART.  Every word read back from a share is used only within its
 *      bounds: memory that passes the check by accident may give a wrong tree, never a store outside its own share.
 *   2. Apply.  The value and the priors are quantised as in bgs_connect_guided_step, word for word, over the leaf's
 *      legal slots in place of its legal columns: w = floor(min(x, 1.0f) * 65536.0f) for x > 0, else 0; W = the sum; if
 *      W = 0 every legal arm gets w = 1; P = floor(w * 65536 / W).  sigma = 1024 + v.  A TERMINAL leaf has sigma = 0 if
 *      the last edge won for its mover (a move into the goal row; a side to move without a move while the mover has
 *      one) and sigma = 1024 for a draw and for a leaf that runs but holds the cap.  An EVALUATE leaf that is not the
 *      root becomes a node if and only if its edge has no child, fewer than C nodes are in use and (edges in use) +
 *      A(leaf) <= E; a node that does not fit is tried again the next time the edge is taken (the forest's rule).  An
 *      EVALUATE leaf that IS the root only receives P.  Every edge k of the path gets n += 1, and s += sigma if node k's
 *      mover is the leaf's mover, else s += 2048 - sigma.
 *   3. Report, through the outputs that are not NULL: visits and scores int32[n][S] = the root's n and s by slot, zeros
 *      on illegal slots; best[i] = the slot with the most visits, then the larger s, then the lower slot, -1 for an
 *      emptied tree or a root with no visit; nodes[i] = the nodes in use, the root not counted; used[i] = the pool edges
 *      in use.
 *   4. Select, unless BGS_GUIDED_FINISH is set, the tree is emptied or the root's N has reached BGS_GUIDED_MAX_VISITS:
 *      each gives IDLE.  An unexpanded root is the leaf: EVALUATE with an empty path.  Otherwise take the arm with the
 *      largest U = Q + E, ties to the lowest arm; Q, E, isqrt((N + 1) << 12), the clamp on N and the range of `cpuct`
 *      are the Connect text's (there is no unplayed-arm-first rule).  Play the stored move; then, the first that applies:
 *      the edge word is an ended or a capped sentinel: TERMINAL, with no move search; the new position ended: the ended
 *      sentinel is written, TERMINAL; it runs and its ply count is at or beyond the cap: the capped sentinel is written,
 *      TERMINAL, and no node is made for it, now or later; the edge has a child: descend; otherwise EVALUATE.
 *      leaf_grid int8[n][h][w] in bgs_read_grid's Bounce encoding, leaf_player[i] = the leaf's ply & 1, leaf_kind[i];
 *      leaf_targets uint64[n][w] (may be NULL): for an EVALUATE leaf the target masks of the pieces in columns 0 .. w - 1
 *      of the leaf's active row, in the bit layout of bgs_bounce_read_targets -- what a caller needs to mask its softmax
 *      --, zeros for every other kind.  IDLE rows carry the root's grid and player.
 * Refused (BGS_ERR_ARG, with a message that names the argument; the outputs and the trees are untouched): a Connect batch,
 * a generic batch, C or E out of range, cpuct outside [0, 4096], max_plies < 1, unknown flag bits, BGS_GUIDED_RESTART
 * together with BGS_GUIDED_FINISH, NULL trees, leaf_grid, leaf_player or leaf_kind, NULL priors or values without
 * BGS_GUIDED_RESTART, a misaligned pointer, trees_bytes too small. */
BGS_API int bgs_bounce_guided_bytes(const bgs_batch* b, int32_t nodes, int32_t edges, size_t* bytes);
BGS_API int bgs_bounce_guided_step(bgs_batch* b, int32_t nodes_cap, int32_t edges, int32_t cpuct, int32_t max_plies,
                                   uint32_t flags, const float* priors, const float* values,
                                   int8_t* leaf_grid, int8_t* leaf_player, int32_t* leaf_kind, uint64_t* leaf_targets,
                                   int32_t* visits, int32_t* scores, int32_t* best, int32_t* nodes, int32_t* used,
                                   void* trees, size_t trees_bytes);
/* Exact solve of every column of every board (Connect, bit-packed boards only): a depth-first alpha-beta search a
 * (board, column), no RNG.  Entry [i][c] is seen from the player to move at board i; the lines searched are at most
 * `depth` plies long, column c itself counted (depth >= height * width: a full solve).
 *   codes int8[n][width]   BGS_SOLVE_WIN: after c the mover can force a win that ends at most `depth` plies from board i;
 *                          BGS_SOLVE_LOSS: after c the opponent can force one within the same horizon;
 *                          BGS_SOLVE_DRAW: neither, and board i has at most `depth` empty cells (no line was cut: exact);
 *                          BGS_SOLVE_UNKNOWN: neither, and the horizon cut some lines;
 *                          BGS_SOLVE_BUDGET: the search of this (board, column) visited more than max_nodes positions;
 *                          BGS_SOLVE_NONE: an illegal column or an ended board.
 *   plies int16[n][width]  (may be NULL) WIN / LOSS: plies from board i to the end when the winner wins fastest and the
 *                          loser loses slowest (1 = c wins at once); DRAW: board i's empty cells; otherwise 0.
 *   nodes                  (may be NULL) positions the search visited in all; its value is implementation-defined.
 * A draw needs a full board, and empty cells and horizon fall by one a ply together: either no line is cut (W / D / L
 * exact) or no draw is reachable (W / L / unknown).  Only BUDGET depends on max_nodes or on the search order.
 * on_device != 0: device pointers (codes and plies 16-byte aligned, nodes 8-byte aligned), enqueued on the batch's
 * stream, no synchronisation, no allocation; otherwise host buffers, filled when the call returns.  The boards and
 * bgs_steps are not modified.  Refused (BGS_ERR_ARG): Bounce and generic batches, depth < 1, max_nodes < 1, NULL codes,
 * a misaligned device pointer. */
#define BGS_SOLVE_NONE (-2)
#define BGS_SOLVE_LOSS (-1)
#define BGS_SOLVE_DRAW 0
#define BGS_SOLVE_WIN 1
#define BGS_SOLVE_UNKNOWN 2
#define BGS_SOLVE_BUDGET 3
BGS_API int bgs_connect_solve_actions(bgs_batch* b, int32_t depth, int64_t max_nodes, int8_t* codes, int16_t* plies,
                                      uint64_t* nodes, int on_device);
/* Exact horizon search of every legal move of every board (Bounce, bit-packed boards only: at most 64 cells, piece
 * values <= 15): a depth-first alpha-beta search a legal (board, move), no RNG.  Bounce games can cycle and have no
 * bound on their length, so there is no full solve: for board i (running, player P to move) and the move m of the piece
 * in column x of the active row to cell c = ty * width + tx (the slots of bgs_bounce_evaluate_moves), the lines searched
 * are at most `depth` plies long, counted from board i (m itself is ply 1), and a game ends exactly as the rules say: a
 * landing in the mover's goal row wins; a move after which the opponent has no legal move wins for the mover if the
 * mover itself could still move, and is a draw if neither can.
 *   codes int8[n][width][height * width]
 *       BGS_SOLVE_WIN      after m, P can force the game to end with P as winner at most `depth` plies from board i;
 *       BGS_SOLVE_LOSS     after m, the opponent can force its own win within the same horizon;
 *       BGS_SOLVE_DRAW     m itself ends the game as a draw (ply 1).  Deeper draws are not reported: a drawn end inside a
 *                          line scores like a cut line (neither side has won), so it can only turn a would-be WIN / LOSS
 *                          into UNKNOWN, never the reverse;
 *       BGS_SOLVE_UNKNOWN  none of the above: within the horizon neither side can force a win;
 *       BGS_SOLVE_BUDGET   the search of this (board, move) visited more than max_nodes positions;
 *       BGS_SOLVE_NONE     an illegal slot, an ended board, a board without a legal move.
 *   plies int16[n][width][height * width]  (may be NULL) WIN / LOSS: plies from board i to the end when the winner wins
 *       as fast as it can and the loser loses as slowly as it can (1 = m wins at once); DRAW: 1; otherwise 0.
 *   nodes  (may be NULL) positions the search visited in all; its value is implementation-defined.
 * Only BUDGET depends on max_nodes or on the order in which moves are searched; everything else is a function of (grid,
 * player, depth) -- the board's ply counter beyond its parity (the player) plays no part, nor do first_game, the way a
 * batch is split or the launch geometry.  A deeper horizon never changes a WIN or LOSS or its plies.  The boards,
 * bgs_steps and the RNG are not touched.
 * on_device: as bgs_connect_solve_actions (codes and plies 16-byte aligned, nodes 8-byte aligned device pointers,
 * enqueued on the batch's stream, no synchronisation, no allocation: scratch comes out of the batch's staging region;
 * otherwise host buffers, filled when the call returns).  Refused (BGS_ERR_ARG): Connect and generic batches, depth < 1,
 * depth > BGS_BOUNCE_SOLVE_MAX_DEPTH (what the search stack is sized for; never clamped: a deeper Bounce horizon is a
 * different question), max_nodes < 1, NULL codes, a misaligned device pointer. */
#define BGS_BOUNCE_SOLVE_MAX_DEPTH 16
BGS_API int bgs_bounce_solve_moves(bgs_batch* b, int32_t depth, int64_t max_nodes, int8_t* codes, int16_t* plies,
                                   uint64_t* nodes, int on_device);
/* env-steps (transitions applied to running boards) since the last bgs_reset / bgs_reset_steps */
BGS_API int bgs_steps(bgs_batch* b, uint64_t* steps);
BGS_API int bgs_reset_steps(bgs_batch* b);

/* ---- observation: packed state -> reference layout, into HOST buffers ----------------------------- */
BGS_API int bgs_read_grid(bgs_batch* b, int8_t* grid);      /* State::get_grid   (connect.cpp:42, bounce.cpp:39) int8[n][h][w] */
BGS_API int bgs_read_player(bgs_batch* b, int8_t* player);  /* State::get_player (connect.cpp:40, bounce.cpp:37) int8[n] */
BGS_API int bgs_read_ended(bgs_batch* b, uint8_t* ended);   /* State::has_ended  (connect.cpp:39, bounce.cpp:36) uint8[n] */
BGS_API int bgs_read_winner(bgs_batch* b, int8_t* winner);  /* JSON key "winner" (tests/test_connect.py:137) int8[n] */
BGS_API int bgs_read_reward(bgs_batch* b, int8_t* reward);  /* State::get_reward (connect.cpp:41, bounce.cpp:38) int8[n][2] */
BGS_API int bgs_read_plies(bgs_batch* b, int32_t* plies);   /* plies played, int32[n] */
/* Connect: State::get_actions as a mask, uint8[n][width] (connect.cpp:43) */
BGS_API int bgs_read_legal(bgs_batch* b, uint8_t* legal);
/* number of legal actions of the side to move, int32[n] (len(state.actions)) */
BGS_API int bgs_read_action_count(bgs_batch* b, int32_t* count);
/* Bounce: State::get_actions_at for every column of the active row (bounce.cpp:41): uint64[n][width + 1]; entry
 * i < width has bit (y*width + x) set for every legal target of the piece in column i of the active row (0 if
 * none); entry [width] is the active row's y (all ones when the board has ended or nothing can move) */
BGS_API int bgs_bounce_read_targets(bgs_batch* b, uint64_t* targets);
/* the same observations into DEVICE memory, enqueued on the batch's stream (no synchronisation): what =
 * 'g' grid int8[n][h][w] (16-byte aligned destination), 'l' Connect legal mask uint8[n][w], 'c' action count int32[n],
 * 't' Bounce target masks uint64[n][w + 1], 'r' reward int8[n][2] */
BGS_API int bgs_export_device(bgs_batch* b, int what, void* device_dst);
/* N2, ONE call per policy ply: bgs_step_actions with the actions in DEVICE memory (int32[n], Bounce int32[n][4]), then --
 * in the same pass over the batch where the kernel exists (one-word Connect boards, even n; otherwise the separate
 * kernels back to back) -- what the policy needs for its next choice, of the boards AFTER the move: device_observation =
 * Connect uint8[n][width] legal mask ('l' above; 16-byte aligned), Bounce uint64[n][width + 1] target masks ('t');
 * device_ended uint8[n] State::has_ended (may be NULL); device_status int32[n] per-board result as bgs_step_actions
 * (may be NULL).  Everything is an enqueue on the batch's stream: no synchronisation, no allocation, capturable in a
 * HIP graph.  The loop README.md:57-65 / examples/agent.py:13-27 make per board, for a batch and a device-side policy:
 * observation -> policy -> bgs_step_actions_observe -> observation -> ... */
BGS_API int bgs_step_actions_observe(bgs_batch* b, const int32_t* device_actions, void* device_observation, uint8_t* device_ended,
                             int32_t* device_status);
/* ... and as the step of a VECTOR ENVIRONMENT (the learner's side of README.md:57-65 for n boards at once): the same call
 * plus device_reward int8[n][2] = State::get_reward of the boards after the move (connect.cpp:41 / bounce.cpp:38: the
 * finished game's pair where device_ended is set, 0 / 0 while it runs; may be NULL), and with BGS_ENV_AUTO_RESET a board
 * that has ended is put back to Config::sample_initial_state() (connect.cpp:32, bounce.cpp:29) in the same pass -- its
 * observation is then the new game's, its ended flag and reward still those of the game that just finished.  Bit-packed
 * boards only with BGS_ENV_AUTO_RESET. */
#define BGS_ENV_AUTO_RESET 1u
BGS_API int bgs_env_step(bgs_batch* b, const int32_t* device_actions, void* device_observation, uint8_t* device_ended,
                 int8_t* device_reward, int32_t* device_status, uint32_t flags);

/* ---- compact outcomes for the multi-GPU reward gather ------------------------------------------------ */
/* 2 bits per board (0 running, 1 / 2 that player won, 3 draw), 4 boards per byte, board 4i in the low bits:
 * device_dst uint8[(n + 3) / 4].  A reward pair (State::get_reward, connect.cpp:41 / bounce.cpp:38) is a function of
 * this code, so ranks exchange 0.25 B per game over xGMI instead of 2 B and expand after the gather. */
BGS_API int bgs_pack_outcomes(bgs_batch* b, void* device_dst);
/* bgs_rollout followed by bgs_pack_outcomes in one call; kernels that can (one-word Connect boards, compile-time
 * multi-word geometries) write the codes themselves, so no second launch follows the rollout.  device_dst: 16-byte
 * aligned, ((n + 63) / 64) * 16 bytes -- what a rank hands to the RCCL gather. */
BGS_API int bgs_rollout_pack(bgs_batch* b, uint64_t seed, int32_t max_plies, uint32_t flags, void* device_dst);
/* inverse, batch-independent: packed codes of n boards -> reward int8[n][2] (8-byte aligned), on `device` / stream */
BGS_API int bgs_expand_outcomes(int device, void* hip_stream, const void* device_packed, int64_t n, int8_t* device_reward);

/* ---- asynchronous hand-over to HOST memory ------------------------------------------------------------
 * The reference hands `reward` out as a host ndarray on every call (State::get_reward, connect.cpp:41 / bounce.cpp:38,
 * tensor.hpp:69-87).  For a batch the hand-over is part of the path: these entry points enqueue it on the batch's
 * stream and return at once; the caller waits on a bgs_event (or bgs_synchronize) before reading the host buffer.
 * Destinations must be page-locked (bgs_host_alloc, hipHostMalloc or torch pin_memory) for the copy to be
 * asynchronous. */
typedef struct bgs_event bgs_event; /* opaque: a HIP event on the batch's device */
BGS_API int bgs_host_alloc(size_t bytes, void** host_ptr);
BGS_API int bgs_host_free(void* host_ptr);
BGS_API int bgs_event_create(int device, bgs_event** out);
BGS_API int bgs_event_destroy(bgs_event* e);
BGS_API int bgs_event_synchronize(bgs_event* e);       /* block the calling thread until the work recorded before it is done */
BGS_API int bgs_event_query(bgs_event* e, int* done);  /* *done = 1 when that work has completed */
/* reward int8[n][2] -> host_dst, then record `done` (may be NULL) */
BGS_API int bgs_read_reward_async(bgs_batch* b, int8_t* host_dst, bgs_event* done);
/* 2-bit outcome codes (as bgs_pack_outcomes) uint8[(n + 3) / 4] -> host_dst, then record `done` (may be NULL): 8x
 * fewer bytes over PCIe than the int8 pairs; bgs_expand_outcomes_host finishes the job on the host */
BGS_API int bgs_read_outcomes_async(bgs_batch* b, uint8_t* host_dst, bgs_event* done);
/* host-side inverse of bgs_pack_outcomes for games [first, first + count) (first a multiple of 4): a table look-up,
 * no game rule; reward int8[n][2] is indexed by game, so callers may split a batch over threads */
BGS_API int bgs_expand_outcomes_host(const uint8_t* packed, int64_t first, int64_t count, int8_t* reward);
/* bgs_rollout followed by bgs_read_reward_async (codes == 0) or bgs_read_outcomes_async (codes != 0): one call per
 * batch step for host loops that are launch-rate bound */
BGS_API int bgs_rollout_to_host(bgs_batch* b, uint64_t seed, int32_t max_plies, uint32_t flags, void* host_dst, int codes,
                        bgs_event* done);

/* A reward sink delivers the rewards of successive batch steps into caller-owned host arrays int8[n][2] while the GPU
 * goes on playing: per submission the outcome codes cross PCIe into one of `slots` pinned buffers and `threads` host
 * worker threads expand them as soon as the copy has landed (with more than one thread the first one only waits for
 * the arrival events and releases the others, so the event latency of a submission overlaps the expansion of the one
 * before it).  Submissions complete in order.  Environment: BGS_SINK_SPIN_US (microseconds a waiter spins before it
 * sleeps, default 0), BGS_SINK_POLL (poll the arrival event), BGS_NO_STREAM_STORES. */
typedef struct bgs_reward_sink bgs_reward_sink;
BGS_API int bgs_sink_create(int device, int64_t max_games, int slots, int threads, bgs_reward_sink** out);
BGS_API int bgs_sink_destroy(bgs_reward_sink* s);
/* enqueue on the batch's stream: the pack kernel stores the codes straight into a page-locked slot (device-mapped host
 * memory: no copy call), an event marks their arrival, the workers expand into host_reward int8[n][2] (any host
 * memory); *ticket identifies the submission.  Blocks only while all slots are still in use. */
BGS_API int bgs_sink_submit(bgs_reward_sink* s, bgs_batch* b, int8_t* host_reward, int64_t* ticket);
/* bgs_rollout followed by bgs_sink_submit: one library call per batch step */
BGS_API int bgs_sink_rollout(bgs_reward_sink* s, bgs_batch* b, uint64_t seed, int32_t max_plies, uint32_t flags,
                     int8_t* host_reward, int64_t* ticket);
/* the same for packed codes that are already on the device (the RCCL-gathered codes of all ranks on rank 0):
 * device_packed uint8[(n_games + 3) / 4], copied on `hip_stream` */
BGS_API int bgs_sink_submit_packed(bgs_reward_sink* s, void* hip_stream, const void* device_packed, int64_t n_games,
                           int8_t* host_reward, int64_t* ticket);
BGS_API int bgs_sink_wait(bgs_reward_sink* s, int64_t ticket); /* until that submission's rewards are in its host array */
/* A GRID sink hands over the boards themselves -- State::get_grid (connect.cpp:42, bounce.cpp:39; the reference returns
 * a host array through the copying caster tensor.hpp:69-87) for every game of a step: the boards cross PCIe bit-packed
 * (Connect: two bit sets over the cells in reference order, 16 B per 6x7 board instead of 42; Bounce: the four value
 * bit-planes; generic batches: the int8 grid itself), one asynchronous copy per step into a page-locked slot, and the
 * worker threads expand them into the caller's int8[n][height][width] (AVX-512: two masked byte adds per 64 cells).
 * Made for batches like `like` (same game, geometry and size); bgs_sink_submit / bgs_sink_rollout / bgs_sink_wait /
 * bgs_sink_completed / bgs_sink_destroy and bgs_pipeline_* work as for a reward sink, with host_reward = the grid array. */
BGS_API int bgs_grid_sink_create(const bgs_batch* like, int slots, int threads, bgs_reward_sink** out);
/* the host half of it, for games [first, first + count) of a batch of n: `wire` holds `sets` bit sets over the cells
 * (cell = y * width + x), word j of set p of game i at ((uint64_t*)wire)[(p * nwc + j) * n + i], nwc = (cells + 63) / 64;
 * a cell's byte = offset + sum of weights[p] over the sets that contain it (Connect: offset -1, weights 1, 1 for
 * "occupied" and "player 1's"; Bounce: offset 0, weights 1, 2, 4, 8); sets = 0: the wire is the int8 grid.  A table
 * look-up per 8 cells or two masked byte adds per 64 (AVX-512; portable != 0 forces the table), no game rule. */
BGS_API int bgs_expand_grid_host(const void* wire, int64_t n, int cells, int sets, int offset, const int32_t* weights, int64_t first,
                         int64_t count, int8_t* grid, int portable);
/* Submissions to one sink may come from several threads (a ticket and its slot are reserved under the sink's lock);
 * they are delivered in ticket order.  *completed = number of submissions whose rewards are in their host arrays. */
BGS_API int bgs_sink_completed(bgs_reward_sink* s, int64_t* completed);

/* Progress words: monotonic int64 counters in host memory -- typically in a shared-memory segment several processes
 * map -- that consumers sleep on (futex on the low half) instead of polling.  bgs_sink_set_progress makes a sink
 * announce its completed count in *word after every delivery (word = NULL stops that; the word must outlive the sink or
 * be unset first); bgs_progress_store raises *word to `value` (never lowers it) and wakes the sleepers;
 * bgs_progress_wait blocks until each of the `count` words words[i * stride_words] is >= target, or fails with
 * BGS_ERR_RUNTIME after timeout_ms (< 0: no timeout), *laggard = index of the word that was behind. */
BGS_API int bgs_sink_set_progress(bgs_reward_sink* s, int64_t* word);
BGS_API int bgs_progress_store(int64_t* word, int64_t value);
/* A barrier of `count` processes on `count` such words (words[i * stride_words], word `mine` this process's): raises
 * its own word to `epoch` (1, 2, 3, ... from barrier to barrier), then waits until every word is >= epoch -- watching
 * them for up to spin_us microseconds before it sleeps as bgs_progress_wait does.  Ranks of one node that run in step
 * meet within a few microseconds, which a collective on the GPU (a launch, a kernel, a synchronise: tens of microseconds)
 * cannot match; bench.py brackets its timed region with it when the shared array exists. */
BGS_API int bgs_progress_barrier(int64_t* words, int64_t count, int64_t stride_words, int64_t mine, int64_t epoch, int64_t spin_us,
                         int64_t timeout_ms);
BGS_API int bgs_progress_wait(const int64_t* words, int64_t count, int64_t stride_words, int64_t target, int64_t timeout_ms,
                      int64_t* laggard);
/* Confine the calling thread (and the threads it creates later) to the CPUs of the NUMA node `device` hangs off,
 * intersected with what the process may use: its first-touch pages, the sink's workers and the launching thread then
 * sit next to the GPU's PCIe root.  *cpus = size of that set, 0 when the topology is unknown (nothing changed). */
BGS_API int bgs_bind_host_thread(int device, int* cpus);

/* ---- the reward gather over RCCL / xGMI, one process per GPU -------------------------------------------------------
 * The path shards without any exchange (rank r plays global game ids [r * n, (r + 1) * n), bgs_set_first_game); the one
 * collective is the hand-over: every rank's 2-bit outcome codes to rank 0's GPU, from there to rank 0's host array
 * int8[world * n][2] (State::get_reward of all games, connect.cpp:41, in global game order).  A bgs_gather owns a
 * persistent communicator (ncclCommInitRank), a communication stream and a communication thread; rank 0's also owns the
 * reward sink.  Per step the launching thread makes ONE call, bgs_gather_rollout, which enqueues the rollout on the
 * batch's stream and returns; send, receives, copy to the host and expansion follow behind it on other threads and
 * streams while the next rollouts play.  The launcher (torch.distributed, MPI, a file) only has to carry the 128-byte
 * id from rank 0 to the others.  RCCL is loaded on first use (dlopen "librccl.so.1"; BGS_RCCL_LIB=<path> names another
 * library with the same nine nccl* entry points: the tests' shared-memory stand-in, tests/c/fake_rccl.hip).
 * The machinery is per GROUP of steps (BGS_GATHER_BATCH, default slots / 2): one stream wait per launch stream, one
 * group of point-to-point calls, one copy kernel, one event.  Rank 0 receives into device memory and a copy kernel takes
 * the gathered codes to the sink's page-locked slots; BGS_GATHER_DIRECT=1 receives straight into the device-mapped slots.
 * With two ranks or more bgs_gather_create sends one message per peer through the transport in that mode and compares
 * what arrives in host memory (a direct receive that does not deliver falls back to the copy kernel, on stderr and in
 * bgs_gather_info).  A one-rank world has nothing to gather: no thread, no stream, a step is bgs_sink_rollout. */
#define BGS_UNIQUE_ID_BYTES 128
typedef struct bgs_gather bgs_gather;
BGS_API int bgs_gather_unique_id(uint8_t* id /* [BGS_UNIQUE_ID_BYTES] */);   /* rank 0; ncclGetUniqueId */
/* collective over the world (ncclCommInitRank).  n_per_rank: games per rank, a multiple of 4; slots: steps that may be
 * in flight (code buffers per rank; on rank 0 also sink slots); host_threads: rank 0's sink workers. */
BGS_API int bgs_gather_create(int device, int rank, int world, const uint8_t* id, int64_t n_per_rank, int slots, int host_threads,
                      bgs_gather** out);
/* bgs_rollout on `b`, then this rank's codes to rank 0 (and there: everybody's rewards into host_reward, which other
 * ranks pass as NULL).  Every rank makes the same sequence of calls; one thread at a time per gather.  The codes of a
 * step leave in a group with its neighbours: when BGS_GATHER_BATCH steps are there, when somebody waits for one of them
 * (bgs_gather_wait), or by themselves BGS_GATHER_FLUSH_US (default 1000) microseconds after the group's first step was
 * submitted -- so a rank that submits a few steps and then blocks on something else still delivers them.  A step that
 * cannot be enqueued on one rank fails THERE (this call, and every later call on that gather); the rank still posts the
 * step's message -- zeros: rank 0 delivers reward 0 / 0 for those rows -- so that no peer is left waiting. */
BGS_API int bgs_gather_rollout(bgs_gather* g, bgs_batch* b, uint64_t seed, int32_t max_plies, uint32_t flags, int8_t* host_reward,
                       int64_t* ticket);
/* rank 0: that step's rewards of all ranks are in its host array; other ranks: this rank's codes have been sent */
BGS_API int bgs_gather_wait(bgs_gather* g, int64_t ticket);
/* how the gather runs: *direct 1 = receives straight into the sink's device-mapped slots, 0 = device memory + copy kernel;
 * *batch = steps per group of point-to-point calls; *transport_check 0 = none (one rank), 1 = the create-time message
 * arrived intact in the mode asked for, 2 = only after falling back from direct receives.  NULL pointers are skipped. */
BGS_API int bgs_gather_info(const bgs_gather* g, int* direct, int* batch, int* transport_check);
/* what the COMMUNICATOR says about itself, asked once when it was created: *ranks = ncclCommCount, *rank =
 * ncclCommUserRank (-1 each when the transport library has no such entry point).  The first line of an N-GPU run should
 * read ranks == N on every rank: bench.py prints it as gather_rccl.gather_info.ranks. */
BGS_API int bgs_gather_comm(const bgs_gather* g, int* ranks, int* rank);
/* name of the transport library in use ("librccl.so.1", or BGS_RCCL_LIB's path), "" when none could be loaded */
BGS_API const char* bgs_gather_transport(void);
BGS_API int bgs_gather_destroy(bgs_gather* g);

/* ---- the rollout loop as ONE call (README.md:45-72 `while not state.has_ended`, for batch after batch) ------------------
 * Step s (s = 0, 1, ... over the pipeline's life) plays every board of batches[s % depth] from the state `flags` says
 * to the end with seed seed0 + s on that batch's stream; with a hand-over the step's rewards go to
 * host_rewards[j % n_host], j = number of hand-overs so far, through `sink` (one GPU; or N ranks, each delivering its
 * rows of a shared array) or `gather` (RCCL to rank 0; other ranks pass NULL entries) -- exactly one of the two, or
 * neither (then n_host = 0 and every step stays on the device).  bgs_pipeline_enqueue returns when `count` more steps
 * are enqueued; it blocks only while the host array a step is about to reuse is still being delivered (so n_host
 * bounds how far the launching thread runs ahead).  time_stride > 0 brackets every time_stride-th launch of the call
 * with timing events on the batch's stream; bgs_pipeline_kernel_ms (after bgs_pipeline_drain) returns their mean and
 * resets them.  bgs_pipeline_drain: every enqueued step's rewards are in their host arrays and the streams are idle.
 * The batches, sink, gather and host arrays belong to the caller and must outlive the pipeline.  A long call of Connect
 * 6x7x4 steps from the initial state may play two steps in one launch on another batch's stream; every batch's stream
 * waits for the steps that played it before the call returns, and what the steps leave is the same. */
typedef struct bgs_pipeline bgs_pipeline;
BGS_API int bgs_pipeline_create(bgs_batch* const* batches, int depth, bgs_reward_sink* sink, bgs_gather* gather,
                        int8_t* const* host_rewards, int n_host, uint64_t seed0, int32_t max_plies, uint32_t flags,
                        bgs_pipeline** out);
BGS_API int bgs_pipeline_enqueue(bgs_pipeline* p, int64_t count, int handover, int time_stride);
/* the same with the seed of every step given by the caller (seeds[i] for the i-th step of this call) instead of
 * seed0 + step index: a burst of a Python loop over arbitrary seeds (simulator.pipeline.RolloutPipeline.run) */
BGS_API int bgs_pipeline_enqueue_seeds(bgs_pipeline* p, const uint64_t* seeds, int64_t count, int handover);
/* The same for a consumer loop that cannot keep up with a launch per step itself (a Python generator): the seeds are FED, a
 * thread of the pipeline's own enqueues a fed step as soon as the host array it lands in is free -- hand-over j waits until
 * the caller has RELEASED hand-over j - n_host -- and the consumer only waits, reads, releases:
 *     bgs_pipeline_feed(p, seeds, K);  for j: bgs_pipeline_wait(p, j); read host_rewards[j % n_host]; bgs_pipeline_release(p, j);
 * bgs_pipeline_wait also waits for a fed hand-over to be enqueued; bgs_pipeline_drain enqueues and delivers whatever is
 * still fed (and releases every array); bgs_pipeline_destroy drops what was fed and not yet enqueued.  Not for pipelines
 * on a shared array (bgs_pipeline_set_ring).  Steps enqueued with bgs_pipeline_enqueue(_seeds) count as released. */
BGS_API int bgs_pipeline_feed(bgs_pipeline* p, const uint64_t* seeds, int64_t count);
BGS_API int bgs_pipeline_release(bgs_pipeline* p, int64_t handover_index);
/* until hand-over number `handover_index` (0, 1, ... over the pipeline's life) is in its host array
 * host_rewards[handover_index % n_host]; BGS_ERR_ARG when a later hand-over has already reused that array */
BGS_API int bgs_pipeline_wait(bgs_pipeline* p, int64_t handover_index);
BGS_API int bgs_pipeline_drain(bgs_pipeline* p);
BGS_API int bgs_pipeline_progress(const bgs_pipeline* p, int64_t* steps, int64_t* handovers);
BGS_API int bgs_pipeline_kernel_ms(bgs_pipeline* p, double* mean_ms, int* pairs);
/* The bracketed launches' start and end, in ms after the first bracket's start (after bgs_pipeline_drain, BEFORE
 * bgs_pipeline_kernel_ms resets the brackets): where the time of a short timed region goes. */
BGS_API int bgs_pipeline_timeline(bgs_pipeline* p, float* start_ms, float* end_ms, int capacity, int* pairs);
/* N ranks delivering into one shared host array (progress words, see above): rank r's sink announces its deliveries in
 * rank_words[r * word_stride] (bgs_sink_set_progress; the sink must serve this pipeline only), the consumer announces
 * the hand-overs it has released in *consumed.  Every rank: hand-over j waits for the release of hand-over j - n_host
 * before it overwrites that array.  The consumer rank (is_consumer; one per ring) also plays the consumer inside its
 * launch loop: before hand-over j it waits until ALL ranks have delivered hand-over j - lag (1 <= lag < n_host) and
 * releases it; bgs_pipeline_drain consumes the rest. */
BGS_API int bgs_pipeline_set_ring(bgs_pipeline* p, const int64_t* rank_words, int64_t word_stride, int world, int64_t* consumed,
                          int is_consumer, int lag, int64_t timeout_ms);
BGS_API int bgs_pipeline_destroy(bgs_pipeline* p);

/* ---- several GPUs of one node from one host process (no torch.distributed needed) ------------------------------
 * Device devices[r] plays Connect games with global ids [r * n_per_device, (r + 1) * n_per_device) from
 * Config::sample_initial_state() to the end (bgs_rollout), the devices' outcome codes are gathered on devices[0] with
 * RCCL point-to-point calls over xGMI, copied to the host once and expanded into host_reward
 * int8[n_devices * n_per_device][2] in global game order; *steps = env-steps of all devices.  The result equals
 * one batch of n_devices * n_per_device boards on one device.  n_per_device must be a multiple of 4.  One-shot: batches,
 * streams and communicators live for the call.  RCCL is loaded on first use (dlopen "librccl.so.1"). */
BGS_API int bgs_multi_connect_rollout(const int* devices, int n_devices, int height, int width, int count, int64_t n_per_device,
                              uint64_t seed, int8_t* host_reward, uint64_t* steps);
/* the same with everything kept between calls -- batches, streams, code buffers and the communicators (ncclCommInitAll)
 * live as long as the handle: bgs_multi_rollout plays one step (seed) on every device and returns with host_reward
 * int8[n_devices * n_per_device][2] filled and *steps = the step's env-steps */
typedef struct bgs_multi bgs_multi;
BGS_API int bgs_multi_create(const int* devices, int n_devices, int height, int width, int count, int64_t n_per_device, bgs_multi** out);
BGS_API int bgs_multi_rollout(bgs_multi* m, uint64_t seed, int8_t* host_reward, uint64_t* steps);
BGS_API int bgs_multi_destroy(bgs_multi* m);

/* ---- loading boards (State::from_json, connect.cpp:46 / bounce.cpp:45; policy-driven stepping) ---- */
/* grid int8[n][h][w]; player int8[n] (Connect: may be NULL, derived from the stone counts); winner int8[n]
 * (NULL = all running; Connect re-derives wins and draws from the grid when NULL); plies int32[n] (Bounce; NULL =
 * player parity).  status (host int32[n], may be NULL) reports malformed boards, which are left untouched. */
BGS_API int bgs_write_state(bgs_batch* b, const int8_t* grid, const int8_t* player, const int8_t* winner,
                    const int32_t* plies, int32_t* status);

/* ---- one round trip for the object API -------------------------------------------------------------- */
/* What one `State` / `Action` operation of the reference needs (connect.cpp:39-46,52; bounce.cpp:36-45,51), fused
 * into one upload, one launch sequence, one download and one synchronisation (batches of at most 4096 boards):
 *   grid != NULL     load the boards first (as bgs_write_state; player and winner required, plies optional);
 *   actions != NULL  then apply one caller-chosen move per board (as bgs_step_actions; negative first entry skips);
 *   then observe: grid int8[n][h][w], player int8[n], winner int8[n], plies int32[n] and the legal moves of the side
 *   to move -- Connect: uint8[n][width] mask, Bounce: uint64[n][width + 1] target masks (bgs_bounce_read_targets) --
 *   and reward int8[n][2] as the device holds it (State::get_reward; may be NULL).
 * status int32[n]: 0, BGS_ERR_ARG (malformed board: nothing loaded) or BGS_ERR_ILLEGAL (move refused). */
BGS_API int bgs_transition(bgs_batch* b, const int8_t* grid, const int8_t* player, const int8_t* winner, const int32_t* plies,
                   const int32_t* actions, int32_t* status, int8_t* grid_out, int8_t* player_out, int8_t* winner_out,
                   int32_t* plies_out, void* legal_out, int8_t* reward_out);

#ifdef __cplusplus
}
#endif
#endif
