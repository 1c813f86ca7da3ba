// bgs_capi.hip -- the C ABI of libbgs.so (include/bgs.h): batch lifetime, arena carving, host<->device staging and
// kernel launches.  No game arithmetic happens on the host: every rule is evaluated by the HIP kernels in
// connect_kernels.hip / bounce_kernels.hip.  There is NO CPU fallback; without a GPU every compute entry point fails
// with BGS_ERR_NO_DEVICE.
#include "../../include/bgs.h"

#include <chrono>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <new>
#include <string>
#include <unordered_map>

#include "bgs_capi_util.h"
#include "bgs_common.h"
#include "bgs_internal.h"
#include "output_plan.h"

// every kernel translation unit carries the hash of its own source, headers and compile flags (csrc/Makefile: -DBGS_TU_ID)
extern "C" const char bgs_tu_id_connect[];
extern "C" const char bgs_tu_id_bounce[];
extern "C" const char bgs_tu_id_generic[];
extern "C" const char bgs_tu_id_evaluate[];
extern "C" const char bgs_tu_id_search[];
extern "C" const char bgs_tu_id_solve[];

namespace {
thread_local char g_error[512] = "";
}

namespace bgs {
#ifdef BGS_TEST_HOOKS
const char* experiment(const char* name) {
    const char* all = getenv("BGS_EXPERIMENT");
    if (!all || !name) return nullptr;
    thread_local std::string value;
    const size_t len = strlen(name);
    for (const char* p = all; *p;) {
        const char* end = strchr(p, ';');
        if (!end) end = p + strlen(p);
        while (p < end && *p == ' ') ++p;
        if ((size_t)(end - p) > len && strncmp(p, name, len) == 0 && p[len] == '=') {
            value.assign(p + len + 1, end);
            return value.c_str();
        }
        if ((size_t)(end - p) == len && strncmp(p, name, len) == 0) {   // a bare name: "on"
            value = "1";
            return value.c_str();
        }
        p = *end ? end + 1 : end;
    }
    return nullptr;
}
#endif

int fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_error, sizeof(g_error), fmt, ap);
    va_end(ap);
    return code;
}
}  // namespace bgs

namespace {

using bgs::fail;

constexpr size_t kAlign = 256;
constexpr size_t kStepBytes = (size_t)BGS_STEP_SHARDS * BGS_STEP_STRIDE * sizeof(unsigned long long);
inline size_t align_up(size_t v) { return (v + kAlign - 1) / kAlign * kAlign; }

struct Layout {
    size_t planes, status, plies, reward, steps, worklist, work_count, pool, gen_masks, gen_cfg, staging, total, staging_bytes;
};

// planes > 0: bit-packed boards (planes x uint64 per board); planes == 0: the generic layout, int8[n][h][w] in the same
// region.  legal_bytes: bytes per board of the legal-move record bgs_transition returns.
Layout layout_for(int planes, int64_t n, int h, int w, size_t legal_bytes = 0, bool bounce_pool = false) {
    Layout l;
    size_t off = 0;
    size_t board_bytes = (size_t)planes * 8;  // the region must hold whichever form the batch turns out to use
    if (board_bytes < (size_t)h * w && legal_bytes) board_bytes = (size_t)h * w;
    l.planes = off; off += align_up(board_bytes * n);
    l.status = off; off += align_up((size_t)n);
    l.plies = off; off += align_up((size_t)n * 2);
    l.reward = off; off += align_up((size_t)n * 2);
    l.steps = off; off += align_up(kStepBytes);
    l.worklist = off; off += align_up((size_t)n * 4);
    l.work_count = off; off += align_up(sizeof(uint32_t) * 2 * BGS_BOUNCE_MAX_PASSES);
    // packed Bounce boards only: the piece-list rollout's device-wide pool of parked boards (counters + entries,
    // bounce_unit.h; 3 MB).  Two-word Connect boards (8x8, 9x10: four planes as well) do not pay for it (round-4 advisor).
    l.pool = off; off += bounce_pool ? align_up(sizeof(uint32_t) * BGS_BOUNCE_POOL_WORDS) : 0;
    l.gen_masks = off; off += align_up(sizeof(uint64_t) * 6 * (BGS_GENERIC_BOUNCE_MAX_CELLS / 64));
    l.gen_cfg = off; off += align_up((size_t)h * w);
    size_t per_board = (size_t)h * w;
    if (per_board < (size_t)8 * (w + 1)) per_board = (size_t)8 * (w + 1);
    if (per_board < 16) per_board = 16;
    if (legal_bytes < per_board) legal_bytes = per_board;
    // unpack / pack scratch for every board, plus bgs_transition's in-block and out-block (object API: <= 4096 boards)
    const size_t small = n < 4096 ? (size_t)n : 4096;
    l.staging_bytes = (size_t)n * (per_board + 16) + small * (per_board + legal_bytes + 96) + 8 * kAlign;
    l.staging = off; off += align_up(l.staging_bytes);
    l.total = off;
    return l;
}

int check_device(int device) {
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count <= 0)
        return fail(BGS_ERR_NO_DEVICE, "no HIP device available (%s); libbgs has no CPU fallback",
                    e == hipSuccess ? "device count is 0" : hipGetErrorString(e));
    if (device < 0 || device >= count) return fail(BGS_ERR_ARG, "device %d out of range (0..%d)", device, count - 1);
    return BGS_OK;
}

bool force_generic() { return bgs::experiment("force_generic") != nullptr; }

// *generic = 1: outside the bit-packed representation's limits (or BGS_FORCE_GENERIC): served by generic_kernels.hip
int connect_geom(int h, int w, int k, ConnectGeom* cg, int* generic) {
    NEED(h >= 1 && h <= BGS_GENERIC_CONNECT_MAX_DIM, "Connect height %d outside 1..%d", h, BGS_GENERIC_CONNECT_MAX_DIM);
    NEED(w >= 1 && w <= BGS_GENERIC_CONNECT_MAX_DIM, "Connect width %d outside 1..%d", w, BGS_GENERIC_CONNECT_MAX_DIM);
    NEED(k >= 1, "Connect count %d must be positive", k);
    const int bits = w * (h + 1);
    *generic = force_generic() || h > BGS_CONNECT_MAX_H || w > BGS_CONNECT_MAX_W || bits > 64 * BGS_CONNECT_MAX_WORDS;
    cg->h = h; cg->w = w; cg->k = k; cg->nw = *generic ? 0 : (bits + 63) / 64;
    return BGS_OK;
}

bool bounce_size_ok(int h, int w) {
    return h >= 3 && w >= 1 && h <= BGS_GENERIC_BOUNCE_MAX_DIM && w <= BGS_GENERIC_BOUNCE_MAX_DIM &&
           h * w <= BGS_GENERIC_BOUNCE_MAX_CELLS;
}

// cfg == nullptr: size check only (arena size query; the values decide between packed and generic at create time,
// the arena size covers both)
int bounce_geom(const int8_t* cfg, int h, int w, BounceGeom* bg, int* generic) {
    NEED(bounce_size_ok(h, w), "Bounce board %dx%d unsupported (need height >= 3, sides <= %d, cells <= %d)", h, w,
         BGS_GENERIC_BOUNCE_MAX_DIM, BGS_GENERIC_BOUNCE_MAX_CELLS);
    *generic = force_generic() || h * w > BGS_BOUNCE_MAX_CELLS;
    memset(bg, 0, sizeof(*bg));
    bg->h = h; bg->w = w;
    if (!cfg) return BGS_OK;
    for (int c = 0; c < h * w; ++c) {
        NEED(cfg[c] >= 0, "Bounce piece value %d at (%d,%d) is negative", cfg[c], c % w, c / w);
        NEED(!(cfg[c] > 0 && (c < w || c >= (h - 1) * w)), "Bounce goal rows must be empty (piece at (%d,%d))", c % w, c / w);
        if (cfg[c] > BGS_BOUNCE_MAX_VALUE) *generic = 1;
    }
    if (*generic) return BGS_OK;
    bg->inv_w = (65536u + (uint32_t)w - 1u) / (uint32_t)w;
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x) {
            const int c = y * w + x;
            const uint64_t bit = 1ull << c;
            const int v = cfg[c];
            bg->all |= bit;
            if (y == 0) bg->goal_bottom |= bit;
            else if (y == h - 1) bg->goal_top |= bit;
            else bg->interior |= bit;
            if (x > 0) bg->not_col0 |= bit;
            if (x < w - 1) bg->not_collast |= bit;
            for (int p = 0; p < 4; ++p)
                if ((v >> p) & 1) bg->init[p] |= bit;
        }
    // the piece list: ascending (value, cell)
    int pieces = 0;
    for (int c = 0; c < h * w; ++c) pieces += cfg[c] > 0;
    if (pieces >= 1 && pieces <= BGS_BOUNCE_MAX_PIECES) {
        int k = 0;
        for (int v = 1; v <= BGS_BOUNCE_MAX_VALUE; ++v)
            for (int c = 0; c < h * w; ++c)
                if (cfg[c] == v) {
                    bg->piece_value[k] = (uint8_t)v;
                    bg->piece_cell[k] = (uint8_t)c;
                    for (int p = 0; p < 4; ++p)
                        if ((k >> p) & 1) bg->piece_idx[p] |= 1ull << c;
                    ++k;
                }
        bg->piece_count = (uint32_t)k;
    }
    return BGS_OK;
}

int carve(bgs_batch* b, void* arena, size_t arena_bytes, const Layout& l) {
    if (arena) {
        NEED(((uintptr_t)arena % kAlign) == 0, "arena must be %zu-byte aligned", kAlign);
        NEED(arena_bytes >= l.total, "arena too small: %zu < %zu bytes", arena_bytes, l.total);
        b->arena = arena;
        b->owns_arena = false;
    } else {
        HIP_TRY(hipMalloc(&b->arena, l.total));
        b->owns_arena = true;
    }
    b->arena_bytes = l.total;
    uint8_t* base = static_cast<uint8_t*>(b->arena);
    b->d_planes = reinterpret_cast<uint64_t*>(base + l.planes);
    b->d_status = base + l.status;
    b->d_plies = reinterpret_cast<uint16_t*>(base + l.plies);
    b->d_reward = reinterpret_cast<int8_t*>(base + l.reward);
    b->d_steps = reinterpret_cast<unsigned long long*>(base + l.steps);
    b->d_worklist = reinterpret_cast<uint32_t*>(base + l.worklist);
    b->d_work_count = reinterpret_cast<uint32_t*>(base + l.work_count);
    b->d_pool = reinterpret_cast<uint32_t*>(base + l.pool);
    b->d_gen_masks = reinterpret_cast<uint64_t*>(base + l.gen_masks);
    b->d_gen_cfg = reinterpret_cast<int8_t*>(base + l.gen_cfg);
    b->d_staging = base + l.staging;
    b->staging_bytes = l.staging_bytes;
    return BGS_OK;
}

// bump allocator over the staging region (one call = one arena lifetime)
struct Stage {
    uint8_t* base;
    size_t cap, off;
    explicit Stage(const bgs_batch* b) : base(b->d_staging), cap(b->staging_bytes), off(0) {}
    template <class T>
    T* take(size_t count) {
        uint8_t* p = base + off;
        off += align_up(count * sizeof(T));
        return off <= cap ? reinterpret_cast<T*>(p) : nullptr;
    }
};

int enter(const bgs_batch* b) {
    NEED(b != nullptr, "batch handle is NULL");
    HIP_TRY(hipSetDevice(b->device));
    return BGS_OK;
}

int finish_launch() {
    HIP_TRY(hipGetLastError());
    return BGS_OK;
}

// Device -> caller's (pageable) host memory.  A direct hipMemcpy into pageable memory runs at a few GB/s; large
// copies go through two pinned bounce buffers instead: chunk k+1 crosses PCIe while the CPU moves chunk k.
constexpr size_t kPinnedChunk = 4u << 20;

int copy_to_host(bgs_batch* b, void* host, const void* dev, size_t bytes) {
    if (bytes <= (256u << 10)) {
        HIP_TRY(hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, b->stream));
        HIP_TRY(hipStreamSynchronize(b->stream));
        return BGS_OK;
    }
    if (!b->pinned[0]) {
        HIP_TRY(hipHostMalloc(&b->pinned[0], kPinnedChunk, hipHostMallocDefault));
        HIP_TRY(hipHostMalloc(&b->pinned[1], kPinnedChunk, hipHostMallocDefault));
        HIP_TRY(hipEventCreateWithFlags(&b->pinned_done[0], hipEventDisableTiming));
        HIP_TRY(hipEventCreateWithFlags(&b->pinned_done[1], hipEventDisableTiming));
    }
    const size_t chunks = (bytes + kPinnedChunk - 1) / kPinnedChunk;
    auto issue = [&](size_t k) -> hipError_t {
        const size_t off = k * kPinnedChunk, len = bytes - off < kPinnedChunk ? bytes - off : kPinnedChunk;
        hipError_t e = hipMemcpyAsync(b->pinned[k & 1], static_cast<const uint8_t*>(dev) + off, len, hipMemcpyDeviceToHost, b->stream);
        return e != hipSuccess ? e : hipEventRecord(b->pinned_done[k & 1], b->stream);
    };
    HIP_TRY(issue(0));
    for (size_t k = 0; k < chunks; ++k) {
        if (k + 1 < chunks) HIP_TRY(issue(k + 1));
        HIP_TRY(hipEventSynchronize(b->pinned_done[k & 1]));
        const size_t off = k * kPinnedChunk, len = bytes - off < kPinnedChunk ? bytes - off : kPinnedChunk;
        memcpy(static_cast<uint8_t*>(host) + off, b->pinned[k & 1], len);
    }
    return BGS_OK;
}

template <class T>
int to_host(bgs_batch* b, T* host, const T* dev, size_t count) {
    return copy_to_host(b, host, dev, count * sizeof(T));
}

template <class T>
int to_device(const bgs_batch* b, T* dev, const T* host, size_t count) {
    HIP_TRY(hipMemcpyAsync(dev, host, count * sizeof(T), hipMemcpyHostToDevice, b->stream));
    return BGS_OK;
}

// the tree memory of a search call: the caller's (`ptr`, `bytes`) or, where ptr may be NULL, the library's own;
// `sizing` is the function that says how large (`need` is its answer)
struct Workspace {
    void* ptr;
    size_t bytes, need;
    const char* sizing;
};

int workspace_check(const Workspace& w, bool on_device) {
    NEED(!on_device || w.ptr != nullptr, "workspace is NULL (on_device: the caller owns it; %s says how large)", w.sizing);
    if (!w.ptr) return BGS_OK;
    NEED((reinterpret_cast<uintptr_t>(w.ptr) & 255u) == 0, "the workspace must be 256-byte aligned");
    NEED(w.bytes >= w.need, "the workspace is too small: %zu bytes, %zu needed", w.bytes, w.need);
    return BGS_OK;
}

// One analysis call through its output plan (output_plan.h; DESIGN.md, "Outputs of an analysis call").  launch(d, tree):
// d[i] is the device pointer of output i, nullptr for an absent optional one; tree is the workspace (nullptr without ws).
// on_device: the caller's pointers, after the alignment checks in declaration order and the workspace's.  Otherwise one
// stream-ordered allocation holds a slice per present output and, without a caller's workspace, the library's own; the
// present outputs are copied back in order, and the buffer is freed whatever happened (an earlier error wins over the
// free's).
template <class Launch>
int run_outputs(bgs_batch* b, const bgs::OutputPlan& plan, bool on_device, const Workspace* ws, Launch&& launch) {
    NEED(plan.ok, "internal: the output plan does not hold this call");
    void* d[bgs::OutputPlan::kMax] = {};
    int rc = BGS_OK;
    if (on_device) {
        const int bad = plan.misaligned();
        NEED(bad < 0, "device %s must be %zu-byte aligned", plan.out[bad].name, plan.out[bad].align);
        if (ws && (rc = workspace_check(*ws, true))) return rc;
        for (int i = 0; i < plan.count; ++i) d[i] = plan.out[i].ptr;
        launch(d, ws ? ws->ptr : nullptr);
        return finish_launch();
    }
    if (ws && (rc = workspace_check(*ws, false))) return rc;
    const bool own = ws && !ws->ptr;
    uint8_t* base = nullptr;
    HIP_TRY(hipMallocAsync(reinterpret_cast<void**>(&base), plan.end + (own ? plan.workspace_room(ws->need) : 0), b->stream));
    for (int i = 0; i < plan.count; ++i)
        if (plan.out[i].ptr) d[i] = base + plan.out[i].offset;
    launch(d, own ? base + plan.workspace_offset(reinterpret_cast<uintptr_t>(base)) : ws ? ws->ptr : nullptr);
    rc = finish_launch();
    for (int i = 0; i < plan.count && rc == BGS_OK; ++i)
        if (plan.out[i].ptr) rc = copy_to_host(b, plan.out[i].ptr, d[i], plan.out[i].bytes);
    const hipError_t e = hipFreeAsync(base, b->stream);
    if (rc) return rc;
    HIP_TRY(e);
    return BGS_OK;
}

inline int32_t* i32(void* p) { return static_cast<int32_t*>(p); }

int policy_check(const char* entry, int policy) {
    NEED(policy == BGS_POLICY_UNIFORM || policy == BGS_POLICY_DECISIVE,
         "%s: unknown policy %d (BGS_POLICY_UNIFORM %d, BGS_POLICY_DECISIVE %d)", entry, policy, BGS_POLICY_UNIFORM,
         BGS_POLICY_DECISIVE);
    return BGS_OK;
}

// `sizing`: the function that says how large the forest is
int forest_pointer(const void* forest, size_t forest_bytes, size_t need, const char* sizing) {
    NEED(forest != nullptr, "forest is NULL (the caller owns it; %s says how large)", sizing);
    NEED((reinterpret_cast<uintptr_t>(forest) & 255u) == 0, "the forest must be 256-byte aligned");
    NEED(forest_bytes >= need, "the forest is too small: %zu bytes, %zu needed", forest_bytes, need);
    return BGS_OK;
}

// scratch of the Bounce evaluation and solver: the boards' legal-move prefix and the workgroups' totals, in the staging
// region (ordered on the stream)
int bounce_move_scratch(const bgs_batch* b, uint64_t** d_ends, uint64_t** d_totals) {
    Stage st(b);
    *d_ends = st.take<uint64_t>((size_t)b->n);
    *d_totals = st.take<uint64_t>((size_t)(b->n + BGS_BLOCK - 1) / BGS_BLOCK);
    NEED(*d_ends && *d_totals, "staging region too small");
    return BGS_OK;
}

// The body of both *_forest_advance entry points behind their checks: `moves` (named `name` in the messages) goes up
// and `kept`, when asked for, comes back.  advance(d_moves, d_kept) launches.
template <class Advance>
int forest_advance(bgs_batch* b, const int32_t* moves, const char* name, int32_t* kept, bool on_device, Advance&& advance) {
    if (on_device) {
        NEED((reinterpret_cast<uintptr_t>(moves) & 3u) == 0, "device %s must be 4-byte aligned", name);
        NEED((reinterpret_cast<uintptr_t>(kept) & 3u) == 0, "device kept must be 4-byte aligned");
        advance(moves, kept);
        return finish_launch();
    }
    // one device buffer: moves, kept
    const size_t board_bytes = (size_t)b->n * sizeof(int32_t);
    int32_t* d = nullptr;
    HIP_TRY(hipMallocAsync(reinterpret_cast<void**>(&d), 2 * board_bytes, b->stream));
    int rc = to_device(b, d, moves, (size_t)b->n);
    if (rc == BGS_OK) {
        advance(d, kept ? d + b->n : nullptr);
        rc = finish_launch();
    }
    if (rc == BGS_OK && kept) rc = copy_to_host(b, kept, d + b->n, board_bytes);
    // (without kept no copy back waits for the stream, and the caller's `moves` must have been read when the call returns)
    if (rc == BGS_OK && !kept && hipStreamSynchronize(b->stream) != hipSuccess) rc = bgs::fail(BGS_ERR_RUNTIME, "hipStreamSynchronize failed");
    const hipError_t e = hipFreeAsync(d, b->stream);
    if (rc) return rc;
    HIP_TRY(e);
    return BGS_OK;
}

// device facts the launch geometry of the fused rollout depends on
int device_facts(bgs_batch* b) {
    int cus = 0;
    HIP_TRY(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, b->device));
    b->num_cus = cus > 0 ? cus : 256;
    // Waves per SIMD of the fused rollout.  Instruction issue is the bound, so what matters is games per lane: when a
    // wave's chunk is exhausted its lanes drain -- they idle until the wave's longest game has ended, about half a game
    // per lane -- so fewer, longer-lived waves waste less.  Aim for >= 4 games per lane (>= 8 for one-word boards, whose
    // games are short: measured on 6x7x4 at 2^20 games, 512 games per wave is as fast as 256 for one launch at a time
    // and 10 % faster with three launches in flight), between 1 and 4 waves per SIMD; one-word boards keep at least 2
    // waves for latency hiding.
    {
        const int64_t lanes_per_wps = (int64_t)b->num_cus * 4 * BGS_WAVE;
        const int64_t games_per_lane = (b->game == BGS_GAME_CONNECT && b->cg.nw == 1) ? kGamesPerLaneOneWord : kGamesPerLane;
        int64_t wps = b->n / (lanes_per_wps * games_per_lane);
        const int64_t floor_wps = (b->game == BGS_GAME_CONNECT && b->cg.nw == 1) ? 2 : 1;
        if (wps < floor_wps) wps = floor_wps;
        if (wps > 4) wps = 4;
        b->rollout_wps = (int)wps;
    }
    if (const char* env = getenv("BGS_ROLLOUT_WPS")) {
        const int v = atoi(env);
        if (v >= 1 && v <= 8) b->rollout_wps = v;
    }
    b->rollout_chunk = 0;
    if (const char* e = bgs::experiment("rollout_chunk")) {
        const int v = atoi(e);
        if (v >= 64 && v <= (1 << 20)) b->rollout_chunk = v;
    }
    b->rng_per_ply = 0;
    b->rollout_generic = bgs::experiment("rollout_generic") != nullptr;
    b->rollout_no_lds = bgs::experiment("rollout_no_lds") != nullptr;
    b->rollout_opening = kRolloutOpeningBlocks;
    if (const char* e = bgs::experiment("rollout_opening")) {
        const int v = atoi(e);
        if (v >= 0 && v <= 4) b->rollout_opening = v;
    }
    // Bounce rollouts: one lane per board with the flattened search (fewest instructions per ply: throughput) for large
    // batches, 8 lanes per board (shortest ply latency) for small ones; BGS_BOUNCE_GROUP = 1 / 8 overrides
    b->bounce_group = b->n >= 32768 ? 1 : 8;
    b->bounce_group_auto = 1;
    if (const char* env = bgs::experiment("bounce_group")) {
        b->bounce_group = atoi(env) == 1 ? 1 : 8;
        b->bounce_group_auto = 0;
    }
    b->bounce_pieces = 1;
    if (const char* env = bgs::experiment("bounce_pieces")) b->bounce_pieces = atoi(env) != 0;
    b->bounce_pool = 1;
    if (const char* env = bgs::experiment("bounce_pool")) b->bounce_pool = atoi(env) != 0;
    b->bounce_wave_grid = 0;
    if (const char* env = bgs::experiment("bounce_wave_grid")) b->bounce_wave_grid = atoi(env);
    b->transition_wave = 1;
    if (const char* env = bgs::experiment("transition_wave")) b->transition_wave = env[0] != '0';
    b->bounce_static_geom = 1;
    if (const char* env = bgs::experiment("bounce_static_geom")) b->bounce_static_geom = atoi(env) != 0;
    b->bounce_flat_chunk = kBounceFlatChunk;
    if (const char* env = bgs::experiment("bounce_chunk")) {
        const int v = atoi(env);
        if (v >= 1 && v <= 4096) b->bounce_flat_chunk = v;
    }
    b->bounce_park = kBouncePark;
    if (const char* env = bgs::experiment("bounce_park")) {
        const int v = atoi(env);
        if (v >= 0 && v <= 32) b->bounce_park = v;
    }
    b->launches_in_flight = 1;
    b->bounce_flat_waves = 0;
    b->bounce_pieces_park = bgs::experiment("bounce_park") ? b->bounce_park : -1;   // (-1: what bounce_shape() says for the launches in flight)
    if (const char* env = bgs::experiment("bounce_pieces_park")) {
        const int v = atoi(env);
        if (v >= 0 && v <= 63) b->bounce_pieces_park = v;
    }
    if (const char* env = bgs::experiment("bounce_flat_waves")) {
        const int v = atoi(env);
        if (v >= 1 && v <= (1 << 16)) b->bounce_flat_waves = v;
    }
    b->bounce_flat_wps = kBounceFlatWps;
    if (const char* env = bgs::experiment("bounce_flat_wps")) {
        const int v = atoi(env);
        if (v >= 1 && v <= 8) b->bounce_flat_wps = v;
    }
    b->bounce_eval_wps = 0;
    if (const char* env = bgs::experiment("bounce_eval_wps")) {
        const int v = atoi(env);
        if (v >= 1 && v <= 8) b->bounce_eval_wps = v;
    }
    // multi-pass Bounce rollout (bounce_kernels.hip, bounce_rollout): "cap:lanes,..."; the last entry's cap is the
    // caller's max_plies whatever it says; "single" = one launch that plays every game to the end
    {
        // default "auto": one launch, except for large from-initial batches on the piece-list kernel, whose handful of
        // very long games (a random Bounce game can go on for ever: it stops at max_plies) is finished by a second pass
        // with 8 lanes per board -- see bounce_rollout()
        // (experiment() hands out a buffer its next call overwrites: the plan is copied before the other knobs are read)
        const char* plan_value = bgs::experiment("bounce_plan");
        const std::string plan_text = plan_value ? plan_value : "auto";
        const char* plan = plan_text.c_str();
        const char* wave_pass = bgs::experiment("bounce_wave_pass");
        b->bounce_wave_pass = !(wave_pass && wave_pass[0] == '0');
        const char* epoch_limit = bgs::experiment("bounce_epoch_limit");
        b->bounce_epoch_limit = epoch_limit ? atoi(epoch_limit) : 0;
        b->bounce_memo_cold = kBounceMemoCold;      // (bounce_kernels.hip, K3w; "bounce_memo_policy=0:0": never without the memo)
        b->bounce_memo_bypass = kBounceMemoBypass;
        if (const char* policy = bgs::experiment("bounce_memo_policy")) {
            int cold = 0, plies = 0;
            if (sscanf(policy, "%d:%d", &cold, &plies) == 2 && cold >= 0 && plies >= 0 && plies <= 65535) {
                b->bounce_memo_cold = cold > 0 ? cold : 0x3FFFFFFF;
                b->bounce_memo_bypass = plies;
            }
        }
        b->bounce_passes = 0;
        b->bounce_plan_auto = strcmp(plan, "auto") == 0;
        if (!b->bounce_plan_auto && strcmp(plan, "single") != 0) {
            const char* p = plan;
            while (*p && b->bounce_passes < BGS_BOUNCE_MAX_PASSES) {
                char* endp = nullptr;
                const long cap = strtol(p, &endp, 10);
                int lanes = 1;
                if (endp && *endp == ':') lanes = (int)strtol(endp + 1, &endp, 10);
                b->bounce_pass_cap[b->bounce_passes] = cap > 0 ? (uint32_t)cap : 0xFFFFFFFFu;
                b->bounce_pass_group[b->bounce_passes] = lanes == 8 ? 8 : lanes == 64 ? 64 : 1;   // 64: one board per wave (K3w), later passes only
                ++b->bounce_passes;
                if (!endp || *endp != ',') break;
                p = endp + 1;
            }
        }
    }
    return BGS_OK;
}

// ---- outcome codes for the reward gather: 2 bits per board (0 running, 1 / 2 winner, 3 draw), 4 boards per byte.
// A reward pair is a function of the status byte, so shipping int8[n][2] over xGMI would move 8x the information.
__global__ void __launch_bounds__(BGS_BLOCK)
k_pack_outcomes(const uint8_t* __restrict__ status, int64_t n, uint8_t* __restrict__ packed) {
    const int64_t t = (int64_t)blockIdx.x * BGS_BLOCK + threadIdx.x;
    const int64_t first = t * 4;
    if (first >= n) return;
    uint32_t four = 0;
    if (first + 3 < n) {
        four = *reinterpret_cast<const uint32_t*>(status + first);
    } else {
        for (int j = 0; first + j < n; ++j) four |= (uint32_t)status[first + j] << (8 * j);
    }
    packed[t] = (uint8_t)((four & 3u) | ((four >> 6) & 0xCu) | ((four >> 12) & 0x30u) | ((four >> 18) & 0xC0u));
}

// the same codes, 64 boards per lane: four 16-byte status loads in, one 16-byte store out, so a wave writes 1 KiB of
// contiguous codes -- the form used when the destination is page-locked HOST memory and every store is a PCIe write
__global__ void __launch_bounds__(BGS_BLOCK)
k_pack_outcomes_wide(const uint8_t* __restrict__ status, int64_t groups, uint4* __restrict__ packed) {
    const int64_t t = (int64_t)blockIdx.x * BGS_BLOCK + threadIdx.x;
    if (t >= groups) return;
    const uint4* src = reinterpret_cast<const uint4*>(status) + t * 4;
    uint32_t out[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const uint4 v = src[q];
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
        uint32_t acc = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t four = w[j];
            acc |= ((four & 3u) | ((four >> 6) & 0xCu) | ((four >> 12) & 0x30u) | ((four >> 18) & 0xC0u)) << (8 * j);
        }
        out[q] = acc;
    }
    packed[t] = make_uint4(out[0], out[1], out[2], out[3]);
}

__global__ void __launch_bounds__(BGS_BLOCK)
k_expand_outcomes(const uint8_t* __restrict__ packed, int64_t n, uint16_t* __restrict__ reward) {
    const int64_t t = (int64_t)blockIdx.x * BGS_BLOCK + threadIdx.x;
    const int64_t first = t * 4;
    if (first >= n) return;
    const uint32_t byte = packed[t];
    uint64_t four = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) four |= (uint64_t)bgs::reward_pair((byte >> (2 * j)) & 3u) << (16 * j);
    if (first + 3 < n) {
        *reinterpret_cast<uint64_t*>(reward + first) = four;
    } else {
        for (int j = 0; first + j < n; ++j) reward[first + j] = (uint16_t)(four >> (16 * j));
    }
}

// bytes per board of the legal-move record bgs_transition returns
size_t legal_bytes_per_board(const bgs_batch* b) {
    if (b->game == BGS_GAME_CONNECT) return (size_t)b->cg.w;
    if (b->generic) return bgs::generic_bounce_legal_bytes(b->gen_h, b->gen_w);
    return 8 * ((size_t)b->bg.w + 1);
}

int make_order_event(bgs_batch* b) {
    HIP_TRY(hipEventCreateWithFlags(&b->order_event, hipEventDisableTiming));
    return BGS_OK;
}

// a batch whose construction failed half-way
void discard(bgs_batch* b) {
    if (b->game == BGS_GAME_BOUNCE) bgs::bounce_book_release(b);
    if (b->owns_arena && b->arena) (void)hipFree(b->arena);
    if (b->order_event) (void)hipEventDestroy(b->order_event);
    delete b;
}

int reset_impl(bgs_batch* b) {
    HIP_TRY(hipMemsetAsync(b->d_steps, 0, kStepBytes, b->stream));
    if (b->generic) bgs::generic_reset(b);
    else if (b->game == BGS_GAME_CONNECT) bgs::connect_reset(b);
    else bgs::bounce_reset(b);
    return finish_launch();
}

// generic Bounce: cell masks and start grid to the device; the device settles a start position without legal moves
int generic_bounce_setup(bgs_batch* b, const int8_t* cfg) {
    constexpr int W = BGS_GENERIC_BOUNCE_MAX_CELLS / 64;
    uint64_t masks[6 * W];
    memset(masks, 0, sizeof(masks));
    const int h = b->gen_h, w = b->gen_w;
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x) {
            const int c = y * w + x;
            const uint64_t bit = 1ull << (c & 63);
            masks[0 * W + (c >> 6)] |= bit;                              // every cell
            if (y > 0 && y < h - 1) masks[1 * W + (c >> 6)] |= bit;      // interior rows
            if (x > 0) masks[2 * W + (c >> 6)] |= bit;
            if (x < w - 1) masks[3 * W + (c >> 6)] |= bit;
            if (y == h - 1) masks[4 * W + (c >> 6)] |= bit;               // player 0's goal row
            if (y == 0) masks[5 * W + (c >> 6)] |= bit;                   // player 1's goal row
        }
    HIP_TRY(hipMemcpyAsync(b->d_gen_masks, masks, sizeof(masks), hipMemcpyHostToDevice, b->stream));
    HIP_TRY(hipMemcpyAsync(b->d_gen_cfg, cfg, (size_t)h * w, hipMemcpyHostToDevice, b->stream));
    HIP_TRY(hipStreamSynchronize(b->stream));  // (masks[] is on this stack frame)
    // load the start grid as board 0 of a one-board view: the pack kernel settles a blocked start position
    bgs_batch one = *b;
    one.n = 1;
    bgs::generic_pack(&one, b->d_gen_cfg, nullptr, nullptr, nullptr, nullptr);
    HIP_TRY(hipGetLastError());
    uint8_t status0 = 0;
    HIP_TRY(hipMemcpyAsync(&status0, b->d_status, 1, hipMemcpyDeviceToHost, b->stream));
    HIP_TRY(hipStreamSynchronize(b->stream));
    b->gen_init_status = status0;
    return BGS_OK;
}

}  // namespace

namespace bgs {
void pack_outcomes(const bgs_batch* b, uint8_t* d_packed) {
    // whole groups of 64 boards go through the wide kernel (16-byte aligned destination), the rest byte by byte
    const int64_t groups = ((uintptr_t)d_packed % 16 == 0) ? b->n / 64 : 0;
    if (groups)
        hipLaunchKernelGGL(k_pack_outcomes_wide, dim3((unsigned)((groups + BGS_BLOCK - 1) / BGS_BLOCK)), dim3(BGS_BLOCK), 0,
                           b->stream, b->d_status, groups, reinterpret_cast<uint4*>(d_packed));
    const int64_t done = groups * 64, rest = b->n - done;
    if (rest > 0) {
        const int64_t bytes = (rest + 3) / 4;
        hipLaunchKernelGGL(k_pack_outcomes, dim3((unsigned)((bytes + BGS_BLOCK - 1) / BGS_BLOCK)), dim3(BGS_BLOCK), 0,
                           b->stream, b->d_status + done, rest, d_packed + done / 4);
    }
}
}  // namespace bgs

namespace bgs {
int rollout_with_codes(bgs_batch* b, uint64_t seed, int32_t max_plies, uint32_t flags, uint8_t* codes_out) {
    int rc = enter(b);
    if (rc) return rc;
    NEED(max_plies >= 0, "max_plies must be >= 0");
    NEED(codes_out != nullptr && ((uintptr_t)codes_out % 16) == 0, "codes destination must be 16-byte aligned");
    bool fused = false;
    NEED((flags & ~(uint32_t)(BGS_ROLLOUT_FROM_INITIAL | BGS_ROLLOUT_DRAW_PER_PLY)) == 0, "unknown rollout flags 0x%x", flags);
    if (b->generic) bgs::generic_play(b, seed, (uint32_t)max_plies, 0xFFFFFFFFu, (flags & BGS_ROLLOUT_FROM_INITIAL) != 0, (flags & BGS_ROLLOUT_DRAW_PER_PLY) != 0);
    else if (b->game == BGS_GAME_CONNECT) fused = bgs::connect_rollout(b, seed, max_plies, flags, reinterpret_cast<uint32_t*>(codes_out));
    else bgs::bounce_rollout(b, seed, max_plies, flags);
    if (!fused) bgs::pack_outcomes(b, codes_out);
    return finish_launch();
}
}  // namespace bgs


// ---- bgs_transition on small batches (the object API's one-board engines) ---------------------------------------
// The staged form of the call costs two copies, a memset and a device-to-device copy around five kernels.  For a
// batch of at most kSmallTransition boards the in-block and the out-block live in page-locked host memory that the
// kernels read and write in place (a few hundred bytes over PCIe).  Optionally the launch sequence -- it depends only
// on which of grid / plies / actions the caller passed -- is captured once per combination and replayed as a HIP graph.
// Measured (tools/object_latency.py, round 3, r3_transition.sh in the git history; Connect 6x7x4 / default Bounce, one thread, with the
// engines leaving out the load of a board the device already holds): staged 53 / 63 us per transition, in place 28 / 46,
// graph 35 / 52 -- hipGraphLaunch costs more than the five launches it replaces.  From 8 threads the order of in place
// and graph changed between runs (30 vs 42 and 48 vs 38 thousand Connect transitions per second).  The default goes one
// step further on the packed geometries: in place, with the move and the whole observation in ONE kernel
// (k_connect_transition / k_bounce_transition) instead of five.  experiment transition=staged | mapped | graph select the
// multi-kernel forms (the only ones for generic geometries and for batches above kSmallTransition boards).
namespace {
constexpr int64_t kSmallTransition = 64;
constexpr size_t kSmallBlock = 64u << 10;

struct SmallTransition {
    uint8_t* h_in = nullptr;
    uint8_t* h_out = nullptr;
    uint8_t* d_in = nullptr;   // the same blocks in the device's address space
    uint8_t* d_out = nullptr;
    hipGraphExec_t exec[8] = {};
    bool graph_failed = false;
    uint32_t ticket = 0;       // of the last fused call: the kernel writes it behind its records (the block's last word)
    uint32_t unsynced = 0;     // fused calls since the stream was last synchronised
};
std::mutex g_small_mu;
std::unordered_map<const bgs_batch*, SmallTransition> g_small;

int transition_mode() {
    static const int mode = [] {
        const char* e = bgs::experiment("transition");
        if (e && !strcmp(e, "staged")) return 0;
        if (e && !strcmp(e, "mapped")) return 1;
        if (e && !strcmp(e, "graph")) return 2;
        return 3;  // in place, and one fused kernel for move + observation (packed geometries)
    }();
    return mode;
}

__global__ void k_copy_small(const uint8_t* __restrict__ src, size_t bytes, uint8_t* __restrict__ dst) {
    for (size_t i = threadIdx.x; i < bytes; i += blockDim.x) dst[i] = src[i];
}

int small_transition(const bgs_batch* b, SmallTransition** out) {
    std::lock_guard<std::mutex> hold(g_small_mu);
    SmallTransition& t = g_small[b];
    if (!t.h_in) {
        void *hi = nullptr, *ho = nullptr, *di = nullptr, *dv = nullptr;
        // coherent: the fused kernel's ticket (and the records before it) are read while the stream is still busy
        HIP_TRY(hipHostMalloc(&hi, kSmallBlock, hipHostMallocMapped | hipHostMallocCoherent));
        HIP_TRY(hipHostMalloc(&ho, kSmallBlock, hipHostMallocMapped | hipHostMallocCoherent));
        memset(ho, 0, kSmallBlock);
        HIP_TRY(hipHostGetDevicePointer(&di, hi, 0));
        HIP_TRY(hipHostGetDevicePointer(&dv, ho, 0));
        t.h_in = static_cast<uint8_t*>(hi); t.h_out = static_cast<uint8_t*>(ho);
        t.d_in = static_cast<uint8_t*>(di); t.d_out = static_cast<uint8_t*>(dv);
    }
    *out = &t;
    return BGS_OK;
}

void drop_small_transition(const bgs_batch* b) {
    std::lock_guard<std::mutex> hold(g_small_mu);
    auto it = g_small.find(b);
    if (it == g_small.end()) return;
    for (hipGraphExec_t e : it->second.exec)
        if (e) (void)hipGraphExecDestroy(e);
    if (it->second.h_in) (void)hipHostFree(it->second.h_in);
    if (it->second.h_out) (void)hipHostFree(it->second.h_out);
    g_small.erase(it);
}
}  // namespace

extern "C" {

int bgs_version(void) { return 200; }

// The identity of the kernels this library was LINKED with: the six units' own ids folded into 16 hex digits (the same
// fold as `make print-id`: h = id_0; h = h * 0x100000001b3 ^ id_k, 64-bit wrap-around).  "unknown..." when a unit was
// compiled outside the Makefile.
const char* bgs_build_id(void) {
    static const std::string id = [] {
        uint64_t h = 0;
        bool first = true;
        for (const char* tu : {bgs_tu_id_connect, bgs_tu_id_bounce, bgs_tu_id_generic, bgs_tu_id_evaluate, bgs_tu_id_search, bgs_tu_id_solve}) {
            char* end = nullptr;
            const uint64_t v = strtoull(tu, &end, 16);
            if (end == tu || *end != 0) return std::string("unknown");
            h = first ? v : (h * 0x100000001b3ull) ^ v;
            first = false;
        }
        char text[17];
        snprintf(text, sizeof text, "%016llx", (unsigned long long)h);
        return std::string(text);
    }();
    return id.c_str();
}

const char* bgs_kernel_unit_id(int unit) {
    switch (unit) {
        case 0: return bgs_tu_id_connect;
        case 1: return bgs_tu_id_bounce;
        case 2: return bgs_tu_id_generic;
        case 3: return bgs_tu_id_evaluate;
        case 4: return bgs_tu_id_search;
        case 5: return bgs_tu_id_solve;
        default: return nullptr;
    }
}

const char* bgs_last_error(void) { return g_error; }

int bgs_device_count(int* count) {
    NEED(count != nullptr, "count is NULL");
    int c = 0;
    hipError_t e = hipGetDeviceCount(&c);
    *count = (e == hipSuccess) ? c : 0;
    return BGS_OK;
}

int bgs_connect_arena_bytes(int height, int width, int count, int64_t n, size_t* bytes) {
    ConnectGeom cg;
    int generic = 0;
    int rc = connect_geom(height, width, count, &cg, &generic);
    if (rc) return rc;
    NEED(n >= 1 && bytes, "n must be >= 1 and bytes non-NULL");
    *bytes = layout_for(2 * cg.nw, n, height, width, generic ? (size_t)width : 0).total;
    return BGS_OK;
}

// one arena layout per board SIZE, for the size query and for the carve alike (up to 64 cells: the packed form's four
// planes, which also hold a small generic board)
static auto bounce_layout(int64_t n, int height, int width) {
    return layout_for(height * width > BGS_BOUNCE_MAX_CELLS ? 0 : 4, n, height, width, bgs::generic_bounce_legal_bytes(height, width),
                      height * width <= BGS_BOUNCE_MAX_CELLS);
}

int bgs_bounce_arena_bytes(int height, int width, int64_t n, size_t* bytes) {
    BounceGeom bg;
    int generic = 0;
    int rc = bounce_geom(nullptr, height, width, &bg, &generic);
    if (rc) return rc;
    NEED(n >= 1 && bytes, "n must be >= 1 and bytes non-NULL");
    // Whether the batch is packed or generic also depends on the piece values (and on BGS_FORCE_GENERIC), which this
    // query cannot see: the size follows the CELL COUNT alone, exactly as bgs_bounce_create carves it
    (void)generic;
    *bytes = bounce_layout(n, height, width).total;
    return BGS_OK;
}

int bgs_connect_create(int height, int width, int count, int64_t n, int device, void* arena, size_t arena_bytes,
                       bgs_batch** out) {
    NEED(out != nullptr, "out is NULL");
    *out = nullptr;
    ConnectGeom cg;
    int generic = 0;
    int rc = connect_geom(height, width, count, &cg, &generic);
    if (rc) return rc;
    NEED(n >= 1, "batch size must be >= 1");
    rc = check_device(device);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(device));
    bgs_batch* b = new (std::nothrow) bgs_batch();
    NEED(b != nullptr, "out of host memory");
    memset(b, 0, sizeof(*b));
    b->game = BGS_GAME_CONNECT;
    b->device = device;
    b->n = n;
    b->cg = cg;
    b->planes = 2 * cg.nw;
    b->generic = generic;
    b->gen_h = height; b->gen_w = width; b->gen_k = count;
    rc = device_facts(b);
    if (rc == BGS_OK) rc = carve(b, arena, arena_bytes, layout_for(b->planes, n, height, width, generic ? (size_t)width : 0));
    if (rc == BGS_OK) rc = make_order_event(b);
    if (rc == BGS_OK) rc = reset_impl(b);
    if (rc != BGS_OK) {
        discard(b);
        return rc;
    }
    *out = b;
    return BGS_OK;
}

int bgs_bounce_create(const int8_t* cfg_grid, int height, int width, int64_t n, int device, void* arena,
                      size_t arena_bytes, bgs_batch** out) {
    NEED(out != nullptr, "out is NULL");
    *out = nullptr;
    BounceGeom bg;
    int generic = 0;
    NEED(cfg_grid != nullptr, "Bounce config grid is NULL");
    int rc = bounce_geom(cfg_grid, height, width, &bg, &generic);
    if (rc) return rc;
    NEED(n >= 1, "batch size must be >= 1");
    rc = check_device(device);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(device));
    bgs_batch* b = new (std::nothrow) bgs_batch();
    NEED(b != nullptr, "out of host memory");
    memset(b, 0, sizeof(*b));
    b->game = BGS_GAME_BOUNCE;
    b->device = device;
    b->n = n;
    b->bg = bg;
    b->planes = generic ? 0 : 4;
    b->generic = generic;
    b->gen_h = height; b->gen_w = width;
    rc = device_facts(b);
    if (rc == BGS_OK) {
        // the arena is sized for whichever form the values select (bgs_bounce_arena_bytes cannot know them)
        rc = carve(b, arena, arena_bytes, bounce_layout(n, height, width));
    }
    if (rc == BGS_OK) rc = make_order_event(b);
    if (rc == BGS_OK && generic) rc = generic_bounce_setup(b, cfg_grid);
    if (rc == BGS_OK && !generic) {
        // a start position whose first player cannot move is already over: let the device settle board 0 once
        // and remember the verdict (the kernels own every rule; the host evaluates none)
        rc = [&]() -> int {
            Stage st(b);
            int8_t* d_grid = st.take<int8_t>((size_t)height * width);
            NEED(d_grid != nullptr, "staging buffer too small");
            bgs_batch one = *b;
            one.n = 1;
            HIP_TRY(hipMemcpyAsync(d_grid, cfg_grid, (size_t)height * width, hipMemcpyHostToDevice, b->stream));
            bgs::bounce_pack(&one, d_grid, nullptr, nullptr, nullptr, nullptr);
            HIP_TRY(hipGetLastError());
            uint8_t status0 = 0;
            HIP_TRY(hipMemcpyAsync(&status0, b->d_status, 1, hipMemcpyDeviceToHost, b->stream));
            HIP_TRY(hipStreamSynchronize(b->stream));
            b->bg.init_status = status0;
            return BGS_OK;
        }();
    }
    if (rc == BGS_OK && !generic) {
        // the opening book of the start position, for the batches the piece-list rollout plays (from 32768 boards): built
        // once per start position and device, shared afterwards.  BGS_BOUNCE_BOOK=0 switches it off, 1..4 = that depth
        // at most, for a batch of any size (the tests' way to reach it with small batches)
        const char* e = getenv("BGS_BOUNCE_BOOK");
        const int want = e ? atoi(e) : (n >= 32768 ? 4 : 0);
        if (want > 0) {
            const int he = bgs::bounce_book_acquire(b, want);
            if (he != 0) rc = fail(BGS_ERR_RUNTIME, "the opening book could not be built: %s", hipGetErrorString((hipError_t)he));
        }
    }
    if (rc == BGS_OK) rc = reset_impl(b);
    if (rc != BGS_OK) {
        discard(b);
        return rc;
    }
    *out = b;
    return BGS_OK;
}

int bgs_destroy(bgs_batch* b) {
    if (!b) return BGS_OK;
    (void)hipSetDevice(b->device);
    (void)hipStreamSynchronize(b->stream);
    drop_small_transition(b);
    if (b->game == BGS_GAME_BOUNCE) bgs::bounce_book_release(b);
    if (b->owns_arena && b->arena) (void)hipFree(b->arena);
    for (int k = 0; k < 2; ++k) {
        if (b->pinned[k]) (void)hipHostFree(b->pinned[k]);
        if (b->pinned_done[k]) (void)hipEventDestroy(b->pinned_done[k]);
    }
    if (b->order_event) (void)hipEventDestroy(b->order_event);
    delete b;
    return BGS_OK;
}

int bgs_set_launches_in_flight(bgs_batch* b, int32_t launches) {
    NEED(b != nullptr, "batch handle is NULL");
    NEED(launches >= 1 && launches <= 1024, "launches in flight %d outside 1..1024", (int)launches);
    b->launches_in_flight = launches;
    return BGS_OK;
}

int bgs_set_stream(bgs_batch* b, void* hip_stream) {
    int rc = enter(b);
    if (rc) return rc;
    hipStream_t next = static_cast<hipStream_t>(hip_stream);
    if (next != b->stream) {
        // whatever the batch has enqueued so far (its reset included) happens before anything the new stream runs:
        // torch's pool streams are non-blocking and do not synchronise with the null stream by themselves
        HIP_TRY(hipEventRecord(b->order_event, b->stream));
        HIP_TRY(hipStreamWaitEvent(next, b->order_event, 0));
        b->stream = next;
    }
    return BGS_OK;
}

int bgs_set_first_game(bgs_batch* b, uint64_t first_game) {
    NEED(b != nullptr, "batch handle is NULL");
    b->first_game = first_game;
    return BGS_OK;
}

int bgs_set_rng_contract(bgs_batch* b, int contract) {
    NEED(b != nullptr, "batch handle is NULL");
    NEED(contract == BGS_RNG_PER_BLOCK || contract == BGS_RNG_PER_PLY, "unknown RNG contract %d", contract);
    b->rng_per_ply = contract == BGS_RNG_PER_PLY;
    return BGS_OK;
}

int bgs_synchronize(bgs_batch* b) {
    int rc = enter(b);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(b->stream));
    return BGS_OK;
}

int bgs_info(const bgs_batch* b, int* game, int* height, int* width, int* count, int64_t* n, int* planes) {
    NEED(b != nullptr, "batch handle is NULL");
    const bool connect = b->game == BGS_GAME_CONNECT;
    if (game) *game = b->game;
    if (height) *height = connect ? b->cg.h : b->bg.h;
    if (width) *width = connect ? b->cg.w : b->bg.w;
    if (count) *count = connect ? b->cg.k : 0;
    if (b->generic) {
        if (height) *height = b->gen_h;
        if (width) *width = b->gen_w;
    }
    if (n) *n = b->n;
    if (planes) *planes = b->planes;
    return BGS_OK;
}

int bgs_legal_bytes(const bgs_batch* b, size_t* bytes, int* generic) {
    NEED(b != nullptr && bytes != nullptr, "NULL argument");
    *bytes = legal_bytes_per_board(b);
    if (generic) *generic = b->generic;
    return BGS_OK;
}

int bgs_buffer(const bgs_batch* b, int buffer_id, void** device_ptr, size_t* bytes) {
    NEED(b != nullptr && device_ptr != nullptr, "NULL argument");
    size_t sz = 0;
    void* p = nullptr;
    switch (buffer_id) {
        case BGS_BUF_PLANES:  // (generic batches: the int8[n][h][w] grid itself)
            p = b->d_planes;
            sz = b->generic ? (size_t)b->n * b->gen_h * b->gen_w : (size_t)b->planes * b->n * 8;
            break;
        case BGS_BUF_STATUS: p = b->d_status; sz = (size_t)b->n; break;
        case BGS_BUF_PLIES: p = b->d_plies; sz = (size_t)b->n * 2; break;
        case BGS_BUF_REWARD: p = b->d_reward; sz = (size_t)b->n * 2; break;
        case BGS_BUF_STEPS: p = b->d_steps; sz = kStepBytes; break;
        case BGS_BUF_STAGING: p = b->d_staging; sz = b->staging_bytes; break;
        default: return fail(BGS_ERR_ARG, "unknown buffer id %d", buffer_id);
    }
    *device_ptr = p;
    if (bytes) *bytes = sz;
    return BGS_OK;
}

int bgs_reset(bgs_batch* b) {
    int rc = enter(b);
    if (rc) return rc;
    return reset_impl(b);
}

int bgs_step_random_n(bgs_batch* b, uint64_t seed, int32_t plies) {
    int rc = enter(b);
    if (rc) return rc;
    NEED(plies >= 0 && plies <= 4096, "plies must be in 0..4096");
    if (plies == 0) return BGS_OK;
    if (b->generic) bgs::generic_play(b, seed, 0xFFFFFFFFu, (uint32_t)plies, false);
    else if (b->game == BGS_GAME_CONNECT) bgs::connect_step_random(b, seed, (uint32_t)plies);
    else bgs::bounce_step_random(b, seed, (uint32_t)plies);
    return finish_launch();
}

int bgs_step_random(bgs_batch* b, uint64_t seed) { return bgs_step_random_n(b, seed, 1); }

int bgs_step_actions(bgs_batch* b, const int32_t* actions, int actions_on_device, int32_t* status) {
    int rc = enter(b);
    if (rc) return rc;
    NEED(actions != nullptr, "actions is NULL");
    const size_t per = b->game == BGS_GAME_CONNECT ? 1 : 4;
    Stage st(b);
    int32_t* d_result = status ? st.take<int32_t>((size_t)b->n) : nullptr;
    NEED(!status || d_result != nullptr, "staging buffer too small");
    const int32_t* d_actions = actions;
    if (!actions_on_device) {
        int32_t* tmp = st.take<int32_t>((size_t)b->n * per);
        NEED(tmp != nullptr, "staging buffer too small");
        rc = to_device(b, tmp, actions, (size_t)b->n * per);
        if (rc) return rc;
        d_actions = tmp;
    }
    if (b->generic) bgs::generic_step_actions(b, d_actions, d_result);
    else if (b->game == BGS_GAME_CONNECT) bgs::connect_step_actions(b, d_actions, d_result);
    else bgs::bounce_step_actions(b, d_actions, d_result);
    rc = finish_launch();
    if (rc) return rc;
    if (status) return to_host(b, status, d_result, (size_t)b->n);
    if (!actions_on_device) HIP_TRY(hipStreamSynchronize(b->stream));  // the host buffer may be reused by the caller
    return BGS_OK;
}

int bgs_env_step(bgs_batch* b, const int32_t* device_actions, void* device_observation, uint8_t* device_ended,
                 int8_t* device_reward, int32_t* device_status, uint32_t flags) {
    int rc = enter(b);
    if (rc) return rc;
    NEED(device_actions != nullptr && device_observation != nullptr, "actions and the observation's destination must not be NULL");
    NEED((flags & ~(uint32_t)BGS_ENV_AUTO_RESET) == 0, "unknown flags 0x%x", flags);
    NEED(!b->generic || b->game == BGS_GAME_CONNECT, "generic Bounce boards have no 64-bit target masks (see bgs_export_device 't')");
    const bool auto_reset = (flags & BGS_ENV_AUTO_RESET) != 0;
    NEED(!auto_reset || !b->generic, "BGS_ENV_AUTO_RESET needs a bit-packed board (Connect up to 192 bits, Bounce up to 64 cells)");
    // one-word Connect boards, even batch: moves, rewards, ended flags, reset and the legal mask in ONE pass over the batch
    if (!b->generic && b->game == BGS_GAME_CONNECT &&
        bgs::connect_step_observe(b, device_actions, device_status, static_cast<uint8_t*>(device_observation), device_ended,
                                  device_reward, auto_reset))
        return finish_launch();
    // everything else: the same result from the kernels of the separate calls, enqueued back to back
    if (b->generic) bgs::generic_step_actions(b, device_actions, device_status);
    else if (b->game == BGS_GAME_CONNECT) bgs::connect_step_actions(b, device_actions, device_status);
    else bgs::bounce_step_actions(b, device_actions, device_status);
    if (device_ended) bgs::status_to_ended(b, device_ended);
    if (device_reward) HIP_TRY(hipMemcpyAsync(device_reward, b->d_reward, (size_t)b->n * 2, hipMemcpyDeviceToDevice, b->stream));
    if (auto_reset) {
        if (b->game == BGS_GAME_CONNECT) bgs::connect_reset_ended(b);
        else bgs::bounce_reset_ended(b);
    }
    if (b->game == BGS_GAME_CONNECT) {
        if (b->generic) bgs::generic_connect_legal(b, static_cast<uint8_t*>(device_observation), nullptr);
        else bgs::connect_legal(b, static_cast<uint8_t*>(device_observation), nullptr);
    } else {
        bgs::bounce_targets(b, static_cast<uint64_t*>(device_observation), nullptr);
    }
    return finish_launch();
}

int bgs_step_actions_observe(bgs_batch* b, const int32_t* device_actions, void* device_observation, uint8_t* device_ended,
                             int32_t* device_status) {
    return bgs_env_step(b, device_actions, device_observation, device_ended, nullptr, device_status, 0u);
}

int bgs_rollout(bgs_batch* b, uint64_t seed, int32_t max_plies, uint32_t flags) {
    int rc = enter(b);
    if (rc) return rc;
    NEED(max_plies >= 0, "max_plies must be >= 0");
    NEED((flags & ~(uint32_t)(BGS_ROLLOUT_FROM_INITIAL | BGS_ROLLOUT_DRAW_PER_PLY)) == 0, "unknown rollout flags 0x%x", flags);
    if (b->generic) bgs::generic_play(b, seed, (uint32_t)max_plies, 0xFFFFFFFFu, (flags & BGS_ROLLOUT_FROM_INITIAL) != 0, (flags & BGS_ROLLOUT_DRAW_PER_PLY) != 0);
    else if (b->game == BGS_GAME_CONNECT) (void)bgs::connect_rollout(b, seed, max_plies, flags, nullptr);
    else bgs::bounce_rollout(b, seed, max_plies, flags);
    return finish_launch();
}

// ---- the analysis calls: evaluation, tree search, forest, solver.  Each declares its outputs in an OutputPlan and
// goes through run_outputs() ("Outputs of an analysis call"); d[i] below is output i in declaration order.

// the outputs the four tree searches of a game share; cells: root moves of the batch (n x width, n x W x H x W)
static void add_search_outputs(bgs::OutputPlan& plan, const bgs_batch* b, size_t cells, int32_t* counts, int32_t* visits,
                               int32_t* best, int32_t* nodes) {
    plan.add("counts", counts, cells * 3 * sizeof(int32_t), false);
    plan.add("visits", visits, cells * sizeof(int32_t));
    plan.add("best", best, (size_t)b->n * sizeof(int32_t));
    plan.add("nodes", nodes, (size_t)b->n * sizeof(int32_t));
}

// the body of both evaluate_actions entry points (the caller has entered the batch's device)
static int connect_evaluate_actions(bgs_batch* b, uint64_t seed, int32_t playouts, int32_t max_plies, int policy, int32_t* counts,
                                    int counts_on_device) {
    NEED(counts != nullptr, "counts is NULL");
    NEED(b->game == BGS_GAME_CONNECT, "evaluate_actions: Connect batches only (Bounce boards are not supported yet)");
    NEED(!b->generic, "evaluate_actions: bit-packed Connect boards only (up to %d bits a plane); %dx%d boards are generic",
         64 * BGS_CONNECT_MAX_WORDS, b->cg.h, b->cg.w);
    NEED(playouts >= 1, "playouts must be >= 1 (got %d)", playouts);
    NEED(max_plies >= 1, "max_plies must be >= 1 (got %d)", max_plies);
    bgs::OutputPlan plan;
    plan.add("counts", counts, (size_t)b->n * b->cg.w * 3 * sizeof(int32_t), false);
    // (this entry point reports a misaligned device pointer before the overflow)
    NEED(!counts_on_device || plan.misaligned() < 0, "device counts must be 16-byte aligned");
    NEED(b->n <= INT64_MAX / b->cg.w / playouts, "n * width * playouts overflows int64 (%lld x %d x %d)", (long long)b->n,
         b->cg.w, playouts);
    return run_outputs(b, plan, counts_on_device, nullptr,
                       [&](void* const* d, void*) { bgs::connect_evaluate(b, seed, playouts, max_plies, i32(d[0]), policy); });
}

int bgs_connect_evaluate_actions(bgs_batch* b, uint64_t seed, int32_t playouts, int32_t max_plies, int32_t* counts,
                                 int counts_on_device) {
    int rc = enter(b);
    if (rc) return rc;
    return connect_evaluate_actions(b, seed, playouts, max_plies, BGS_POLICY_UNIFORM, counts, counts_on_device);
}

int bgs_connect_evaluate_actions_policy(bgs_batch* b, uint64_t seed, int32_t playouts, int32_t max_plies, int policy, int32_t* counts,
                                        int counts_on_device) {
    int rc = enter(b);
    if (rc) return rc;
    rc = policy_check("evaluate_actions", policy);
    if (rc) return rc;
    return connect_evaluate_actions(b, seed, playouts, max_plies, policy, counts, counts_on_device);
}

int bgs_connect_evaluate_actions_halving(bgs_batch* b, uint64_t seed, int32_t budget, int32_t max_plies, int policy, int32_t* counts,
                                         int32_t* given, int32_t* best, int on_device) {
    int rc = enter(b);
    if (rc) return rc;
    NEED(counts != nullptr, "counts is NULL");
    NEED(b->game == BGS_GAME_CONNECT, "evaluate_actions_halving: Connect batches only");
    NEED(!b->generic, "evaluate_actions_halving: bit-packed Connect boards only (up to %d bits a plane); %dx%d boards are generic",
         64 * BGS_CONNECT_MAX_WORDS, b->cg.h, b->cg.w);
    rc = policy_check("evaluate_actions_halving", policy);
    if (rc) return rc;
    NEED(budget >= bgs::connect_halving_min_budget(b->cg.w),
         "budget must be >= width * max(1, ceil(log2 width)) = %d, the least that gives every round a playout a column (got %d)",
         bgs::connect_halving_min_budget(b->cg.w), budget);
    NEED(max_plies >= 1, "max_plies must be >= 1 (got %d)", max_plies);
    NEED(b->n <= INT64_MAX / b->cg.w / budget, "n * width * budget overflows int64 (%lld x %d x %d)", (long long)b->n, b->cg.w, budget);
    const size_t cells = (size_t)b->n * b->cg.w;
    bgs::OutputPlan plan;
    plan.add("counts", counts, cells * 3 * sizeof(int32_t), false);
    plan.add("given", given, cells * sizeof(int32_t));
    plan.add("best", best, (size_t)b->n * sizeof(int32_t));
    return run_outputs(b, plan, on_device, nullptr, [&](void* const* d, void*) {
        bgs::connect_evaluate_halving(b, seed, budget, max_plies, policy, i32(d[0]), i32(d[1]), i32(d[2]));
    });
}

// the checks of the search parameters, the same in the four search entry points; `entry` names the caller in the messages
// (the plain entry points come here behind *_search_check, which has refused iterations < 1 already: the first check is
// the forest entry points')
static int search_params_check(const char* entry, const bgs_batch* b, int32_t iterations, int32_t leaf_playouts, int32_t explore,
                               int32_t max_plies, int policy) {
    NEED(iterations >= 1, "iterations must be >= 1 (got %d)", iterations);
    NEED(leaf_playouts >= 1, "leaf_playouts must be >= 1 (got %d)", leaf_playouts);
    NEED((int64_t)iterations * leaf_playouts <= ((int64_t)1 << 29),
         "iterations * leaf_playouts must be <= 2^29, so that scores stay in int32 (got %d x %d)", iterations, leaf_playouts);
    NEED(explore >= 0 && explore <= (1 << 18), "explore must be 0 .. 2^18 = 262144 (got %d)", explore);
    NEED(max_plies >= 1, "max_plies must be >= 1 (got %d)", max_plies);
    const int rc = policy_check(entry, policy);
    if (rc) return rc;
    NEED(b->n <= INT64_MAX / iterations / leaf_playouts, "n * iterations * leaf_playouts overflows int64 (%lld x %d x %d)",
         (long long)b->n, iterations, leaf_playouts);
    return BGS_OK;
}

// the checks of the search entry points that need no device; *bytes: the workspace of the batch; `entry` names the caller
static int connect_search_check(const bgs_batch* b, int32_t iterations, size_t* bytes, const char* entry = "search_actions") {
    NEED(b->game == BGS_GAME_CONNECT, "%s: Connect batches only", entry);
    NEED(!b->generic, "%s: bit-packed Connect boards only (up to %d bits a plane); %dx%d boards are generic", entry,
         64 * BGS_CONNECT_MAX_WORDS, b->cg.h, b->cg.w);
    NEED(iterations >= 1, "iterations must be >= 1 (got %d)", iterations);
    const uint64_t root = bgs::connect_search_root_bytes(b->cg.w, iterations);
    NEED((uint64_t)b->n <= (uint64_t)(SIZE_MAX / 2) / root, "the workspace of %lld boards x %d iterations overflows size_t",
         (long long)b->n, iterations);
    *bytes = (size_t)((uint64_t)b->n * root);
    return BGS_OK;
}

int bgs_connect_search_workspace_bytes(const bgs_batch* b, int32_t iterations, size_t* bytes) {
    NEED(b != nullptr, "batch is NULL");
    NEED(bytes != nullptr, "bytes is NULL");
    return connect_search_check(b, iterations, bytes);
}

// bgs_connect_search_actions and bgs_connect_search_actions_proving: the same checks and workspace; `entry` names the
// caller in the messages, and the proving entry point declares two more outputs
static int connect_search_entry(const char* entry, bool proving, bgs_batch* b, uint64_t seed, int32_t iterations,
                                int32_t leaf_playouts, int32_t explore, int32_t max_plies, int policy, int32_t* counts,
                                int32_t* visits, int32_t* best, int32_t* nodes, int8_t* proved, int32_t* done, void* workspace,
                                size_t workspace_bytes, int on_device) {
    int rc = enter(b);
    if (rc) return rc;
    NEED(counts != nullptr, "counts is NULL");
    size_t need = 0;
    rc = connect_search_check(b, iterations, &need, entry);
    if (rc) return rc;
    rc = search_params_check(entry, b, iterations, leaf_playouts, explore, max_plies, policy);
    if (rc) return rc;
    const size_t cells = (size_t)b->n * b->cg.w;
    bgs::OutputPlan plan;
    add_search_outputs(plan, b, cells, counts, visits, best, nodes);
    if (proving) {
        plan.add("proved", proved, cells * sizeof(int8_t));
        plan.add("done", done, (size_t)b->n * sizeof(int32_t));
    }
    const Workspace ws{workspace, workspace_bytes, need, "bgs_connect_search_workspace_bytes"};
    return run_outputs(b, plan, on_device, &ws, [&](void* const* d, void* tree) {
        if (proving) {
            bgs::connect_search_proving(b, seed, iterations, leaf_playouts, explore, max_plies, policy, i32(d[0]), i32(d[1]), i32(d[2]),
                                        i32(d[3]), static_cast<int8_t*>(d[4]), i32(d[5]), tree);
        } else {
            bgs::connect_search(b, seed, iterations, leaf_playouts, explore, max_plies, policy, i32(d[0]), i32(d[1]), i32(d[2]),
                                i32(d[3]), tree);
        }
    });
}

int bgs_connect_search_actions(bgs_batch* b, uint64_t seed, int32_t iterations, int32_t leaf_playouts, int32_t explore,
                               int32_t max_plies, int policy, int32_t* counts, int32_t* visits, int32_t* best, int32_t* nodes,
                               void* workspace, size_t workspace_bytes, int on_device) {
    return connect_search_entry("search_actions", false, b, seed, iterations, leaf_playouts, explore, max_plies, policy, counts, visits,
                                best, nodes, nullptr, nullptr, workspace, workspace_bytes, on_device);
}

int bgs_connect_search_actions_proving(bgs_batch* b, uint64_t seed, int32_t iterations, int32_t leaf_playouts, int32_t explore,
                                       int32_t max_plies, int policy, int32_t* counts, int32_t* visits, int32_t* best,
                                       int32_t* nodes, int8_t* proved, int32_t* done, void* workspace, size_t workspace_bytes,
                                       int on_device) {
    return connect_search_entry("search_actions_proving", true, b, seed, iterations, leaf_playouts, explore, max_plies, policy, counts,
                                visits, best, nodes, proved, done, workspace, workspace_bytes, on_device);
}

// the checks of the three forest entry points that need no device; *bytes: the forest of the batch
static int connect_forest_check(const bgs_batch* b, int32_t capacity, size_t* bytes) {
    NEED(b->game == BGS_GAME_CONNECT, "forest: Connect batches only");
    NEED(!b->generic, "forest: bit-packed Connect boards only (up to %d bits a plane); %dx%d boards are generic",
         64 * BGS_CONNECT_MAX_WORDS, b->cg.h, b->cg.w);
    NEED(capacity >= 2 && capacity <= BGS_CONNECT_FOREST_MAX_CAPACITY, "capacity must be 2 .. %d nodes a tree (got %d)",
         BGS_CONNECT_FOREST_MAX_CAPACITY, capacity);
    const uint64_t tree = bgs::connect_forest_tree_bytes(b->cg.w, capacity);
    NEED((uint64_t)b->n <= (uint64_t)(SIZE_MAX / 2) / tree, "the forest of %lld boards x %d nodes overflows size_t", (long long)b->n,
         capacity);
    *bytes = (size_t)((uint64_t)b->n * tree);
    return BGS_OK;
}

int bgs_connect_forest_bytes(const bgs_batch* b, int32_t capacity, size_t* bytes) {
    NEED(b != nullptr, "batch is NULL");
    NEED(bytes != nullptr, "bytes is NULL");
    return connect_forest_check(b, capacity, bytes);
}

int bgs_connect_forest_search(bgs_batch* b, uint64_t seed, int32_t iterations, int32_t leaf_playouts, int32_t explore,
                              int32_t max_plies, int policy, int32_t capacity, int restart, int32_t* counts, int32_t* visits,
                              int32_t* best, int32_t* nodes, int32_t* carried, void* forest, size_t forest_bytes, int on_device) {
    int rc = enter(b);
    if (rc) return rc;
    NEED(counts != nullptr, "counts is NULL");
    size_t need = 0;
    rc = connect_forest_check(b, capacity, &need);
    if (rc) return rc;
    rc = search_params_check("forest_search", b, iterations, leaf_playouts, explore, max_plies, policy);
    if (rc) return rc;
    rc = forest_pointer(forest, forest_bytes, need, "bgs_connect_forest_bytes");
    if (rc) return rc;
    bgs::OutputPlan plan;
    add_search_outputs(plan, b, (size_t)b->n * b->cg.w, counts, visits, best, nodes);
    plan.add("carried", carried, (size_t)b->n * sizeof(int32_t));
    return run_outputs(b, plan, on_device, nullptr, [&](void* const* d, void*) {
        bgs::connect_forest_search(b, seed, iterations, leaf_playouts, explore, max_plies, policy, capacity, restart, i32(d[0]),
                                   i32(d[1]), i32(d[2]), i32(d[3]), i32(d[4]), forest);
    });
}

int bgs_connect_forest_advance(bgs_batch* b, const int32_t* columns, int32_t capacity, int32_t* kept, void* forest,
                               size_t forest_bytes, int on_device) {
    int rc = enter(b);
    if (rc) return rc;
    NEED(columns != nullptr, "columns is NULL");
    size_t need = 0;
    rc = connect_forest_check(b, capacity, &need);
    if (rc) return rc;
    rc = forest_pointer(forest, forest_bytes, need, "bgs_connect_forest_bytes");
    if (rc) return rc;
    return forest_advance(b, columns, "columns", kept, on_device, [&](const int32_t* d_columns, int32_t* d_kept) {
        bgs::connect_forest_advance(b, d_columns, capacity, d_kept, forest);
    });
}

// the checks of both guided entry points that need no device; *bytes: the trees of the batch
static int connect_guided_check(const bgs_batch* b, int32_t capacity, size_t* bytes) {
    NEED(b->game == BGS_GAME_CONNECT, "guided: Connect batches only");
    NEED(!b->generic, "guided: bit-packed Connect boards only (up to %d bits a plane); %dx%d boards are generic",
         64 * BGS_CONNECT_MAX_WORDS, b->cg.h, b->cg.w);
    NEED(capacity >= 2 && capacity <= BGS_GUIDED_MAX_CAPACITY, "capacity must be 2 .. %d nodes a tree (got %d)",
         BGS_GUIDED_MAX_CAPACITY, capacity);
    const uint64_t tree = bgs::connect_guided_tree_bytes(b->cg.h, b->cg.w, capacity);
    NEED((uint64_t)b->n <= (uint64_t)(SIZE_MAX / 2) / tree, "the trees of %lld boards x %d nodes overflow size_t", (long long)b->n,
         capacity);
    *bytes = (size_t)((uint64_t)b->n * tree);
    return BGS_OK;
}

int bgs_connect_guided_bytes(const bgs_batch* b, int32_t capacity, size_t* bytes) {
    NEED(b != nullptr, "batch is NULL");
    NEED(bytes != nullptr, "bytes is NULL");
    return connect_guided_check(b, capacity, bytes);
}

// What both guided steps check once their game's size check has said `need`.  `max_plies` is Bounce's (NULL: Connect has
// none).  `named` are the device pointers of the call but the trees, in the order of its arguments: priors and values, which
// may be NULL with BGS_GUIDED_RESTART only, then leaf_grid, leaf_player and leaf_kind, which may not, then the game's other
// outputs.  `sizing` is the call that says how large the trees are.
struct GuidedPointer {
    const char* name;
    const void* ptr;
};
static int guided_step_check(int32_t cpuct, const int32_t* max_plies, uint32_t flags, const GuidedPointer* named, size_t count,
                             const void* trees, size_t trees_bytes, size_t need, const char* sizing) {
    NEED(cpuct >= 0 && cpuct <= 4096, "cpuct must be 0 .. 4096, c_puct in Q8 (got %d)", cpuct);
    NEED(max_plies == nullptr || *max_plies >= 1, "max_plies must be >= 1 (got %d)", *max_plies);
    NEED((flags & ~(BGS_GUIDED_RESTART | BGS_GUIDED_FINISH)) == 0u, "unknown flag bits 0x%x (BGS_GUIDED_RESTART 0x%x, BGS_GUIDED_FINISH 0x%x)",
         flags & ~(BGS_GUIDED_RESTART | BGS_GUIDED_FINISH), BGS_GUIDED_RESTART, BGS_GUIDED_FINISH);
    NEED((flags & BGS_GUIDED_RESTART) == 0u || (flags & BGS_GUIDED_FINISH) == 0u,
         "BGS_GUIDED_RESTART with BGS_GUIDED_FINISH: a restarted tree has nothing to finish");
    NEED(trees != nullptr, "trees is NULL (the caller owns them; %s says how large)", sizing);
    for (size_t i = 2; i < 5; ++i) NEED(named[i].ptr != nullptr, "%s is NULL", named[i].name);
    for (size_t i = 0; i < 2; ++i)
        NEED((flags & BGS_GUIDED_RESTART) != 0u || named[i].ptr != nullptr, "%s is NULL (allowed with BGS_GUIDED_RESTART only)", named[i].name);
    NEED((reinterpret_cast<uintptr_t>(trees) & 255u) == 0, "trees must be 256-byte aligned");
    for (size_t i = 0; i < count; ++i)
        NEED((reinterpret_cast<uintptr_t>(named[i].ptr) & 15u) == 0, "device %s must be 16-byte aligned", named[i].name);
    NEED(trees_bytes >= need, "the trees are too small: %zu bytes, %zu needed", trees_bytes, need);
    return BGS_OK;
}

int bgs_connect_guided_step(bgs_batch* b, int32_t capacity, int32_t cpuct, uint32_t flags, const float* priors, const float* values,
                            int8_t* leaf_grid, int8_t* leaf_player, int32_t* leaf_kind, int32_t* visits, int32_t* scores,
                            int32_t* best, int32_t* nodes, void* trees, size_t trees_bytes) {
    int rc = enter(b);
    if (rc) return rc;
    size_t need = 0;
    rc = connect_guided_check(b, capacity, &need);
    if (rc) return rc;
    const GuidedPointer named[] = {{"priors", priors}, {"values", values}, {"leaf_grid", leaf_grid}, {"leaf_player", leaf_player},
                                   {"leaf_kind", leaf_kind}, {"visits", visits}, {"scores", scores}, {"best", best}, {"nodes", nodes}};
    rc = guided_step_check(cpuct, nullptr, flags, named, sizeof(named) / sizeof(named[0]), trees, trees_bytes, need, "bgs_connect_guided_bytes");
    if (rc) return rc;
    bgs::connect_guided_step(b, capacity, cpuct, flags, priors, values, leaf_grid, leaf_player, leaf_kind, visits, scores, best, nodes,
                             trees);
    return finish_launch();
}

int bgs_connect_guided_advance(bgs_batch* b, const int32_t* columns, int32_t capacity, int32_t* kept, void* trees, size_t trees_bytes) {
    int rc = enter(b);
    if (rc) return rc;
    size_t need = 0;
    rc = connect_guided_check(b, capacity, &need);
    if (rc) return rc;
    NEED(capacity <= BGS_GUIDED_ADVANCE_MAX_CAPACITY,
         "capacity must be at most %d nodes a tree for an advance: the re-rooting keeps its scratch on the chip (got %d)",
         BGS_GUIDED_ADVANCE_MAX_CAPACITY, capacity);
    NEED(columns != nullptr, "columns is NULL");
    NEED(trees != nullptr, "trees is NULL (the caller owns them; bgs_connect_guided_bytes says how large)");
    NEED((reinterpret_cast<uintptr_t>(trees) & 255u) == 0, "trees must be 256-byte aligned");
    NEED((reinterpret_cast<uintptr_t>(columns) & 15u) == 0, "device columns must be 16-byte aligned");
    NEED((reinterpret_cast<uintptr_t>(kept) & 15u) == 0, "device kept must be 16-byte aligned");
    NEED(trees_bytes >= need, "the trees are too small: %zu bytes, %zu needed", trees_bytes, need);
    bgs::connect_guided_advance(b, columns, capacity, kept, trees);
    return finish_launch();
}

// the outputs of both solvers; d[2], the node counter, keeps its 8-byte rule, and without a caller's counter the total
// goes to the batch's own scratch word (behind the work-queue head)
static void add_solve_outputs(bgs::OutputPlan& plan, size_t cells, int8_t* codes, int16_t* plies, uint64_t* nodes) {
    plan.add("codes", codes, cells * sizeof(int8_t), false);
    plan.add("plies", plies, cells * sizeof(int16_t));
    plan.add("nodes", nodes, sizeof(uint64_t), true, 8);
}
static unsigned long long* solve_counter(const bgs_batch* b, void* d_nodes) {
    return d_nodes ? static_cast<unsigned long long*>(d_nodes) : reinterpret_cast<unsigned long long*>(b->d_work_count) + 1;
}

int bgs_connect_solve_actions(bgs_batch* b, int32_t depth, int64_t max_nodes, int8_t* codes, int16_t* plies, uint64_t* nodes,
                              int on_device) {
    int rc = enter(b);
    if (rc) return rc;
    NEED(codes != nullptr, "codes is NULL");
    NEED(b->game == BGS_GAME_CONNECT, "solve_actions: Connect batches only");
    NEED(!b->generic, "solve_actions: bit-packed Connect boards only (up to %d bits a plane); %dx%d boards are generic",
         64 * BGS_CONNECT_MAX_WORDS, b->cg.h, b->cg.w);
    NEED(depth >= 1, "depth must be >= 1 (got %d)", depth);
    NEED(max_nodes >= 1, "max_nodes must be >= 1 (got %lld)", (long long)max_nodes);
    bgs::OutputPlan plan;
    add_solve_outputs(plan, (size_t)b->n * b->cg.w, codes, plies, nodes);
    return run_outputs(b, plan, on_device, nullptr, [&](void* const* d, void*) {
        bgs::connect_solve(b, depth, max_nodes, static_cast<int8_t*>(d[0]), static_cast<int16_t*>(d[1]), solve_counter(b, d[2]));
    });
}

static size_t bounce_slots(const bgs_batch* b) { return (size_t)b->bg.w * (size_t)b->bg.h * (size_t)b->bg.w; }

// bgs_bounce_evaluate_moves and bgs_bounce_evaluate_moves_policy behind their entry checks (enter(b), the policy's range)
static int bounce_evaluate_moves(bgs_batch* b, uint64_t seed, int32_t playouts, int32_t max_plies, int policy, int32_t* counts,
                                 int counts_on_device) {
    NEED(counts != nullptr, "counts is NULL");
    NEED(b->game == BGS_GAME_BOUNCE, "evaluate_moves: Bounce batches only (Connect boards: bgs_connect_evaluate_actions)");
    NEED(!b->generic, "evaluate_moves: bit-packed Bounce boards only (up to %d cells, piece values up to %d); this %dx%d board is generic",
         BGS_BOUNCE_MAX_CELLS, BGS_BOUNCE_MAX_VALUE, b->gen_h, b->gen_w);
    NEED(playouts >= 1, "playouts must be >= 1 (got %d)", playouts);
    NEED(max_plies >= 1, "max_plies must be >= 1 (got %d)", max_plies);
    const int64_t slots = (int64_t)bounce_slots(b);
    bgs::OutputPlan plan;
    plan.add("counts", counts, (size_t)b->n * (size_t)slots * 3 * sizeof(int32_t), false);
    // (this entry point reports a misaligned device pointer before the overflow)
    NEED(!counts_on_device || plan.misaligned() < 0, "device counts must be 16-byte aligned");
    NEED(b->n <= INT64_MAX / slots / playouts, "n * width * height * width * playouts overflows int64 (%lld x %lld x %d)",
         (long long)b->n, (long long)slots, playouts);
    uint64_t *d_ends, *d_totals;
    const int rc = bounce_move_scratch(b, &d_ends, &d_totals);
    if (rc) return rc;
    return run_outputs(b, plan, counts_on_device, nullptr, [&](void* const* d, void*) {
        bgs::bounce_evaluate(b, seed, playouts, max_plies, i32(d[0]), d_ends, d_totals, policy);
    });
}

int bgs_bounce_evaluate_moves(bgs_batch* b, uint64_t seed, int32_t playouts, int32_t max_plies, int32_t* counts,
                              int counts_on_device) {
    int rc = enter(b);
    if (rc) return rc;
    return bounce_evaluate_moves(b, seed, playouts, max_plies, BGS_POLICY_UNIFORM, counts, counts_on_device);
}

int bgs_bounce_evaluate_moves_policy(bgs_batch* b, uint64_t seed, int32_t playouts, int32_t max_plies, int policy, int32_t* counts,
                                     int counts_on_device) {
    int rc = enter(b);
    if (rc) return rc;
    rc = policy_check("evaluate_moves", policy);
    if (rc) return rc;
    return bounce_evaluate_moves(b, seed, playouts, max_plies, policy, counts, counts_on_device);
}

int bgs_bounce_evaluate_moves_halving(bgs_batch* b, uint64_t seed, int32_t budget, int32_t max_plies, int policy, int32_t* counts,
                                      int32_t* given, int32_t* best, int on_device) {
    int rc = enter(b);
    if (rc) return rc;
    NEED(counts != nullptr, "counts is NULL");
    NEED(b->game == BGS_GAME_BOUNCE, "evaluate_moves_halving: Bounce batches only (Connect boards: bgs_connect_evaluate_actions_halving)");
    NEED(!b->generic,
         "evaluate_moves_halving: bit-packed Bounce boards only (up to %d cells, piece values up to %d); this %dx%d board is generic",
         BGS_BOUNCE_MAX_CELLS, BGS_BOUNCE_MAX_VALUE, b->gen_h, b->gen_w);
    rc = policy_check("evaluate_moves_halving", policy);
    if (rc) return rc;
    NEED(budget >= 1, "budget must be >= 1 (got %d)", budget);
    NEED(max_plies >= 1, "max_plies must be >= 1 (got %d)", max_plies);
    const int64_t slots = (int64_t)bounce_slots(b);
    NEED(b->n <= INT64_MAX / slots / budget, "n * width * height * width * budget overflows int64 (%lld x %lld x %d)", (long long)b->n,
         (long long)slots, budget);
    const size_t cells = (size_t)b->n * (size_t)slots;
    bgs::OutputPlan plan;
    plan.add("counts", counts, cells * 3 * sizeof(int32_t), false);
    plan.add("given", given, cells * sizeof(int32_t));
    plan.add("best", best, (size_t)b->n * sizeof(int32_t));
    return run_outputs(b, plan, on_device, nullptr, [&](void* const* d, void*) {
        bgs::bounce_evaluate_halving(b, seed, budget, max_plies, policy, i32(d[0]), i32(d[1]), i32(d[2]));
    });
}

// the checks of both Bounce search entry points that need no device; *bytes: the workspace of the batch
static int bounce_search_check(const bgs_batch* b, int32_t iterations, int32_t edges, size_t* bytes) {
    NEED(b->game == BGS_GAME_BOUNCE, "search_moves: Bounce batches only (Connect boards: bgs_connect_search_actions)");
    NEED(!b->generic, "search_moves: bit-packed Bounce boards only (up to %d cells, piece values up to %d); this %dx%d board is generic",
         BGS_BOUNCE_MAX_CELLS, BGS_BOUNCE_MAX_VALUE, b->gen_h, b->gen_w);
    NEED(iterations >= 1, "iterations must be >= 1 (got %d)", iterations);
    const int32_t least = BGS_BOUNCE_SEARCH_MIN_EDGES(b->bg.h, b->bg.w);
    NEED(edges >= least, "edges must be >= BGS_BOUNCE_SEARCH_MIN_EDGES(%d, %d) = %d, the most arms a position can have (got %d)", b->bg.h,
         b->bg.w, least, edges);
    const uint64_t root = bgs::bounce_search_root_bytes(iterations, edges);
    NEED((uint64_t)b->n <= (uint64_t)(SIZE_MAX / 2) / root, "the workspace of %lld boards x %d iterations x %d edges overflows size_t",
         (long long)b->n, iterations, edges);
    *bytes = (size_t)((uint64_t)b->n * root);
    return BGS_OK;
}

int bgs_bounce_search_workspace_bytes(const bgs_batch* b, int32_t iterations, int32_t edges, size_t* bytes) {
    NEED(b != nullptr, "batch is NULL");
    NEED(bytes != nullptr, "bytes is NULL");
    return bounce_search_check(b, iterations, edges, bytes);
}

// bgs_bounce_search_moves and bgs_bounce_search_moves_proving: the same checks and workspace; `entry` names the caller
// in the messages, and the proving entry point declares two more outputs
static int bounce_search_entry(const char* entry, bool proving, bgs_batch* b, uint64_t seed, int32_t iterations, int32_t leaf_playouts,
                               int32_t explore, int32_t max_plies, int policy, int32_t edges, int32_t* counts, int32_t* visits,
                               int32_t* best, int32_t* nodes, int32_t* used, int8_t* proved, int32_t* done, void* workspace,
                               size_t workspace_bytes, int on_device) {
    int rc = enter(b);
    if (rc) return rc;
    NEED(counts != nullptr, "counts is NULL");
    size_t need = 0;
    rc = bounce_search_check(b, iterations, edges, &need);
    if (rc) return rc;
    rc = search_params_check(entry, b, iterations, leaf_playouts, explore, max_plies, policy);
    if (rc) return rc;
    const size_t cells = (size_t)b->n * bounce_slots(b);
    bgs::OutputPlan plan;
    add_search_outputs(plan, b, cells, counts, visits, best, nodes);
    plan.add("used", used, (size_t)b->n * sizeof(int32_t));
    if (proving) {
        plan.add("proved", proved, cells * sizeof(int8_t));
        plan.add("done", done, (size_t)b->n * sizeof(int32_t));
    }
    const Workspace ws{workspace, workspace_bytes, need, "bgs_bounce_search_workspace_bytes"};
    return run_outputs(b, plan, on_device, &ws, [&](void* const* d, void* tree) {
        if (proving) {
            bgs::bounce_search_proving(b, seed, iterations, leaf_playouts, explore, max_plies, policy, edges, i32(d[0]), i32(d[1]),
                                       i32(d[2]), i32(d[3]), i32(d[4]), static_cast<int8_t*>(d[5]), i32(d[6]), tree);
        } else {
            bgs::bounce_search(b, seed, iterations, leaf_playouts, explore, max_plies, policy, edges, i32(d[0]), i32(d[1]), i32(d[2]),
                               i32(d[3]), i32(d[4]), tree);
        }
    });
}

int bgs_bounce_search_moves(bgs_batch* b, uint64_t seed, int32_t iterations, int32_t leaf_playouts, int32_t explore, int32_t max_plies,
                            int policy, int32_t edges, int32_t* counts, int32_t* visits, int32_t* best, int32_t* nodes, int32_t* used,
                            void* workspace, size_t workspace_bytes, int on_device) {
    return bounce_search_entry("search_moves", false, b, seed, iterations, leaf_playouts, explore, max_plies, policy, edges, counts, visits,
                               best, nodes, used, nullptr, nullptr, workspace, workspace_bytes, on_device);
}

int bgs_bounce_search_moves_proving(bgs_batch* b, uint64_t seed, int32_t iterations, int32_t leaf_playouts, int32_t explore,
                                    int32_t max_plies, int policy, int32_t edges, int32_t* counts, int32_t* visits, int32_t* best,
                                    int32_t* nodes, int32_t* used, int8_t* proved, int32_t* done, void* workspace,
                                    size_t workspace_bytes, int on_device) {
    return bounce_search_entry("search_moves_proving", true, b, seed, iterations, leaf_playouts, explore, max_plies, policy, edges, counts,
                               visits, best, nodes, used, proved, done, workspace, workspace_bytes, on_device);
}

// the game, board, nodes_cap and edges checks of the Bounce forest and guided entry points; `what` begins the messages about
// the batch, `connect_call` is where they send a Connect batch
static int bounce_trees_check(const bgs_batch* b, const char* what, const char* connect_call, int32_t nodes_cap, int32_t edges) {
    NEED(b->game == BGS_GAME_BOUNCE, "%s: Bounce batches only (Connect boards: %s)", what, connect_call);
    NEED(!b->generic, "%s: bit-packed Bounce boards only (up to %d cells, piece values up to %d); this %dx%d board is generic", what,
         BGS_BOUNCE_MAX_CELLS, BGS_BOUNCE_MAX_VALUE, b->gen_h, b->gen_w);
    NEED(nodes_cap >= 2 && nodes_cap <= BGS_BOUNCE_FOREST_MAX_NODES, "nodes_cap must be 2 .. %d nodes a tree (got %d)",
         BGS_BOUNCE_FOREST_MAX_NODES, nodes_cap);
    const int32_t least = BGS_BOUNCE_SEARCH_MIN_EDGES(b->bg.h, b->bg.w);
    NEED(edges >= least && edges <= BGS_BOUNCE_FOREST_MAX_EDGES,
         "edges must be BGS_BOUNCE_SEARCH_MIN_EDGES(%d, %d) = %d, the most arms a position can have, .. %d (got %d)", b->bg.h, b->bg.w,
         least, BGS_BOUNCE_FOREST_MAX_EDGES, edges);
    return BGS_OK;
}

// the checks of the three Bounce forest entry points that need no device; *bytes: the forest of the batch
static int bounce_forest_check(const bgs_batch* b, int32_t nodes_cap, int32_t edges, size_t* bytes) {
    const int rc = bounce_trees_check(b, "bounce_forest", "bgs_connect_forest_search", nodes_cap, edges);
    if (rc) return rc;
    const uint64_t tree = bgs::bounce_forest_tree_bytes(nodes_cap, edges);
    NEED((uint64_t)b->n <= (uint64_t)(SIZE_MAX / 2) / tree, "the forest of %lld boards x %d nodes x %d edges overflows size_t",
         (long long)b->n, nodes_cap, edges);
    *bytes = (size_t)((uint64_t)b->n * tree);
    return BGS_OK;
}

int bgs_bounce_forest_bytes(const bgs_batch* b, int32_t nodes, int32_t edges, size_t* bytes) {
    NEED(b != nullptr, "batch is NULL");
    NEED(bytes != nullptr, "bytes is NULL");
    return bounce_forest_check(b, nodes, edges, bytes);
}

int bgs_bounce_forest_search(bgs_batch* b, uint64_t seed, int32_t iterations, int32_t leaf_playouts, int32_t explore, int32_t max_plies,
                             int policy, int32_t nodes_cap, int32_t edges, int restart, int32_t* counts, int32_t* visits, int32_t* best,
                             int32_t* nodes, int32_t* used, int32_t* carried, void* forest, size_t forest_bytes, int on_device) {
    int rc = enter(b);
    if (rc) return rc;
    NEED(counts != nullptr, "counts is NULL");
    size_t need = 0;
    rc = bounce_forest_check(b, nodes_cap, edges, &need);
    if (rc) return rc;
    rc = search_params_check("bounce_forest_search", b, iterations, leaf_playouts, explore, max_plies, policy);
    if (rc) return rc;
    rc = forest_pointer(forest, forest_bytes, need, "bgs_bounce_forest_bytes");
    if (rc) return rc;
    bgs::OutputPlan plan;
    add_search_outputs(plan, b, (size_t)b->n * bounce_slots(b), counts, visits, best, nodes);
    plan.add("used", used, (size_t)b->n * sizeof(int32_t));
    plan.add("carried", carried, (size_t)b->n * sizeof(int32_t));
    return run_outputs(b, plan, on_device, nullptr, [&](void* const* d, void*) {
        bgs::bounce_forest_search(b, seed, iterations, leaf_playouts, explore, max_plies, policy, nodes_cap, edges, restart, i32(d[0]),
                                  i32(d[1]), i32(d[2]), i32(d[3]), i32(d[4]), i32(d[5]), forest);
    });
}

int bgs_bounce_forest_advance(bgs_batch* b, const int32_t* slots, int32_t nodes_cap, int32_t edges, int32_t* kept, void* forest,
                              size_t forest_bytes, int on_device) {
    int rc = enter(b);
    if (rc) return rc;
    NEED(slots != nullptr, "slots is NULL");
    size_t need = 0;
    rc = bounce_forest_check(b, nodes_cap, edges, &need);
    if (rc) return rc;
    rc = forest_pointer(forest, forest_bytes, need, "bgs_bounce_forest_bytes");
    if (rc) return rc;
    return forest_advance(b, slots, "slots", kept, on_device, [&](const int32_t* d_slots, int32_t* d_kept) {
        bgs::bounce_forest_advance(b, d_slots, nodes_cap, edges, d_kept, forest);
    });
}

// the checks of both Bounce guided entry points that need no device; *bytes: the trees of the batch
static int bounce_guided_check(const bgs_batch* b, int32_t nodes_cap, int32_t edges, size_t* bytes) {
    const int rc = bounce_trees_check(b, "bounce_guided", "bgs_connect_guided_step", nodes_cap, edges);
    if (rc) return rc;
    const uint64_t tree = bgs::bounce_guided_tree_bytes(nodes_cap, edges);
    NEED((uint64_t)b->n <= (uint64_t)(SIZE_MAX / 2) / tree, "the trees of %lld boards x %d nodes x %d edges overflow size_t",
         (long long)b->n, nodes_cap, edges);
    *bytes = (size_t)((uint64_t)b->n * tree);
    return BGS_OK;
}

int bgs_bounce_guided_bytes(const bgs_batch* b, int32_t nodes, int32_t edges, size_t* bytes) {
    NEED(b != nullptr, "batch is NULL");
    NEED(bytes != nullptr, "bytes is NULL");
    return bounce_guided_check(b, nodes, edges, bytes);
}

int bgs_bounce_guided_step(bgs_batch* b, int32_t nodes_cap, int32_t edges, int32_t cpuct, int32_t max_plies, uint32_t flags,
                           const float* priors, const float* values, int8_t* leaf_grid, int8_t* leaf_player, int32_t* leaf_kind,
                           uint64_t* leaf_targets, int32_t* visits, int32_t* scores, int32_t* best, int32_t* nodes, int32_t* used,
                           void* trees, size_t trees_bytes) {
    int rc = enter(b);
    if (rc) return rc;
    size_t need = 0;
    rc = bounce_guided_check(b, nodes_cap, edges, &need);
    if (rc) return rc;
    const GuidedPointer named[] = {{"priors", priors}, {"values", values}, {"leaf_grid", leaf_grid}, {"leaf_player", leaf_player},
                                   {"leaf_kind", leaf_kind}, {"leaf_targets", leaf_targets}, {"visits", visits}, {"scores", scores},
                                   {"best", best}, {"nodes", nodes}, {"used", used}};
    rc = guided_step_check(cpuct, &max_plies, flags, named, sizeof(named) / sizeof(named[0]), trees, trees_bytes, need, "bgs_bounce_guided_bytes");
    if (rc) return rc;
    bgs::bounce_guided_step(b, nodes_cap, edges, cpuct, max_plies, flags, priors, values, leaf_grid, leaf_player, leaf_kind, leaf_targets,
                            visits, scores, best, nodes, used, trees);
    return finish_launch();
}

int bgs_bounce_solve_moves(bgs_batch* b, int32_t depth, int64_t max_nodes, int8_t* codes, int16_t* plies, uint64_t* nodes,
                           int on_device) {
    int rc = enter(b);
    if (rc) return rc;
    NEED(codes != nullptr, "codes is NULL");
    NEED(b->game == BGS_GAME_BOUNCE, "solve_moves: Bounce batches only (Connect boards: bgs_connect_solve_actions)");
    NEED(!b->generic, "solve_moves: bit-packed Bounce boards only (up to %d cells, piece values up to %d); this %dx%d board is generic",
         BGS_BOUNCE_MAX_CELLS, BGS_BOUNCE_MAX_VALUE, b->gen_h, b->gen_w);
    NEED(depth >= 1, "depth must be >= 1 (got %d)", depth);
    NEED(depth <= BGS_BOUNCE_SOLVE_MAX_DEPTH, "depth %d is beyond the maximum of %d plies the search stack is sized for", depth,
         BGS_BOUNCE_SOLVE_MAX_DEPTH);
    NEED(max_nodes >= 1, "max_nodes must be >= 1 (got %lld)", (long long)max_nodes);
    uint64_t *d_ends, *d_totals;
    rc = bounce_move_scratch(b, &d_ends, &d_totals);
    if (rc) return rc;
    bgs::OutputPlan plan;
    add_solve_outputs(plan, (size_t)b->n * bounce_slots(b), codes, plies, nodes);
    return run_outputs(b, plan, on_device, nullptr, [&](void* const* d, void*) {
        bgs::bounce_solve(b, depth, max_nodes, static_cast<int8_t*>(d[0]), static_cast<int16_t*>(d[1]), solve_counter(b, d[2]), d_ends,
                          d_totals);
    });
}

int bgs_steps(bgs_batch* b, uint64_t* steps) {
    int rc = enter(b);
    if (rc) return rc;
    NEED(steps != nullptr, "steps is NULL");
    static thread_local unsigned long long shards[BGS_STEP_SHARDS * BGS_STEP_STRIDE];
    rc = to_host(b, shards, b->d_steps, (size_t)BGS_STEP_SHARDS * BGS_STEP_STRIDE);
    unsigned long long v = 0;
    for (int i = 0; i < BGS_STEP_SHARDS; ++i) v += shards[i * BGS_STEP_STRIDE];
    *steps = v;
    return rc;
}

int bgs_reset_steps(bgs_batch* b) {
    int rc = enter(b);
    if (rc) return rc;
    HIP_TRY(hipMemsetAsync(b->d_steps, 0, kStepBytes, b->stream));
    return BGS_OK;
}

int bgs_read_grid(bgs_batch* b, int8_t* grid) {
    int rc = enter(b);
    if (rc) return rc;
    NEED(grid != nullptr, "grid is NULL");
    const bool connect = b->game == BGS_GAME_CONNECT;
    const size_t cells = (size_t)b->n * (connect ? b->cg.h * b->cg.w : b->bg.h * b->bg.w);
    if (b->generic)  // the grid is stored in the reference layout already
        return to_host(b, grid, reinterpret_cast<const int8_t*>(b->d_planes), cells);
    Stage st(b);
    int8_t* d = st.take<int8_t>(cells);
    NEED(d != nullptr, "staging buffer too small");
    if (connect) bgs::connect_unpack_grid(b, d);
    else bgs::bounce_unpack_grid(b, d);
    rc = finish_launch();
    if (rc) return rc;
    return to_host(b, grid, d, cells);
}

static int read_meta(bgs_batch* b, int8_t* player, uint8_t* ended, int8_t* winner, int32_t* plies) {
    int rc = enter(b);
    if (rc) return rc;
    Stage st(b);
    int8_t* dp = player ? st.take<int8_t>((size_t)b->n) : nullptr;
    uint8_t* de = ended ? st.take<uint8_t>((size_t)b->n) : nullptr;
    int8_t* dw = winner ? st.take<int8_t>((size_t)b->n) : nullptr;
    int32_t* dl = plies ? st.take<int32_t>((size_t)b->n) : nullptr;
    NEED((!player || dp) && (!ended || de) && (!winner || dw) && (!plies || dl), "staging buffer too small");
    if (b->generic) bgs::generic_meta(b, dp, de, dw, dl);
    else if (b->game == BGS_GAME_CONNECT) bgs::connect_meta(b, dp, de, dw, dl);
    else bgs::bounce_meta(b, dp, de, dw, dl);
    rc = finish_launch();
    if (rc) return rc;
    if (player) HIP_TRY(hipMemcpyAsync(player, dp, (size_t)b->n, hipMemcpyDeviceToHost, b->stream));
    if (ended) HIP_TRY(hipMemcpyAsync(ended, de, (size_t)b->n, hipMemcpyDeviceToHost, b->stream));
    if (winner) HIP_TRY(hipMemcpyAsync(winner, dw, (size_t)b->n, hipMemcpyDeviceToHost, b->stream));
    if (plies) HIP_TRY(hipMemcpyAsync(plies, dl, (size_t)b->n * 4, hipMemcpyDeviceToHost, b->stream));
    HIP_TRY(hipStreamSynchronize(b->stream));
    return BGS_OK;
}

int bgs_read_player(bgs_batch* b, int8_t* player) {
    NEED(player != nullptr, "player is NULL");
    return read_meta(b, player, nullptr, nullptr, nullptr);
}

int bgs_read_ended(bgs_batch* b, uint8_t* ended) {
    NEED(ended != nullptr, "ended is NULL");
    return read_meta(b, nullptr, ended, nullptr, nullptr);
}

int bgs_read_winner(bgs_batch* b, int8_t* winner) {
    NEED(winner != nullptr, "winner is NULL");
    return read_meta(b, nullptr, nullptr, winner, nullptr);
}

int bgs_read_plies(bgs_batch* b, int32_t* plies) {
    NEED(plies != nullptr, "plies is NULL");
    return read_meta(b, nullptr, nullptr, nullptr, plies);
}

int bgs_read_reward(bgs_batch* b, int8_t* reward) {
    int rc = enter(b);
    if (rc) return rc;
    NEED(reward != nullptr, "reward is NULL");
    return to_host(b, reward, b->d_reward, (size_t)b->n * 2);
}

int bgs_read_legal(bgs_batch* b, uint8_t* legal) {
    int rc = enter(b);
    if (rc) return rc;
    NEED(legal != nullptr, "legal is NULL");
    NEED(b->game == BGS_GAME_CONNECT, "bgs_read_legal is a Connect entry point; use bgs_bounce_read_targets");
    Stage st(b);
    uint8_t* d = st.take<uint8_t>((size_t)b->n * b->cg.w);
    NEED(d != nullptr, "staging buffer too small");
    if (b->generic) bgs::generic_connect_legal(b, d, nullptr);
    else bgs::connect_legal(b, d, nullptr);
    rc = finish_launch();
    if (rc) return rc;
    return to_host(b, legal, d, (size_t)b->n * b->cg.w);
}

int bgs_read_action_count(bgs_batch* b, int32_t* count) {
    int rc = enter(b);
    if (rc) return rc;
    NEED(count != nullptr, "count is NULL");
    Stage st(b);
    int32_t* d = st.take<int32_t>((size_t)b->n);
    NEED(d != nullptr, "staging buffer too small");
    if (b->generic && b->game == BGS_GAME_CONNECT) bgs::generic_connect_legal(b, nullptr, d);
    else if (b->generic) bgs::generic_bounce_targets(b, nullptr, d);
    else if (b->game == BGS_GAME_CONNECT) bgs::connect_legal(b, nullptr, d);
    else bgs::bounce_targets(b, nullptr, d);
    rc = finish_launch();
    if (rc) return rc;
    return to_host(b, count, d, (size_t)b->n);
}

int bgs_bounce_read_targets(bgs_batch* b, uint64_t* targets) {
    int rc = enter(b);
    if (rc) return rc;
    NEED(targets != nullptr, "targets is NULL");
    NEED(b->game == BGS_GAME_BOUNCE, "bgs_bounce_read_targets needs a Bounce batch");
    NEED(!b->generic, "this Bounce board does not fit 64-bit target masks (more than 64 cells or values above 15): "
                      "read its moves through bgs_transition's wide legal record");
    Stage st(b);
    uint64_t* d = st.take<uint64_t>((size_t)b->n * (b->bg.w + 1));
    NEED(d != nullptr, "staging buffer too small");
    bgs::bounce_targets(b, d, nullptr);
    rc = finish_launch();
    if (rc) return rc;
    return to_host(b, targets, d, (size_t)b->n * (b->bg.w + 1));
}

int bgs_export_device(bgs_batch* b, int what, void* device_dst) {
    int rc = enter(b);
    if (rc) return rc;
    NEED(device_dst != nullptr, "destination is NULL");
    switch (what) {
        case 'g':
            NEED(((uintptr_t)device_dst % 16) == 0, "grid destination must be 16-byte aligned");
            if (b->generic) bgs::generic_unpack_grid(b, static_cast<int8_t*>(device_dst));
            else if (b->game == BGS_GAME_CONNECT) bgs::connect_unpack_grid(b, static_cast<int8_t*>(device_dst));
            else bgs::bounce_unpack_grid(b, static_cast<int8_t*>(device_dst));
            break;
        case 'l':
            NEED(b->game == BGS_GAME_CONNECT, "'l' (legal mask) is Connect only");
            if (b->generic) bgs::generic_connect_legal(b, static_cast<uint8_t*>(device_dst), nullptr);
            else bgs::connect_legal(b, static_cast<uint8_t*>(device_dst), nullptr);
            break;
        case 'c':
            if (b->generic && b->game == BGS_GAME_CONNECT) bgs::generic_connect_legal(b, nullptr, static_cast<int32_t*>(device_dst));
            else if (b->generic) bgs::generic_bounce_targets(b, nullptr, static_cast<int32_t*>(device_dst));
            else if (b->game == BGS_GAME_CONNECT) bgs::connect_legal(b, nullptr, static_cast<int32_t*>(device_dst));
            else bgs::bounce_targets(b, nullptr, static_cast<int32_t*>(device_dst));
            break;
        case 't':
            NEED(b->game == BGS_GAME_BOUNCE, "'t' (target masks) is Bounce only");
            NEED(!b->generic, "'t' needs a board of at most 64 cells with values up to 15 (64-bit target masks)");
            bgs::bounce_targets(b, static_cast<uint64_t*>(device_dst), nullptr);
            break;
        case 'r':
            HIP_TRY(hipMemcpyAsync(device_dst, b->d_reward, (size_t)b->n * 2, hipMemcpyDeviceToDevice, b->stream));
            break;
        default:
            return fail(BGS_ERR_ARG, "unknown export kind '%c'", what);
    }
    return finish_launch();
}

int bgs_pack_outcomes(bgs_batch* b, void* device_dst) {
    int rc = enter(b);
    if (rc) return rc;
    NEED(device_dst != nullptr, "destination is NULL");
    bgs::pack_outcomes(b, static_cast<uint8_t*>(device_dst));
    return finish_launch();
}

int bgs_rollout_pack(bgs_batch* b, uint64_t seed, int32_t max_plies, uint32_t flags, void* device_dst) {
    NEED(b != nullptr, "batch handle is NULL");
    return bgs::rollout_with_codes(b, seed, max_plies, flags, static_cast<uint8_t*>(device_dst));
}

int bgs_expand_outcomes(int device, void* hip_stream, const void* device_packed, int64_t n, int8_t* device_reward) {
    NEED(device_packed != nullptr && device_reward != nullptr && n >= 0, "bad argument");
    int rc = check_device(device);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(device));
    NEED(((uintptr_t)device_reward % 8) == 0, "reward buffer must be 8-byte aligned");
    if (n == 0) return BGS_OK;
    const int64_t bytes = (n + 3) / 4;
    hipLaunchKernelGGL(k_expand_outcomes, dim3((unsigned)((bytes + BGS_BLOCK - 1) / BGS_BLOCK)), dim3(BGS_BLOCK), 0,
                       static_cast<hipStream_t>(hip_stream), static_cast<const uint8_t*>(device_packed), n,
                       reinterpret_cast<uint16_t*>(device_reward));
    return finish_launch();
}

int bgs_write_state(bgs_batch* b, const int8_t* grid, const int8_t* player, const int8_t* winner, const int32_t* plies,
                    int32_t* status) {
    int rc = enter(b);
    if (rc) return rc;
    NEED(grid != nullptr, "grid is NULL");
    const bool connect = b->game == BGS_GAME_CONNECT;
    const size_t cells = (size_t)b->n * (connect ? b->cg.h * b->cg.w : b->bg.h * b->bg.w);
    Stage st(b);
    int8_t* dg = st.take<int8_t>(cells);
    int8_t* dp = player ? st.take<int8_t>((size_t)b->n) : nullptr;
    int8_t* dw = winner ? st.take<int8_t>((size_t)b->n) : nullptr;
    int32_t* dl = (plies && !connect) ? st.take<int32_t>((size_t)b->n) : nullptr;
    int32_t* dr = st.take<int32_t>((size_t)b->n);
    NEED(dg != nullptr && dr != nullptr && (!player || dp) && (!winner || dw) && (!(plies && !connect) || dl),
         "staging buffer too small");
    if ((rc = to_device(b, dg, grid, cells))) return rc;
    if (player && (rc = to_device(b, dp, player, (size_t)b->n))) return rc;
    if (winner && (rc = to_device(b, dw, winner, (size_t)b->n))) return rc;
    if (dl && (rc = to_device(b, dl, plies, (size_t)b->n))) return rc;
    if (b->generic) bgs::generic_pack(b, dg, dp, dw, dl, dr);
    else if (connect) bgs::connect_pack(b, dg, dp, dw, dr);
    else bgs::bounce_pack(b, dg, dp, dw, dl, dr);
    rc = finish_launch();
    if (rc) return rc;
    if (status) return to_host(b, status, dr, (size_t)b->n);
    HIP_TRY(hipStreamSynchronize(b->stream));
    return BGS_OK;
}

int bgs_transition(bgs_batch* b, const int8_t* grid, const int8_t* player, const int8_t* winner, const int32_t* plies,
                   const int32_t* actions, int32_t* status, int8_t* grid_out, int8_t* player_out, int8_t* winner_out,
                   int32_t* plies_out, void* legal_out, int8_t* reward_out) {
    int rc = enter(b);
    if (rc) return rc;
    NEED(status && grid_out && player_out && winner_out && plies_out && legal_out, "output pointer is NULL");
    NEED(b->n <= 4096, "bgs_transition serves the object API: batches of at most 4096 boards");
    const bool connect = b->game == BGS_GAME_CONNECT;
    const size_t n = (size_t)b->n;
    const size_t hw = connect ? (size_t)b->cg.h * b->cg.w : (size_t)b->bg.h * b->bg.w;
    const size_t per_action = connect ? 1 : 4;
    const size_t legal_bytes = n * legal_bytes_per_board(b);
    auto up8 = [](size_t v) { return (v + 7) & ~(size_t)7; };
    // in-block: [grid][player][winner][plies][actions]; out-block: [load status][step status][grid][player][winner][plies][legal]
    const size_t in_grid = 0, in_player = up8(n * hw), in_winner = in_player + up8(n), in_plies = in_winner + up8(n),
                 in_actions = in_plies + 4 * n, in_bytes = in_actions + 4 * n * per_action;
    const size_t out_load = 0, out_step = 4 * n, out_legal = up8(out_step + 4 * n),
                 out_grid = (out_legal + legal_bytes + 15) & ~(size_t)15,  // the unpack tile store needs 16-byte alignment
                
                 out_player = up8(out_grid + n * hw), out_winner = out_player + up8(n), out_plies = out_winner + up8(n),
                 out_reward = out_plies + 4 * n, out_bytes = out_reward + 2 * n;
    const bool load = grid != nullptr;
    if (load) NEED(player != nullptr && winner != nullptr, "player and winner are required with a grid");
    // small batches: blocks in host memory the device addresses, launches replayed from a graph (see SmallTransition)
    const int mode = (b->n <= kSmallTransition && in_bytes <= kSmallBlock && out_bytes <= kSmallBlock - 64) ? transition_mode() : 0;
    SmallTransition* small = nullptr;
    uint8_t *d_in, *d_out, *h_in, *h_out;
    if (mode) {
        rc = small_transition(b, &small);
        if (rc) return rc;
        d_in = small->d_in; d_out = small->d_out; h_in = small->h_in; h_out = small->h_out;
    } else {
        Stage st(b);
        d_in = st.take<uint8_t>(in_bytes);
        d_out = st.take<uint8_t>(out_bytes);
        NEED(d_in && d_out, "staging buffer too small");
        if (!b->pinned[0]) {
            HIP_TRY(hipHostMalloc(&b->pinned[0], kPinnedChunk, hipHostMallocDefault));
            HIP_TRY(hipHostMalloc(&b->pinned[1], kPinnedChunk, hipHostMallocDefault));
            HIP_TRY(hipEventCreateWithFlags(&b->pinned_done[0], hipEventDisableTiming));
            HIP_TRY(hipEventCreateWithFlags(&b->pinned_done[1], hipEventDisableTiming));
        }
        NEED(in_bytes <= kPinnedChunk && out_bytes <= kPinnedChunk,
             "batch too large for bgs_transition (%zu bytes per call): use fewer boards per call", out_bytes);
        h_in = static_cast<uint8_t*>(b->pinned[0]);
        h_out = static_cast<uint8_t*>(b->pinned[1]);
    }
    if (load) {
        memcpy(h_in + in_grid, grid, n * hw);
        memcpy(h_in + in_player, player, n);
        memcpy(h_in + in_winner, winner, n);
        if (plies) memcpy(h_in + in_plies, plies, 4 * n);
    }
    if (actions) memcpy(h_in + in_actions, actions, 4 * n * per_action);
    if (mode) {
        memset(h_out, 0, 8 * n);  // the two status words per board
    } else {
        if (load || actions) HIP_TRY(hipMemcpyAsync(d_in, h_in, in_bytes, hipMemcpyHostToDevice, b->stream));
        HIP_TRY(hipMemsetAsync(d_out, 0, 8 * n, b->stream));
    }
    // The fused kernel publishes a ticket behind its records: the host takes them as soon as it SEES the ticket, which is
    // earlier than the stream's completion signal comes back (experiment transition_spin=0: wait for the stream as before).  The
    // kernel that wrote the ticket has nothing left to do, so the next call may reuse the blocks; the stream itself is
    // synchronised now and then, and whenever the ticket does not show within 2 ms (a failed launch reports itself there).
    static const bool spin_wanted = [] { const char* e = bgs::experiment("transition_spin"); return !(e && e[0] == '0'); }();
    const bool spin = mode == 3 && spin_wanted && !b->generic;
    bool fused = false;
    auto launch_all = [&]() -> int {
        int32_t* d_load = reinterpret_cast<int32_t*>(d_out + out_load);
        int32_t* d_step = reinterpret_cast<int32_t*>(d_out + out_step);
        if (load) {
            const int8_t* dg = reinterpret_cast<const int8_t*>(d_in + in_grid);
            const int8_t* dp = reinterpret_cast<const int8_t*>(d_in + in_player);
            const int8_t* dw = reinterpret_cast<const int8_t*>(d_in + in_winner);
            const int32_t* dl = plies ? reinterpret_cast<const int32_t*>(d_in + in_plies) : nullptr;
            if (b->generic) bgs::generic_pack(b, dg, dp, dw, dl, d_load);
            else if (connect) bgs::connect_pack(b, dg, dp, dw, d_load);
            else bgs::bounce_pack(b, dg, dp, dw, dl, d_load);
        }
        int8_t* og = reinterpret_cast<int8_t*>(d_out + out_grid);
        int8_t* op = reinterpret_cast<int8_t*>(d_out + out_player);
        int8_t* ow = reinterpret_cast<int8_t*>(d_out + out_winner);
        int32_t* ol = reinterpret_cast<int32_t*>(d_out + out_plies);
        if (mode == 3 && !b->generic) {
            // the move and the whole observation in one launch (k_connect_transition / k_bounce_transition)
            const int32_t* da = actions ? reinterpret_cast<const int32_t*>(d_in + in_actions) : nullptr;
            int8_t* orw = reinterpret_cast<int8_t*>(d_out + out_reward);
            uint32_t* d_done = spin ? reinterpret_cast<uint32_t*>(d_out + kSmallBlock - 64) : nullptr;
            const uint32_t ticket = spin ? ++small->ticket : 0;
            if (connect) bgs::connect_transition(b, da, d_step, og, op, ow, ol, d_out + out_legal, orw, d_done, ticket);
            else bgs::bounce_transition(b, da, d_step, og, op, ow, ol, reinterpret_cast<uint64_t*>(d_out + out_legal), orw, d_done, ticket);
            fused = true;
            return finish_launch();
        }
        if (actions) {
            const int32_t* da = reinterpret_cast<const int32_t*>(d_in + in_actions);
            if (b->generic) bgs::generic_step_actions(b, da, d_step);
            else if (connect) bgs::connect_step_actions(b, da, d_step);
            else bgs::bounce_step_actions(b, da, d_step);
        }
        if (b->generic) {
            bgs::generic_unpack_grid(b, og);
            bgs::generic_meta(b, op, nullptr, ow, ol);
            if (connect) bgs::generic_connect_legal(b, d_out + out_legal, nullptr);
            else bgs::generic_bounce_targets(b, d_out + out_legal, nullptr);
        } else if (connect) {
            bgs::connect_unpack_grid(b, og);
            bgs::connect_meta(b, op, nullptr, ow, ol);
            bgs::connect_legal(b, d_out + out_legal, nullptr);
        } else {
            bgs::bounce_unpack_grid(b, og);
            bgs::bounce_meta(b, op, nullptr, ow, ol);
            bgs::bounce_targets(b, reinterpret_cast<uint64_t*>(d_out + out_legal), nullptr);
        }
        // the reward pairs as the kernels wrote them (State::get_reward): no host-side rule
        if (mode) hipLaunchKernelGGL(k_copy_small, dim3(1), dim3(64), 0, b->stream, reinterpret_cast<const uint8_t*>(b->d_reward), 2 * n, d_out + out_reward);
        else HIP_TRY(hipMemcpyAsync(d_out + out_reward, b->d_reward, 2 * n, hipMemcpyDeviceToDevice, b->stream));
        return finish_launch();
    };
    bool replayed = false;
    if (mode == 2 && b->stream != nullptr && !small->graph_failed) {
        const int key = (load ? 1 : 0) | (plies ? 2 : 0) | (actions ? 4 : 0);
        if (!small->exec[key]) {
            hipGraph_t graph = nullptr;
            hipError_t e = hipStreamBeginCapture(b->stream, hipStreamCaptureModeThreadLocal);
            if (e == hipSuccess) {
                const int launched = launch_all();
                e = hipStreamEndCapture(b->stream, &graph);
                if (e == hipSuccess && launched) e = hipErrorLaunchFailure;
            }
            if (e == hipSuccess && graph) e = hipGraphInstantiate(&small->exec[key], graph, nullptr, nullptr, 0);
            if (graph) (void)hipGraphDestroy(graph);
            if (e != hipSuccess) {  // this runtime does not capture the sequence: launch it directly from now on
                small->exec[key] = nullptr;
                small->graph_failed = true;
                (void)hipGetLastError();
            }
        }
        if (small->exec[key]) {
            HIP_TRY(hipGraphLaunch(small->exec[key], b->stream));
            replayed = true;
        }
    }
    if (!replayed) {
        rc = launch_all();
        if (rc) return rc;
    }
    if (!mode) HIP_TRY(hipMemcpyAsync(h_out, d_out, out_bytes, hipMemcpyDeviceToHost, b->stream));
    bool seen = false;
    if (spin && fused && ++small->unsynced < 1024) {
        const volatile uint32_t* done = reinterpret_cast<const volatile uint32_t*>(h_out + kSmallBlock - 64);
        const auto t0 = std::chrono::steady_clock::now();
        for (uint32_t turn = 1; !(seen = __atomic_load_n(done, __ATOMIC_ACQUIRE) == small->ticket); ++turn) {
            __builtin_ia32_pause();
            if ((turn & 255u) == 0 && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(2)) break;
        }
    }
    if (!seen) {
        HIP_TRY(hipStreamSynchronize(b->stream));
        if (small) small->unsynced = 0;
    }
    // a malformed board was left untouched and an illegal move changed nothing: report the first problem per board
    const int32_t* load_status = reinterpret_cast<const int32_t*>(h_out + out_load);
    const int32_t* step_status = reinterpret_cast<const int32_t*>(h_out + out_step);
    for (size_t i = 0; i < n; ++i) status[i] = load_status[i] ? load_status[i] : step_status[i];
    memcpy(grid_out, h_out + out_grid, n * hw);
    memcpy(player_out, h_out + out_player, n);
    memcpy(winner_out, h_out + out_winner, n);
    memcpy(plies_out, h_out + out_plies, 4 * n);
    memcpy(legal_out, h_out + out_legal, legal_bytes);
    if (reward_out) memcpy(reward_out, h_out + out_reward, 2 * n);
    return BGS_OK;
}

}  // extern "C"
