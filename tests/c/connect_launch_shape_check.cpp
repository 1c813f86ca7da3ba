// Stand-alone check of the rollout launch shape and of K2o's admission predicate (connect_unit.h:
// connect_launch_shape, connect_opened_ok, connect_opened_blocks; tests/test_connect_launch_shape.py compiles and runs it,
// once plain and once with -fsanitize=address,undefined).  The expectations are the formulas the three launchers
// (connect_rollout, connect_steps_ok, connect_rollout_steps) each wrote out before the header had them, restated here.
// It prints the number of shapes and predicate cases checked and exits 1 after the first failures.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "connect_unit.h"

static int failures = 0;

static void fail(const char* what, long long n, int cus, int wps, int chunk) {
    std::printf("FAIL %s: n %lld CUs %d wps %d chunk %d\n", what, n, cus, wps, chunk);
    if (++failures >= 10) std::exit(1);
}

int main() {
    // the bench's shape: 2^20 one-word boards on 256 CUs at two waves a SIMD
    static_assert(connect_launch_shape(1 << 20, 256, 2, 0).per_wave == 512, "eight games a lane");
    static_assert(connect_launch_shape(1 << 20, 256, 2, 0).blocks == 512, "2048 waves");
    static_assert(connect_launch_shape(333, 256, 2, 128).waves == 3, "two whole chunks and one of 77 games");

    std::vector<long long> ns;
    for (long long n = 1; n <= 4096; ++n) ns.push_back(n);
    for (long long n : {65535ll, 65536ll, 1ll << 20, (1ll << 20) + 1, 1ll << 24, (1ll << 31) + 5}) ns.push_back(n);
    long long shapes = 0;
    for (long long n : ns)
        for (int wps = 1; wps <= 8; ++wps)
            for (int chunk : {0, 64, 128})
                for (int cus : {1, 8, 256}) {
                    const ConnectLaunchShape s = connect_launch_shape(n, cus, wps, chunk);
                    ++shapes;
                    // as the launchers computed it
                    const long long resident = (long long)cus * 4 * wps;
                    long long per_wave = chunk > 0 ? chunk : (n + resident - 1) / resident;
                    per_wave = (per_wave + 64 - 1) / 64 * 64;
                    const long long waves = (n + per_wave - 1) / per_wave;
                    if (s.per_wave != per_wave || s.waves != waves) fail("per_wave / waves", n, cus, wps, chunk);
                    if (s.blocks != (unsigned)((waves + 3) / 4)) fail("blocks", n, cus, wps, chunk);
                    if (s.code_lds != (size_t)4 * (per_wave / 16) * sizeof(uint32_t)) fail("code_lds", n, cus, wps, chunk);
                    if (s.outcome_lds != (size_t)4 * per_wave) fail("outcome_lds", n, cus, wps, chunk);
                    if (s.outcome_lds2 != (size_t)4 * 2 * per_wave || s.outcome_lds2 != (size_t)8 * per_wave)
                        fail("outcome_lds2", n, cus, wps, chunk);
                    // what the kernels rest on
                    if (s.per_wave <= 0 || s.per_wave % 64 != 0) fail("per_wave is no multiple of 64", n, cus, wps, chunk);
                    if (!(s.waves * s.per_wave >= n && n > (s.waves - 1) * s.per_wave)) fail("waves do not cover n once", n, cus, wps, chunk);
                    if ((long long)s.blocks * 4 < s.waves || ((long long)s.blocks - 1) * 4 >= s.waves) fail("blocks do not cover the waves", n, cus, wps, chunk);
                    if (chunk > 0 && s.per_wave != chunk) fail("a chunk of whole waves is taken as it is", n, cus, wps, chunk);
                }

    // K2o's admission and its opening blocks, as connect_rollout wrote them: over every one-, two- and three-word geometry
    // of up to 9 x 9, both entry states, cap or none, every opening setting and a chunk on either side of the LDS limit
    long long cases = 0;
    for (int h = 1; h <= 9; ++h)
        for (int w = 1; w <= 9; ++w)
            for (int k = 2; k <= 6; ++k)
                for (int initial = 0; initial <= 1; ++initial)
                    for (int capped = 0; capped <= 1; ++capped)
                        for (int opening = -1; opening <= 7; ++opening)
                            for (int chunk : {64, 8192, 8256}) {
                                const ConnectGeom cg = {h, w, k, (w * (h + 1) + 63) / 64};
                                const ConnectLaunchShape s = connect_launch_shape(100000, 256, 2, chunk);
                                ++cases;
                                const bool nibble_ok = cg.nw == 1 && cg.w <= 8 && cg.h <= 8;
                                const size_t outcome_lds = (size_t)4 * s.per_wave;
                                const bool want = nibble_ok && initial && !capped && opening && cg.h >= 4 && cg.w >= 2 && cg.k >= 3 &&
                                                  cg.h * cg.w <= 48 && outcome_lds <= (32u << 10);
                                if (connect_nibble_ok(cg) != nibble_ok) fail("connect_nibble_ok", h * 100 + w * 10 + k, initial, capped, opening);
                                if (connect_opened_ok(cg, initial != 0, capped != 0, opening, s) != want)
                                    fail("connect_opened_ok", h * 100 + w * 10 + k, initial, capped, opening);
                                const bool deep = cg.k >= 4 && cg.h >= 6;
                                int blocks = 4;   // (the launcher's switch: 1, 2, 3, and 4 for everything else)
                                switch (deep ? opening : 1) {
                                    case 1: blocks = 1; break;
                                    case 2: blocks = 2; break;
                                    case 3: blocks = 3; break;
                                    default: break;
                                }
                                if (connect_opened_blocks(cg, opening) != blocks) fail("connect_opened_blocks", h * 100 + w * 10 + k, initial, capped, opening);
                            }
    const ConnectGeom c4 = {6, 7, 4, 1};
    if (!connect_opened_ok(c4, true, false, kRolloutOpeningBlocks, connect_launch_shape(1 << 20, 256, 2, 0))) fail("the bench's call is K2o's", 1 << 20, 256, 2, 0);
    if (connect_opened_blocks(c4, kRolloutOpeningBlocks) != kRolloutOpeningBlocks) fail("the default opening", 1 << 20, 256, 2, 0);

    std::printf("%lld shapes and %lld predicate cases checked, %d failures\n", shapes, cases, failures);
    return failures ? 1 : 0;
}
