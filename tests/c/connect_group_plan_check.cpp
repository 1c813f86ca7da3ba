// Stand-alone check of connect_group_plan.h (tests/test_connect_group_plan.py compiles and runs it, once plain and once
// with -fsanitize=address,undefined).  It sweeps every call length, pipeline depth, steps per launch, host-array count
// and ring size the test names and checks what the header promises; it prints the number of plans checked and a few
// sample plans, and exits 1 at the first plan that breaks a promise.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "connect_group_plan.h"

static int failures = 0;

static void fail(const char* what, long long count, int depth, int steps, int hosts, int ring, const std::vector<int>& plan) {
    std::printf("FAIL %s: count %lld depth %d S %d host arrays %d ring %d plan", what, count, depth, steps, hosts, ring);
    for (int k : plan) std::printf(" %d", k);
    std::printf("\n");
    if (++failures >= 10) std::exit(1);
}

static std::vector<int> launches(long long count, int depth, int steps, int hosts, int ring) {
    ConnectGroupPlan p = connect_group_plan(count, depth, steps, hosts, ring);
    std::vector<int> out;
    for (int k; (k = connect_group_next(p)) != 0;) {
        out.push_back(k);
        if ((long long)out.size() > count + 1) break;   // (a plan that never ends is reported below: its sum is off)
    }
    return out;
}

int main() {
    static_assert(connect_group_taper_steps(8, 3) == 7, "4 + 2 + 1");
    static_assert(connect_group_taper_steps(2, 3) == 3, "1, padded to three launches");
    static_assert(connect_group_taper_steps(6, 4) == 6, "3 + 1, padded to four launches");
    const int step_choices[] = {1, 2, 3, 4, 6, 8};
    const int rings[] = {9, 32};
    long long checked = 0;
    for (long long count = 0; count <= 300; ++count)
        for (int depth = 1; depth <= 4; ++depth)
            for (int steps : step_choices)
                for (int hosts = steps; hosts <= 12; ++hosts)
                    for (int ring : rings) {
                        const std::vector<int> plan = launches(count, depth, steps, hosts, ring);
                        ++checked;
                        // covered once, in order: the sizes are positive and add up to the call
                        long long sum = 0;
                        bool positive = true;
                        for (int k : plan) {
                            sum += k;
                            positive = positive && k >= 1;
                        }
                        if (sum != count || !positive) {
                            fail("the launches do not cover the call", count, depth, steps, hosts, ring, plan);
                            continue;
                        }
                        // the last `depth` steps are launches of one (each goes to its own batch's stream)
                        const long long singles = count < depth ? count : depth;
                        bool last_ok = (long long)plan.size() >= singles;
                        for (long long j = 0; last_ok && j < singles; ++j) last_ok = plan[plan.size() - 1 - j] == 1;
                        if (!last_ok) fail("the last steps are not launches of one", count, depth, steps, hosts, ring, plan);
                        // no launch above S, the host arrays or the ring; a launch claims its tickets before it is
                        // enqueued, the sink lets a claim through while fewer than `ring` are outstanding, so with every
                        // launch at most `ring` the tickets outstanding never exceed it (modelled: nothing completes
                        // until a claim blocks, then the oldest launch does)
                        std::vector<int> in_flight;
                        long long outstanding = 0, most = 0;
                        bool size_ok = true;
                        for (size_t j = 0; j + singles < plan.size(); ++j) {
                            const int k = plan[j];
                            size_ok = size_ok && k <= steps && k <= hosts && k <= ring;
                            for (int q = 0; q < k; ++q) {
                                while (outstanding >= ring && !in_flight.empty()) {
                                    outstanding -= in_flight.front();
                                    in_flight.erase(in_flight.begin());
                                }
                                ++outstanding;
                                most = outstanding > most ? outstanding : most;
                            }
                            in_flight.push_back(k);
                        }
                        if (!size_ok) fail("a launch is too large", count, depth, steps, hosts, ring, plan);
                        if (most > ring) fail("more tickets outstanding than the ring holds", count, depth, steps, hosts, ring, plan);
                        // the tapered tail: in the last 2 x depth launches no launch is larger than half the one before
                        // it, unless it is a launch of one already
                        const size_t window = 2 * (size_t)depth < plan.size() ? 2 * (size_t)depth : plan.size();
                        bool taper_ok = true;
                        for (size_t j = plan.size() - window; j < plan.size(); ++j)
                            if (j >= 1 && plan[j] != 1 && 2 * plan[j] > plan[j - 1]) taper_ok = false;
                        if (!taper_ok) fail("the tail does not taper", count, depth, steps, hosts, ring, plan);
                    }
    const long long samples[][5] = {{27, 3, 8, 9, 32}, {40, 3, 8, 9, 32}, {100, 3, 8, 9, 32}, {200, 3, 8, 9, 32}, {200, 3, 2, 9, 32},
                                    {12, 3, 8, 9, 32}, {30, 2, 8, 8, 32}, {50, 3, 6, 12, 9}};
    for (const auto& s : samples) {
        std::printf("count %lld depth %lld S %lld host arrays %lld ring %lld:", s[0], s[1], s[2], s[3], s[4]);
        for (int k : launches(s[0], (int)s[1], (int)s[2], (int)s[3], (int)s[4])) std::printf(" %d", k);
        std::printf("\n");
    }
    std::printf("%lld plans checked, %d failures\n", checked, failures);
    return failures ? 1 : 0;
}
