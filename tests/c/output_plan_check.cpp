// Stand-alone check of output_plan.h (tests/test_output_plan.py compiles and runs it, once plain and once with
// -fsanitize=address,undefined).  It declares the outputs of every call shape bgs_capi.hip uses -- evaluate, halving,
// search, proving search, forest search (each search with and without Bounce's `used`) and solve -- for n in 1..70
// boards, 1..16 root moves a board and every subset of absent optional outputs, and checks what the header promises.  It
// prints the number of plans checked and exits 1 after ten broken promises.
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "output_plan.h"

using bgs::OutputPlan;

static int failures = 0;

static void fail(const char* what, const char* shape, int n, int width, unsigned absent, int output) {
    std::printf("FAIL %s: shape %s n %d width %d absent mask 0x%x output %d\n", what, shape, n, width, absent, output);
    if (++failures >= 10) std::exit(1);
}

struct Field {
    const char* name;
    size_t per_cell, per_board, fixed;   // bytes = cells * per_cell + n * per_board + fixed
    bool optional;
    size_t align;
};
struct Shape {
    const char* name;
    bool workspace;   // a search: the library's own workspace may follow the outputs
    int count;
    Field field[OutputPlan::kMax];
};

static const Field COUNTS = {"counts", 12, 0, 0, false, 16}, VISITS = {"visits", 4, 0, 0, true, 16}, GIVEN = {"given", 4, 0, 0, true, 16},
                   BEST = {"best", 0, 4, 0, true, 16}, NODES = {"nodes", 0, 4, 0, true, 16}, USED = {"used", 0, 4, 0, true, 16},
                   PROVED = {"proved", 1, 0, 0, true, 16}, DONE = {"done", 0, 4, 0, true, 16}, CARRIED = {"carried", 0, 4, 0, true, 16},
                   CODES = {"codes", 1, 0, 0, false, 16}, PLIES = {"plies", 2, 0, 0, true, 16}, TOTAL = {"nodes", 0, 0, 8, true, 8};
static const Shape SHAPES[] = {
    {"evaluate", false, 1, {COUNTS}},
    {"halving", false, 3, {COUNTS, GIVEN, BEST}},
    {"search", true, 4, {COUNTS, VISITS, BEST, NODES}},
    {"search+used", true, 5, {COUNTS, VISITS, BEST, NODES, USED}},
    {"proving", true, 6, {COUNTS, VISITS, BEST, NODES, PROVED, DONE}},
    {"proving+used", true, 7, {COUNTS, VISITS, BEST, NODES, USED, PROVED, DONE}},
    {"forest", false, 5, {COUNTS, VISITS, BEST, NODES, CARRIED}},
    {"forest+used", false, 6, {COUNTS, VISITS, BEST, NODES, USED, CARRIED}},
    {"solve", false, 3, {CODES, PLIES, TOTAL}},
};

alignas(16) static char memory[16 * OutputPlan::kMax + 16];   // pointers to tell present from absent: never dereferenced

static OutputPlan declare(const Shape& s, int n, int width, unsigned absent, int bumped = -1) {
    OutputPlan plan;
    for (int i = 0, opt = 0; i < s.count; ++i) {
        const Field& f = s.field[i];
        const bool gone = f.optional && ((absent >> opt) & 1u);
        opt += f.optional;
        char* p = gone ? nullptr : memory + 16 * i + (i == bumped ? f.align / 2 : 0);
        plan.add(f.name, p, (size_t)n * width * f.per_cell + (size_t)n * f.per_board + f.fixed, f.optional, f.align);
    }
    return plan;
}

int main() {
    long long checked = 0;
    for (const Shape& s : SHAPES) {
        int optional = 0;
        for (int i = 0; i < s.count; ++i) optional += s.field[i].optional;
        for (int n = 1; n <= 70; ++n)
            for (int width = 1; width <= 16; ++width)
                for (unsigned absent = 0; absent < (1u << optional); ++absent) {
                    const OutputPlan plan = declare(s, n, width, absent);
                    ++checked;
                    if (!plan.ok || plan.count != s.count) fail("the plan refuses the shape", s.name, n, width, absent, -1);
                    if (plan.misaligned() != -1) fail("aligned pointers reported", s.name, n, width, absent, plan.misaligned());
                    size_t at = 0;   // the end of the slices so far
                    for (int i = 0; i < plan.count; ++i) {
                        const OutputPlan::Output& o = plan.out[i];
                        if (!o.ptr) continue;
                        if (o.offset % 16) fail("slice not 16-byte aligned", s.name, n, width, absent, i);
                        if (o.offset < at) fail("slice overlaps the one before", s.name, n, width, absent, i);
                        if (o.offset - at >= 16) fail("more than the rounding between slices", s.name, n, width, absent, i);
                        if (o.offset + o.bytes > plan.end) fail("slice passes the end", s.name, n, width, absent, i);
                        at = o.offset + o.bytes;
                        // a device pointer that breaks this output's rule, and no other, is the one reported
                        if (declare(s, n, width, absent, i).misaligned() != i) fail("misaligned pointer missed", s.name, n, width, absent, i);
                    }
                    if (plan.end != at) fail("end is not the last byte used", s.name, n, width, absent, -1);
                    if (!s.workspace) continue;
                    const size_t need = (size_t)n * width * 40 + 1, total = plan.end + OutputPlan::workspace_room(need);
                    for (uintptr_t residue = 0; residue < 256; ++residue) {
                        const uintptr_t base = (uintptr_t)0x7f0000001000ull + residue;
                        const size_t off = plan.workspace_offset(base);
                        if ((base + off) % 256) fail("workspace not 256-byte aligned", s.name, n, width, absent, (int)residue);
                        if (off < plan.end) fail("workspace overlaps the outputs", s.name, n, width, absent, (int)residue);
                        if (off + need > total) fail("workspace passes the allocation", s.name, n, width, absent, (int)residue);
                    }
                }
    }
    // what add() refuses: a required output that is NULL, and one output too many
    OutputPlan bad;
    bad.add("counts", nullptr, 16, false);
    if (bad.ok || bad.count != 0) fail("NULL required output accepted", "-", 0, 0, 0, 0);
    OutputPlan full;
    for (int i = 0; i <= OutputPlan::kMax; ++i) full.add("x", memory, 4);
    if (full.ok || full.count != OutputPlan::kMax) fail("too many outputs accepted", "-", 0, 0, 0, OutputPlan::kMax);
    std::printf("%lld plans checked, %d failures\n", checked, failures);
    return failures ? 1 : 0;
}
