// output_plan.h -- where the outputs of one analysis call go (bgs_capi.hip, run_outputs).  Host code only, no HIP: the
// layout is a pure function of the declared outputs and tests/test_output_plan.py compiles it into a program of its own.
//
// An entry point declares its outputs in order with add().  When the caller's pointers are host memory the call works in
// ONE device allocation: every PRESENT output (pointer not NULL) gets a slice, in declaration order, each starting at a
// multiple of 16 bytes from the base; an absent optional output takes no room.  `end` is the byte behind the last slice.
// A search without a caller's workspace asks for workspace_room(need) further bytes, and its workspace begins at the
// first 256-byte boundary behind the outputs of the ACTUAL allocation (workspace_offset(base)), wherever the pool put it.
// When the caller's pointers are device memory nothing is laid out: misaligned() names the first output that breaks its
// alignment rule (NULL never does).
#pragma once

#include <stddef.h>
#include <stdint.h>

namespace bgs {

struct OutputPlan {
    static constexpr int kMax = 8;   // the most outputs a call has (bgs_bounce_search_moves_proving: 7)
    struct Output {
        const char* name;
        void* ptr;      // the caller's; NULL: absent
        size_t bytes;
        size_t align;   // required of a device pointer: 16, 8 or 4
        bool optional;  // may be NULL
        size_t offset;  // of the slice (present outputs only)
    };
    Output out[kMax] = {};
    int count = 0;
    size_t end = 0;
    bool ok = true;

    static constexpr size_t up(size_t x, size_t a) { return (x + a - 1) & ~(a - 1); }

    // (ok = false: a required output is NULL or there are more than kMax -- the entry points refuse their NULLs first)
    void add(const char* name, void* ptr, size_t bytes, bool optional = true, size_t align = 16) {
        if (count >= kMax || (!ptr && !optional)) {
            ok = false;
            return;
        }
        Output& o = out[count++];
        o = Output{name, ptr, bytes, align, optional, 0};
        if (ptr) {
            o.offset = up(end, 16);
            end = o.offset + bytes;
        }
    }

    // the first output whose (device) pointer breaks its alignment rule, -1 when none does
    int misaligned() const {
        for (int i = 0; i < count; ++i)
            if (reinterpret_cast<uintptr_t>(out[i].ptr) & (out[i].align - 1)) return i;
        return -1;
    }

    static constexpr size_t workspace_room(size_t need) { return need + 256; }
    // from the base of the allocation to the library's own workspace
    size_t workspace_offset(uintptr_t base) const { return up(base + end, 256) - base; }
};

}  // namespace bgs
