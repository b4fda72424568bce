// arg_ranges_test.cpp — rustray_amd/csrc/rr_arg_ranges.h on the CPU (tests/test_arg_ranges.py builds it with
// -fsanitize=address,undefined): arg_ranges_first_conflict against a brute-force model that marks every byte of a small address
// space -- every pair of ranges with start 0 .. 47 and length 0 .. 8, every input / output role, in-place partner on and off -- plus
// the cases the record calls (rr_denoise_records, rr_accumulate_records, rr_motion_records, rr_surface_pixels) rely on by name.
// The addresses are numbers, never dereferenced; 0 is NULL, so the model's address a is the pointer BASE + a.
#include "../../rustray_amd/csrc/rr_arg_ranges.h"

#include <cstdint>
#include <cstdio>

static int failures = 0;
#define CHECK(cond)                                                            \
    do {                                                                       \
        if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); failures++; } \
    } while (0)

static const uintptr_t BASE = 0x100000;
static const void* at(uintptr_t a) { return (const void*)a; }
static bool same(ArgConflict c, int a, int b) { return c.a == a && c.b == b; }

// the rule, stated independently: the bytes of both ranges marked in a set of 64 addresses
static bool expected_conflict(int s0, int l0, bool out0, int s1, int l1, bool out1, bool partner) {
    bool bytes0[64] = {}, shared = false;
    for (int k = 0; k < l0; k++) bytes0[s0 + k] = true;
    for (int k = 0; k < l1; k++) shared = shared || bytes0[s1 + k];
    if (!shared || (!out0 && !out1)) return false;
    return !(partner && out0 != out1 && s0 == s1);
}

int main() {
    // ---- every pair against the model.  Entry 0 comes first in the table; the partner, where declared, is the input of an output / input pair
    long n = 0, n_conflict = 0;
    for (int s0 = 0; s0 < 48; s0++)
        for (int l0 = 0; l0 <= 8; l0++)
            for (int s1 = 0; s1 < 48; s1++)
                for (int l1 = 0; l1 <= 8; l1++)
                    for (int roles = 0; roles < 4; roles++)
                        for (int partner = 0; partner < 2; partner++) {
                            const bool out0 = roles & 1, out1 = roles & 2;
                            const ArgRange t[2] = {{at(BASE + s0), (unsigned long long)l0, "a", out0, partner && out0 && !out1 ? 1 : -1},
                                                   {at(BASE + s1), (unsigned long long)l1, "b", out1, partner && out1 && !out0 ? 0 : -1}};
                            const ArgConflict c = arg_ranges_first_conflict(t, 2);
                            const bool want = expected_conflict(s0, l0, out0, s1, l1, out1, partner != 0);
                            // an output / input pair is reported from the output's side, a pair of outputs from the earlier one's
                            CHECK(want ? (out0 ? same(c, 0, 1) : same(c, 1, 0)) : same(c, -1, -1));
                            n++; n_conflict += want ? 1 : 0;
                        }
    CHECK(n == 48L * 9 * 48 * 9 * 4 * 2 && n_conflict > 0 && n_conflict < n);

    // ---- by name.  A frame of 4 records of 32 B: records (input), out (output, in place with records), variance (output)
    const unsigned long long R = 32;
    auto table = [&](uintptr_t records, uintptr_t out, uintptr_t variance) {
        const ArgRange t[3] = {{at(records), 4 * R, "records", false, -1}, {at(out), 4 * R, "out", true, 0}, {at(variance), 16, "variance_out", true, -1}};
        return arg_ranges_first_conflict(t, 3);
    };
    CHECK(same(table(BASE, BASE + 4 * R, BASE + 8 * R), -1, -1));          // touching ranges: the end of one is the start of the next
    CHECK(same(table(BASE, BASE + 4 * R - 1, BASE + 8 * R), 1, 0));        // a one-byte overlap
    CHECK(same(table(BASE + 4 * R - 1, BASE, BASE + 8 * R), 1, 0));        // ... from the other side
    CHECK(same(table(0, BASE, BASE), 1, 2));                               // NULL entries: left out, whatever their size says
    CHECK(same(table(BASE, BASE, 0), -1, -1));
    CHECK(same(table(0, BASE, 0), -1, -1));
    CHECK(same(table(BASE, BASE, BASE + 4 * R), -1, -1));                  // exact in-place equality is allowed
    CHECK(same(table(BASE, BASE + R, BASE + 8 * R), 1, 0));                // ... shifted by one 32-byte record it is not
    CHECK(same(table(BASE + R, BASE, BASE + 8 * R), 1, 0));
    CHECK(same(table(BASE, BASE + 8 * R, BASE), 2, 0));                    // the partner is out's alone: variance_out == records is refused
    {   // inputs may alias each other, an output may alias neither
        const ArgRange t[3] = {{at(BASE), 64, "history", false, -1}, {at(BASE + 8), 64, "motion", false, -1}, {at(BASE + 256), 64, "out", true, -1}};
        CHECK(same(arg_ranges_first_conflict(t, 3), -1, -1));
        const ArgRange u[3] = {t[0], t[1], {at(BASE + 71), 64, "out", true, -1}};
        CHECK(same(arg_ranges_first_conflict(u, 3), 2, 1));
    }
    {   // a zero-byte range conflicts with nothing, even inside another
        const ArgRange t[2] = {{at(BASE), 64, "records", false, -1}, {at(BASE + 8), 0, "out", true, -1}};
        CHECK(same(arg_ranges_first_conflict(t, 2), -1, -1));
    }
    {   // a range ending at the last addressable byte: start + bytes is 2^64, which no sum here forms
        const uintptr_t top = UINTPTR_MAX - 63; // 64 bytes: top .. UINTPTR_MAX
        const ArgRange alone[2] = {{at(top), 64, "records", false, -1}, {at(BASE), 64, "out", true, -1}};
        CHECK(same(arg_ranges_first_conflict(alone, 2), -1, -1));
        const ArgRange touching[2] = {{at(top), 64, "records", false, -1}, {at(top - 64), 64, "out", true, -1}};
        CHECK(same(arg_ranges_first_conflict(touching, 2), -1, -1));
        const ArgRange inside[2] = {{at(top), 64, "records", false, -1}, {at(UINTPTR_MAX), 1, "out", true, -1}};
        CHECK(same(arg_ranges_first_conflict(inside, 2), 1, 0));
        const ArgRange below[2] = {{at(top - 1), 2, "out", true, -1}, {at(top), 64, "records", false, -1}};
        CHECK(same(arg_ranges_first_conflict(below, 2), 0, 1));
        // a range that would wrap: one byte more is refused by itself, before any pair is looked at, input or output
        const ArgRange wraps[2] = {{at(BASE), 64, "out", true, -1}, {at(top), 65, "records", false, -1}};
        CHECK(same(arg_ranges_first_conflict(wraps, 2), 1, 1));
        const ArgRange far[2] = {{at(BASE), ~0ull, "out", true, -1}, {at(top), 64, "records", false, -1}};
        CHECK(same(arg_ranges_first_conflict(far, 2), 0, 0));
        const ArgRange whole[1] = {{at(1), ~0ull, "out", true, -1}}; // 1 .. UINTPTR_MAX: every address but NULL
        CHECK(same(arg_ranges_first_conflict(whole, 1), -1, -1));
    }
    {   // the search order on a table with two conflicts at once: outputs in table order, inputs before the later outputs
        const ArgRange t[4] = {{at(BASE), 64, "in0", false, -1}, {at(BASE + 512), 64, "out0", true, -1}, {at(BASE + 32), 64, "out1", true, -1},
                               {at(BASE + 540), 64, "in1", false, -1}};
        CHECK(same(arg_ranges_first_conflict(t, 4), 1, 3));                // out0 / in1 comes before out1 / in0: out0 is the earlier output
        const ArgRange u[4] = {{at(BASE), 64, "in0", false, -1}, {at(BASE + 16), 64, "out0", true, -1}, {at(BASE + 32), 64, "out1", true, -1},
                               {at(BASE + 40), 64, "in1", false, -1}};
        CHECK(same(arg_ranges_first_conflict(u, 4), 1, 0));                // out0 overlaps in0, in1 and out1: the inputs in table order first
        const ArgRange v[3] = {{at(BASE), 64, "out0", true, -1}, {at(BASE + 16), 64, "out1", true, -1}, {at(BASE + 60), 64, "in0", false, -1}};
        CHECK(same(arg_ranges_first_conflict(v, 3), 0, 2));                // ... an input after the outputs in the table still comes before them
    }
    CHECK(same(arg_ranges_first_conflict(nullptr, 0), -1, -1));
    if (failures) { std::printf("%d check(s) failed\n", failures); return 1; }
    std::printf("arg ranges test OK (%ld pairs, %ld conflicts)\n", n, n_conflict);
    return 0;
}
