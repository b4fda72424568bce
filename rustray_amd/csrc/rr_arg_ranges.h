// rr_arg_ranges.h — do the buffers a caller handed to one call overlap where they must not?  Plain host logic, no HIP calls, nothing
// included: a call describes its buffer arguments as one table, arg_ranges_first_conflict finds the first forbidden pair, the caller
// (check_arg_ranges, rr_api_query.h) words the message; tests/native/arg_ranges_test.cpp checks it on the CPU against a byte-set model.
//
// THE rule.  Two ranges conflict when both pointers are non-NULL, their bytes intersect and at least one of them is an output: inputs
// may alias each other.  An output and its declared in-place partner do not conflict when the two pointers are exactly equal (the
// in-place call; shifted by anything, they do).  A range of zero bytes conflicts with nothing, and ranges that only touch (the end of
// one is the start of the other) do not conflict.  A range whose end lies beyond the address space conflicts with itself.
// The search order: first every range by itself, in table order; then the outputs in table order, each against the inputs in table
// order and then against the outputs after it.
#pragma once

struct ArgRange {
    const void* p;            // NULL: an optional argument the caller left out
    unsigned long long bytes;
    const char* name;         // for the caller's message
    bool is_output;
    int in_place_partner;     // of an output: the table index of the input it may be exactly equal to, or -1
};

// a, b: table indices -- a the output the search stood at, b what it overlaps (a == b: the range wraps); -1, -1: no conflict
struct ArgConflict { int a, b; };

// No sum of an address and a size is formed, so nothing overflows: a start lies inside the other range when its distance from that
// range's start is less than that range's size.
inline bool arg_ranges_intersect(const ArgRange& x, const ArgRange& y) {
    if (!x.p || !y.p || x.bytes == 0 || y.bytes == 0) return false;
    const unsigned long long xs = (unsigned long long)x.p, ys = (unsigned long long)y.p;
    return xs <= ys ? ys - xs < x.bytes : xs - ys < y.bytes;
}

inline ArgConflict arg_ranges_first_conflict(const ArgRange* t, int n) {
    for (int i = 0; i < n; i++) // (the last byte of a range has an address: start + bytes - 1 <= the largest one)
        if (t[i].p && t[i].bytes && t[i].bytes - 1 > ~0ull - (unsigned long long)t[i].p) return ArgConflict{i, i};
    for (int o = 0; o < n; o++) {
        if (!t[o].is_output) continue;
        for (int i = 0; i < n; i++)
            if (!t[i].is_output && arg_ranges_intersect(t[o], t[i]) && !(t[o].in_place_partner == i && t[o].p == t[i].p)) return ArgConflict{o, i};
        for (int o2 = o + 1; o2 < n; o2++)
            if (t[o2].is_output && arg_ranges_intersect(t[o], t[o2])) return ArgConflict{o, o2};
    }
    return ArgConflict{-1, -1};
}
