// rr_beam.h — the candidate test of the packet top level (rr_trace.h beam_candidates) and the rule by which the items of a
// scene are cut into spatial groups for it (rr_scene_build.h build_item_groups).  Plain float arithmetic that compiles as host
// C++ too: tests/native/beam_groups_test.cpp runs the grouped search against the flat one on the CPU.
//
// Offers: BeamRay, beam_axis, beam_box_test, beam_item_passes, beam_group_passes, beam_ray_takes_groups; beam_grouped,
//         RR_BEAM_GROUP_SHIFT, beam_group_count, beam_group_records.
//
// Every float below must be compiled without contraction (-ffp-contract=off, as the library is).
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define RR_BEAM_HD __host__ __device__ inline
#else
#define RR_BEAM_HD inline
#endif

// An item's REPORTED toi can lie in front of its box by up to 1e-3 of the distance (rr_trace.h RR_TOI_SLACK has the story):
// a candidate's key is taken that much nearer than its box distance.
#define RR_BEAM_TOI_SLACK 1.001f

// The interval ray of a packet: component ranges of the origins and of |1 / d| over its 64 rays, and the direction signs they share.
struct BeamRay {
    bool negx, negy, negz;
    float oxl, oxh, oyl, oyh, ozl, ozh; // origins
    float axl, axh, ayl, ayh, azl, azh; // |1 / d|, already widened by the caller (0 <= lo <= hi, finite)
};

// one axis of the interval-ray slab test: lower bound of the entry distance and upper bound of the exit distance over
// all rays with origin in [olo, ohi] and |1/d| in [alo, ahi], direction sign `neg` (wave-uniform)
RR_BEAM_HD void beam_axis(bool neg, float blo, float bhi, float olo, float ohi, float alo, float ahi, float* tn, float* tf) {
    const float un = neg ? olo - bhi : blo - ohi; // smallest signed distance to the near plane
    const float wf = neg ? ohi - blo : bhi - olo; // largest signed distance to the far plane
    *tn = un * (un >= 0.0f ? alo : ahi);
    *tf = wf * (wf >= 0.0f ? ahi : alo);
}
// A box against the interval ray.  *key: a lower bound on any toi an item inside the box can report; *tf: an upper bound of the
// distance at which the last ray leaves the box.
RR_BEAM_HD void beam_box_test(const BeamRay& r, float lx, float ly, float lz, float hx, float hy, float hz, float* key, float* tf) {
    float tnx, tfx, tny, tfy, tnz, tfz;
    beam_axis(r.negx, lx, hx, r.oxl, r.oxh, r.axl, r.axh, &tnx, &tfx);
    beam_axis(r.negy, ly, hy, r.oyl, r.oyh, r.ayl, r.ayh, &tny, &tfy);
    beam_axis(r.negz, lz, hz, r.ozl, r.ozh, r.azl, r.azh, &tnz, &tfz);
    const float tn = fmaxf(fmaxf(tnx, tny), fmaxf(tnz, 0.0f));
    *tf = fminf(fminf(tfx, tfy), tfz);
    *key = tn * (1.0f / RR_BEAM_TOI_SLACK) * 0.99999f;
}
// an ITEM's box: a candidate when some ray can be inside it at or before `far`
RR_BEAM_HD bool beam_item_passes(float key, float tf, float far) { return key <= tf * 1.00001f && key <= far; }
// A GROUP's box: the same test in the negated form, so that a test that evaluates to NaN lets the group through (its members
// are then judged one by one).
RR_BEAM_HD bool beam_group_passes(float key, float tf, float far) { return !(key > tf * 1.00001f) && !(key > far); }

// ---- the groups ------------------------------------------------------------------------------------------------------------
// Scenes of 65 .. 512 items (above 64 one wave pass no longer covers the items; above 512 there is no packet form) carry their
// items a second time, sorted in space and cut into runs of 8: at most 64 groups, so that one wave pass covers them.  (A size
// that follows n_items -- 2, 4, 8 -- makes more and smaller groups in the smaller scenes, and costs the kernels registers for
// the shift and the mask, which they do not have.)  The last group may be short: its missing members are the sorted slots
// >= n_items, which nobody stores and nobody reads.
#define RR_BEAM_GROUP_SHIFT 3u // log2 of the group size
RR_BEAM_HD bool beam_grouped(uint32_t n_items) { return n_items > 64u && n_items <= 512u; }
RR_BEAM_HD uint32_t beam_group_count(uint32_t n_items) { return (n_items + (1u << RR_BEAM_GROUP_SHIFT) - 1u) >> RR_BEAM_GROUP_SHIFT; }
// The group records behind the 4 n float4 of the item boxes, in float4 units (g = beam_group_count(n)):
//   [4 n, 6 n)               the members' CORNER boxes in group order: (lo.xyz, bits(item index)), (hi.xyz, 0) per sorted slot
//   [6 n, 8 n)               the members' SURFACE boxes, same order and form
//   [8 n, 8 n + 2 g)         the groups' boxes over their members' corner boxes (lo, hi)
//   [8 n + 2 g, 8 n + 4 g)   the groups' boxes over their members' surface boxes
// so box set s (0 corner, 1 surface) has its items at 2 n s, its members at 4 n + 2 n s and its groups at 8 n + 2 g s.
RR_BEAM_HD uint32_t beam_group_records(uint32_t n_items) { return beam_grouped(n_items) ? 4u * n_items + 4u * beam_group_count(n_items) : 0u; }
// The groups are searched only by a packet whose lower reciprocal bounds are all positive.  Then no product of the test is
// inf * 0 and (origins being finite, group bounds never NaN) no group test is NaN; beam_candidates takes the flat pass otherwise.
RR_BEAM_HD bool beam_ray_takes_groups(const BeamRay& r) { return fminf(fminf(r.axl, r.ayl), r.azl) > 0.0f; }
