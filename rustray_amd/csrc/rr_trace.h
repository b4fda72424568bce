// rr_trace.h — layer 3 of the device code: one ray, or one packet of 64, against the whole scene.  Stands for Raytracing::trace
// (reference src/raytracing.rs:429-490) with Scene::get_possible_hits_by_ray (src/scene.rs:1715-1722) as the top-level tree, for
// closest-hit rays and for shadow rays (first item hit in bbox-distance order, :483-486), including what the reference's
// arithmetic does with non-finite rays and NaN hits.
//
// Offers: Closest, reference_face_id, ray_nonfinite, trace_closest_ray, trace_closest_packet, trace_closest_nonfinite, trace_closest_ordered;
// ShadowSel, trace_shadow_ray, trace_shadow_packet (trace_shadow_nonfinite through trace_shadow_ray), shadow_deciding_hit.  The per-item functions
// (aabb_cast2, item_passes, closest_item*, shadow_item, shadow_blocker_item, trace_shadow_blockers) and the packet top level
// (the wave_min_* / wave_max_* reductions, beam_candidates, beam_next; the box test itself is rr_beam.h's, shared with the host) are this layer's own.
// No macro leaves this file: RR_TOI_SLACK and RR_SHADOW_BOUND are its own, and the node step of rr_walk.h, whose last user
// is here, is un-defined at the end with STK and RR_SENTINEL.  RR_UTIL / RR_UTIL_KIND stay for the kernels.
// Needs: rr_walk.h, rr_beam.h.
#pragma once
#include "rr_beam.h"
#include "rr_walk.h"

// An item's REPORTED toi can lie in front of its box.  ray_toi_with_ball takes the root of b^2 - a c, which cancels
// catastrophically when the origin is far from the sphere: the discriminant of a grazing ray is rounding noise of the order
// u b^2, and the reported toi is off by up to sqrt(u) ~ 2.4e-4 of the distance (a sphere 2e4 units away "hit" 7 units in
// front of its box, by a ray that misses it: tools/fuzz_rays.py far, seed 419).  Wherever the top level prunes by distance
// -- against the best hit, or against the light -- the bound is therefore taken 1e-3 wider than the box distance says
// (and kept finite: the unused child slots of a node are boxes at infinity, which only a finite bound rejects).
#define RR_TOI_SLACK RR_BEAM_TOI_SLACK

// ---------------------------------------------------------------------------
// Raytracing::trace (reference src/raytracing.rs:429-490) per item
// ---------------------------------------------------------------------------
// Aabb::cast_local_ray with the entry distance kept beside the returned toi: origin inside a
// non-solid box returns the EXIT distance as toi (the sort key) although hits may be nearer.
RR_DEV bool aabb_cast2(const float* mins, const float* maxs, const LRay& ray, bool solid, float* toi, float* tmin_out) {
    float tmin = 0.0f, tmax = RR_FLT_MAX;
    const float o[3] = {ray.o.x, ray.o.y, ray.o.z};
    const float d[3] = {ray.d.x, ray.d.y, ray.d.z};
#pragma unroll
    for (int i = 0; i < 3; i++) {
        if (d[i] == 0.0f) {
            if (o[i] < mins[i] || o[i] > maxs[i]) return false;
        } else {
            float denom = 1.0f / d[i];
            float a = (mins[i] - o[i]) * denom;
            float b = (maxs[i] - o[i]) * denom;
            float inear = (a > b) ? b : a;
            float ifar = (a > b) ? a : b;
            tmin = rs_max(tmin, inear);
            tmax = rs_min(tmax, ifar);
            if (tmin > tmax) return false;
        }
    }
    *toi = (tmin == 0.0f && !solid) ? tmax : tmin;
    *tmin_out = tmin;
    return true;
}

// candidate filter of :454 on the texture-less material cache
RR_DEV bool item_passes(uint32_t flags, bool for_shadow, uint32_t depth) {
    if (!(flags & RR_IF_VISIBLE)) return false;
    if (!(flags & RR_IF_CACHE_ALPHA_POS)) return false;
    if (for_shadow && !(flags & RR_IF_CACHE_CAST_SHADOW)) return false;
    if ((flags & RR_IF_CACHE_REFL_ONLY) && !(depth > 1u)) return false;
    return true;
}

struct Closest { float t; int item; uint32_t face; float key; bool found; bool nan_seen; }; // nan_seen: a ball answered Some(NaN) (trace_closest_ordered)

// The reference's face id of a raw closest hit on item `it` (`face`: Closest::face = leaf-order slot | negated << 30 | back << 31): the
// triangle record's original face index (DTriX::t0.w), plus n_tris for a back face; 0 for a ball.
RR_DEV uint32_t reference_face_id(const DItem* it, const DTriX* trix, uint32_t face) {
    if (it->flags & RR_IF_SPHERE) return 0u;
    return __float_as_uint(trix[(unsigned long long)it->tri_base + (face & 0x3fffffffu)].t0.w) + ((face >> 31) ? it->n_tris : 0u);
}

// The reference sorts candidates by bbox distance (stable) and keeps strictly
// smaller toi, so among equal toi the smaller (bbox distance, item index) wins.
// `it`: item idx -- its DItem, or its ItemRec where all lanes visit the same item (item_rec_uniform).
template <class Item> RR_DEV void closest_item(const DSceneView& sc, int idx, const Item& it, f3 o, f3 d, uint32_t depth,
                         int* s_stack, int sp_base, Closest* best) {
    RR_UTIL(1)
    uint32_t flags = it.flags;
    if (!item_passes(flags, false, depth)) return;
    LRay lr = inverse_ray(it, o, d, sc.general_w != 0u);
    bool solid = (flags & RR_IF_SOLID_BASE) != 0u;
    float key;
    if (!aabb_cast(it.bmin, it.bmax, lr, solid, &key)) return;
    if (key != key) return; // NaN distance: treated as a miss (the reference panics)
    float t; uint32_t face;
    if (flags & RR_IF_SPHERE) {
        bool inside;
        if (!ray_ball(it.radius, lr, solid, &t, &inside)) return;
        if (t != t) { best->nan_seen = true; return; } // Some(NaN): what it does to the result depends on the candidate ORDER (trace_closest_ordered)
        face = 0u;
    } else {
        if (it.n_tris == 0u) return;
        TriBest tb;
        blas_closest<true>(sc, it, lr, best->found ? best->t : RR_FLT_MAX, s_stack, sp_base, &tb);
        if (!tb.found) return;
        t = tb.t;
        face = tb.slot | (tb.side << 30); // bit31 back face, bit30 negated normal
    }
    bool better = !best->found || t < best->t ||
                  (t == best->t && (key < best->key || (key == best->key && idx < best->item)));
    if (better) { best->found = true; best->t = t; best->item = idx; best->face = face; best->key = key; }
}

// closest_item for a candidate that ALL lanes of a packet visit together (trace_closest_packet): a mesh is walked once per wave
// (blas_closest_packet), with the lanes whose exact box test passed taking part.  Same result as closest_item, lane by lane.
RR_DEV void closest_item_packet(const DSceneView& sc, int idx, f3 o, f3 d, uint32_t depth, int* s_stack, Closest* best) {
    const ItemRec it = item_rec_uniform(sc.items, idx, sc.general_w != 0u); // (wave-uniform: one item, fetched once for the wave)
    const uint32_t flags = it.flags;
    if (flags & RR_IF_SPHERE) { closest_item(sc, idx, it, o, d, depth, s_stack, 0, best); return; }
    RR_UTIL(1)
    bool in = item_passes(flags, false, depth) && it.n_tris != 0u;
    const LRay lr = inverse_ray(it, o, d, sc.general_w != 0u);
    float key = 0.0f;
    in = in && aabb_cast(it.bmin, it.bmax, lr, (flags & RR_IF_SOLID_BASE) != 0u, &key);
    in = in && key == key; // NaN distance: treated as a miss (the reference panics)
    if (__ballot(in) == 0ull) return;
    const float gbound = best->found ? best->t : RR_FLT_MAX;
    TriBest tb; tb.found = false; tb.t = RR_FLT_MAX; tb.slot = 0u; tb.face = 0xffffffffu; tb.side = 0u;
    if (!blas_closest_packet(sc, it, lr, in, gbound, s_stack, 0, &tb)) {
        if (in) blas_closest<true>(sc, it, lr, gbound, s_stack, 0, &tb);
    }
    if (in && tb.found) {
        const float t = tb.t;
        const uint32_t face = tb.slot | (tb.side << 30); // bit31 back face, bit30 negated normal
        const bool better = !best->found || t < best->t || (t == best->t && (key < best->key || (key == best->key && idx < best->item)));
        if (better) { best->found = true; best->t = t; best->item = idx; best->face = face; best->key = key; }
    }
}

RR_DEV void trace_closest_ray(const DSceneView& sc, f3 o, f3 d, uint32_t depth, int* s_stack, Closest* best) {
    best->found = false; best->nan_seen = false; best->t = RR_FLT_MAX; best->item = -1; best->face = 0u; best->key = 0.0f;
    // top level: world-space boxes over items (stands in for Scene::get_possible_hits_by_ray,
    // reference src/scene.rs:1715-1722; any conservative candidate set gives the same result)
    // the top level in the 4-wide form of the per-mesh trees, same step (sentinel-terminated stack)
    const Slab4 ws = make_slab4(make_slab(o, d), 0u);
    int sp = 1;
    STK(0) = RR_SENTINEL;
    int cur = sc.tlas_root4c; // (the closest-hit tree: surface boxes)
    // while-while: every lane walks the top level until it holds a candidate item (or is done), so the per-mesh
    // walks below run with the lanes of the wave together instead of one straggler at a time
    for (;;) {
        while (cur >= 0) { RR_NODE4_STEP(sc.tnodes4c, ws, fminf(best->t * RR_TOI_SLACK, RR_FLT_MAX)) }
        if (cur == RR_SENTINEL) break;
        const int idx = (int)RR_LEAF_FIRST((uint32_t)~cur); // one item per top-level leaf
        closest_item(sc, idx, rr_global(sc.items)[idx], o, d, depth, s_stack, sp, best);
        sp--; cur = STK(sp);
    }
}

// Rays with a non-finite component (a NaN normal, e.g. from a normal map on a sphere whose tangent degenerates, reflects
// into one).  The reference has no special case for them and its arithmetic decides: in item-local space such a ray
// is NaN in all components of its origin or direction, ray_toi_with_ball's comparisons are then all false and EVERY
// candidate sphere reports Some(NaN); a triangle's toi comes out NaN or infinite and fails `toi <= max_toi`.  The
// candidate loop (src/raytracing.rs:466-487) keeps the first such sphere in (bbox distance, item) order, since nothing
// compares smaller than NaN, and the hit shades with NaN position and normal (texel (0, 0), finite ambient term).
// The top-level walk has no defined order for these rays (NaN passes or fails a slab test by the instruction used), so they take this walk over the items
// instead: exact for spheres; meshes are skipped, which is what the reference's triangle test amounts to.
RR_DEV bool ray_nonfinite(f3 o, f3 d) {
    const float z = ((o.x - o.x) + (o.y - o.y) + (o.z - o.z)) + ((d.x - d.x) + (d.y - d.y) + (d.z - d.z)); // x - x: 0 for finite x, NaN otherwise
    return z != 0.0f;
}
RR_DEV void trace_closest_nonfinite(const DSceneView& sc, f3 o, f3 d, uint32_t depth, Closest* best) {
    best->found = false; best->nan_seen = false; best->t = RR_FLT_MAX; best->item = -1; best->face = 0u; best->key = 0.0f;
    Closest first = *best; // the first candidate in the reference's order that is hit at all
    for (int idx = 0; idx < (int)sc.n_items; idx++) {
        const DItem& it = rr_global(sc.items)[idx];
        const uint32_t flags = it.flags;
        if (!(flags & RR_IF_SPHERE) || !item_passes(flags, false, depth)) continue;
        LRay lr = inverse_ray(it, o, d, true); // (w is NaN for a non-finite origin: see to_local_point)
        float key, t; bool inside;
        if (!aabb_cast(it.bmin, it.bmax, lr, (flags & RR_IF_SOLID_BASE) != 0u, &key) || key != key) continue;
        if (!ray_ball(it.radius, lr, (flags & RR_IF_SOLID_BASE) != 0u, &t, &inside)) continue;
        if (!first.found || key < first.key || (key == first.key && idx < first.item)) { first.found = true; first.t = t; first.item = idx; first.key = key; }
        if (t == t && (!best->found || t < best->t || (t == best->t && (key < best->key || (key == best->key && idx < best->item))))) {
            best->found = true; best->t = t; best->item = idx; best->key = key;
        }
    }
    if (first.found && first.t != first.t) *best = first; // a NaN toi is never replaced (`toi < best` is false)
}

// A FINITE ray can get Some(NaN) from a ball too: where ray_toi_with_ball's products overflow (a ball of radius 1e12 under a
// transform that shrinks it to one unit: b * b = inf, a * c = inf, delta = NaN, every comparison false).  The reference's loop
// (src/raytracing.rs:466-487) walks the candidates in (bbox distance, item) order and replaces its best hit on `toi < best`: a NaN
// hit is THE result if it is the first candidate hit at all in that order (nothing compares smaller than NaN afterwards) and is
// ignored otherwise.  The walks above visit candidates in another order and keep a minimum, which is only order-free while every
// toi is a number; they leave a NaN hit out and flag the ray (Closest::nan_seen), and the flagged rays -- none in any scene whose
// balls have sane sizes -- take this pass over all items in the reference's own terms.
RR_DEV void trace_closest_ordered(const DSceneView& sc, f3 o, f3 d, uint32_t depth, int* s_stack, Closest* best) {
    Closest fin; fin.found = false; fin.nan_seen = false; fin.t = RR_FLT_MAX; fin.item = -1; fin.face = 0u; fin.key = 0.0f;
    Closest first = fin; // the first candidate in the reference's order that is hit at all
    for (int idx = 0; idx < (int)sc.n_items; idx++) {
        const DItem& it = rr_global(sc.items)[idx];
        const uint32_t flags = it.flags;
        if (!item_passes(flags, false, depth)) continue;
        const LRay lr = inverse_ray(it, o, d, sc.general_w != 0u);
        const bool solid = (flags & RR_IF_SOLID_BASE) != 0u;
        float key, t; uint32_t face = 0u;
        if (!aabb_cast(it.bmin, it.bmax, lr, solid, &key) || key != key) continue;
        if (flags & RR_IF_SPHERE) {
            bool inside;
            if (!ray_ball(it.radius, lr, solid, &t, &inside)) continue;
        } else {
            if (it.n_tris == 0u) continue;
            TriBest tb;
            blas_closest<true>(sc, it, lr, RR_FLT_MAX, s_stack, 0, &tb);
            if (!tb.found) continue;
            t = tb.t; face = tb.slot | (tb.side << 30);
        }
        if (!first.found || key < first.key || (key == first.key && idx < first.item)) { first.found = true; first.t = t; first.item = idx; first.face = face; first.key = key; }
        if (t == t && (!fin.found || t < fin.t || (t == fin.t && (key < fin.key || (key == fin.key && idx < fin.item))))) {
            fin.found = true; fin.t = t; fin.item = idx; fin.face = face; fin.key = key;
        }
    }
    *best = (first.found && first.t != first.t) ? first : fin;
}

// ---------------------------------------------------------------------------
// The top level for a coherent packet.  The top level is only a candidate filter: every item it lets through is
// tested exactly in its own space, and the winner is a minimum that does not depend on the order.  A packet whose 64
// rays share their direction signs (64 samples of one pixel do) therefore does not walk the top-level tree 64 times:
// the wave bounds its rays by an interval ray (component ranges of origin and reciprocal direction), tests the items'
// world boxes against it with one ITEM per lane (above 64 items: one group of 8 items per lane first), and all lanes then visit the few candidates together, nearest box
// first, until the next box starts behind every lane's best hit.  On the contract frame the per-ray walk spent a third
// of the kernel's vector instructions in the top level (7.8 node steps per ray over 194 items).
// All 64 lanes must be active.  Returns false (nothing touched) when the packet is not coherent, the scene has more
// items than a few passes cover, or more than 64 items survive: the caller walks the tree per ray instead.
// ---------------------------------------------------------------------------
// Exact wave reductions on INTEGERS: six DPP steps, each one instruction, leave the result in lane 63.  Within a row of 16:
// quad_perm [1,0,3,2] and [2,3,0,1], row_half_mirror, row_mirror (every lane reads a lane of the wave: bound_ctrl changes nothing and
// lets the compiler fold the move into the min / max); then row_bcast:15 carries a row's result into the next row (rows 1 and 3
// take it, the others keep theirs) and row_bcast:31 that of the first half into rows 2 and 3.  All 64 lanes must be active.
// (The float forms cost twice as much: fminf of a value that comes out of a lane move is preceded by an instruction that quiets
// a signalling NaN, and the move is not folded.)
#define RR_WAVE_REDUCE(T, OP, IDENTITY)                                                                            \
    v = OP(v, (T)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xf, 0xf, true));                /* quad_perm [1,0,3,2] */ \
    v = OP(v, (T)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E, 0xf, 0xf, true));                /* quad_perm [2,3,0,1] */ \
    v = OP(v, (T)__builtin_amdgcn_update_dpp(0, (int)v, 0x141, 0xf, 0xf, true));               /* row_half_mirror */     \
    v = OP(v, (T)__builtin_amdgcn_update_dpp(0, (int)v, 0x140, 0xf, 0xf, true));               /* row_mirror */          \
    v = OP(v, (T)__builtin_amdgcn_update_dpp((int)(IDENTITY), (int)v, 0x142, 0xa, 0xf, false)); /* row_bcast:15 */        \
    v = OP(v, (T)__builtin_amdgcn_update_dpp((int)(IDENTITY), (int)v, 0x143, 0xc, 0xf, false)); /* row_bcast:31 */        \
    return (T)__builtin_amdgcn_readlane((int)v, 63);
RR_DEV uint32_t wave_min_u32(uint32_t v) { RR_WAVE_REDUCE(uint32_t, min, 0xffffffffu) }
RR_DEV uint32_t wave_max_u32(uint32_t v) { RR_WAVE_REDUCE(uint32_t, max, 0u) }
RR_DEV int wave_min_i32(int v) { RR_WAVE_REDUCE(int, min, 0x7fffffff) }
RR_DEV int wave_max_i32(int v) { RR_WAVE_REDUCE(int, max, (int)0x80000000u) }
#undef RR_WAVE_REDUCE
// Floats through them.  The bits of a float that is not NaN, with the low 31 flipped when the sign is set, order as signed
// integers exactly as the floats do (-0 below +0, as v_min_f32 / v_max_f32 have it); the map is its own inverse, and the
// minimum and maximum of a set do not depend on the order of combination.  No lane may hold a NaN.
RR_DEV int float_order(int bits) { return bits ^ (int)((uint32_t)(bits >> 31) >> 1); }
RR_DEV float wave_min_f32(float v) { return __int_as_float(float_order(wave_min_i32(float_order(__float_as_int(v))))); }
RR_DEV float wave_max_f32(float v) { return __int_as_float(float_order(wave_max_i32(float_order(__float_as_int(v))))); }
// the same for floats >= +0, whose bits order as unsigned integers
RR_DEV float wave_min_pos_f32(float v) { return __uint_as_float(wave_min_u32(__float_as_uint(v))); }
RR_DEV float wave_max_pos_f32(float v) { return __uint_as_float(wave_max_u32(__float_as_uint(v))); }
// how many lanes below this one a ballot names (two instructions, and no lane mask to keep in registers)
RR_DEV uint32_t lanes_below(unsigned long long m) { return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u)); }
// The candidate list of a packet: lane l of the wave holds candidate l as (sort key, item); the key keeps the upper bits
// of the distance at which the item's box can first be entered by any ray of the packet (a lower bound) and the lane in
// its low six bits, 0xffffffff = none.  `far`: (wave-uniform) boxes that start beyond it are of no interest.
// `set`: 0 = the items' corner boxes (shadow packets, whose order and bounds are the LOCAL boxes' entry distances, which only a world box
// around the local box bounds from below), 1 = their surface boxes (closest-hit packets); rr_scene_build.h build_tlas, sc.item_boxes.
// (A shadow packet that also dropped the items whose surface box none of its rays reaches gained nothing: 6.00 -> 6.02 ms.)
//
// Above 64 items the search has two levels (rr_beam.h has the records, rr_scene_build.h build_item_groups makes them): one GROUP box per
// lane first, then the members of the surviving groups, one per lane, each against its OWN box.  Why no ray's result can change:
// (a) The candidate set is the same set.  A group box contains its members' boxes bound by bound, and every step of the test is
//     monotone in the box bounds: un and wf (a float difference), their products with a non-negative factor chosen by their
//     sign, fmaxf / fminf, the constant factors.  So a group's key is at most each member's and its tf at least each member's: a
//     rejected group has only rejected members.  What would break the chain is a NaN on one side only: a member bound that is
//     not finite opens that side of the group box (build_item_groups), and the groups are searched only while every lower
//     reciprocal bound is positive (beam_ray_takes_groups; else inf * 0 could make a member's axis NaN, which fminf / fmaxf drop,
//     while the group's stays a number), the flat pass otherwise.  A group test that is NaN all the same passes (beam_group_passes).
// (b) The list ORDER changes -- among equal truncated keys it followed the item index and now follows the group order -- and
//     nothing depends on it: the closest-hit winner is a minimum over (t, key, idx) (closest_item_packet), the shadow
//     selection a minimum over (key, idx) (shadow_item), and the `break` conditions of the two packet loops read the key only.
// A member's key is that of the flat pass bit for bit: the same test on the same box.
RR_DEV float4 box_row(const float4* boxes, uint32_t byte_off) { return *(const float4*)((const char*)boxes + byte_off); }
RR_DEV bool beam_candidates(const DSceneView& sc, uint32_t set, f3 o, f3 d, float far, int* s_stack, uint32_t* sk_out, int* item_out, uint32_t min_items = RR_BEAM_MIN_ITEMS) {
    const uint32_t n_items = sc.n_items;
    if (n_items > RR_BEAM_MAX_ITEMS || n_items < min_items) return false;
    // coherent: finite rays, no zero direction component, one sign per axis
    const bool bad = ray_nonfinite(o, d) || !(fabsf(d.x) > 1e-30f) || !(fabsf(d.y) > 1e-30f) || !(fabsf(d.z) > 1e-30f);
    const unsigned long long nx_ = __ballot(d.x < 0.0f), ny_ = __ballot(d.y < 0.0f), nz_ = __ballot(d.z < 0.0f);
    if (__ballot(bad) != 0ull || (nx_ != 0ull && ~nx_ != 0ull) || (ny_ != 0ull && ~ny_ != 0ull) || (nz_ != 0ull && ~nz_ != 0ull)) return false;
    const float ax = fabsf(__builtin_amdgcn_rcpf(d.x)), ay = fabsf(__builtin_amdgcn_rcpf(d.y)), az = fabsf(__builtin_amdgcn_rcpf(d.z));
    BeamRay br;
    br.negx = nx_ != 0ull; br.negy = ny_ != 0ull; br.negz = nz_ != 0ull;
    br.oxl = wave_min_f32(o.x); br.oxh = wave_max_f32(o.x); br.oyl = wave_min_f32(o.y); br.oyh = wave_max_f32(o.y); br.ozl = wave_min_f32(o.z); br.ozh = wave_max_f32(o.z);
    br.axl = wave_min_pos_f32(ax) * 0.99999f; br.axh = wave_max_pos_f32(ax) * 1.00001f;
    br.ayl = wave_min_pos_f32(ay) * 0.99999f; br.ayh = wave_max_pos_f32(ay) * 1.00001f;
    br.azl = wave_min_pos_f32(az) * 0.99999f; br.azh = wave_max_pos_f32(az) * 1.00001f;
    const uint32_t lane = threadIdx.x & (RR_WAVE - 1), wave_col = threadIdx.x & ~(RR_WAVE - 1u);
    // The boxes against the interval ray, one per lane; survivors appended to a list in the wave's own columns of two stack rows
    // (nothing is on the stack yet).  Up to 64 items the slots of a pass are the items themselves.  Above, the first pass has the
    // groups for its slots and leaves the survivors, in order, in a third stack row; the slots of the passes after it are their
    // members: slot s is member s & 7 of survivor s >> 3.  One loop, so that there is one copy of the test.
    // (Everything is addressed from sc.item_boxes by a 32-bit offset that changes inside the loop: a pointer per record kind, or a
    // lane's address of its group, does not change from packet to packet and would be kept in registers across the whole walk.)
    const float4* __restrict__ boxes = sc.item_boxes;
    const bool grouped = n_items > RR_WAVE && beam_ray_takes_groups(br); // (wave-uniform)
    bool groups_now = grouped;
    uint32_t n_slots = grouped ? beam_group_count(n_items) : n_items;
    uint32_t first = grouped ? 8u * n_items + 2u * n_slots * set : 2u * n_items * set;
    uint32_t total = 0, base = 0;
    while (base < n_slots) {
        uint32_t slot = base + lane, j = slot;
        bool in = slot < n_slots;
        if (grouped && !groups_now) { // (the last group may be short: its missing members are no candidates)
            slot = in ? ((uint32_t)s_stack[3 * RR_BLOCK + wave_col + (slot >> RR_BEAM_GROUP_SHIFT)] << RR_BEAM_GROUP_SHIFT) + (slot & ((1u << RR_BEAM_GROUP_SHIFT) - 1u)) : n_items;
            in = slot < n_items;
        }
        bool cand = false, through = false; float key = 0.0f;
        if (in) {
            const uint32_t at = (first + 2u * slot) << 4;
            const float4 lo = box_row(boxes, at), hi = box_row(boxes, at + 16u);
            float tf;
            beam_box_test(br, lo.x, lo.y, lo.z, hi.x, hi.y, hi.z, &key, &tf); // key: a lower bound on any toi the item can report
            cand = beam_item_passes(key, tf, far);
            through = beam_group_passes(key, tf, far);
            if (grouped) j = __float_as_uint(lo.w);
        }
        if (groups_now) {
            const unsigned long long gm = __ballot(through);
            if (through) s_stack[3 * RR_BLOCK + wave_col + lanes_below(gm)] = (int)slot;
            __builtin_amdgcn_wave_barrier();
            groups_now = false;
            n_slots = (uint32_t)__popcll(gm) << RR_BEAM_GROUP_SHIFT;
            first = 4u * n_items + 2u * n_items * set;
            continue; // (base stays 0: there are at most 64 groups)
        }
        const unsigned long long m = __ballot(cand);
        const uint32_t pos = total + lanes_below(m);
        total += (uint32_t)__popcll(m);
        if (total > RR_WAVE) return false; // (wave-uniform) more candidates than lanes: not a packet worth treating as one
        if (cand) { s_stack[1 * RR_BLOCK + wave_col + pos] = __float_as_int(key); s_stack[2 * RR_BLOCK + wave_col + pos] = (int)j; }
        base += RR_WAVE;
    }
    __builtin_amdgcn_wave_barrier();
    uint32_t sk = 0xffffffffu; int item = 0;
    if (lane < total) { sk = ((uint32_t)s_stack[1 * RR_BLOCK + wave_col + lane] & ~63u) | lane; item = s_stack[2 * RR_BLOCK + wave_col + lane]; }
    __builtin_amdgcn_wave_barrier();
    *sk_out = sk; *item_out = item;
    return true;
}
// next candidate in box-distance order: (wave-uniform) false when none is left; *key = the lower bound of its box distance
RR_DEV bool beam_next(uint32_t& sk, int item, float* key, int* idx) {
    const uint32_t m = wave_min_u32(sk);
    if (m == 0xffffffffu) return false;
    const uint32_t src = m & 63u;
    *key = __uint_as_float(m & ~63u);
    *idx = __builtin_amdgcn_readlane(item, src);
    if ((threadIdx.x & (RR_WAVE - 1)) == src) sk = 0xffffffffu;
    return true;
}
RR_DEV bool trace_closest_packet(const DSceneView& sc, f3 o, f3 d, uint32_t depth, int* s_stack, Closest* best) {
    uint32_t sk; int item;
    if (!beam_candidates(sc, 1u, o, d, RR_FLT_MAX, s_stack, &sk, &item, RR_BEAM_MIN_ITEMS_CLOSEST)) return false;
    best->found = false; best->nan_seen = false; best->t = RR_FLT_MAX; best->item = -1; best->face = 0u; best->key = 0.0f;
    float key; int idx;
    while (beam_next(sk, item, &key, &idx)) {
        // the remaining boxes all start at or behind this one: done when that is behind every lane's best hit
        if (__ballot(!best->found || key <= best->t) == 0ull) break;
        closest_item_packet(sc, idx, o, d, depth, s_stack, best);
    }
    return true;
}

// Shadow rays stop at the first ITEM (in bbox-distance order) that is hit at all
// (reference src/raytracing.rs:483-486), not at the nearest hit.
struct ShadowSel { float key; int item; bool found; bool within; float t; uint32_t face; };

// `it`: item idx, as for closest_item.
template <class Item> RR_DEV void shadow_item(const DSceneView& sc, int idx, const Item& it, f3 o, f3 d, uint32_t depth, float limit,
                        int* s_stack, int sp_base, ShadowSel* sel) {
    RR_UTIL(1)
    uint32_t flags = it.flags;
    if (!item_passes(flags, true, depth)) return;
    LRay lr = inverse_ray(it, o, d, sc.general_w != 0u);
    float key, tmin;
    if (!aabb_cast2(it.bmin, it.bmax, lr, false, &key, &tmin)) return; // for_shadow forces solid = false
    if (key != key) return;
    // An item whose box starts beyond the light can never be hit within the light distance; it is skipped in this
    // pass.  It can still matter as a BLOCKER (hit, ordered before the occluder found here): trace_shadow_ray
    // runs a second pass for exactly that case.
    if (tmin > limit * RR_TOI_SLACK) return;
    if (sel->found && !(key < sel->key || (key == sel->key && idx < sel->item))) return;
    bool any = false, within = false; float t = 0.0f; uint32_t face = 0u;
    if (flags & RR_IF_SPHERE) {
        bool inside;
        if (ray_ball(it.radius, lr, false, &t, &inside)) { any = true; within = !(t > limit); } // (`in_light = toi > len`, :890: false for a NaN toi)
    } else if (it.n_tris != 0u) {
        if (flags & RR_IF_OCCLUDER_ALPHA_TEX) { // the occluder's alpha map needs the true nearest hit
            TriBest tb;
            blas_closest<false>(sc, it, lr, RR_FLT_MAX, s_stack, sp_base, &tb);
            if (tb.found) { any = true; t = tb.t; within = t <= limit; face = tb.face + ((tb.side & 2u) ? it.n_tris : 0u); }
        } else {
            blas_any(sc, it, lr, limit, s_stack, sp_base, &any, &within);
        }
    }
    if (any) { sel->found = true; sel->key = key; sel->item = idx; sel->within = within; sel->t = t; sel->face = face; }
}

// What a shadow QUERY reports beyond the decision (k_query_shadow): the deciding item's nearest hit, as the reference's
// Shape::intersect returns it for the item its loop stopped at.  shadow_item knows it for balls and for alpha-mapped occluders;
// any other mesh was walked for ANY hit (blas_any), so that one item is walked once more for its nearest one: toi, and the
// reference's face id as shadow_item forms it.  For an occluded ray only (sel->found && sel->within); a NaN ball (a blocker of
// trace_shadow_blockers, a non-finite ray) is a ball and keeps t = NaN, face = 0.
RR_DEV void shadow_deciding_hit(const DSceneView& sc, f3 o, f3 d, int* s_stack, ShadowSel* sel) {
    const DItem& it = rr_global(sc.items)[sel->item];
    const uint32_t flags = it.flags;
    if ((flags & (RR_IF_SPHERE | RR_IF_OCCLUDER_ALPHA_TEX)) != 0u || it.n_tris == 0u) return;
    const LRay lr = inverse_ray(it, o, d, sc.general_w != 0u);
    TriBest tb;
    blas_closest<false>(sc, it, lr, RR_FLT_MAX, s_stack, 0, &tb);
    if (tb.found) { sel->t = tb.t; sel->face = tb.face + ((tb.side & 2u) ? it.n_tris : 0u); }
}

// Second pass of a shadow query: is there an item whose box starts BEYOND the light (skipped above), ordered before
// the selected occluder (sel), that is hit at all?  The reference tries candidates in bbox-distance order and the
// first one that is hit decides (src/raytracing.rs:466-487); its hit lies beyond the light, so the receiver is lit --
// unless it is a ball whose arithmetic overflowed into Some(NaN): `in_light = toi > len` is false for that, the receiver is
// in ITS shadow (trace_closest_ordered has the story).  Returns 0: no blocker, 1: a hit beyond the light, 2: a NaN hit.
RR_DEV int shadow_blocker_item(const DSceneView& sc, int idx, f3 o, f3 d, uint32_t depth, float limit, const ShadowSel& sel,
                               int* s_stack, int sp_base, float* key_out) {
    const DItem& it = rr_global(sc.items)[idx];
    const uint32_t flags = it.flags;
    if (!item_passes(flags, true, depth)) return 0;
    LRay lr = inverse_ray(it, o, d, sc.general_w != 0u);
    float key, tmin;
    if (!aabb_cast2(it.bmin, it.bmax, lr, false, &key, &tmin)) return 0;
    if (key != key || !(tmin > limit * RR_TOI_SLACK)) return 0;
    if (!(key < sel.key || (key == sel.key && idx < sel.item))) return 0;
    *key_out = key;
    if (flags & RR_IF_SPHERE) { float t; bool inside; return ray_ball(it.radius, lr, false, &t, &inside) ? (t != t ? 2 : 1) : 0; }
    if (it.n_tris == 0u) return 0;
    bool any = false, within = false;
    blas_any(sc, it, lr, RR_FLT_MAX, s_stack, sp_base, &any, &within);
    return any ? 1 : 0;
}

// Updates *sel to the outcome: lit (within = false) if the first blocker in the reference's order has a hit beyond the light, in the
// shadow of that blocker if its toi is NaN, untouched without a blocker.  A scene without balls that can overflow (RR_VIEW_NAN_BALLS,
// the usual case) is done at the first blocker found: they all say "lit".
RR_DEV void trace_shadow_blockers(const DSceneView& sc, f3 o, f3 d, uint32_t depth, float limit, ShadowSel* sel, int* s_stack) {
    const float bound = sel->key * 1.00001f + 1e-6f; // a blocker's box starts before the occluder's key
    const bool nan_balls = (sc.compat & RR_VIEW_NAN_BALLS) != 0u;
    ShadowSel first = *sel; // the first blocker in (key, item) order so far; starts as the occluder it must precede
    int first_kind = 0;
    const Slab4 ws = make_slab4(make_slab(o, d), 0u);
    int sp = 1;
    STK(0) = RR_SENTINEL;
    int cur = sc.tlas_root4;
    for (;;) {
        while (cur >= 0) { RR_NODE4_STEP_PLAIN(sc.tnodes4, ws, bound) }
        if (cur == RR_SENTINEL) break;
        const int idx = (int)RR_LEAF_FIRST((uint32_t)~cur);
        float key = 0.0f;
        const int kind = shadow_blocker_item(sc, idx, o, d, depth, limit, first, s_stack, sp, &key);
        if (kind != 0) {
            first.key = key; first.item = idx; first_kind = kind;
            if (!nan_balls) break;
        }
        sp--; cur = STK(sp);
    }
    if (first_kind == 1) sel->within = false;
    else if (first_kind == 2) { sel->key = first.key; sel->item = first.item; sel->within = true; sel->t = __uint_as_float(0x7fc00000u); sel->face = 0u; }
}

// A non-finite shadow ray (a NaN normal puts the origin at NaN) in the reference: every candidate sphere reports Some(NaN)
// (see trace_closest_nonfinite), triangles report nothing, the first sphere in (bbox distance, item) order is THE
// intersection, and `in_light = toi > len` is false for a NaN toi -- the receiver is in shadow, for every kind of light
// (src/raytracing.rs:884-892).  Its alpha map, if it has one, is then sampled at a NaN uv (a NaN texel under the
// bilinear filter: the sample turns the pixel white).  Found by tools/fuzz_parity.py rich, seed 6601.
RR_DEV void trace_shadow_nonfinite(const DSceneView& sc, f3 o, f3 d, uint32_t depth, float limit, ShadowSel* sel) {
    sel->found = false; sel->within = false; sel->key = 0.0f; sel->item = -1; sel->t = 0.0f; sel->face = 0u;
    for (int idx = 0; idx < (int)sc.n_items; idx++) {
        const DItem& it = sc.items[idx];
        const uint32_t flags = it.flags;
        if (!(flags & RR_IF_SPHERE) || !item_passes(flags, true, depth)) continue;
        LRay lr = inverse_ray(it, o, d, true); // (w is NaN for a non-finite origin: see to_local_point)
        float key, tmin, t; bool inside;
        if (!aabb_cast2(it.bmin, it.bmax, lr, false, &key, &tmin) || key != key) continue; // for_shadow forces solid = false
        if (!ray_ball(it.radius, lr, false, &t, &inside)) continue;
        if (!sel->found || key < sel->key || (key == sel->key && idx < sel->item)) {
            sel->found = true; sel->key = key; sel->item = idx; sel->t = t; sel->within = !(t > limit);
        }
    }
}

RR_DEV void trace_shadow_ray(const DSceneView& sc, f3 o, f3 d, uint32_t depth, float limit, int* s_stack, ShadowSel* sel) {
    if (ray_nonfinite(o, d)) { trace_shadow_nonfinite(sc, o, d, depth, limit, sel); return; }
    sel->found = false; sel->within = false; sel->key = 0.0f; sel->item = -1; sel->t = 0.0f; sel->face = 0u;
    // an item whose world box starts beyond the light, or beyond the selected item's key, cannot matter
#define RR_SHADOW_BOUND fminf(sel->found ? fminf(limit * RR_TOI_SLACK, sel->key * 1.00001f + 1e-6f) : limit * RR_TOI_SLACK, RR_FLT_MAX)
    const Slab4 ws = make_slab4(make_slab(o, d), 0u);
    int sp = 1;
    STK(0) = RR_SENTINEL;
    int cur = sc.tlas_root4;
    for (;;) {
        while (cur >= 0) { RR_NODE4_STEP_PLAIN(sc.tnodes4, ws, RR_SHADOW_BOUND) }
        if (cur == RR_SENTINEL) break;
        const int idx = (int)RR_LEAF_FIRST((uint32_t)~cur);
        shadow_item(sc, idx, rr_global(sc.items)[idx], o, d, depth, limit, s_stack, sp, sel);
        sp--; cur = STK(sp);
    }
    // The occluder found has a hit within the light distance.  Only if its sort key lies beyond the light (its box
    // contains the ray origin, so the key is the box EXIT distance) can an item that starts beyond the light precede it.
    if (sel->found && sel->within && sel->key > limit) trace_shadow_blockers(sc, o, d, depth, limit, sel, s_stack);
}

// The packet form of trace_shadow_ray's first pass (see trace_closest_packet): candidates in box-distance order, until the
// next box starts beyond every lane's bound (the light, or the key of the occluder selected so far).
RR_DEV bool trace_shadow_packet(const DSceneView& sc, f3 o, f3 d, uint32_t depth, float limit, int* s_stack, ShadowSel* sel) {
    uint32_t sk; int item;
    if (!beam_candidates(sc, 0u, o, d, wave_max_f32(limit == limit ? limit : 0.0f), s_stack, &sk, &item)) return false;
    sel->found = false; sel->within = false; sel->key = 0.0f; sel->item = -1; sel->t = 0.0f; sel->face = 0u;
    float key; int idx;
    while (beam_next(sk, item, &key, &idx)) {
        if (__ballot(key <= RR_SHADOW_BOUND) == 0ull) break; // (a NaN light distance compares false: that lane wants nothing, as in the per-ray walk)
        // (wave-uniform: one item, its record fetched once for the wave; every lane walks it by itself)
        shadow_item(sc, idx, item_rec_uniform(sc.items, idx, sc.general_w != 0u), o, d, depth, limit, s_stack, 0, sel);
    }
    if (sel->found && sel->within && sel->key > limit) trace_shadow_blockers(sc, o, d, depth, limit, sel, s_stack);
    return true;
}

#undef RR_TOI_SLACK
#undef RR_SHADOW_BOUND
// the node step of rr_walk.h: the top-level walks above were its last user
#undef RR_NODE4_STEP
#undef RR_NODE4_STEP_PLAIN
#undef RR_NODE4_STEP_ANY
#undef RR_NODE4_FORM
#undef RR_NODE4_ROWS_VECTOR
#undef RR_NODE4_ROWS_UNIFORM
#undef RR_NODE4_TESTS
#undef RR_NODE4_SINGLE_HIT
#undef RR_NODE4_DESCEND_SORTED
#undef RR_NODE4_DESCEND_SORTED_PLAIN
#undef RR_NODE4_DESCEND_ANY
#undef RR_ROW
#undef RR_CHILD
#undef RR_CSWAP
#undef RR_UTIL_UNI
#undef RR_UTIL_ONE
#undef RR_UTIL_NODE_SLOT
#undef STK
#undef RR_SENTINEL
