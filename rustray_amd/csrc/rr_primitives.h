// rr_primitives.h — layer 1 of the device code: the exact primitive tests, one ray against one box, triangle or ball in
// item-local space.  parry3d 0.13 restated (ray_aabb.rs, ray_triangle.rs, ray_ball.rs) with the reference's transforms around
// them (ShapeBasics::get_inverse_ray, src/shape/mod.rs:755-761).  These decide every hit; all layers above only choose
// which of them to run.
//
// Offers: LRay, ItemRec, item_rec_uniform, inverse_ray, to_local_point, to_world_normal, aabb_cast, ray_triangle, ray_ball.  No macros.
// Needs: rr_device.h (DItem), rr_math.h.
#pragma once
#include "rr_device.h"
#include "rr_math.h"

// ---------------------------------------------------------------------------
// geometry primitives: parry3d 0.13 restated (ray_aabb.rs, ray_triangle.rs, ray_ball.rs)
// ---------------------------------------------------------------------------
struct LRay { f3 o, d; };

// What a walk needs from an item, in registers (the way MatR is for materials, rr_surface.h): the inverse rows, the local box
// with the radius and the flags in its w lanes, and the 16-byte group that names the mesh's tree.  Fields read through a
// `const DItem&` are fetched where they are used, behind the early exits of the box test: one dependent round trip per group,
// eight or nine per candidate.  The field names are DItem's, so the tests below take either: the per-ray walks, whose item
// differs from lane to lane, keep reading DItem where they use it (the same groups loaded together per lane cost the deeper
// levels' kernels scratch and did not pay on the contract frame: profiles/r13_dropped.txt).
struct ItemRec {
    float4 inv0, inv1, inv2, inv3; // (inv3 is loaded under general_w only, and read under it only)
    float bmin[3]; float radius;
    float bmax[3]; uint32_t flags;
    uint32_t tri_base, n_tris, node_base4; int32_t root4;
};
static_assert(offsetof(DItem, inv0) == 0 && offsetof(DItem, inv1) == 16 && offsetof(DItem, inv2) == 32 && offsetof(DItem, inv3) == 48, "ItemRec: inverse rows");
static_assert(offsetof(DItem, bmin) == 112 && offsetof(DItem, radius) == 124 && offsetof(DItem, bmax) == 128 && offsetof(DItem, flags) == 140, "ItemRec: box rows");
static_assert(offsetof(DItem, tri_base) == 160 && offsetof(DItem, n_tris) == 164 && offsetof(DItem, node_base4) == 168 && offsetof(DItem, root4) == 172, "ItemRec: tree group");
static_assert(sizeof(DItem) == 176, "ItemRec: record size (every group is 16-byte aligned)");
typedef float rr_f4v __attribute__((ext_vector_type(4)));
// The record of a WAVE-UNIFORM item (every lane of a packet visits the same candidate): through the constant address space,
// like the node rows of a uniform step (rr_walk.h node_row_uniform) -- the groups are issued together and waited for once,
// and arrive in scalar registers.  The items array is written by no trace kernel; edits happen between launches.
// (The empty asm statement reads the groups where they are loaded.  Without it the compiler sinks each load to its first use,
// behind the branches of the box test, where every group is a round trip of its own again: three waits in the shadow kernel.)
RR_DEV ItemRec item_rec_uniform(const DItem* items, int idx, bool general_w) {
    const __attribute__((address_space(4))) char* p = (const __attribute__((address_space(4))) char*)(uintptr_t)items
                                                      + (unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane(idx) * sizeof(DItem);
#define RR_ITEM_ROW(off) (*(const __attribute__((address_space(4))) rr_f4v*)(p + (off)))
    const rr_f4v i0 = RR_ITEM_ROW(0), i1 = RR_ITEM_ROW(16), i2 = RR_ITEM_ROW(32), lo = RR_ITEM_ROW(112), hi = RR_ITEM_ROW(128), g = RR_ITEM_ROW(160);
    rr_f4v i3 = {0.0f, 0.0f, 0.0f, 1.0f};
    if (general_w) i3 = RR_ITEM_ROW(48);
#undef RR_ITEM_ROW
    asm volatile("" :: "s"(i0), "s"(i1), "s"(i2), "s"(lo), "s"(hi), "s"(g));
    ItemRec r;
    r.inv0 = make_float4(i0.x, i0.y, i0.z, i0.w); r.inv1 = make_float4(i1.x, i1.y, i1.z, i1.w); r.inv2 = make_float4(i2.x, i2.y, i2.z, i2.w);
    r.inv3 = make_float4(i3.x, i3.y, i3.z, i3.w);
    r.bmin[0] = lo.x; r.bmin[1] = lo.y; r.bmin[2] = lo.z; r.radius = lo.w;
    r.bmax[0] = hi.x; r.bmax[1] = hi.y; r.bmax[2] = hi.z; r.flags = __float_as_uint(hi.w);
    r.tri_base = __float_as_uint(g.x); r.n_tris = __float_as_uint(g.y); r.node_base4 = __float_as_uint(g.z); r.root4 = __float_as_int(g.w);
    return r;
}

// ShapeBasics::get_inverse_ray, reference src/shape/mod.rs:755-761.  Item: DItem or ItemRec.
template <class Item> RR_DEV LRay inverse_ray(const Item& it, f3 o, f3 d, bool general_w) {
    LRay r;
    float ox = row4(it.inv0, o.x, o.y, o.z, 1.0f);
    float oy = row4(it.inv1, o.x, o.y, o.z, 1.0f);
    float oz = row4(it.inv2, o.x, o.y, o.z, 1.0f);
    if (general_w) { // Point3::from_homogeneous divides by w; w == 1 exactly for affine inverses
        float w = row4(it.inv3, o.x, o.y, o.z, 1.0f);
        ox = ox / w; oy = oy / w; oz = oz / w;
    }
    r.o = mk3(ox, oy, oz);
    r.d = mk3(row4(it.inv0, d.x, d.y, d.z, 0.0f), row4(it.inv1, d.x, d.y, d.z, 0.0f), row4(it.inv2, d.x, d.y, d.z, 0.0f));
    return r;
}
// (the w of an affine inverse is ((0 x + 0 y) + 0 z) + 1: exactly 1 for a finite point, NaN for any other -- 0 times an
// infinity -- so a non-finite point always takes the dividing form, and comes out NaN in every component as in the reference)
RR_DEV f3 to_local_point(const DItem& it, f3 p, bool general_w) {
    float x = row4(it.inv0, p.x, p.y, p.z, 1.0f);
    float y = row4(it.inv1, p.x, p.y, p.z, 1.0f);
    float z = row4(it.inv2, p.x, p.y, p.z, 1.0f);
    if (general_w || ((p.x - p.x) + (p.y - p.y)) + (p.z - p.z) != 0.0f) { float w = row4(it.inv3, p.x, p.y, p.z, 1.0f); x = x / w; y = y / w; z = z / w; }
    return mk3(x, y, z);
}
RR_DEV f3 to_world_normal(const DItem& it, f3 n) {
    return normalize3(mk3(row4(it.tr0, n.x, n.y, n.z, 0.0f), row4(it.tr1, n.x, n.y, n.z, 0.0f), row4(it.tr2, n.x, n.y, n.z, 0.0f)));
}

// Aabb::cast_local_ray(ray, f32::MAX, solid)
RR_DEV bool aabb_cast(const float* mins, const float* maxs, const LRay& ray, bool solid, float* toi) {
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
    return true;
}

// local_ray_intersection_with_triangle: toi and side only (the normal is rebuilt when shading).
// `back` is parry's FeatureId side (d >= 0); `neg` says the returned normal is -normalize(n) (t < 0).
// They differ only when the origin lies exactly in the triangle's plane.
// Written with a single exit: every arithmetic result is the same IEEE value as in parry's two branches
// (v = -ac.e | ac.e, w = ab.e | -ab.e, toi = -t/d | t/d; negation is exact), rejections keep parry's
// comparison forms so NaNs fall through exactly as they do there; the division runs for accepted hits only.
RR_DEV bool ray_triangle(f3 a, f3 ab, f3 ac, const LRay& ray, float* toi_out, uint32_t* side_out) {
    // ab = b - a, ac = c - a: computed once per triangle on the host (DTriX), with the IEEE sequence parry uses per ray
    const f3 n = cross3(ab, ac);
    const float d = dot3(n, ray.d);
    const f3 ap = ray.o - a;
    const float t = dot3(ap, n);
    const bool rej0 = (d == 0.0f) || (t < 0.0f && d < 0.0f) || (t > 0.0f && d > 0.0f);
    const bool back = !(d < 0.0f);
    const float dabs = rr_abs(d);
    const f3 e = -cross3(ray.d, ap);
    const float x = dot3(ac, e), y = dot3(ab, e);
    const bool neg = t < 0.0f;
    const float v = neg ? -x : x;
    const float w = neg ? y : -y;
    const bool rej1 = (v < 0.0f) || (v > dabs) || (w < 0.0f) || (v + w > dabs);
    if (rej0 || rej1) return false;
    const float invd = 1.0f / dabs;
    const float toi = (neg ? -t : t) * invd;
    if (!(toi <= RR_FLT_MAX)) return false;
    *toi_out = toi;
    *side_out = (back ? 2u : 0u) | (neg ? 1u : 0u);
    return true;
}

// ray_toi_with_ball + Ball::cast_local_ray_and_get_normal (centre = local origin)
RR_DEV bool ray_ball(float radius, const LRay& ray, bool solid, float* toi_out, bool* inside_out) {
    float a = dot3(ray.d, ray.d);
    float b = dot3(ray.o, ray.d);
    float c = dot3(ray.o, ray.o) - radius * radius;
    bool inside; float toi;
    if (a == 0.0f) {
        if (c > 0.0f) return false;
        inside = true; toi = 0.0f;
    } else if (c > 0.0f && b > 0.0f) {
        return false;
    } else {
        float delta = b * b - a * c;
        if (delta < 0.0f) return false;
        float sq = sqrtf(delta);
        float t = (-b - sq) / a;
        if (t <= 0.0f) { inside = true; toi = solid ? 0.0f : (-b + sq) / a; }
        else { inside = false; toi = t; }
    }
    if (toi > RR_FLT_MAX) return false;
    *toi_out = toi; *inside_out = inside;
    return true;
}
