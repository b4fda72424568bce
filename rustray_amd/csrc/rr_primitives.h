// rr_primitives.h — layer 1 of the device code: the exact primitive tests, one ray against one box, triangle or ball in
// item-local space.  parry3d 0.13 restated (ray_aabb.rs, ray_triangle.rs, ray_ball.rs) with the reference's transforms around
// them (ShapeBasics::get_inverse_ray, src/shape/mod.rs:755-761).  These decide every hit; all layers above only choose
// which of them to run.
//
// Offers: LRay, inverse_ray, to_local_point, to_world_normal, aabb_cast, ray_triangle, ray_ball.  No macros.
// Needs: rr_device.h (DItem), rr_math.h.
#pragma once
#include "rr_device.h"
#include "rr_math.h"

// ---------------------------------------------------------------------------
// geometry primitives: parry3d 0.13 restated (ray_aabb.rs, ray_triangle.rs, ray_ball.rs)
// ---------------------------------------------------------------------------
struct LRay { f3 o, d; };

// ShapeBasics::get_inverse_ray, reference src/shape/mod.rs:755-761
RR_DEV LRay inverse_ray(const DItem& it, f3 o, f3 d, bool general_w) {
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
