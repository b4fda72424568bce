// rr_surface.h — layer 4 of the device code: what a hit looks like.  Texture sampling (reference src/raytracing.rs:629-675,
// src/shape/mod.rs:510-629), the material record in registers, uv of spheres and meshes (src/shape/mesh.rs:105-161, :204-259;
// src/shape/sphere.rs:69-99), the jitter of a direction on the counter-based generator (src/raytracing.rs:565-626) and
// fresnel (:535-563).
//
// Offers: c_u8_to_f32 (filled by rr_api_scene.h rr_scene_create); texel, tex_wrap, tex_bilinear, MatR, load_material, uniform_row, load_material_uniform,
// tex_color (both forms); item_color; area_weights (both forms), sphere_uv, mesh_uv; RngKey, jitter; fresnel; HitItem, load_hit_item,
// load_hit_item_uniform; the steps of a hit's surface (HitWeights, hit_normal, hit_uv, mapped_normal, roughness_spread, hit_colors,
// hit_reflectivity, tangent_frame, hit_ambient_occlusion) and their composition (SurfaceAt, surface_at).  No macros.
// Needs: rr_primitives.h (to_local_point, inverse_ray, ray_ball, to_world_normal), rr_walk.h (rr_global), rr_trace.h (ray_nonfinite).
#pragma once
#include "rr_walk.h"
#include "rr_trace.h"

__constant__ float c_u8_to_f32[256]; // i / 255.0f, exactly as `(p[0] as f32) / 255.0`

// ---------------------------------------------------------------------------
// textures: reference src/raytracing.rs:629-675, src/shape/mod.rs:510-629
// ---------------------------------------------------------------------------
// `lut`: the u8 -> f32 table (c_u8_to_f32, or a workgroup's copy of it in LDS: four dependent reads per texel)
RR_DEV float4 texel(const DSceneView& sc, const DTexture& t, uint32_t x, uint32_t y, const float* lut = c_u8_to_f32) {
    uint32_t p = rr_global(sc.texels)[t.offset + (uint64_t)y * t.width + x];
    return make_float4(lut[p & 255u], lut[(p >> 8) & 255u], lut[(p >> 16) & 255u], lut[p >> 24]);
}
RR_DEV uint32_t tex_wrap(float val, uint32_t bound) {
    int32_t sb = (int32_t)bound;
    const int32_t x = as_i32(val * (float)bound);
    // power-of-two sizes: the mask IS the remainder made non-negative (x % sb, plus sb when negative), without the integer division
    if ((bound & (bound - 1u)) == 0u) return (uint32_t)x & (bound - 1u);
    int32_t w = x % sb;
    return (w < 0) ? (uint32_t)(w + sb) : (uint32_t)w;
}
RR_DEV float lerp1(float a, float b, float f) { return a + f * (b - a); } // helper::interpolate
RR_DEV float4 tex_bilinear(const DSceneView& sc, const DTexture& t, float u, float v, const float* lut = c_u8_to_f32) {
    uint32_t width = t.width, height = t.height;
    float x = u * (float)width, y = v * (float)height;
    if (x < 0.0f) x = x + (float)width;
    if (y < 0.0f) y = y + (float)height;
    uint32_t x0 = as_u32(floorf(x)), x1 = as_u32(ceilf(x));
    uint32_t y0 = as_u32(floorf(y)), y1 = as_u32(ceilf(y));
    if (x0 >= width) x0 = width - 1u;
    if (y0 >= height) y0 = height - 1u;
    if (x1 >= width) x1 = width - 1u;
    if (y1 >= height) y1 = height - 1u;
    float fx = x - (float)x0, fy = y - (float)y0;
    float4 p0 = texel(sc, t, x0, y0, lut), p1 = texel(sc, t, x1, y0, lut), p2 = texel(sc, t, x0, y1, lut), p3 = texel(sc, t, x1, y1, lut);
    float4 a = make_float4(lerp1(p0.x, p1.x, fx), lerp1(p0.y, p1.y, fx), lerp1(p0.z, p1.z, fx), lerp1(p0.w, p1.w, fx));
    float4 b = make_float4(lerp1(p2.x, p3.x, fx), lerp1(p2.y, p3.y, fx), lerp1(p2.z, p3.z, fx), lerp1(p2.w, p3.w, fx));
    return make_float4(lerp1(a.x, b.x, fy), lerp1(a.y, b.y, fy), lerp1(a.z, b.z, fy), lerp1(a.w, b.w, fy));
}
// The material of a hit, copied into registers once (four 16-B loads + the flag word): the shading code stores to
// queues and accumulators between its uses, so fields read through the pointer would be re-fetched one dword at a
// time, each fetch a dependent round trip.  Texture slots are only looked at when the flag word says they are set.
struct MatR {
    f3 ambient, base, specular;
    float alpha, shininess, reflectivity, refraction_index, normal_map_strength, shadow_softness, roughness;
    float cos_shadow_softness, cos_roughness; // jitter()'s z_lo for the two constant spreads (host-evaluated, DMaterial)
    uint32_t flags;
    const DMaterial* p;
    const DMaterial* up; // the same record where every lane of the wave shades this material (load_material_uniform: a scalar), else NULL
    const float* lut; // u8 -> f32 table of the workgroup (LDS)
};
static_assert(offsetof(DMaterial, ambient) == 0 && offsetof(DMaterial, alpha) == 12 && offsetof(DMaterial, base) == 16 && offsetof(DMaterial, specular) == 32
              && offsetof(DMaterial, refraction_index) == 48 && offsetof(DMaterial, roughness) == 60, "MatR: colour and scalar groups");
static_assert(offsetof(DMaterial, tex) == 64 && offsetof(DMaterial, flags) == 96 && offsetof(DMaterial, cos_shadow_softness) == 100 && offsetof(DMaterial, cos_roughness) == 104
              && offsetof(DMaterial, texd) == 112 && sizeof(DMaterial) == 240, "MatR: flag group, texture descriptors, record size");
template <class F4> RR_DEV MatR material_regs(F4 a, F4 b, F4 c, F4 d, F4 e, const DMaterial* p, const DMaterial* up, const float* lut) {
    MatR m;
    m.ambient = mk3(a.x, a.y, a.z); m.alpha = a.w;
    m.base = mk3(b.x, b.y, b.z); m.shininess = b.w;
    m.specular = mk3(c.x, c.y, c.z); m.reflectivity = c.w;
    m.refraction_index = d.x; m.normal_map_strength = d.y; m.shadow_softness = d.z; m.roughness = d.w;
    m.flags = __float_as_uint(e.x); m.cos_shadow_softness = e.y; m.cos_roughness = e.z; m.p = p; m.up = up; m.lut = lut;
    return m;
}
RR_DEV MatR load_material(const DMaterial* p, const float* lut) {
    const float4* q = (const float4*)p;
    const float4 a = q[0], b = q[1], c = q[2], d = q[3], e = q[6]; // q[4], q[5]: the texture slots, read when a slot's flag is set
    return material_regs(a, b, c, d, e, p, nullptr, lut);
}
// 16 bytes of a record at a WAVE-UNIFORM address, through the constant address space: a scalar request, the value arrives in SGPRs
RR_DEV rr_f4v uniform_row(const void* record, uint32_t byte_off) {
    return *(const __attribute__((address_space(4))) rr_f4v*)((const __attribute__((address_space(4))) char*)(uintptr_t)record + byte_off);
}
// The material of a WAVE-UNIFORM hit (`material`: a scalar, HitItem::material of load_hit_item_uniform): the same five groups through the
// constant address space, issued together and waited for once (item_rec_uniform, rr_primitives.h, has the story of the empty asm
// statement).  Materials are written by no kernel; edits happen between launches.
RR_DEV MatR load_material_uniform(const DMaterial* materials, int material, const float* lut) {
    const DMaterial* up = materials + material;
    const rr_f4v a = uniform_row(up, 0u), b = uniform_row(up, 16u), c = uniform_row(up, 32u), d = uniform_row(up, 48u), e = uniform_row(up, 96u);
    asm volatile("" :: "s"(a), "s"(b), "s"(c), "s"(d), "s"(e));
    return material_regs(a, b, c, d, e, up, up, lut);
}
RR_DEV bool tex_color(const DSceneView& sc, const MatR& m, bool has_uv, f2 uv, int slot, float4* out) {
    if (!(m.flags & (RR_MF_TEX_SLOT0 << slot)) || !has_uv) return false; // slot bit = index >= 0 and width > 0
    DTexture t; // the slot's descriptor sits in the material record itself (DMaterial::texd): one 16-B load at an address known since the material was
    if (m.up) { // (a scalar test: one request for the wave, and the texel addresses below are formed from scalars)
        const rr_f4v q = uniform_row(m.up, (uint32_t)offsetof(DMaterial, texd) + 16u * (uint32_t)slot);
        t.offset = (uint64_t)__float_as_uint(q.x) | ((uint64_t)__float_as_uint(q.y) << 32); t.width = __float_as_uint(q.z); t.height = __float_as_uint(q.w);
    } else
    { const uint4 q = *(const uint4*)&m.p->texd[slot]; t.offset = (uint64_t)q.x | ((uint64_t)q.y << 32); t.width = q.z; t.height = q.w; }
    if (m.flags & RR_MF_NEAREST) *out = texel(sc, t, tex_wrap(uv.x, t.width), tex_wrap(uv.y, t.height), m.lut);
    else *out = tex_bilinear(sc, t, uv.x, uv.y, m.lut);
    return true;
}
// get_tex_color: false = None
RR_DEV bool tex_color(const DSceneView& sc, const DMaterial& m, bool has_uv, f2 uv, int slot, float4* out) {
    int ti = m.tex[slot];
    if (ti < 0 || !has_uv) return false;
    DTexture t; t.offset = m.texd[slot].offset; t.width = m.texd[slot].width; t.height = m.texd[slot].height;
    if (t.width == 0u) return false;
    if (m.flags & RR_MF_NEAREST) *out = texel(sc, t, tex_wrap(uv.x, t.width), tex_wrap(uv.y, t.height));
    else *out = tex_bilinear(sc, t, uv.x, uv.y);
    return true;
}

// get_item_color, reference src/raytracing.rs:677-712
RR_DEV float4 item_color(const DSceneView& sc, const MatR& m, bool has_uv, f2 uv, f3 rgb, int slot) {
    float4 c = make_float4(rgb.x, rgb.y, rgb.z, 1.0f);
    float4 t;
    if (tex_color(sc, m, has_uv, uv, slot, &t)) { c.x *= t.x; c.y *= t.y; c.z *= t.z; c.w *= t.w; }
    return c;
}

// ---------------------------------------------------------------------------
// uv / normals: reference src/shape/mesh.rs:105-161, :204-259; src/shape/sphere.rs:69-99
// ---------------------------------------------------------------------------
RR_DEV void area_weights(f3 a, f3 b, f3 c, f3 p, float* a1, float* a2, float* a3) {
    f3 f1 = a - p, f2v = b - p, f3v = c - p;
    float area = norm3(cross3(a - b, a - c));
    *a1 = norm3(cross3(f2v, f3v)) / area;
    *a2 = norm3(cross3(f3v, f1)) / area;
    *a3 = norm3(cross3(f1, f2v)) / area;
}
// the same with the triangle's area from the host (DTri::v1.w: the value of the line `area = ...` above, bit for bit)
RR_DEV void area_weights(f3 a, f3 b, f3 c, f3 p, float area, float* a1, float* a2, float* a3) {
    f3 f1 = a - p, f2v = b - p, f3v = c - p;
    *a1 = norm3(cross3(f2v, f3v)) / area;
    *a2 = norm3(cross3(f3v, f1)) / area;
    *a3 = norm3(cross3(f1, f2v)) / area;
}
RR_DEV f2 sphere_uv(const DItem& it, f3 hit, bool general_w) {
    f3 p = to_local_point(it, hit, general_w);
    float theta = rr_atan2(-(p.z - 0.0f), p.x - 0.0f);
    float u = (theta + RR_PI_F) / (2.0f * RR_PI_F);
    float phi = rr_acos((-(p.y - 0.0f)) / it.radius);
    float v = phi / RR_PI_F;
    f2 r; r.x = u; r.y = -v; return r;
}
RR_DEV f2 mesh_uv(const DSceneView& sc, const DItem& it, uint32_t slot, f3 hit, bool general_w) {
    f2 r; r.x = 0.0f; r.y = 0.0f;
    const DTriAttr at = rr_global(sc.attrs)[it.tri_base + slot];
    if (!(__float_as_uint(at.s3.w) & 1u)) return r;
    f3 p = to_local_point(it, hit, general_w);
    const DTri tr = rr_global(sc.tris)[it.tri_base + slot];
    float a1, a2, a3;
    area_weights(mk3(tr.v0.x, tr.v0.y, tr.v0.z), mk3(tr.v1.x, tr.v1.y, tr.v1.z), mk3(tr.v2.x, tr.v2.y, tr.v2.z), p, &a1, &a2, &a3);
    float ux = (at.s0.w * a1 + at.s2.w * a2) + at.s3.y * a3;
    float uy = (at.s1.w * a1 + at.s3.x * a2) + at.s3.z * a3;
    r.x = ux; r.y = -uy;
    return r;
}

// ---------------------------------------------------------------------------
// jitter (reference src/raytracing.rs:565-626) on the counter-based generator
// ---------------------------------------------------------------------------
struct RngKey { uint32_t seed_lo, seed_hi, pixel, sample, node; };
// z_lo = rr_cos(spread * RR_PI_F): passed in, because for the two spreads that are material constants (shadow_softness, roughness
// without a map) the host has evaluated it once per material (DMaterial::cos_*) with the same rr_cos
RR_DEV f3 jitter(f3 dir, float spread, float z_lo, const RngKey& k, uint32_t stream) {
    if (spread <= 0.0f) return dir;
    f3 b3 = normalize3(dir);
    f3 diff = (rr_abs(b3.x) < 0.5f) ? mk3(1.0f, 0.0f, 0.0f) : mk3(0.0f, 1.0f, 0.0f);
    f3 b1 = normalize3(cross3(b3, diff));
    f3 b2 = cross3(b1, b3);
    if (!(z_lo < 1.0f)) return dir;
    uint32_t r0, r1;
    philox4x32_10(k.pixel, k.sample, k.node, stream, k.seed_lo, k.seed_hi, &r0, &r1);
    float z = uniform_f32(r0, z_lo, 1.0f);
    float r = sqrtf(1.0f - z * z);
    float theta = uniform_f32(r1, -RR_PI_F, RR_PI_F);
    float s, c;
    rr_sincos(theta, &s, &c);
    float x = r * c, y = r * s;
    f3 nd = (x * b1 + y * b2) + z * b3;
    return normalize3(nd);
}

// fresnel, reference src/raytracing.rs:535-563 (cos_i = |cos_t| as written there)
RR_DEV float fresnel(f3 incident, f3 normal, float index) {
    float i_dot_n = dot3(incident, normal);
    float eta_i = 1.0f, eta_t = index;
    if (i_dot_n > 0.0f) { eta_i = eta_t; eta_t = 1.0f; }
    float sin_t = eta_i / eta_t * sqrtf(rs_max(1.0f - i_dot_n * i_dot_n, 0.0f));
    if (sin_t > 1.0f) return 1.0f;
    float cos_t = sqrtf(rs_max(1.0f - sin_t * sin_t, 0.0f));
    float cos_i = rr_abs(cos_t);
    float r_s = ((eta_t * cos_i) - (eta_i * cos_t)) / ((eta_t * cos_i) + (eta_i * cos_t));
    float r_p = ((eta_i * cos_i) - (eta_t * cos_t)) / ((eta_i * cos_i) + (eta_t * cos_t));
    return (r_s * r_s + r_p * r_p) / 2.0f;
}

// ---------------------------------------------------------------------------
// the surface of a closest hit: what get_color_depth_normal_id evaluates between `trace` and the light loop (reference
// src/raytracing.rs:747-811, :928-933, :985-991), in the reference's steps.  k_shade calls the steps where it needs their values,
// between its own sums, jitter and recursion; surface_at (rr_surface_rays) is their composition for callers that want the values.
// ---------------------------------------------------------------------------
// The words of a hit's item that every hit reads, in registers (see MatR); the matrix rows and the radius, which smooth, textured and
// sphere hits alone read, stay behind `const DItem&`.
struct HitItem { uint32_t flags, id, wn_base, tri_base; int32_t material; };
static_assert(offsetof(DItem, id) == 144 && offsetof(DItem, material) == 148 && offsetof(DItem, wn_base) == 152, "HitItem: id group");
RR_DEV HitItem load_hit_item(const DItem& it) {
    HitItem h; h.flags = it.flags; h.id = it.id; h.wn_base = it.wn_base; h.tri_base = it.tri_base; h.material = it.material;
    return h;
}
// The same of a WAVE-UNIFORM item (`idx`: the same in every active lane, at least one of them): the flag word, the id group and the tree
// group's first word through the constant address space, issued together and waited for once, as item_rec_uniform does for the walks.
RR_DEV HitItem load_hit_item_uniform(const DItem* items, int idx) {
    const DItem* it = items + (uint32_t)__builtin_amdgcn_readfirstlane(idx);
    const rr_f4v box = uniform_row(it, 128u), g = uniform_row(it, 144u), tree = uniform_row(it, 160u); // (flags: the box row's w lane, as in ItemRec)
    asm volatile("" :: "s"(box), "s"(g), "s"(tree));
    HitItem h; h.flags = __float_as_uint(box.w); h.id = __float_as_uint(g.x); h.material = __float_as_int(g.y); h.wn_base = __float_as_uint(g.z); h.tri_base = __float_as_uint(tree.x);
    return h;
}

// The area weights of a mesh hit and its triangle's attributes: they serve the interpolated normal AND the uv (Mesh::get_normal and
// Mesh::get_uv compute the same three numbers from the same inputs, src/shape/mesh.rs:105-161, :204-259)
struct HitWeights { DTriAttr at; float a1, a2, a3; bool have; };
// The entry of DSceneView::flat_normals that holds a hit's world normal (`hit_z`: the walks' face word, as hit_normal reads it) -- a
// flat-shaded triangle of an item that does not flip normals --, else RR_NO_FRAME: mapped_normal takes the entry's tangent frame instead
// of deriving it from the normal.  (A flipped normal is not an entry's: zeros of the frame of -n differ in sign from the negated frame
// of n, so that frame is derived per hit.)
#define RR_NO_FRAME 0xffffffffu
RR_DEV uint32_t flat_frame_entry(const HitItem& hi, uint32_t hit_z) {
    if (hi.flags & (RR_IF_SPHERE | RR_IF_SMOOTH | RR_IF_FLIP_NORMALS)) return RR_NO_FRAME;
    return hi.wn_base + 2u * (hit_z & 0x3fffffffu) + ((hit_z >> 30) & 1u);
}

// World normal: Shape::intersect (mesh.rs:76-98, sphere.rs:61-65).  `hi`: the caller's register copies of the item's words (HitItem);
// `hit_z`: the walks' face word (leaf-order slot | negated << 30 | back << 31); `gw`: DSceneView::general_w.
RR_DEV f3 hit_normal(const DSceneView& sc, const DItem& it, const HitItem& hi, const MatR& m, f3 ro, f3 rd, f3 hit_point, uint32_t hit_z, bool gw, HitWeights* w) {
    const uint32_t it_flags = hi.flags, it_tri_base = hi.tri_base;
    const uint32_t slot = hit_z & 0x3fffffffu;
    const bool back = (hit_z >> 31) != 0u, neg = ((hit_z >> 30) & 1u) != 0u;
    f3 normal;
    DTriAttr at; float a1 = 0.0f, a2 = 0.0f, a3 = 0.0f; bool have_weights = false;
    at.s0 = at.s1 = at.s2 = at.s3 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (it_flags & RR_IF_SPHERE) {
        LRay lr = inverse_ray(it, ro, rd, gw || ray_nonfinite(ro, rd)); // (see to_local_point)
        float t2 = 0.0f; bool inside = false;
        ray_ball(it.radius, lr, (it_flags & RR_IF_SOLID_BASE) != 0u, &t2, &inside);
        f3 nl = normalize3(lr.o + lr.d * t2);
        normal = to_world_normal(it, inside ? -nl : nl);
    } else {
        const DTri* trp = &rr_global(sc.tris)[it_tri_base + slot];
        if ((it_flags & RR_IF_SMOOTH) || (m.flags & RR_MF_ANY_TEX)) {
            const float4 v0 = trp->v0, v1 = trp->v1, v2 = trp->v2;
            at = rr_global(sc.attrs)[it_tri_base + slot];
            const f3 p = to_local_point(it, hit_point, gw);
            area_weights(mk3(v0.x, v0.y, v0.z), mk3(v1.x, v1.y, v1.z), mk3(v2.x, v2.y, v2.z), p, v1.w, &a1, &a2, &a3); // v1.w: the triangle's area (host)
            have_weights = true;
        }
        if (it_flags & RR_IF_SMOOTH) {
            f3 p1 = mk3(at.s0.x, at.s0.y, at.s0.z) * a1, p2 = mk3(at.s1.x, at.s1.y, at.s1.z) * a2, p3 = mk3(at.s2.x, at.s2.y, at.s2.z) * a3;
            normal = to_world_normal(it, mk3(p1.x + p2.x + p3.x, p1.y + p2.y + p3.y, p1.z + p2.z + p3.z));
            if (back) normal = -normal;
        } else {
            // to_world_normal(it, neg ? -ng : ng) with ng = DTri::v3, evaluated once per instanced triangle by k_world_normals
            const uint32_t entry = hi.wn_base + 2u * slot + (neg ? 1u : 0u);
            const float4 wn = rr_global(sc.flat_normals)[(uint64_t)entry * RR_FLAT_ENTRY_F4];
            normal = mk3(wn.x, wn.y, wn.z);
        }
        if (it_flags & RR_IF_FLIP_NORMALS) normal = -normal;
    }
    w->at = at; w->a1 = a1; w->a2 = a2; w->a3 = a3; w->have = have_weights;
    return normal;
}
// uv (:749-754): get_uv where the material has any texture (the return value), else (0, 0)
RR_DEV bool hit_uv(const DItem& it, uint32_t it_flags, const MatR& m, f3 hit_point, bool gw, const HitWeights& w, f2* uv_out) {
    bool has_uv = false; f2 uv; uv.x = 0.0f; uv.y = 0.0f;
    if (m.flags & RR_MF_ANY_TEX) {
        if (it_flags & RR_IF_SPHERE) uv = sphere_uv(it, hit_point, gw);
        else if (w.have && (__float_as_uint(w.at.s3.w) & 1u)) { // Mesh::get_uv with the weights of hit_normal
            uv.x = (w.at.s0.w * w.a1 + w.at.s2.w * w.a2) + w.at.s3.y * w.a3;
            uv.y = -((w.at.s1.w * w.a1 + w.at.s3.x * w.a2) + w.at.s3.z * w.a3);
        }
        has_uv = true;
    }
    *uv_out = uv;
    return has_uv;
}
// The tangent frame of normal mapping (:757-784): a function of the normal alone.  k_world_normals evaluates it once per entry of
// DSceneView::flat_normals, mapped_normal per hit for the normals that are not such an entry's.
struct TangentFrame { f3 tangent, bitangent; };
RR_DEV TangentFrame tangent_frame(f3 normal) {
    f3 tangent = cross3(normal, mk3(0.0f, 1.0f, 0.0f));
    if (norm3(tangent) <= 0.0001f) tangent = cross3(normal, mk3(0.0f, 0.0f, 1.0f));
    TangentFrame f;
    f.tangent = normalize3(tangent);
    f.bitangent = normalize3(cross3(normal, f.tangent));
    return f;
}
// normal mapping (:757-784): `normal` where the material has no normal map.  `frame_entry`: flat_frame_entry of the hit, or RR_NO_FRAME
// (smooth-shaded and sphere hits, flipped normals, a caller without a table): the frame is then derived here.
RR_DEV f3 mapped_normal(const DSceneView& sc, const MatR& m, bool has_uv, f2 uv, f3 normal, uint32_t frame_entry) {
    f3 surface_normal = normal;
    float4 tc;
    if (tex_color(sc, m, has_uv, uv, 3, &tc)) {
        TangentFrame f;
        if (frame_entry != RR_NO_FRAME) {
            const float4* e = &rr_global(sc.flat_normals)[(uint64_t)frame_entry * RR_FLAT_ENTRY_F4];
            const float4 t = e[1], b = e[2];
            f.tangent = mk3(t.x, t.y, t.z); f.bitangent = mk3(b.x, b.y, b.z);
        } else f = tangent_frame(normal);
        const f3 tangent = f.tangent, bitangent = f.bitangent;
        f3 nm = mk3((tc.x * 2.0f) - 1.0f, (tc.y * 2.0f) - 1.0f, (tc.z * 2.0f) - 1.0f);
        nm.x *= m.normal_map_strength; nm.y *= m.normal_map_strength;
        nm = normalize3(nm);
        f3 t;
        t.x = (tangent.x * nm.x + bitangent.x * nm.y) + normal.x * nm.z;
        t.y = (tangent.y * nm.x + bitangent.y * nm.y) + normal.y * nm.z;
        t.z = (tangent.z * nm.x + bitangent.z * nm.y) + normal.z * nm.z;
        surface_normal = normalize3(t);
    }
    return surface_normal;
}
// roughness (:787-798): the spread a jitter of the normal takes -- the material's, or its roughness map's texel (the return value says which)
RR_DEV bool roughness_spread(const DSceneView& sc, const MatR& m, bool has_uv, f2 uv, float* roughness) {
    float4 tc;
    const bool has_rtc = tex_color(sc, m, has_uv, uv, 5, &tc);
    *roughness = m.roughness;
    if (has_rtc) *roughness = (1.0f / RR_PI_F / 2.0f) * tc.x;
    return has_rtc;
}
// colours (get_item_color) and alpha (:801-811), returned as one value: through four pointers k_shade spills VGPRs at its 128
struct HitColors { float4 ambient, base, specular; float alpha; };
RR_DEV HitColors hit_colors(const DSceneView& sc, const MatR& m, bool has_uv, f2 uv) {
    HitColors c;
    c.ambient = item_color(sc, m, has_uv, uv, m.ambient, 1);
    c.base = item_color(sc, m, has_uv, uv, m.base, 0);
    c.specular = item_color(sc, m, has_uv, uv, m.specular, 2);
    c.alpha = m.alpha * c.base.w;
    float4 tc;
    if (tex_color(sc, m, has_uv, uv, 4, &tc)) c.alpha *= tc.x;
    return c;
}
// reflectivity (:928-933)
RR_DEV float hit_reflectivity(const DSceneView& sc, const MatR& m, bool has_uv, f2 uv) {
    float reflectivity = m.reflectivity;
    float4 tc;
    if (tex_color(sc, m, has_uv, uv, 7, &tc)) reflectivity = tc.x;
    return reflectivity;
}
// ambient occlusion (:985-991)
RR_DEV float hit_ambient_occlusion(const DSceneView& sc, const MatR& m, bool has_uv, f2 uv) {
    float ao = 1.0f;
    float4 tc;
    if (tex_color(sc, m, has_uv, uv, 6, &tc)) ao = tc.x;
    return ao;
}

struct SurfaceAt {
    f3 position, normal, shading_normal; // origin + direction * toi; Shape::intersect's world normal; after normal mapping, before any jitter
    f2 uv; bool has_uv;                  // get_uv where the material has any texture, else (0, 0) and false
    float4 base_color, ambient_color, specular_color; // get_item_color
    float alpha, reflectivity, roughness, ambient_occlusion; // roughness: the spread, whether or not monte_carlo asks for a jitter
};
RR_DEV SurfaceAt surface_at(const DSceneView& sc, const DItem& it, const MatR& m, f3 ro, f3 rd, float hit_dist, uint32_t hit_z) {
    SurfaceAt s;
    const bool gw = sc.general_w != 0u;
    const HitItem hi = load_hit_item(it);
    const uint32_t it_flags = hi.flags;
    HitWeights w;
    s.position = ro + (rd * hit_dist);
    s.normal = hit_normal(sc, it, hi, m, ro, rd, s.position, hit_z, gw, &w);
    s.has_uv = hit_uv(it, it_flags, m, s.position, gw, w, &s.uv);
    s.shading_normal = mapped_normal(sc, m, s.has_uv, s.uv, s.normal, flat_frame_entry(hi, hit_z));
    roughness_spread(sc, m, s.has_uv, s.uv, &s.roughness);
    const HitColors c = hit_colors(sc, m, s.has_uv, s.uv);
    s.ambient_color = c.ambient; s.base_color = c.base; s.specular_color = c.specular; s.alpha = c.alpha;
    s.reflectivity = hit_reflectivity(sc, m, s.has_uv, s.uv);
    s.ambient_occlusion = hit_ambient_occlusion(sc, m, s.has_uv, s.uv);
    return s;
}
