// rr_scene_build.h — everything a scene's device records are made of before the first upload: the checks of the caller's arrays,
// the record makers, the per-mesh trees and the top level over the items' world boxes.  Plain host arithmetic, no HIP runtime
// calls (rr_api_scene.h uploads what this builds; tests/native/scene_build_test.cpp checks it on the CPU).
//
// Errors go through the library's one channel: `fail` sets the calling thread's rr_last_error text and returns the code.  It is
// defined by whoever includes this file (rr_api_base.h; the native test).  RR_FAULT_POINT is rr_api_base.h's test-only fault hook.
#pragma once
#include "../../include/rustray_hip.h"
#include "rr_beam.h"
#include "rr_bvh.h"
#include "rr_device.h"
#include "rr_math.h"

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstring>
#include <exception>
#include <thread>
#include <vector>

static int fail(int code, const char* fmt, ...) noexcept;
#ifndef RR_FAULT_POINT
#define RR_FAULT_POINT(name) ((void)0)
#endif

// Host worker threads (mesh tree builds, one thread per device in rr_render_multi): an exception inside a worker is carried to the
// calling thread and rethrown there, a thread that cannot be started is not fatal (the caller does that work itself), and the
// destructor joins -- no path ends in std::terminate.
struct Workers {
    std::vector<std::thread> threads;
    std::atomic_flag taken = ATOMIC_FLAG_INIT;
    std::exception_ptr first; // written by the one worker that wins `taken`, read after join()
    Workers() = default;
    Workers(const Workers&) = delete;
    Workers& operator=(const Workers&) = delete;
    ~Workers() { join(); }
    // runs f() on a new thread; false = no thread could be started (the caller runs f itself)
    template <class F> bool spawn(F f) {
        try {
            threads.emplace_back([this, f]() mutable { run(f); });
            return true;
        } catch (...) { return false; }
    }
    // f() on the calling thread, under the same net
    template <class F> void run(F& f) noexcept {
        try { f(); }
        catch (...) { if (!taken.test_and_set()) first = std::current_exception(); }
    }
    void join() noexcept { for (std::thread& t : threads) if (t.joinable()) t.join(); }
    void join_and_rethrow() { join(); if (first) std::rethrow_exception(first); }
};

// ---------------------------------------------------------------------------
// checks: what rr_scene_create and the scene edits refuse, one definition each
// ---------------------------------------------------------------------------
static bool finite16(const float* m) { for (int i = 0; i < 16; i++) if (!std::isfinite(m[i])) return false; return true; }
// the bottom row of an inverse matrix is (0, 0, 0, 1): rays keep w = 1 in the item's space (DItem::inv3; column-major m[3], m[7], m[11], m[15])
static bool affine_inverse(const float4& row3) { return row3.x == 0.0f && row3.y == 0.0f && row3.z == 0.0f && row3.w == 1.0f; }

static int check_textures(const rr_texture* textures, uint32_t n) {
    for (uint32_t i = 0; i < n; i++) {
        const rr_texture& t = textures[i];
        if ((uint64_t)t.width * t.height > 0 && !t.rgba8) return fail(RR_ERR_INVALID_ARGUMENT, "texture %u has no pixels", i);
        if (t.width > 32768u || t.height > 32768u) return fail(RR_ERR_UNSUPPORTED, "texture %u is %ux%u", i, t.width, t.height);
    }
    return RR_OK;
}
static int check_material_textures(const rr_material* materials, uint32_t n, size_t n_textures) {
    for (uint32_t i = 0; i < n; i++)
        for (int k = 0; k < RR_TEX_COUNT; k++) {
            int32_t t = materials[i].texture[k];
            if (t >= (int32_t)n_textures) return fail(RR_ERR_INVALID_ARGUMENT, "material %u texture slot %d = %d out of range", i, k, t);
        }
    return RR_OK;
}
// a material cache carries no textures (reference src/shape/mod.rs:769-772); the callers name the item or the material in their message
static bool carries_textures(const rr_material& m) {
    for (int k = 0; k < RR_TEX_COUNT; k++) if (m.texture[k] >= 0) return true;
    return false;
}
static int check_lights(const rr_light* lights, uint32_t n) {
    for (uint32_t i = 0; i < n; i++)
        if (lights[i].light_type > RR_LIGHT_SPOT) return fail(RR_ERR_INVALID_ARGUMENT, "light %u: type %u", i, lights[i].light_type);
    return RR_OK;
}
static int check_item_transform(uint32_t i, const float* trans, const float* trans_inv) {
    if (!finite16(trans) || !finite16(trans_inv)) return fail(RR_ERR_INVALID_ARGUMENT, "item %u: non-finite transform", i);
    return RR_OK;
}

// the meshes of a scene, or those appended to one (rr_scene_add_meshes: `first` = the index of meshes[0] in the scene's list)
static int check_meshes(const rr_mesh* meshes, uint32_t n, uint32_t first) {
    for (uint32_t j = 0; j < n; j++) {
        const rr_mesh& m = meshes[j];
        const uint32_t i = first + j;
        if ((m.n_vertices && !m.positions) || (m.n_triangles && !m.indices)) return fail(RR_ERR_INVALID_ARGUMENT, "mesh %u: missing positions/indices", i);
        if ((m.n_uvs && !m.uvs) || (m.n_uv_faces && !m.uv_indices) || (m.n_normals && !m.normals) || (m.n_normal_faces && !m.normal_indices))
            return fail(RR_ERR_INVALID_ARGUMENT, "mesh %u: attribute pointer is NULL with a non-zero count", i);
        if (m.n_triangles >= (1u << 28)) return fail(RR_ERR_UNSUPPORTED, "mesh %u: %u triangles", i, m.n_triangles);
        for (size_t k = 0; k < (size_t)m.n_triangles * 3; k++)
            if (m.indices[k] >= m.n_vertices) return fail(RR_ERR_INVALID_ARGUMENT, "mesh %u: vertex index %u out of range", i, m.indices[k]);
        for (size_t k = 0; k < (size_t)m.n_uv_faces * 3; k++)
            if (m.uv_indices[k] >= m.n_uvs) return fail(RR_ERR_INVALID_ARGUMENT, "mesh %u: uv index %u out of range", i, m.uv_indices[k]);
        for (size_t k = 0; k < (size_t)m.n_normal_faces * 3; k++)
            if (m.normal_indices[k] >= m.n_normals) return fail(RR_ERR_INVALID_ARGUMENT, "mesh %u: normal index %u out of range", i, m.normal_indices[k]);
        // Mesh::get_normal indexes normals_indices[face] unchecked (reference src/shape/mesh.rs:216): the reference would panic
        if (m.n_normals > 0 && m.n_normal_faces > 0 && m.n_normal_faces < m.n_triangles)
            return fail(RR_ERR_INVALID_ARGUMENT, "mesh %u: %u normal faces for %u triangles (the reference panics on this)", i, m.n_normal_faces, m.n_triangles);
    }
    return RR_OK;
}
// an item list against the material list it names and the number of meshes it may name (rr_scene_create, rr_scene_set_items)
static int check_items(const rr_item* items, uint32_t n_items, const rr_material* materials, uint32_t n_materials, size_t n_meshes) {
    if (n_items >= (1u << 27)) return fail(RR_ERR_UNSUPPORTED, "%u items (the shadow-ray record keeps the item index in 27 bits)", n_items);
    for (uint32_t i = 0; i < n_items; i++) {
        const rr_item& it = items[i];
        if (it.kind != RR_ITEM_SPHERE && it.kind != RR_ITEM_MESH) return fail(RR_ERR_INVALID_ARGUMENT, "item %u: kind %u", i, it.kind);
        if (it.material < 0 || it.material >= (int32_t)n_materials || it.material_cache < 0 || it.material_cache >= (int32_t)n_materials)
            return fail(RR_ERR_INVALID_ARGUMENT, "item %u: material index out of range", i);
        if (carries_textures(materials[it.material_cache]))
            return fail(RR_ERR_INVALID_ARGUMENT, "item %u: material_cache must not carry textures (reference src/shape/mod.rs:769-772)", i);
        if (it.kind == RR_ITEM_MESH && (it.mesh < 0 || (size_t)it.mesh >= n_meshes)) return fail(RR_ERR_INVALID_ARGUMENT, "item %u: mesh index %d", i, it.mesh);
        const int rc = check_item_transform(i, it.trans, it.trans_inv);
        if (rc != RR_OK) return rc;
    }
    return RR_OK;
}

static int validate_scene(const rr_flat_scene* fs) {
    if (!fs) return fail(RR_ERR_INVALID_ARGUMENT, "scene is NULL");
    if (fs->abi_version != RR_ABI_VERSION) return fail(RR_ERR_INVALID_ARGUMENT, "abi_version %u, library speaks %u", fs->abi_version, RR_ABI_VERSION);
    if ((fs->n_items && !fs->items) || (fs->n_meshes && !fs->meshes) || (fs->n_materials && !fs->materials) ||
        (fs->n_textures && !fs->textures) || (fs->n_lights && !fs->lights))
        return fail(RR_ERR_INVALID_ARGUMENT, "array pointer is NULL with a non-zero count");
    if (fs->n_items >= (1u << 27)) return fail(RR_ERR_UNSUPPORTED, "%u items (the shadow-ray record keeps the item index in 27 bits)", fs->n_items);
    int rc = check_textures(fs->textures, fs->n_textures);
    if (rc == RR_OK) rc = check_material_textures(fs->materials, fs->n_materials, fs->n_textures);
    if (rc == RR_OK) rc = check_meshes(fs->meshes, fs->n_meshes, 0);
    if (rc == RR_OK) rc = check_items(fs->items, fs->n_items, fs->materials, fs->n_materials, fs->n_meshes);
    if (rc != RR_OK) return rc;
    return check_lights(fs->lights, fs->n_lights);
}

// ---------------------------------------------------------------------------
// record makers
// ---------------------------------------------------------------------------
// what of an item the flag words are rebuilt from (rr_scene_update_materials, rr_scene_update_item_flags)
struct ItemHost { uint32_t kind; int32_t material, material_cache; bool visible, flip_normals, mesh_has_normals, mesh_degenerate; int32_t mesh; };

// The RGBA8 pool holds the images in list order: an image's offset is the texel count of those before it.  Appending to a list gives
// the existing images the offsets they have and the new ones those a scene created with the longer list gives them.
static uint64_t pool_texels(const std::vector<DTexture>& dtex) {
    return dtex.empty() ? 0 : dtex.back().offset + (uint64_t)dtex.back().width * dtex.back().height;
}
static void append_texture_layout(const rr_texture* textures, uint32_t n, std::vector<DTexture>* dtex, std::vector<uint32_t>* tex_width) {
    uint64_t n_texels = pool_texels(*dtex);
    for (uint32_t i = 0; i < n; i++) {
        DTexture d;
        d.offset = n_texels; d.width = textures[i].width; d.height = textures[i].height;
        dtex->push_back(d);
        tex_width->push_back(textures[i].width);
        n_texels += (uint64_t)textures[i].width * textures[i].height;
    }
}

// Material (reference src/shape/mod.rs:95-134) -> device record; has_texture = the slot names an image of width > 0
static DMaterial make_dmaterial(const rr_material& m, const std::vector<uint32_t>& tex_width, const std::vector<DTexture>& dtex) {
    DMaterial d;
    memset(&d, 0, sizeof d);
    for (int k = 0; k < 3; k++) { d.ambient[k] = m.ambient_color[k]; d.base[k] = m.base_color[k]; d.specular[k] = m.specular_color[k]; }
    d.alpha = m.alpha; d.shininess = m.shininess; d.reflectivity = m.reflectivity; d.refraction_index = m.refraction_index;
    d.normal_map_strength = m.normal_map_strength; d.shadow_softness = m.shadow_softness; d.roughness = m.roughness;
    d.cos_shadow_softness = rr_cos(m.shadow_softness * RR_PI_F); d.cos_roughness = rr_cos(m.roughness * RR_PI_F); // jitter()'s z_lo, see DMaterial
    bool any = false;
    uint32_t slots = 0u;
    for (int k = 0; k < RR_TEX_COUNT; k++) {
        d.tex[k] = m.texture[k];
        if (m.texture[k] >= 0) { const DTexture& t = dtex[m.texture[k]]; d.texd[k].offset = t.offset; d.texd[k].width = t.width; d.texd[k].height = t.height; }
        if (m.texture[k] >= 0 && tex_width[m.texture[k]] > 0) { any = true; slots |= RR_MF_TEX_SLOT0 << k; }
    }
    d.flags = slots | (m.texture_filtering_nearest ? RR_MF_NEAREST : 0u) | (m.receive_shadow ? RR_MF_RECEIVE_SHADOW : 0u) |
              (m.monte_carlo ? RR_MF_MONTE_CARLO : 0u) | (any ? RR_MF_ANY_TEX : 0u);
    return d;
}

// The flag word of an item: what Raytracing::trace reads of the texture-less material cache (src/raytracing.rs:450-458),
// intersect_b_box's `solid` (src/shape/mesh.rs:51-59) and the occluder-alpha-map test of the shadow code (:899-912).
static uint32_t item_flags(const ItemHost& it, const rr_material& cache, const rr_material& full, const std::vector<uint32_t>& tex_width) {
    uint32_t f = 0;
    if (it.visible) f |= RR_IF_VISIBLE;
    if (it.flip_normals) f |= RR_IF_FLIP_NORMALS;
    if (cache.alpha > 0.0f) f |= RR_IF_CACHE_ALPHA_POS;
    if (cache.cast_shadow) f |= RR_IF_CACHE_CAST_SHADOW;
    if (cache.reflection_only) f |= RR_IF_CACHE_REFL_ONLY;
    if (!(cache.alpha < 1.0f) && cache.backface_cullig) f |= RR_IF_SOLID_BASE; // the cache never has textures
    if (full.texture[RR_TEX_ALPHA] >= 0 && tex_width[full.texture[RR_TEX_ALPHA]] > 0) f |= RR_IF_OCCLUDER_ALPHA_TEX;
    if (it.kind == RR_ITEM_SPHERE) f |= RR_IF_SPHERE | RR_IF_UV_MAY_BE_NAN;
    else {
        if (cache.smooth_shading && it.mesh_has_normals) f |= RR_IF_SMOOTH;
        if (it.mesh_degenerate) f |= RR_IF_UV_MAY_BE_NAN;
    }
    return f;
}

// Light (reference src/scene.rs:40-51) -> device record.  Disabled lights keep their slot: the slot is the RNG stream of their shadow jitter.
static DLight make_dlight(const rr_light& l) {
    DLight d;
    memset(&d, 0, sizeof d);
    for (int k = 0; k < 3; k++) { d.pos[k] = l.pos[k]; d.dir[k] = l.dir[k]; d.color[k] = l.color[k]; }
    d.intensity = l.intensity; d.max_angle = l.max_angle;
    d.type = l.light_type | (l.enabled ? 0u : 0x80u);
    return d;
}
// the whole list, in the caller's order; *n_enabled: how many of them shine
static std::vector<DLight> make_dlights(const rr_light* lights, uint32_t n, uint32_t* n_enabled) {
    std::vector<DLight> dl(n);
    *n_enabled = 0;
    for (uint32_t i = 0; i < n; i++) {
        dl[i] = make_dlight(lights[i]);
        if (lights[i].enabled) ++*n_enabled;
    }
    return dl;
}

static void fill_item_matrices(DItem& d, const float* trans, const float* inv) {
    // rows of the column-major matrices
    d.inv0 = make_float4(inv[0], inv[4], inv[8], inv[12]);
    d.inv1 = make_float4(inv[1], inv[5], inv[9], inv[13]);
    d.inv2 = make_float4(inv[2], inv[6], inv[10], inv[14]);
    d.inv3 = make_float4(inv[3], inv[7], inv[11], inv[15]);
    d.tr0 = make_float4(trans[0], trans[4], trans[8], trans[12]);
    d.tr1 = make_float4(trans[1], trans[5], trans[9], trans[13]);
    d.tr2 = make_float4(trans[2], trans[6], trans[10], trans[14]);
}

// Per-triangle constants of the shading (DTri::v1.w, v3), with the IEEE binary32 sequence of rr_math.h's cross3 / dot3 / norm3 /
// normalize3 as k_shade evaluated them per hit (the library is built without contraction and without fast-math on the host side too;
// sqrtf and the division are correctly rounded on both; tests/test_gpu_math.py compares the two builds bit for bit):
//   area = norm3(cross3(a - b, a - c))            Mesh::get_normal / get_uv, src/shape/mesh.rs:127-143 (area_weights)
//   ng   = normalize3(cross3(b - a, c - a))       the triangle's own normal, src/shape/mesh.rs:76-98
static void tri_shading_constants(const float* a, const float* b, const float* c, float* ng, float* area) {
    auto cross = [](const float* u, const float* v, float* r) {
        r[0] = u[1] * v[2] - u[2] * v[1]; r[1] = u[2] * v[0] - u[0] * v[2]; r[2] = u[0] * v[1] - u[1] * v[0];
    };
    auto norm = [](const float* u) { return sqrtf((u[0] * u[0] + u[1] * u[1]) + u[2] * u[2]); };
    const float amb[3] = {a[0] - b[0], a[1] - b[1], a[2] - b[2]}, amc[3] = {a[0] - c[0], a[1] - c[1], a[2] - c[2]};
    float x[3];
    cross(amb, amc, x);
    *area = norm(x);
    const float bma[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]}, cma[3] = {c[0] - a[0], c[1] - a[1], c[2] - a[2]};
    cross(bma, cma, x);
    const float n = norm(x);
    ng[0] = x[0] / n; ng[1] = x[1] / n; ng[2] = x[2] / n;
}

// ---------------------------------------------------------------------------
// scene records: what rr_scene_create builds before its first upload
// ---------------------------------------------------------------------------
// The binary trees of the meshes are independent: built by a few host threads (a scene of 194 meshes / 559 k triangles:
// 0.4 s on one core).  The workers pull mesh indices from one counter, so threads that could not be started only mean
// fewer hands; an exception in any worker (the builder's vectors are sized by the caller's meshes) is rethrown here.
static void build_mesh_trees(const rr_mesh* meshes, uint32_t n_meshes, int depth_limit, std::vector<rr::BvhResult>* built, std::vector<char>* built_ok) {
    std::atomic<uint32_t> next_mesh{0};
    auto worker = [&]() {
        for (;;) {
            const uint32_t mi = next_mesh.fetch_add(1);
            if (mi >= n_meshes) break;
            RR_FAULT_POINT("scene_create.mesh_worker");
            const rr_mesh& m = meshes[mi];
            const uint32_t nt = m.n_triangles;
            std::vector<float> lo(3 * (size_t)nt), hi(3 * (size_t)nt);
            for (uint32_t f = 0; f < nt; f++)
                for (int k = 0; k < 3; k++) {
                    float a = m.positions[3 * (size_t)m.indices[3 * (size_t)f] + k];
                    float b = m.positions[3 * (size_t)m.indices[3 * (size_t)f + 1] + k];
                    float c = m.positions[3 * (size_t)m.indices[3 * (size_t)f + 2] + k];
                    lo[3 * (size_t)f + k] = std::min(a, std::min(b, c));
                    hi[3 * (size_t)f + k] = std::max(a, std::max(b, c));
                }
            (*built_ok)[mi] = rr::build_bvh(lo.data(), hi.data(), nt, RR_MAX_LEAF_TRIS, depth_limit, &(*built)[mi]) ? 1 : 0;
        }
    };
    const unsigned hw = std::thread::hardware_concurrency();
    const uint32_t n_threads = std::min<uint32_t>(std::min<uint32_t>(hw ? hw : 4u, 16u), std::max<uint32_t>(n_meshes, 1u));
    Workers pool;
    for (uint32_t t = 1; t < n_threads; t++)
        if (!pool.spawn(worker)) break;
    pool.run(worker);
    pool.join_and_rethrow();
}
static void build_mesh_trees(const rr_flat_scene* fs, int depth_limit, std::vector<rr::BvhResult>* built, std::vector<char>* built_ok) {
    build_mesh_trees(fs->meshes, fs->n_meshes, depth_limit, built, built_ok);
}

// ---- shares of the traversal stack (RR_STACK_DEPTH entries per lane): a top level over n items never needs more
// than n - 1 pending entries, so a scene of few items leaves more levels to its per-mesh trees (a 320 k-triangle
// mesh traces 3 % faster with 30 levels than with 24, and 7 % slower with 20)
// More than 2^RR_TLAS_MAX_DEPTH items (the reference has no limit: `items: Vec<..>`, src/scene.rs:69-83): the top level takes the
// levels it needs -- ceil(log2 n): the builder falls back to object-median splits where the budget gets tight -- out of the
// per-mesh trees' share, down to 16 levels for those (8 * 2^16 triangles per mesh at worst); RR_MAX_ITEMS = 2^20 is where that ends.
// The share depends on the item count alone and changes with it only below 14 and above 2^RR_TLAS_MAX_DEPTH items: an edit of the
// item list (rr_scene_set_items) that changes it rebuilds the per-mesh trees, which are built and collapsed for their share.
static int stack_shares(uint32_t n_items, int* tlas_depth_limit, int* blas_depth_limit) {
    *tlas_depth_limit = (int)std::min<uint32_t>(RR_TLAS_MAX_DEPTH, std::max<uint32_t>(1u, n_items > 1 ? n_items - 1 : 1u));
    if (n_items > (1u << RR_TLAS_MAX_DEPTH)) {
        if (n_items > RR_MAX_ITEMS) return fail(RR_ERR_UNSUPPORTED, "%u items (RR_MAX_ITEMS = %u)", n_items, RR_MAX_ITEMS);
        int need = RR_TLAS_MAX_DEPTH;
        while ((1u << need) < n_items) need++;
        *tlas_depth_limit = need;
    }
    *blas_depth_limit = RR_STACK_DEPTH - 3 - *tlas_depth_limit;
    return RR_OK;
}

// What an item takes from the mesh it names: where the mesh's records sit in the arenas, and what its flag word needs.
struct MeshDev { uint32_t tri_base, n_tris; uint32_t node_base4; int32_t root4; bool has_normals, degenerate; };

// The meshes' records, one mesh after the other.  A mesh's triangle records start at tri_base (all of tris, trix, attrs and
// face_slot) and its nodes at node_base4; everything inside a mesh's records is relative to those two, so appending meshes leaves
// the records of the meshes before them as they are.  tris_before / nodes4_before: records that precede the vectors' first element
// (rr_scene_add_meshes builds the records of the new meshes alone, behind those resident on the device).
struct MeshArenas {
    std::vector<DNode4> nodes4;     // the meshes' trees, one after the other
    std::vector<DTri> tris;         // per mesh triangle, in leaf order: what k_shade reads
    std::vector<DTriX> trix;        // ... what the triangle test reads
    std::vector<DTriAttr> attrs;    // ... its normals and uvs
    std::vector<uint32_t> face_slot; // per mesh triangle: original face index -> leaf-order slot (the way back: the bits of DTri::v0.w)
    std::vector<MeshDev> meshes;    // per mesh
    size_t tris_before = 0, nodes4_before = 0;
};

// A scene's own copy of a checked mesh (the caller's arrays are only borrowed for the call): what the per-mesh trees are rebuilt
// from when an edit of the item list changes their share of the traversal stack.
struct HostMesh {
    std::vector<float> positions, uvs, normals;
    std::vector<uint32_t> indices, uv_indices, normal_indices;
    explicit HostMesh(const rr_mesh& m)
        : positions(m.positions, m.positions + 3 * (size_t)m.n_vertices), uvs(m.uvs, m.uvs + 2 * (size_t)m.n_uvs), normals(m.normals, m.normals + 3 * (size_t)m.n_normals),
          indices(m.indices, m.indices + 3 * (size_t)m.n_triangles), uv_indices(m.uv_indices, m.uv_indices + 3 * (size_t)m.n_uv_faces),
          normal_indices(m.normal_indices, m.normal_indices + 3 * (size_t)m.n_normal_faces) {}
    rr_mesh view() const {
        rr_mesh m;
        memset(&m, 0, sizeof m);
        m.positions = positions.data(); m.indices = indices.data(); m.uvs = uvs.data(); m.uv_indices = uv_indices.data();
        m.normals = normals.data(); m.normal_indices = normal_indices.data();
        m.n_vertices = (uint32_t)(positions.size() / 3); m.n_triangles = (uint32_t)(indices.size() / 3); m.n_uvs = (uint32_t)(uvs.size() / 2);
        m.n_uv_faces = (uint32_t)(uv_indices.size() / 3); m.n_normals = (uint32_t)(normals.size() / 3); m.n_normal_faces = (uint32_t)(normal_indices.size() / 3);
        return m;
    }
};

// Appends the records of `n` checked meshes (check_meshes) to the arenas: one BLAS per mesh, shared by every item that names it;
// the binary trees are built by a few threads for `blas_depth_limit` levels, then collapsed and laid out one after the other.
// `n_items`: for the message of a mesh that does not fit.  On failure the arenas are left with a part of the new records.
static int append_mesh_records(const rr_mesh* meshes, uint32_t n, int blas_depth_limit, uint32_t n_items, MeshArenas* arenas) {
    MeshArenas& ar = *arenas;
    const uint32_t first = (uint32_t)ar.meshes.size();
    std::vector<rr::BvhResult> built(n);
    std::vector<char> built_ok(n, 0);
    build_mesh_trees(meshes, n, blas_depth_limit, &built, &built_ok);
    for (uint32_t k = 0; k < n; k++) {
        const rr_mesh& m = meshes[k];
        const uint32_t mi = first + k;
        uint32_t nt = m.n_triangles;
        if (!built_ok[k]) return fail(RR_ERR_UNSUPPORTED, "mesh %u: %u triangles need a deeper tree than the %d levels left beside a top level over %u items",
                                      mi, nt, blas_depth_limit, n_items);
        rr::BvhResult& r = built[k];
        MeshDev md;
        md.tri_base = (uint32_t)(ar.tris_before + ar.tris.size());
        md.n_tris = nt;
        md.has_normals = m.n_normals > 0 && m.n_normal_faces > 0;
        md.degenerate = false;
        {
            int pending = 0;
            md.node_base4 = (uint32_t)(ar.nodes4_before + ar.nodes4.size());
            md.root4 = rr::collapse_bvh4(r, blas_depth_limit, true, &ar.nodes4, &pending);
            if (pending > blas_depth_limit) return fail(RR_ERR_UNSUPPORTED, "mesh %u: BVH4 stack bound exceeded", mi);
        }
        size_t fs_base = ar.face_slot.size();
        ar.face_slot.resize(fs_base + nt);
        for (uint32_t slot = 0; slot < nt; slot++) {
            uint32_t f = r.order[slot];
            ar.face_slot[fs_base + f] = slot;
            const uint32_t* ix = m.indices + 3 * (size_t)f;
            const float *a = m.positions + 3 * (size_t)ix[0], *b = m.positions + 3 * (size_t)ix[1], *c = m.positions + 3 * (size_t)ix[2];
            {   // Mesh::get_uv divides by the triangle's area (src/shape/mesh.rs:127-143): a zero (or non-finite) area makes the uv of ANY point
                // on that face non-finite.  Judged in double with a generous margin: a false positive only costs shadow rays that a
                // zero light term would have skipped (k_shade, want_shadow)
                const double u[3] = {(double)a[0] - b[0], (double)a[1] - b[1], (double)a[2] - b[2]}, v[3] = {(double)a[0] - c[0], (double)a[1] - c[1], (double)a[2] - c[2]};
                const double cx = u[1] * v[2] - u[2] * v[1], cy = u[2] * v[0] - u[0] * v[2], cz = u[0] * v[1] - u[1] * v[0];
                const double area2 = cx * cx + cy * cy + cz * cz, scale2 = (u[0] * u[0] + u[1] * u[1] + u[2] * u[2]) * (v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
                if (!(area2 > 1e-10 * scale2) || !(area2 > 1e-24) || !std::isfinite(area2)) md.degenerate = true;
            }
            DTri t;
            float fbits; memcpy(&fbits, &f, 4);
            float ng[3], area;
            tri_shading_constants(a, b, c, ng, &area);
            t.v0 = make_float4(a[0], a[1], a[2], fbits);
            t.v1 = make_float4(b[0], b[1], b[2], area);
            t.v2 = make_float4(c[0], c[1], c[2], 0.0f);
            t.v3 = make_float4(ng[0], ng[1], ng[2], 0.0f);
            ar.tris.push_back(t);
            {   // the edge vectors parry's test evaluates per ray: ab = b - a, ac = c - a
                const float ab[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]}, ac[3] = {c[0] - a[0], c[1] - a[1], c[2] - a[2]};
                DTriX x;
                x.t0 = t.v0;
                x.t1 = make_float4(ab[0], ab[1], ab[2], ac[0]);
                x.t2 = make_float4(ac[1], ac[2], 0.0f, 0.0f);
                ar.trix.push_back(x);
            }
            DTriAttr at;
            float n[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}}, uv[3][2] = {{0, 0}, {0, 0}, {0, 0}};
            if (md.has_normals)
                for (int v = 0; v < 3; v++)
                    for (int k = 0; k < 3; k++) n[v][k] = m.normals[3 * (size_t)m.normal_indices[3 * (size_t)f + v] + k];
            uint32_t flags = 0;
            if (f < m.n_uv_faces) { // Mesh::get_uv bounds test, reference src/shape/mesh.rs:116
                flags |= 1u;
                for (int v = 0; v < 3; v++)
                    for (int k = 0; k < 2; k++) uv[v][k] = m.uvs[2 * (size_t)m.uv_indices[3 * (size_t)f + v] + k];
            }
            float flb; memcpy(&flb, &flags, 4);
            at.s0 = make_float4(n[0][0], n[0][1], n[0][2], uv[0][0]);
            at.s1 = make_float4(n[1][0], n[1][1], n[1][2], uv[0][1]);
            at.s2 = make_float4(n[2][0], n[2][1], n[2][2], uv[1][0]);
            at.s3 = make_float4(uv[1][1], uv[2][0], uv[2][1], flb);
            ar.attrs.push_back(at);
        }
        ar.meshes.push_back(md);
    }
    static_assert(sizeof(DTriX) == 48 && sizeof(DNode4) == 128 && sizeof(DMaterial) == 240, "layouts the kernels address by byte offset");
    if (ar.nodes4_before + ar.nodes4.size() >= (1u << 25)) return fail(RR_ERR_UNSUPPORTED, "%zu BVH4 nodes (nodes are addressed with 32-bit byte offsets)", ar.nodes4_before + ar.nodes4.size());
    if (ar.tris_before + ar.trix.size() >= (1u << 26)) return fail(RR_ERR_UNSUPPORTED, "%zu triangles (addressed with 32-bit byte offsets)", ar.tris_before + ar.trix.size());
    return RR_OK;
}

// What depends on the item list: the item records in list order, with their share of the flat-normal arena (wn_base, assigned in
// item order), what their flag words are rebuilt from, and the two hints of the view.
struct ItemRecords {
    std::vector<DItem> items;
    std::vector<ItemHost> item_host;
    uint64_t n_flat_normals = 0;    // entries of DSceneView::flat_normals: two per instanced triangle
    bool general_w = false;         // some item's inverse is not affine
    bool any_alpha_occluder = false;
};
// The records of a checked item list (check_items) over the meshes of `mesh_table`, with the materials the items name.
static int build_item_records(const rr_item* items, uint32_t n_items, const rr_material* materials, const std::vector<MeshDev>& mesh_table,
                              const std::vector<uint32_t>& tex_width, ItemRecords* out) {
    ItemRecords& s = *out;
    s = ItemRecords();
    s.items.resize(n_items);
    s.item_host.resize(n_items);
    for (uint32_t i = 0; i < n_items; i++) {
        const rr_item& it = items[i];
        DItem& d = s.items[i];
        memset(&d, 0, sizeof d);
        fill_item_matrices(d, it.trans, it.trans_inv);
        if (!affine_inverse(d.inv3)) s.general_w = true;
        for (int k = 0; k < 3; k++) { d.bmin[k] = it.bbox_min[k]; d.bmax[k] = it.bbox_max[k]; }
        d.radius = it.radius;
        d.id = it.id;
        d.material = it.material;
        ItemHost& ih = s.item_host[i];
        ih = ItemHost{it.kind, it.material, it.material_cache, it.visible != 0, it.flip_normals != 0, false, false, it.kind != RR_ITEM_SPHERE ? (int32_t)it.mesh : -1};
        if (it.kind != RR_ITEM_SPHERE) {
            const MeshDev& m = mesh_table[it.mesh];
            d.tri_base = m.tri_base; d.n_tris = m.n_tris;
            d.node_base4 = m.node_base4; d.root4 = m.root4;
            if (s.n_flat_normals + 2ull * m.n_tris > 0xffffffffull) return fail(RR_ERR_UNSUPPORTED, "more than 2^31 instanced triangles");
            d.wn_base = (uint32_t)s.n_flat_normals; s.n_flat_normals += 2ull * m.n_tris;
            ih.mesh_has_normals = m.has_normals; ih.mesh_degenerate = m.degenerate;
        }
        d.flags = item_flags(ih, materials[it.material_cache], materials[it.material], tex_width);
        if (d.flags & RR_IF_OCCLUDER_ALPHA_TEX) s.any_alpha_occluder = true;
    }
    return RR_OK;
}

// Which items of an edited list keep the derived data -- flat world normals, surface spans -- of an item of the list before: those
// whose matrices, mesh records and flag word are bit for bit what an old item had (both derive from exactly these; the flag word
// says ball or mesh).  keep_from[i] = the index of such an old item (the first, where several are alike), or -1 = derive anew.
static void plan_item_reuse(const std::vector<DItem>& old_items, const std::vector<DItem>& new_items, std::vector<int32_t>* keep_from) {
    struct Key {
        float4 m[7]; uint32_t tri_base, n_tris, flags, zero;
        bool operator<(const Key& o) const { return memcmp(this, &o, sizeof(Key)) < 0; }
    };
    static_assert(sizeof(Key) == 7 * 16 + 16, "no padding: keys are compared as bytes");
    auto key_of = [](const DItem& d) {
        Key k;
        k.m[0] = d.inv0; k.m[1] = d.inv1; k.m[2] = d.inv2; k.m[3] = d.inv3; k.m[4] = d.tr0; k.m[5] = d.tr1; k.m[6] = d.tr2;
        k.tri_base = d.tri_base; k.n_tris = d.n_tris; k.flags = d.flags; k.zero = 0u;
        return k;
    };
    std::vector<std::pair<Key, int32_t>> olds(old_items.size());
    for (size_t i = 0; i < old_items.size(); i++) olds[i] = std::make_pair(key_of(old_items[i]), (int32_t)i);
    std::sort(olds.begin(), olds.end());
    keep_from->assign(new_items.size(), -1);
    for (size_t i = 0; i < new_items.size(); i++) {
        const Key k = key_of(new_items[i]);
        auto it = std::lower_bound(olds.begin(), olds.end(), std::make_pair(k, (int32_t)-1));
        if (it != olds.end() && memcmp(&it->first, &k, sizeof(Key)) == 0) (*keep_from)[i] = it->second;
    }
}

// The size of DSceneView::flat_normals for `n_entries` entries (ItemRecords::n_flat_normals: at most 2^32): RR_FLAT_ENTRY_F4 float4 each --
// normal, tangent, bitangent --, and an empty table still gets a buffer.
inline size_t flat_normals_bytes(uint64_t n_entries) { return std::max<size_t>((size_t)n_entries * RR_FLAT_ENTRY_F4 * sizeof(float4), sizeof(float4)); }

// The chunk map of an item list: (item, first triangle) per workgroup of k_world_normals / k_item_spans, RR_HOST_ITEM_CHUNK triangles
// each; every item has at least one chunk, and the chunks of one item are consecutive.
#define RR_HOST_ITEM_CHUNK 8192u // = RR_ITEM_CHUNK of rr_kernels.hip (rr_api_scene.h asserts it)
static void item_chunk_map(const std::vector<DItem>& items, std::vector<uint2>* chunks, std::vector<uint32_t>* chunk_item) {
    chunks->clear(); chunk_item->clear();
    for (uint32_t i = 0; i < (uint32_t)items.size(); i++) {
        const uint32_t nt = (items[i].flags & RR_IF_SPHERE) ? 0u : items[i].n_tris;
        for (uint32_t first = 0; first == 0u || first < nt; first += RR_HOST_ITEM_CHUNK) { chunks->push_back(make_uint2(i, first)); chunk_item->push_back(i); }
    }
}

struct SceneRecords : MeshArenas, ItemRecords {
    int tlas_depth_limit = RR_TLAS_MAX_DEPTH, blas_depth_limit = RR_BLAS_MAX_DEPTH; // shares of the traversal stack (stack_shares)
    std::vector<DMaterial> dmat;
    std::vector<DLight> dlights;
    uint32_t n_enabled_lights = 0;
    std::vector<DTexture> dtex;     // where each image sits in the RGBA8 pool
    std::vector<uint32_t> tex_width;
};

// The records of a validated scene (validate_scene).
static int build_scene_records(const rr_flat_scene* fs, SceneRecords* out) {
    SceneRecords& s = *out;
    s = SceneRecords();
    append_texture_layout(fs->textures, fs->n_textures, &s.dtex, &s.tex_width);
    s.dmat.resize(fs->n_materials);
    for (uint32_t i = 0; i < fs->n_materials; i++) s.dmat[i] = make_dmaterial(fs->materials[i], s.tex_width, s.dtex);
    s.dlights = make_dlights(fs->lights, fs->n_lights, &s.n_enabled_lights);
    int rc = stack_shares(fs->n_items, &s.tlas_depth_limit, &s.blas_depth_limit);
    if (rc == RR_OK) rc = append_mesh_records(fs->meshes, fs->n_meshes, s.blas_depth_limit, fs->n_items, &s);
    if (rc != RR_OK) return rc;
    ItemRecords ir;
    rc = build_item_records(fs->items, fs->n_items, fs->materials, s.meshes, s.tex_width, &ir);
    static_cast<ItemRecords&>(s) = std::move(ir);
    return rc;
}

// ---------------------------------------------------------------------------
// top level: world boxes over the items
// ---------------------------------------------------------------------------
// The reference has no world-space test: a ray is moved into an item's space with the item's f32 inverse matrix and
// tested there against the local box (Shape::intersect_b_box, src/shape/mod.rs:80-105).  The top-level tree may only
// skip an item if that local test would fail, so an item's world box is the exact box of its transformed local corners
// (Bounded::aabb, src/shape/mod.rs:48-78; in double) grown by a bound on how far the f32 local ray can sit from the
// true one, mapped back to world space.  With M, N the given matrix and inverse, t, t' their translations, u = 2^-24,
// and origins with |o_c| <= reach_c:  the local ray is  N o + t' + do,  N d + dd  with  |do| <= g (|N| |o| + |t'|),
// |dd| <= g |N| |d|  (g = 16 u covers the four-term dot products and the local slab test's own rounding), so a point of
// it maps to the world point  (o + s d) + [E o + e + M do] + s [E d + M dd],  E = M N - I,  e = M t' + t  (N is an f32
// inverse: E is of the order u cond(M)).  s |d| is at most reach + the box's own extent, which bounds the last term.
// Far from the origin, or with a badly conditioned transform, this is orders of magnitude more than float spacing
// (tools/fuzz_parity.py far: a sheared sphere 1e5 away needs 15 units on a 10-unit box); on ordinary scenes it is
// ~1e-6 of the scene size.  An inverse with a projective bottom row gets an unbounded box (always a candidate).
//
// Tighter than the corners, for meshes: a mesh only ever contributes through a triangle its own tree lets the ray reach (a candidate
// whose box is hit and whose triangles are missed changes nothing: src/raytracing.rs:471-487 looks at `intersect`'s result only),
// and the walks of rr_kernels.hip test a triangle only under a leaf box that the local ray passes -- boxes of the mesh's own
// vertices, padded by 4e-6 of their coordinates (rr_bvh.cpp).  So whatever the triangle test then reports, NaN included, it
// reports for a ray that passes the padded box of the mesh's VERTICES; in world space that is the box of the transformed
// vertices, which for a rotated item is much smaller than the box of the rotated local box (a unit cube turned by 45 degrees
// about two axes: 1.7 x per axis).  The world box is the intersection of the two, grown by the leaf padding mapped to world
// space; the padding of padded_world_box (how far the f32 local ray sits from the true one) applies as before.
// NOT for balls: ray_ball has no box in front of it, and where its arithmetic overflows (a tiny ball: local coordinates
// ~1e12) it answers Some(NaN) for ANY ray that passes the local box -- tests/golden/fuzz_568 holds such a scene -- so a ball
// keeps the box of its local box's corners.  Not for a mesh whose tree is a single leaf either (nothing is culled in front of
// its triangles).  The extent of the vertices along the transform's rows comes from the device (k_item_spans), where the triangles live.
struct WorldBox { double lo[3], hi[3]; bool tight[3]; double ext[3]; }; // tight[r]: axis r comes from the vertices; ext: largest |local coordinate| per local axis
// `span`: the 9 doubles k_item_spans wrote for this item (extent of the mesh's vertices along the transform's rows), or NULL = corners only
static WorldBox exact_world_box(const DItem& it, const double* span) {
    WorldBox b;
    const float4 rows[3] = {it.tr0, it.tr1, it.tr2};
    for (int r = 0; r < 3; r++) { b.lo[r] = 1e300; b.hi[r] = -1e300; b.tight[r] = false; b.ext[r] = 0.0; }
    for (int c = 0; c < 8; c++) {
        const double p[3] = {(c & 1) ? it.bmax[0] : it.bmin[0], (c & 2) ? it.bmax[1] : it.bmin[1], (c & 4) ? it.bmax[2] : it.bmin[2]};
        for (int r = 0; r < 3; r++) {
            const double v = (double)rows[r].x * p[0] + (double)rows[r].y * p[1] + (double)rows[r].z * p[2] + (double)rows[r].w;
            b.lo[r] = std::min(b.lo[r], v); b.hi[r] = std::max(b.hi[r], v);
        }
    }
    if (!(it.flags & RR_IF_SPHERE) && it.root4 >= 0 && span) {
        bool finite = true;
        for (int k = 0; k < 9; k++) finite = finite && std::isfinite(span[k]);
        if (finite) {
            for (int c = 0; c < 3; c++) b.ext[c] = span[6 + c]; // what the leaf padding is relative to
            for (int r = 0; r < 3; r++) {
                const double mx = rows[r].x, my = rows[r].y, mz = rows[r].z;
                const double leaf_pad = 2.0e-5 * (std::fabs(mx) * b.ext[0] + std::fabs(my) * b.ext[1] + std::fabs(mz) * b.ext[2]) + 1e-30;
                const double tlo = span[r] + (double)rows[r].w - leaf_pad, thi = span[3 + r] + (double)rows[r].w + leaf_pad;
                if (std::isfinite(tlo) && std::isfinite(thi) && tlo <= thi && (tlo > b.lo[r] || thi < b.hi[r])) { b.lo[r] = std::max(b.lo[r], tlo); b.hi[r] = std::min(b.hi[r], thi); b.tight[r] = true; }
            }
        }
    }
    return b;
}
static void padded_world_box(const DItem& it, const WorldBox& b, const double reach[3], float* lo, float* hi) {
    const double M[3][4] = {{it.tr0.x, it.tr0.y, it.tr0.z, it.tr0.w}, {it.tr1.x, it.tr1.y, it.tr1.z, it.tr1.w}, {it.tr2.x, it.tr2.y, it.tr2.z, it.tr2.w}};
    const double N[3][4] = {{it.inv0.x, it.inv0.y, it.inv0.z, it.inv0.w}, {it.inv1.x, it.inv1.y, it.inv1.z, it.inv1.w}, {it.inv2.x, it.inv2.y, it.inv2.z, it.inv2.w}};
    const bool affine = affine_inverse(it.inv3);
    const double g = 16.0 / 16777216.0;
    for (int r = 0; r < 3; r++) {
        double pad = 0.0;
        for (int c = 0; c < 3; c++) {
            double e = (r == c) ? -1.0 : 0.0, a = 0.0;
            for (int k = 0; k < 3; k++) { e += M[r][k] * N[k][c]; a += std::fabs(M[r][k]) * std::fabs(N[k][c]); }
            const double extent = std::max(std::fabs(b.lo[c]), std::fabs(b.hi[c]));
            pad += (std::fabs(e) + g * a) * (2.0 * reach[c] + extent);
        }
        double et = M[r][3], at = 0.0;
        for (int k = 0; k < 3; k++) { et += M[r][k] * N[k][3]; at += std::fabs(M[r][k]) * std::fabs(N[k][3]); }
        pad += std::fabs(et) + g * at;
        if (b.tight[r]) {
            // a leaf's slab test lets a ray through whose entry and exit distances differ by up to 8e-6 of themselves (RR_CHILD): planes moved
            // by that share of the way travelled along a local axis, which is at most the local reach plus the mesh's own extent
            for (int c = 0; c < 3; c++) {
                double way = std::fabs(N[c][3]) + b.ext[c];
                for (int k = 0; k < 3; k++) way += std::fabs(N[c][k]) * 2.0 * reach[k];
                pad += std::fabs(M[r][c]) * 1.0e-5 * way;
            }
        }
        pad = 2.0 * pad + 1e-6 * std::max(std::fabs(b.lo[r]), std::fabs(b.hi[r])) + 1e-30; // + float rounding of the box and of the walk's plane distances
        lo[r] = (float)(b.lo[r] - pad); hi[r] = (float)(b.hi[r] + pad);
        if (!affine || !std::isfinite(lo[r]) || lo[r] < -3.0e38f) lo[r] = -3.0e38f;
        if (!affine || !std::isfinite(hi[r]) || hi[r] > 3.0e38f) hi[r] = 3.0e38f;
    }
}

// One top-level tree over the items' boxes lo / hi (n * 3 floats): binned SAH, one item per leaf, collapsed to 4-wide nodes.
static int tlas_tree(const std::vector<DItem>& items, int depth_limit, const float* lo, const float* hi, uint32_t n, std::vector<DNode4>* tlas4, int32_t* root4) {
    tlas4->clear();
    rr::BvhResult r;
    if (!rr::build_bvh(lo, hi, n, 1, depth_limit, &r))
        return fail(RR_ERR_UNSUPPORTED, "internal: top level over %u items does not fit %d levels", n, depth_limit);
    // leaves must name item indices directly: leaf order is a permutation, so re-code each 1-item leaf
    for (DNode& nd : r.nodes) {
        int32_t c[2];
        memcpy(&c[0], &nd.n3.x, 4); memcpy(&c[1], &nd.n3.y, 4);
        for (int k = 0; k < 2; k++)
            if (c[k] < 0) { uint32_t first = RR_LEAF_FIRST(~c[k]); c[k] = ~(int32_t)r.order[first]; }
        memcpy(&nd.n3.x, &c[0], 4); memcpy(&nd.n3.y, &c[1], 4);
    }
    if (r.root < 0) r.root = ~(int32_t)r.order[RR_LEAF_FIRST(~r.root)];
    // the form the kernels walk: collapsed to 4-wide nodes within the top level's share of the traversal stack
    int pending = 0;
    *root4 = rr::collapse_bvh4(r, depth_limit, false, tlas4, &pending);
    if (pending > depth_limit) return fail(RR_ERR_UNSUPPORTED, "top level: BVH4 stack bound exceeded");
    // Balls before meshes among the children of a node.  A walk takes the children of a node nearest box first and, at equal entry
    // distance, in slot order -- and equal is the rule where it matters: a ray that starts inside an environment sphere AND inside an
    // object's box (every secondary ray of such a scene) enters both at distance 0.  A ball is decided by a dozen instructions and
    // its toi then bounds the mesh walk that follows (closest_item passes the best hit so far down); the other way round the mesh is
    // walked without a bound first.  helmet_syn's secondary rays all end on its solid environment sphere at toi 0: with the sphere
    // in front, the walk of the 80 k-triangle mesh ends at its root.  The candidate SET and the result do not depend on the order.
    for (DNode4& nd : *tlas4) {
        int32_t code[4];
        memcpy(code, &nd.q[6], 16);
        auto is_ball = [&](int k) { return code[k] < 0 && code[k] != (int32_t)0x80000000 && (items[RR_LEAF_FIRST((uint32_t)~code[k])].flags & RR_IF_SPHERE) != 0u; };
        int order[4], m = 0;
        for (int k = 0; k < 4; k++) if (is_ball(k)) order[m++] = k;
        if (m == 0) continue;
        for (int k = 0; k < 4; k++) if (!is_ball(k) && code[k] != (int32_t)0x80000000) order[m++] = k;
        for (int k = 0; k < 4; k++) if (code[k] == (int32_t)0x80000000) order[m++] = k;
        DNode4 src = nd;
        for (int r = 0; r < 7; r++) {
            const float v[4] = {src.q[r].x, src.q[r].y, src.q[r].z, src.q[r].w};
            nd.q[r] = make_float4(v[order[0]], v[order[1]], v[order[2]], v[order[3]]);
        }
    }
    return RR_OK;
}

// The group records of the packet top level (rr_beam.h has the layout and the rule; rr_trace.h beam_candidates reads them).
// `boxes`: the 4 n float4 of build_tlas (corner boxes, then surface boxes).  Items are sorted by the Morton code of their corner
// box's centre (30 bits over the extent of the finite centres; ties and non-finite centres by item index) and cut into runs of
// 1 << RR_BEAM_GROUP_SHIFT: one membership for both box sets.  A group's box is the float min / max of its members' boxes, so it
// contains them bound by bound; a member bound that is not finite opens that side of the group (-inf / +inf): an infinite
// bound has to, and a NaN bound never constrains the member's own test (fmaxf / fminf drop it), so it must not constrain the
// group's either.  Deterministic: `records` depends on `boxes` alone.  Empty outside 65 .. 512 items.
static void build_item_groups(const std::vector<float4>& boxes, uint32_t n, std::vector<float4>* records) {
    records->clear();
    if (!beam_grouped(n) || boxes.size() != 4 * (size_t)n) return;
    double clo[3] = {INFINITY, INFINITY, INFINITY}, chi[3] = {-INFINITY, -INFINITY, -INFINITY};
    std::vector<double> centre(3 * (size_t)n);
    for (uint32_t i = 0; i < n; i++) {
        const float l[3] = {boxes[2 * (size_t)i].x, boxes[2 * (size_t)i].y, boxes[2 * (size_t)i].z}, h[3] = {boxes[2 * (size_t)i + 1].x, boxes[2 * (size_t)i + 1].y, boxes[2 * (size_t)i + 1].z};
        for (int c = 0; c < 3; c++) {
            const double m = 0.5 * ((double)l[c] + (double)h[c]);
            centre[3 * (size_t)i + c] = m;
            if (std::isfinite(m)) { clo[c] = std::min(clo[c], m); chi[c] = std::max(chi[c], m); }
        }
    }
    std::vector<std::pair<uint32_t, uint32_t>> order(n); // (Morton code, item)
    for (uint32_t i = 0; i < n; i++) {
        uint32_t code = 0;
        for (int c = 0; c < 3; c++) {
            const double m = centre[3 * (size_t)i + c], w = chi[c] - clo[c];
            uint32_t q = 0;
            if (std::isfinite(m) && w > 0.0 && std::isfinite(w)) q = (uint32_t)std::min(1023.0, std::max(0.0, (m - clo[c]) / w * 1024.0));
            for (int b = 0; b < 10; b++) code |= ((q >> b) & 1u) << (3 * b + c);
        }
        order[i] = {code, i};
    }
    std::sort(order.begin(), order.end());
    const uint32_t shift = RR_BEAM_GROUP_SHIFT, g = beam_group_count(n);
    records->resize(beam_group_records(n));
    const float inf = INFINITY;
    for (uint32_t set = 0; set < 2; set++) {
        const float4* src = boxes.data() + 2 * (size_t)n * set;
        float4* members = records->data() + 2 * (size_t)n * set;
        float4* groups = records->data() + 4 * (size_t)n + 2 * (size_t)g * set;
        for (uint32_t k = 0; k < g; k++) { groups[2 * k] = make_float4(inf, inf, inf, 0.0f); groups[2 * k + 1] = make_float4(-inf, -inf, -inf, 0.0f); }
        for (uint32_t slot = 0; slot < n; slot++) {
            const uint32_t item = order[slot].second;
            float4 lo = src[2 * (size_t)item], hi = src[2 * (size_t)item + 1];
            memcpy(&lo.w, &item, 4);
            hi.w = 0.0f;
            members[2 * (size_t)slot] = lo; members[2 * (size_t)slot + 1] = hi;
            float4& glo = groups[2 * (slot >> shift)];
            float4& ghi = groups[2 * (slot >> shift) + 1];
            const float l[3] = {lo.x, lo.y, lo.z}, h[3] = {hi.x, hi.y, hi.z};
            float* gl[3] = {&glo.x, &glo.y, &glo.z};
            float* gh[3] = {&ghi.x, &ghi.y, &ghi.z};
            for (int c = 0; c < 3; c++) {
                *gl[c] = std::isfinite(l[c]) ? std::min(*gl[c], l[c]) : -inf;
                *gh[c] = std::isfinite(h[c]) ? std::max(*gh[c], h[c]) : inf;
            }
        }
    }
}

// Builds the top-level trees over `items` for ray origins within +-want_reach (grown to cover the items themselves: the
// origins of secondary and shadow rays lie on them).  `spans`: 9 doubles per item (exact_world_box), or empty = corner boxes only.
// Writes nothing of a scene: the reach it was built for, the RR_VIEW_NAN_BALLS hint and the item boxes travel in TlasTrees, and
// rr_api_scene.h's upload_tlas keeps them once the device has the trees.  `item_groups` (build_item_groups) follows `item_boxes` in the
// device buffer; it is a vector of its own because the scene keeps the boxes on the host and has no use for the groups there.
struct TlasTrees {
    std::vector<DNode4> corner, surface; int32_t root = (int32_t)0x80000000, root_surface = (int32_t)0x80000000; bool has_surface = false;
    double reach[3] = {0.0, 0.0, 0.0}; bool nan_balls = false; std::vector<float4> item_boxes, item_groups;
};
static int build_tlas(const std::vector<DItem>& items, const std::vector<double>& spans, int depth_limit, const double want_reach[3], TlasTrees* trees) {
    uint32_t n = (uint32_t)items.size();
    *trees = TlasTrees();
    double* reach_c = trees->reach;
    for (int c = 0; c < 3; c++) reach_c[c] = want_reach[c];
    if (n == 0) return RR_OK; // empty scene: every walk ends at once (both roots RR_SENTINEL)
    // two boxes per item: the box of its local box's corners -- what the tree is built over and what shadow packets are tested against:
    // the shadow query orders items by the distance at which the LOCAL box is entered, and prunes by it, which only a world box that
    // contains the local box bounds from below -- and the box of its surface (exact_world_box), which the closest-hit packets use:
    // there an item matters through its nearest hit alone, and that lies in the tighter box
    std::vector<WorldBox> exact(n), surf(n);
    for (uint32_t i = 0; i < n; i++) {
        exact[i] = exact_world_box(items[i], nullptr);
        surf[i] = exact_world_box(items[i], spans.size() == 9 * (size_t)n ? &spans[9 * (size_t)i] : nullptr);
        for (int c = 0; c < 3; c++) {
            const double m = std::max(std::fabs(exact[i].lo[c]), std::fabs(exact[i].hi[c])) * 1.001 + 0.01; // + the shadow bias along the normal
            if (std::isfinite(m)) reach_c[c] = std::max(reach_c[c], m);
        }
    }
    // Can some ball's ray_toi_with_ball overflow (b * b, a * c beyond f32: delta = NaN and the ball answers Some(NaN))?  Judged with six
    // orders of magnitude to spare on the ray directions; a hint for trace_shadow_blockers only (the closest-hit walks detect the NaN itself).
    for (uint32_t i = 0; i < n; i++) {
        const DItem& it = items[i];
        if (!(it.flags & RR_IF_SPHERE)) continue;
        const float4 rows[3] = {it.inv0, it.inv1, it.inv2};
        double nmax = 0.0, tmax = 0.0;
        for (int r = 0; r < 3; r++) {
            nmax = std::max(nmax, std::fabs((double)rows[r].x) + std::fabs((double)rows[r].y) + std::fabs((double)rows[r].z));
            tmax = std::max(tmax, std::fabs((double)rows[r].w));
        }
        const double reach = std::max(reach_c[0], std::max(reach_c[1], reach_c[2]));
        const double on = nmax * reach + tmax, dn = nmax * 1e6, rad = std::fabs((double)it.radius);
        if (!affine_inverse(it.inv3) || !(on * dn < 1e18) || !(rad * dn < 1e18) || !(on < 1e18) || !(rad < 1e18)) trees->nan_balls = true;
    }
    std::vector<float> lo(3 * (size_t)n), hi(3 * (size_t)n);
    std::vector<float4>& boxes = trees->item_boxes;
    boxes.resize(4 * (size_t)n); // [0, 2n): corner boxes (lo, hi); [2n, 4n): surface boxes
    for (uint32_t i = 0; i < n; i++) {
        padded_world_box(items[i], exact[i], reach_c, &lo[3 * (size_t)i], &hi[3 * (size_t)i]);
        boxes[2 * (size_t)i] = make_float4(lo[3 * (size_t)i], lo[3 * (size_t)i + 1], lo[3 * (size_t)i + 2], 0.0f);
        boxes[2 * (size_t)i + 1] = make_float4(hi[3 * (size_t)i], hi[3 * (size_t)i + 1], hi[3 * (size_t)i + 2], 0.0f);
        float tl[3], th[3];
        padded_world_box(items[i], surf[i], reach_c, tl, th);
        boxes[2 * ((size_t)n + i)] = make_float4(tl[0], tl[1], tl[2], 0.0f);
        boxes[2 * ((size_t)n + i) + 1] = make_float4(th[0], th[1], th[2], 0.0f);
    }
    build_item_groups(boxes, n, &trees->item_groups);
    int rc = tlas_tree(items, depth_limit, lo.data(), hi.data(), n, &trees->corner, &trees->root);
    if (rc != RR_OK) return rc;
    // The per-ray closest-hit walks get a tree of their own over the SURFACE boxes (the argument above holds for any closest-hit query: an
    // item matters through its nearest hit alone; until round 4 only the packet form used them): fewer items are set up per ray and fewer
    // mesh walks entered.  Shadow queries keep the tree over the corner boxes (their order is the local boxes' entry distance).
    bool differs = false;
    for (size_t k = 0; k < 2 * (size_t)n && !differs; k++)
        differs = memcmp(&boxes[k], &boxes[2 * (size_t)n + k], sizeof(float4)) != 0;
    trees->has_surface = differs;
    if (differs) {
        for (uint32_t i = 0; i < n; i++) {
            const float4 tl = boxes[2 * ((size_t)n + i)], th = boxes[2 * ((size_t)n + i) + 1];
            lo[3 * (size_t)i] = tl.x; lo[3 * (size_t)i + 1] = tl.y; lo[3 * (size_t)i + 2] = tl.z;
            hi[3 * (size_t)i] = th.x; hi[3 * (size_t)i + 1] = th.y; hi[3 * (size_t)i + 2] = th.z;
        }
        rc = tlas_tree(items, depth_limit, lo.data(), hi.data(), n, &trees->surface, &trees->root_surface);
        if (rc != RR_OK) return rc;
    }
    return RR_OK;
}
