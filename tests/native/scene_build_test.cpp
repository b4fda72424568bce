// Host-only test of rustray_amd/csrc/rr_scene_build.h (built with g++ -fsanitize=address,undefined by tests/test_scene_build.py,
// linked with rr_bvh.cpp and the oracle): the top level's padded boxes against the reference's own candidate test, the surface
// boxes, the shape of the top-level trees, the records of a small scene, and every rejection of the shared checks.
// `scene_build_test --digest` prints an FNV-1a digest of every array the builder makes for two scenes and checks nothing: the
// way to see that a change of the builder that should not change its output does not.
#include <cstdarg>
#include <cstdio>
#include <random>
#include <set>
#include <string>

#include "../../rustray_amd/csrc/rr_scene_build.h"

static std::string g_error;
static int fail(int code, const char* fmt, ...) noexcept {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    try { g_error = buf; } catch (...) { }
    return code;
}
extern "C" int rro_item_box_hit(const rr_item* item, const float* origin, const float* dir); // oracle/oracle.cpp: inverse_ray + the local box test

#define CHECK(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s (last error: %s)\n", __FILE__, __LINE__, #c, g_error.c_str()); return 1; } } while (0)
static const int32_t SENTINEL = (int32_t)0x80000000;
typedef std::mt19937_64 Rng;
static double U(Rng& rng) { return std::uniform_real_distribution<double>(-1.0, 1.0)(rng); }

// ---- scenes ----------------------------------------------------------------------------------------------------------------
// mode 0: ordinary, 1: far from the origin, 2: sheared and scaled up to 1e+-2, 3: both; the inverse is computed in double and rounded
static void random_transform(Rng& rng, int mode, rr_item* item) {
    const double ax = U(rng) * 3.14, ay = U(rng) * 3.14, az = U(rng) * 3.14;
    const double cx = cos(ax), sx = sin(ax), cy = cos(ay), sy = sin(ay), cz = cos(az), sz = sin(az);
    const double R[3][3] = {{cy * cz, -cy * sz, sy}, {sx * sy * cz + cx * sz, -sx * sy * sz + cx * cz, -sx * cy}, {-cx * sy * cz + sx * sz, cx * sy * sz + sx * cz, cx * cy}};
    double sc[3], M[3][4], N[3][4];
    for (int k = 0; k < 3; k++) sc[k] = pow(10.0, (mode >= 2 ? 2.0 : 0.5) * U(rng));
    const double sh = mode >= 2 ? U(rng) * 3 : 0.0, far = (mode == 1 || mode == 3) ? 1e5 : 10.0;
    for (int r = 0; r < 3; r++) { for (int c = 0; c < 3; c++) M[r][c] = R[r][c] * sc[c]; M[r][1] += sh * M[r][0]; }
    for (int r = 0; r < 3; r++) M[r][3] = U(rng) * far;
    const double a = M[0][0], b = M[0][1], c = M[0][2], d = M[1][0], e = M[1][1], f = M[1][2], g = M[2][0], h = M[2][1], i = M[2][2];
    const double det = a * (e * i - f * h) - b * (d * i - f * g) + c * (d * h - e * g);
    const double inv[3][3] = {{(e * i - f * h) / det, (c * h - b * i) / det, (b * f - c * e) / det}, {(f * g - d * i) / det, (a * i - c * g) / det, (c * d - a * f) / det},
                              {(d * h - e * g) / det, (b * g - a * h) / det, (a * e - b * d) / det}};
    for (int x = 0; x < 3; x++) { for (int y = 0; y < 3; y++) N[x][y] = inv[x][y]; N[x][3] = -(inv[x][0] * M[0][3] + inv[x][1] * M[1][3] + inv[x][2] * M[2][3]); }
    memset(item->trans, 0, sizeof item->trans); memset(item->trans_inv, 0, sizeof item->trans_inv);
    for (int r = 0; r < 3; r++) for (int col = 0; col < 4; col++) { item->trans[4 * col + r] = (float)M[r][col]; item->trans_inv[4 * col + r] = (float)N[r][col]; }
    item->trans[15] = 1.0f; item->trans_inv[15] = 1.0f;
}

struct MeshData {
    std::vector<float> pos, uvs, normals;
    std::vector<uint32_t> idx;
    bool attrs = false; // uvs and normals per vertex, indexed like the positions
    rr_mesh view() const {
        rr_mesh m;
        memset(&m, 0, sizeof m);
        m.positions = pos.data(); m.indices = idx.data(); m.n_vertices = (uint32_t)pos.size() / 3; m.n_triangles = (uint32_t)idx.size() / 3;
        if (attrs) {
            m.uvs = uvs.data(); m.uv_indices = idx.data(); m.n_uvs = (uint32_t)uvs.size() / 2; m.n_uv_faces = m.n_triangles;
            m.normals = normals.data(); m.normal_indices = idx.data(); m.n_normals = (uint32_t)normals.size() / 3; m.n_normal_faces = m.n_triangles;
        }
        return m;
    }
};
static MeshData grid_mesh(int grid, int salt, bool attrs) { // grid x grid quads over a bumpy height field (as tests/native/guard_c99.c)
    MeshData m;
    m.attrs = attrs;
    for (int y = 0; y <= grid; y++)
        for (int x = 0; x <= grid; x++) {
            m.pos.insert(m.pos.end(), {(float)x, (float)((x * 7 + y * 13 + salt) % 5) * 0.25f, (float)y});
            m.uvs.insert(m.uvs.end(), {(float)x / grid, (float)y / grid});
            m.normals.insert(m.normals.end(), {0.0f, 1.0f, 0.0f});
        }
    for (int y = 0; y < grid; y++)
        for (int x = 0; x < grid; x++) {
            const uint32_t a = (uint32_t)(y * (grid + 1) + x), b = a + 1u, c = a + (uint32_t)(grid + 1), d = c + 1u;
            m.idx.insert(m.idx.end(), {a, b, c, b, d, c});
        }
    return m;
}
static rr_material plain_material() {
    rr_material m;
    memset(&m, 0, sizeof m);
    for (int k = 0; k < 3; k++) m.base_color[k] = 0.5f;
    m.alpha = 1.0f; m.shininess = 8.0f; m.refraction_index = 1.0f; m.shadow_softness = 0.01f; m.roughness = 0.2f;
    for (int k = 0; k < RR_TEX_COUNT; k++) m.texture[k] = -1;
    m.cast_shadow = m.receive_shadow = m.smooth_shading = m.backface_cullig = 1;
    return m;
}

struct Scene {
    std::vector<MeshData> mesh_data;
    std::vector<rr_mesh> meshes;
    std::vector<rr_item> items;
    std::vector<rr_material> materials;
    std::vector<rr_texture> textures;
    std::vector<rr_light> lights;
    std::vector<uint8_t> pixels = std::vector<uint8_t>(64, 200);
    rr_flat_scene flat() {
        meshes.clear();
        for (const MeshData& m : mesh_data) meshes.push_back(m.view());
        rr_flat_scene fs;
        memset(&fs, 0, sizeof fs);
        fs.abi_version = RR_ABI_VERSION;
        fs.n_items = (uint32_t)items.size(); fs.items = items.data();
        fs.n_meshes = (uint32_t)meshes.size(); fs.meshes = meshes.data();
        fs.n_materials = (uint32_t)materials.size(); fs.materials = materials.data();
        fs.n_textures = (uint32_t)textures.size(); fs.textures = textures.data();
        fs.n_lights = (uint32_t)lights.size(); fs.lights = lights.data();
        return fs;
    }
    // an item of mesh `mesh` (-1: a ball of radius 1) with a random transform; the local box is the box of the mesh's vertices
    void add_item(Rng& rng, int mode, int mesh, int material) {
        rr_item it;
        memset(&it, 0, sizeof it);
        it.kind = mesh < 0 ? RR_ITEM_SPHERE : RR_ITEM_MESH; it.id = (uint32_t)items.size() + 1u; it.material = material; it.material_cache = 0; it.mesh = mesh;
        it.radius = 1.0f; it.visible = 1;
        random_transform(rng, mode, &it);
        for (int k = 0; k < 3; k++) { it.bbox_min[k] = -1.0f; it.bbox_max[k] = 1.0f; }
        if (mesh >= 0) {
            const std::vector<float>& p = mesh_data[mesh].pos;
            for (int k = 0; k < 3; k++) { it.bbox_min[k] = 1e30f; it.bbox_max[k] = -1e30f; }
            for (size_t v = 0; v < p.size(); v++) { it.bbox_min[v % 3] = std::min(it.bbox_min[v % 3], p[v]); it.bbox_max[v % 3] = std::max(it.bbox_max[v % 3], p[v]); }
        }
        items.push_back(it);
    }
};

// meshes: 0 plain grid, 1 grid with uvs and normals, 2 holds a degenerate triangle, 3 a single triangle (its tree is one leaf);
// items: a ball, mesh 0 twice (the second with the alpha-mapped material), meshes 1, 2, 3; two lights, one of them disabled
static Scene hand_made_scene() {
    Scene s;
    Rng rng(11);
    s.mesh_data = {grid_mesh(8, 0, false), grid_mesh(6, 3, true), grid_mesh(4, 1, false), MeshData()};
    s.mesh_data[2].idx.insert(s.mesh_data[2].idx.end(), {0u, 0u, 1u}); // two corners coincide
    s.mesh_data[3].pos = {0, 0, 0, 1, 0, 0, 0, 1, 0}; s.mesh_data[3].idx = {0, 1, 2};
    s.materials = {plain_material(), plain_material()};
    s.materials[1].texture[RR_TEX_ALPHA] = 0; s.materials[1].texture[RR_TEX_BASE] = 1;
    s.textures = {rr_texture{2, 2, s.pixels.data()}, rr_texture{4, 1, s.pixels.data()}};
    const int mesh_of[6] = {-1, 0, 0, 1, 2, 3};
    for (int i = 0; i < 6; i++) s.add_item(rng, 0, mesh_of[i], i == 2 ? 1 : 0);
    rr_light l;
    memset(&l, 0, sizeof l);
    l.pos[1] = 10.0f; l.dir[1] = -1.0f; l.color[0] = l.color[1] = l.color[2] = 1.0f; l.intensity = 1.0f; l.light_type = RR_LIGHT_POINT; l.enabled = 1;
    s.lights = {l, l};
    s.lights[1].enabled = 0; s.lights[1].light_type = RR_LIGHT_SPOT;
    return s;
}
// n_items balls and instances of a dozen grid meshes (a few thousand triangles), of all four transform classes
static Scene random_scene(uint64_t seed, uint32_t n_items) {
    Scene s;
    Rng rng(seed);
    for (int m = 0; m < 12; m++) s.mesh_data.push_back(grid_mesh(6 + m, m, m % 3 == 0));
    s.materials = {plain_material()};
    for (uint32_t i = 0; i < n_items; i++) s.add_item(rng, (int)(i % 4u), i % 5u == 0u ? -1 : (int)(rng() % 12u), 0);
    return s;
}

// what k_item_spans computes on the device: per item the extent of its triangles' vertices along the rows of its transform (without the
// translation), and the largest |coordinate| per local axis; balls and empty meshes: +inf / -inf / 0
static std::vector<double> spans_of(const SceneRecords& r) {
    const double inf = std::numeric_limits<double>::infinity();
    std::vector<double> spans;
    for (const DItem& it : r.items) {
        double lo[3] = {inf, inf, inf}, hi[3] = {-inf, -inf, -inf}, ext[3] = {0, 0, 0};
        const float4 rows[3] = {it.tr0, it.tr1, it.tr2};
        for (uint32_t t = 0; !(it.flags & RR_IF_SPHERE) && t < it.n_tris; t++)
            for (const float4& v : {r.tris[it.tri_base + t].v0, r.tris[it.tri_base + t].v1, r.tris[it.tri_base + t].v2}) {
                const double p[3] = {v.x, v.y, v.z};
                for (int k = 0; k < 3; k++) {
                    const double w = (double)rows[k].x * p[0] + (double)rows[k].y * p[1] + (double)rows[k].z * p[2];
                    lo[k] = std::min(lo[k], w); hi[k] = std::max(hi[k], w); ext[k] = std::max(ext[k], std::fabs(p[k]));
                }
            }
        for (int k = 0; k < 3; k++) spans.push_back(lo[k]);
        for (int k = 0; k < 3; k++) spans.push_back(hi[k]);
        for (int k = 0; k < 3; k++) spans.push_back(ext[k]);
    }
    return spans;
}

// ---- 1. the top level never skips an item the reference would test ---------------------------------------------------------
// Whenever the reference's local test of a ray passes (the ray moved into the item's space with the f32 inverse, against the local box),
// a double-precision slab test of the same ray against the padded corner box passes.  Rays start within the reach the box was padded
// for -- the item's own extent, and a reach grown 3 x -- aim at and around the box (grazing it), and every fifth starts on the item.
static bool slab_hit(const float* o, const float* d, const float* lo, const float* hi) {
    double tmin = 0.0, tmax = 1e300;
    for (int c = 0; c < 3; c++) {
        const double oo = o[c], dd = d[c];
        if (dd == 0.0) { if (oo < lo[c] || oo > hi[c]) return false; continue; }
        double a = (lo[c] - oo) / dd, b = (hi[c] - oo) / dd;
        if (a > b) std::swap(a, b);
        tmin = std::max(tmin, a); tmax = std::min(tmax, b);
    }
    return tmin <= tmax;
}
static int test_padded_boxes_keep_every_candidate() {
    Rng rng(1);
    const long n_items = 12000, rays_per_item = 400;
    long tested = 0, local_hits = 0, misses = 0;
    for (long i = 0; i < n_items; i++) {
        rr_item item;
        memset(&item, 0, sizeof item);
        random_transform(rng, (int)(i % 4), &item);
        for (int k = 0; k < 3; k++) { const double a = U(rng) * 2, b = U(rng) * 2; item.bbox_min[k] = (float)std::min(a, b); item.bbox_max[k] = (float)std::max(a, b); }
        DItem d;
        memset(&d, 0, sizeof d);
        fill_item_matrices(d, item.trans, item.trans_inv);
        for (int k = 0; k < 3; k++) { d.bmin[k] = item.bbox_min[k]; d.bmax[k] = item.bbox_max[k]; }
        d.flags = RR_IF_SPHERE;
        const WorldBox wb = exact_world_box(d, nullptr);
        double reach[3];
        for (int c = 0; c < 3; c++) reach[c] = std::max(std::fabs(wb.lo[c]), std::fabs(wb.hi[c])) * 1.001 + 0.01; // as build_tlas
        if (i % 8 >= 4) for (int c = 0; c < 3; c++) reach[c] *= 3.0; // a camera further out
        float lo[3], hi[3];
        padded_world_box(d, wb, reach, lo, hi);
        for (long k = 0; k < rays_per_item; k++) {
            double o[3], dir[3], tgt[3], len = 0.0;
            for (int c = 0; c < 3; c++) { const double t = U(rng) * 0.5 + 0.5; tgt[c] = wb.lo[c] + (wb.hi[c] - wb.lo[c]) * (t * 1.2 - 0.1); o[c] = U(rng) * reach[c]; }
            if (k % 5 == 0) for (int c = 0; c < 3; c++) o[c] = tgt[c];
            for (int c = 0; c < 3; c++) { dir[c] = (k % 5 == 0) ? U(rng) : tgt[c] - o[c]; len += dir[c] * dir[c]; }
            len = sqrt(len);
            if (!(len > 0.0)) continue;
            float of[3], df[3];
            for (int c = 0; c < 3; c++) { of[c] = (float)o[c]; df[c] = (float)(dir[c] / len); }
            tested++;
            if (!rro_item_box_hit(&item, of, df)) continue;
            local_hits++;
            if (!slab_hit(of, df, lo, hi)) { if (misses++ < 5) std::printf("MISSED item %ld (class %ld) ray %ld\n", i, i % 4, k); }
        }
    }
    std::printf("padded boxes: %ld rays, %ld pass the reference's local test, %ld of those miss the padded box\n", tested, local_hits, misses);
    CHECK(misses == 0);
    CHECK(local_hits >= 1000000); // the property is about rays that reach the items
    return 0;
}

// ---- 2. surface boxes ----------------------------------------------------------------------------------------------------
static int test_surface_boxes() {
    Scene s = random_scene(5, 200);
    rr_flat_scene fs = s.flat();
    SceneRecords r;
    CHECK(validate_scene(&fs) == RR_OK && build_scene_records(&fs, &r) == RR_OK);
    std::vector<double> spans = spans_of(r);
    int tightened = 0;
    for (size_t i = 0; i < r.items.size(); i++) {
        const DItem& it = r.items[i];
        const WorldBox corner = exact_world_box(it, nullptr), surf = exact_world_box(it, &spans[9 * i]);
        for (int c = 0; c < 3; c++) {
            CHECK(surf.lo[c] >= corner.lo[c] && surf.hi[c] <= corner.hi[c] && !corner.tight[c]);
            if (it.flags & RR_IF_SPHERE) CHECK(!surf.tight[c] && surf.lo[c] == corner.lo[c] && surf.hi[c] == corner.hi[c]);
            tightened += surf.tight[c] ? 1 : 0;
        }
        const float4 rows[3] = {it.tr0, it.tr1, it.tr2};
        for (uint32_t t = 0; !(it.flags & RR_IF_SPHERE) && t < it.n_tris; t++)
            for (const float4& v : {r.tris[it.tri_base + t].v0, r.tris[it.tri_base + t].v1, r.tris[it.tri_base + t].v2})
                for (int c = 0; c < 3; c++) {
                    const double w = (double)rows[c].x * v.x + (double)rows[c].y * v.y + (double)rows[c].z * v.z + (double)rows[c].w;
                    CHECK(w >= surf.lo[c] && w <= surf.hi[c]);
                }
    }
    CHECK(tightened > 100); // turned meshes: most axes come from the vertices
    // fall-backs to the corners: a non-finite span, a mesh whose tree is a single leaf; an unbounded box for a projective inverse
    size_t mesh_item = 0;
    while (r.items[mesh_item].flags & RR_IF_SPHERE) mesh_item++;
    DItem it = r.items[mesh_item];
    const WorldBox corner = exact_world_box(it, nullptr);
    double span[9];
    memcpy(span, &spans[9 * mesh_item], sizeof span);
    auto same = [&](const WorldBox& b) { return memcmp(b.lo, corner.lo, sizeof b.lo) == 0 && memcmp(b.hi, corner.hi, sizeof b.hi) == 0 && !b.tight[0] && !b.tight[1] && !b.tight[2]; };
    CHECK(!same(exact_world_box(it, span)));
    span[4] = std::numeric_limits<double>::quiet_NaN();
    CHECK(same(exact_world_box(it, span)));
    memcpy(span, &spans[9 * mesh_item], sizeof span);
    it.root4 = ~0; // a leaf code
    CHECK(same(exact_world_box(it, span)));
    it.root4 = 0; it.inv3.x = 0.5f;
    const double reach[3] = {10, 10, 10};
    float lo[3], hi[3];
    padded_world_box(it, corner, reach, lo, hi);
    for (int c = 0; c < 3; c++) CHECK(lo[c] == -3.0e38f && hi[c] == 3.0e38f);
    return 0;
}

// ---- 3. the top-level trees -----------------------------------------------------------------------------------------------
static int32_t code_of(const DNode4& n, int k) { const float v[4] = {n.q[6].x, n.q[6].y, n.q[6].z, n.q[6].w}; int32_t c; memcpy(&c, &v[k], 4); return c; }
struct TreeStats { std::multiset<uint32_t> leaves; int depth = 0, pending = 0; bool ordered = true, in_range = true; };
static void walk(const std::vector<DNode4>& nodes, const std::vector<DItem>& items, int32_t code, int depth, int pending, TreeStats* st) {
    if (code == SENTINEL) return;
    if (code < 0) { st->leaves.insert(RR_LEAF_FIRST((uint32_t)~code)); st->pending = std::max(st->pending, pending); return; }
    if ((size_t)code >= nodes.size()) { st->in_range = false; return; }
    st->depth = std::max(st->depth, depth + 1);
    int valid = 0, rank_seen = 0; // rank: 0 ball, 1 mesh or inner node, 2 unused slot -- never decreasing along the slots
    for (int k = 0; k < 4; k++) {
        const int32_t c = code_of(nodes[code], k);
        const bool ball = c < 0 && c != SENTINEL && RR_LEAF_FIRST((uint32_t)~c) < items.size() && (items[RR_LEAF_FIRST((uint32_t)~c)].flags & RR_IF_SPHERE);
        const int rank = c == SENTINEL ? 2 : (ball ? 0 : 1);
        if (rank < rank_seen) st->ordered = false;
        rank_seen = rank;
        valid += c != SENTINEL;
    }
    for (int k = 0; k < 4; k++) walk(nodes, items, code_of(nodes[code], k), depth + 1, pending + valid - 1, st);
}
static int check_tree(const std::vector<DNode4>& nodes, int32_t root, const std::vector<DItem>& items, int depth_limit) {
    TreeStats st;
    walk(nodes, items, root, 0, 0, &st);
    CHECK(st.in_range && st.ordered);
    CHECK(st.leaves.size() == items.size() && std::set<uint32_t>(st.leaves.begin(), st.leaves.end()).size() == items.size()); // exactly one leaf each
    CHECK(items.empty() || *st.leaves.rbegin() == items.size() - 1);
    CHECK(st.depth <= depth_limit && st.pending <= depth_limit);
    return 0;
}
static int test_top_level_trees() {
    const double none[3] = {0, 0, 0};
    for (uint32_t n : {0u, 1u, 2u, 7u, 300u, 5000u}) {
        Scene s = random_scene(100 + n, n);
        rr_flat_scene fs = s.flat();
        SceneRecords r;
        CHECK(validate_scene(&fs) == RR_OK && build_scene_records(&fs, &r) == RR_OK);
        CHECK(r.tlas_depth_limit == (n > 4096u ? 13 : (int)std::min(12u, std::max(1u, n > 1u ? n - 1u : 1u)))); // beyond 2^12 items: the deeper share
        CHECK(r.blas_depth_limit == RR_STACK_DEPTH - 3 - r.tlas_depth_limit);
        TlasTrees corners_only, both;
        CHECK(build_tlas(r.items, std::vector<double>(), r.tlas_depth_limit, none, &corners_only) == RR_OK);
        CHECK(!corners_only.has_surface && corners_only.surface.empty() && corners_only.root_surface == SENTINEL); // identical boxes: one tree
        CHECK(build_tlas(r.items, spans_of(r), r.tlas_depth_limit, none, &both) == RR_OK);
        for (const TlasTrees* t : {&corners_only, &both}) {
            CHECK(t->item_boxes.size() == 4 * (size_t)n);
            if (n == 0) { CHECK(t->root == SENTINEL && t->root_surface == SENTINEL && t->corner.empty() && !t->has_surface); continue; }
            CHECK(check_tree(t->corner, t->root, r.items, r.tlas_depth_limit) == 0);
            if (t->has_surface) CHECK(check_tree(t->surface, t->root_surface, r.items, r.tlas_depth_limit) == 0);
            for (int c = 0; c < 3; c++) CHECK(t->reach[c] > 0.0);
        }
        if (n >= 7) CHECK(both.has_surface); // turned meshes: their surface boxes are tighter
        CHECK(n == 0 || memcmp(corners_only.item_boxes.data(), both.item_boxes.data(), 2 * (size_t)n * sizeof(float4)) == 0); // the corner boxes do not depend on the spans
    }
    return 0;
}

// ---- 4. the records of a small scene ---------------------------------------------------------------------------------------
static bool same_bits(const float4& a, const float4& b) { return memcmp(&a, &b, sizeof a) == 0; }
static int test_scene_records() {
    Scene s = hand_made_scene();
    rr_flat_scene fs = s.flat();
    SceneRecords r;
    CHECK(validate_scene(&fs) == RR_OK && build_scene_records(&fs, &r) == RR_OK);
    size_t n_tris = 0;
    for (const rr_mesh& m : s.meshes) n_tris += m.n_triangles;
    CHECK(r.tris.size() == n_tris && r.trix.size() == n_tris && r.attrs.size() == n_tris && r.face_slot.size() == n_tris);
    CHECK(r.items.size() == 6 && r.item_host.size() == 6 && r.dmat.size() == 2 && r.dtex.size() == 2 && r.tlas_depth_limit == 5 && r.blas_depth_limit == RR_STACK_DEPTH - 8);
    std::vector<std::pair<uint32_t, uint32_t>> normals; // [first, end) of every mesh item's flat world normals
    for (size_t i = 0; i < r.items.size(); i++) {
        const DItem& it = r.items[i];
        CHECK(((it.flags & RR_IF_SPHERE) != 0) == (i == 0));
        CHECK(((it.flags & RR_IF_UV_MAY_BE_NAN) != 0) == (i == 0 || i == 4)); // every ball, and the mesh with the degenerate triangle
        CHECK(((it.flags & RR_IF_OCCLUDER_ALPHA_TEX) != 0) == (i == 2));
        CHECK(((it.flags & RR_IF_SMOOTH) != 0) == (i == 3)); // the one mesh that has normals
        if (i == 0) continue;
        const rr_mesh& m = s.meshes[s.items[i].mesh];
        CHECK(it.n_tris == m.n_triangles && (size_t)it.tri_base + it.n_tris <= n_tris && (it.root4 >= 0) == (i != 5));
        for (uint32_t slot = 0; slot < it.n_tris; slot++) { // inverse permutations of the mesh's faces
            const DTri& t = r.tris[it.tri_base + slot];
            const DTriX& x = r.trix[it.tri_base + slot];
            uint32_t f; memcpy(&f, &t.v0.w, 4); // the slot's face: the bits of v0.w
            CHECK(f < it.n_tris && r.face_slot[it.tri_base + f] == slot);
            CHECK(same_bits(x.t0, t.v0));
            CHECK(same_bits(x.t1, make_float4(t.v1.x - t.v0.x, t.v1.y - t.v0.y, t.v1.z - t.v0.z, t.v2.x - t.v0.x)));
            CHECK(same_bits(x.t2, make_float4(t.v2.y - t.v0.y, t.v2.z - t.v0.z, 0.0f, 0.0f)));
            for (int k = 0; k < 3; k++) CHECK(t.v0.x == m.positions[3 * m.indices[3 * f]] && (&t.v1.x)[k] == m.positions[3 * m.indices[3 * f + 1] + k]);
        }
        normals.push_back({it.wn_base, it.wn_base + 2u * it.n_tris});
    }
    CHECK(r.items[1].tri_base == r.items[2].tri_base && r.items[1].node_base4 == r.items[2].node_base4); // two items, one mesh
    uint64_t total = 0;
    for (size_t a = 0; a < normals.size(); a++) {
        total += normals[a].second - normals[a].first;
        for (size_t b = a + 1; b < normals.size(); b++) CHECK(normals[a].second <= normals[b].first || normals[b].second <= normals[a].first);
    }
    CHECK(total == r.n_flat_normals);
    CHECK(!r.general_w && r.any_alpha_occluder && r.n_enabled_lights == 1 && r.dlights.size() == 2 && r.dlights[1].type == (RR_LIGHT_SPOT | 0x80u));
    CHECK(r.dmat[1].texd[RR_TEX_BASE].offset == 4 && r.dmat[1].texd[RR_TEX_BASE].width == 4 && (r.dmat[1].flags & RR_MF_ANY_TEX) && !(r.dmat[0].flags & RR_MF_ANY_TEX));
    // the scene-wide switches follow their inputs
    s.materials[1].texture[RR_TEX_ALPHA] = -1;
    s.items[3].trans_inv[3] = 0.5f;
    fs = s.flat();
    CHECK(validate_scene(&fs) == RR_OK && build_scene_records(&fs, &r) == RR_OK);
    CHECK(r.general_w && !r.any_alpha_occluder);
    return 0;
}

// ---- 5. rejections and the texture layout ----------------------------------------------------------------------------------
static int test_rejections_and_texture_layout() {
    auto rejected = [](Scene& s, int code, const char* message) {
        rr_flat_scene fs = s.flat();
        g_error.clear();
        return validate_scene(&fs) == code && g_error.find(message) != std::string::npos;
    };
    { Scene s = hand_made_scene(); CHECK(validate_scene(nullptr) == RR_ERR_INVALID_ARGUMENT); rr_flat_scene fs = s.flat(); CHECK(validate_scene(&fs) == RR_OK); }
    { Scene s = hand_made_scene(); s.textures[1].rgba8 = nullptr; CHECK(rejected(s, RR_ERR_INVALID_ARGUMENT, "texture 1 has no pixels")); }
    { Scene s = hand_made_scene(); s.textures[0].width = 40000; CHECK(rejected(s, RR_ERR_UNSUPPORTED, "texture 0 is 40000x2")); }
    { Scene s = hand_made_scene(); s.materials[1].texture[3] = 2; CHECK(rejected(s, RR_ERR_INVALID_ARGUMENT, "material 1 texture slot 3 = 2 out of range")); }
    { Scene s = hand_made_scene(); s.items[4].material_cache = 1; CHECK(rejected(s, RR_ERR_INVALID_ARGUMENT, "item 4: material_cache must not carry textures")); }
    { Scene s = hand_made_scene(); s.lights[1].light_type = 3; CHECK(rejected(s, RR_ERR_INVALID_ARGUMENT, "light 1: type 3")); }
    { Scene s = hand_made_scene(); s.items[2].trans[5] = std::numeric_limits<float>::infinity(); CHECK(rejected(s, RR_ERR_INVALID_ARGUMENT, "item 2: non-finite transform")); }
    { Scene s = hand_made_scene(); s.items[5].trans_inv[12] = std::numeric_limits<float>::quiet_NaN(); CHECK(rejected(s, RR_ERR_INVALID_ARGUMENT, "item 5: non-finite transform")); }
    // the same functions as the scene edits call them
    Scene s = hand_made_scene();
    CHECK(check_textures(s.textures.data(), 2) == RR_OK && check_lights(s.lights.data(), 2) == RR_OK && check_material_textures(s.materials.data(), 2, 2) == RR_OK);
    CHECK(check_material_textures(s.materials.data(), 2, 1) == RR_ERR_INVALID_ARGUMENT && g_error == "material 1 texture slot 0 = 1 out of range");
    CHECK(carries_textures(s.materials[1]) && !carries_textures(s.materials[0]));
    CHECK(check_item_transform(7, s.items[0].trans, s.items[0].trans_inv) == RR_OK);
    CHECK(affine_inverse(make_float4(0, 0, 0, 1)) && !affine_inverse(make_float4(0, 1e-30f, 0, 1)) && !affine_inverse(make_float4(0, 0, 0, 2)));
    // appending B to the layout of A gives the layout of A + B (an empty image in between keeps its place)
    const rr_texture list[5] = {{2, 2, s.pixels.data()}, {0, 0, nullptr}, {4, 1, s.pixels.data()}, {3, 5, s.pixels.data()}, {1, 1, s.pixels.data()}};
    for (uint32_t split = 0; split <= 5; split++) {
        std::vector<DTexture> whole, parts;
        std::vector<uint32_t> whole_w, parts_w;
        append_texture_layout(list, 5, &whole, &whole_w);
        append_texture_layout(list, split, &parts, &parts_w);
        CHECK(pool_texels(parts) == (split == 0 ? 0u : split <= 2 ? 4u : split == 3 ? 8u : split == 4 ? 23u : 24u));
        append_texture_layout(list + split, 5 - split, &parts, &parts_w);
        CHECK(whole.size() == 5 && parts.size() == 5 && whole_w == parts_w && pool_texels(whole) == 24);
        for (int i = 0; i < 5; i++) CHECK(whole[i].offset == parts[i].offset && whole[i].width == parts[i].width && whole[i].height == parts[i].height);
    }
    return 0;
}

// ---- digests -------------------------------------------------------------------------------------------------------------
template <class T> static unsigned long long fnv(const std::vector<T>& v) {
    unsigned long long h = 1469598103934665603ull;
    const unsigned char* p = (const unsigned char*)v.data();
    for (size_t i = 0; i < v.size() * sizeof(T); i++) { h ^= p[i]; h *= 1099511628211ull; }
    return h;
}
static void print_digests(const char* name, const SceneRecords& r, const TlasTrees& t) {
    std::printf("%s: %zu items %zu triangles limits %d/%d flat normals %llu switches %d%d lights on %u roots %d %d surface %d nan_balls %d\n", name, r.items.size(), r.tris.size(),
                r.tlas_depth_limit, r.blas_depth_limit, (unsigned long long)r.n_flat_normals, (int)r.general_w, (int)r.any_alpha_occluder, r.n_enabled_lights, t.root, t.root_surface,
                (int)t.has_surface, (int)t.nan_balls);
    std::printf("  nodes4 %016llx tris %016llx trix %016llx attrs %016llx face_slot %016llx\n", fnv(r.nodes4), fnv(r.tris), fnv(r.trix), fnv(r.attrs), fnv(r.face_slot));
    std::printf("  items %016llx item_host %016llx dmat %016llx dlights %016llx dtex %016llx tex_width %016llx\n", fnv(r.items), fnv(r.item_host), fnv(r.dmat), fnv(r.dlights), fnv(r.dtex), fnv(r.tex_width));
    std::printf("  tlas corner %016llx surface %016llx item_boxes %016llx reach %016llx\n", fnv(t.corner), fnv(t.surface), fnv(t.item_boxes), fnv(std::vector<double>(t.reach, t.reach + 3)));
}
static int print_digests(const char* name, Scene s) {
    rr_flat_scene fs = s.flat();
    SceneRecords r;
    CHECK(validate_scene(&fs) == RR_OK && build_scene_records(&fs, &r) == RR_OK);
    TlasTrees t;
    const double none[3] = {0, 0, 0};
    CHECK(build_tlas(r.items, spans_of(r), r.tlas_depth_limit, none, &t) == RR_OK);
    print_digests(name, r, t);
    return 0;
}

int main(int argc, char** argv) {
    if (argc > 1 && std::string(argv[1]) == "--digest") return print_digests("hand-made", hand_made_scene()) || print_digests("random seed 7", random_scene(7, 300));
    if (test_surface_boxes() || test_top_level_trees() || test_scene_records() || test_rejections_and_texture_layout() || test_padded_boxes_keep_every_candidate()) return 1;
    std::printf("scene build test OK\n");
    return 0;
}
