// Host-only test of the two halves of build_scene_records (rustray_amd/csrc/rr_scene_build.h) that rr_scene_add_meshes and
// rr_scene_set_items are made of; built with g++ -fsanitize=address,undefined by tests/test_scene_items.py, linked with rr_bvh.cpp.
//   append_mesh_records: "the first k meshes, then the rest" gives the arenas and the per-mesh table of the whole list, byte for
//     byte, at every split -- appended in place, and appended alone behind `before` resident records (the device form)
//   build_item_records: a permuted / shortened / lengthened item list over resident meshes gives the records of a fresh build
//   plan_item_reuse: exactly the items whose matrices, mesh records and flag word are bitwise an old item's are kept
//   check_items / check_meshes / stack_shares: every rejection, and where the stack share changes with the item count
#include <cstdarg>
#include <cstdio>
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
#define CHECK(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s (last error: %s)\n", __FILE__, __LINE__, #c, g_error.c_str()); return 1; } } while (0)

// ---- scenes ----------------------------------------------------------------------------------------------------------------
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
static MeshData grid_mesh(int grid, int salt, bool attrs) { // grid x grid quads over a bumpy height field
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
// an item of mesh `mesh` (-1: a ball) scaled by s and moved to (x, y, z); the inverse is exact for these
static rr_item make_item(uint32_t id, int mesh, int material, int cache, float s, float x, float y, float z) {
    rr_item it;
    memset(&it, 0, sizeof it);
    it.kind = mesh < 0 ? RR_ITEM_SPHERE : RR_ITEM_MESH; it.id = id; it.material = material; it.material_cache = cache; it.mesh = mesh;
    it.radius = 1.0f; it.visible = 1;
    it.trans[0] = it.trans[5] = it.trans[10] = s; it.trans[15] = 1.0f; it.trans[12] = x; it.trans[13] = y; it.trans[14] = z;
    it.trans_inv[0] = it.trans_inv[5] = it.trans_inv[10] = 1.0f / s; it.trans_inv[15] = 1.0f;
    it.trans_inv[12] = -x / s; it.trans_inv[13] = -y / s; it.trans_inv[14] = -z / s;
    for (int k = 0; k < 3; k++) { it.bbox_min[k] = -1.0f; it.bbox_max[k] = 16.0f; }
    return it;
}

struct Scene {
    std::vector<MeshData> mesh_data;
    std::vector<rr_mesh> meshes;
    std::vector<rr_item> items;
    std::vector<rr_material> materials;
    std::vector<rr_texture> textures;
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
        return fs;
    }
};
// meshes: 0 plain grid, 1 grid with uvs and normals, 2 holds a degenerate triangle, 3 a single triangle (one leaf), 4 no triangles,
// 5 a larger grid with attributes, 6 a grid of its own; materials: 0 full, 1 full with an alpha map, 2 the texture-less cache;
// items: a ball, mesh 0 twice (the second alpha-mapped), meshes 1 .. 6
static Scene hand_made_scene() {
    Scene s;
    s.mesh_data = {grid_mesh(8, 0, false), grid_mesh(6, 3, true), grid_mesh(4, 1, false), MeshData(), MeshData(), grid_mesh(19, 2, true), grid_mesh(5, 4, false)};
    s.mesh_data[2].idx.insert(s.mesh_data[2].idx.end(), {0u, 0u, 1u}); // two corners coincide
    s.mesh_data[3].pos = {0, 0, 0, 1, 0, 0, 0, 1, 0}; s.mesh_data[3].idx = {0, 1, 2};
    s.materials = {plain_material(), plain_material(), plain_material()};
    s.materials[1].texture[RR_TEX_ALPHA] = 0; s.materials[1].texture[RR_TEX_BASE] = 1;
    s.textures = {rr_texture{2, 2, s.pixels.data()}, rr_texture{4, 1, s.pixels.data()}};
    const int mesh_of[9] = {-1, 0, 0, 1, 2, 3, 4, 5, 6};
    for (int i = 0; i < 9; i++) s.items.push_back(make_item(100u + i, mesh_of[i], i == 2 ? 1 : 0, 2, 1.0f + 0.25f * i, 3.0f * i, 0.5f * i, -2.0f * i));
    return s;
}

template <class T> static bool same_bytes(const std::vector<T>& a, const std::vector<T>& b) {
    return a.size() == b.size() && (a.empty() || memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0);
}
template <class T> static bool same_tail(const std::vector<T>& whole, size_t before, const std::vector<T>& tail) {
    return whole.size() == before + tail.size() && (tail.empty() || memcmp(whole.data() + before, tail.data(), tail.size() * sizeof(T)) == 0);
}
static bool same_table(const std::vector<MeshDev>& a, const std::vector<MeshDev>& b) {
    if (a.size() != b.size()) return false;
    for (size_t i = 0; i < a.size(); i++)
        if (a[i].tri_base != b[i].tri_base || a[i].n_tris != b[i].n_tris || a[i].node_base4 != b[i].node_base4 || a[i].root4 != b[i].root4 ||
            a[i].has_normals != b[i].has_normals || a[i].degenerate != b[i].degenerate) return false;
    return true;
}
static bool same_arenas(const MeshArenas& a, const MeshArenas& b) {
    return same_bytes(a.nodes4, b.nodes4) && same_bytes(a.tris, b.tris) && same_bytes(a.trix, b.trix) && same_bytes(a.attrs, b.attrs) &&
           same_bytes(a.face_slot, b.face_slot) && same_table(a.meshes, b.meshes);
}
static bool same_host(const std::vector<ItemHost>& a, const std::vector<ItemHost>& b) {
    if (a.size() != b.size()) return false;
    for (size_t i = 0; i < a.size(); i++)
        if (a[i].kind != b[i].kind || a[i].material != b[i].material || a[i].material_cache != b[i].material_cache || a[i].visible != b[i].visible ||
            a[i].flip_normals != b[i].flip_normals || a[i].mesh_has_normals != b[i].mesh_has_normals || a[i].mesh_degenerate != b[i].mesh_degenerate || a[i].mesh != b[i].mesh) return false;
    return true;
}
static bool same_items(const ItemRecords& a, const ItemRecords& b) {
    return same_bytes(a.items, b.items) && same_host(a.item_host, b.item_host) && a.n_flat_normals == b.n_flat_normals && a.general_w == b.general_w &&
           a.any_alpha_occluder == b.any_alpha_occluder;
}

// ---- the meshes, appended -----------------------------------------------------------------------------------------------------
static int test_split_append(Scene s, const char* what) {
    rr_flat_scene fs = s.flat();
    SceneRecords whole;
    CHECK(validate_scene(&fs) == RR_OK && build_scene_records(&fs, &whole) == RR_OK);
    CHECK(whole.meshes.size() == fs.n_meshes && whole.tris.size() == whole.trix.size() && whole.tris.size() == whole.face_slot.size());
    for (uint32_t k = 0; k <= fs.n_meshes; k++) {
        MeshArenas a; // in place: the first k, then the rest
        CHECK(append_mesh_records(fs.meshes, k, whole.blas_depth_limit, fs.n_items, &a) == RR_OK);
        const size_t tris_k = a.tris.size(), nodes_k = a.nodes4.size();
        const std::vector<MeshDev> table_k = a.meshes;
        CHECK(append_mesh_records(fs.meshes + k, fs.n_meshes - k, whole.blas_depth_limit, fs.n_items, &a) == RR_OK);
        CHECK(same_arenas(a, whole));
        MeshArenas b; // alone, behind the records of the first k (what rr_scene_add_meshes uploads behind the resident ones)
        b.meshes = table_k; b.tris_before = tris_k; b.nodes4_before = nodes_k;
        CHECK(append_mesh_records(fs.meshes + k, fs.n_meshes - k, whole.blas_depth_limit, fs.n_items, &b) == RR_OK);
        CHECK(same_table(b.meshes, whole.meshes));
        CHECK(same_tail(whole.nodes4, nodes_k, b.nodes4) && same_tail(whole.tris, tris_k, b.tris) && same_tail(whole.trix, tris_k, b.trix) &&
              same_tail(whole.attrs, tris_k, b.attrs) && same_tail(whole.face_slot, tris_k, b.face_slot));
        // the scene's own copies of the caller's arrays give the same records (what a changed stack share rebuilds from)
        std::vector<HostMesh> copies;
        std::vector<rr_mesh> views;
        for (uint32_t i = 0; i < fs.n_meshes; i++) copies.emplace_back(fs.meshes[i]);
        for (const HostMesh& m : copies) views.push_back(m.view());
        MeshArenas c;
        CHECK(append_mesh_records(views.data(), fs.n_meshes, whole.blas_depth_limit, fs.n_items, &c) == RR_OK && same_arenas(c, whole));
    }
    std::printf("%s: %u meshes, %zu triangles, %zu nodes: every split appends to the whole list's records\n", what, fs.n_meshes, whole.tris.size(), whole.nodes4.size());
    return 0;
}

// ---- the items, from a list ----------------------------------------------------------------------------------------------------
static int check_list(Scene& s, const SceneRecords& resident, const std::vector<rr_item>& list, const char* what, bool want_general_w, bool want_alpha) {
    Scene f = s;
    f.items = list;
    rr_flat_scene fs = f.flat();
    SceneRecords fresh;
    CHECK(validate_scene(&fs) == RR_OK && build_scene_records(&fs, &fresh) == RR_OK);
    if (fresh.blas_depth_limit != resident.blas_depth_limit) return 0; // another share: the meshes are rebuilt first (test_shares)
    CHECK(check_items(list.data(), (uint32_t)list.size(), f.materials.data(), (uint32_t)f.materials.size(), resident.meshes.size()) == RR_OK);
    ItemRecords got;
    CHECK(build_item_records(list.data(), (uint32_t)list.size(), f.materials.data(), resident.meshes, resident.tex_width, &got) == RR_OK);
    CHECK(same_items(got, fresh));
    CHECK(got.general_w == want_general_w && got.any_alpha_occluder == want_alpha);
    uint64_t base = 0; // wn_base in item order
    for (const DItem& d : got.items)
        if (!(d.flags & RR_IF_SPHERE)) { CHECK(d.wn_base == base); base += 2ull * d.n_tris; }
    CHECK(base == got.n_flat_normals);
    std::printf("item list %s: %zu items, %llu flat normals\n", what, list.size(), (unsigned long long)got.n_flat_normals);
    return 0;
}
static int test_item_lists() {
    Scene s = hand_made_scene();
    for (int i = 9; i < 16; i++) s.items.push_back(make_item(100u + i, i % 7, 0, 2, 0.5f + 0.1f * i, -2.0f * i, 1.0f, 4.0f * i)); // 16 items: the share of 14 and more
    rr_flat_scene fs = s.flat();
    SceneRecords r;
    CHECK(validate_scene(&fs) == RR_OK && build_scene_records(&fs, &r) == RR_OK);
    const std::vector<rr_item> all = s.items;
    if (check_list(s, r, all, "as created", false, true)) return 1;
    std::vector<rr_item> v(all.rbegin(), all.rend());
    if (check_list(s, r, v, "reversed", false, true)) return 1;
    v = all; std::swap(v[1], v[7]); std::swap(v[0], v[15]); std::swap(v[3], v[4]);
    if (check_list(s, r, v, "permuted", false, true)) return 1;
    v = all; v.erase(v.begin() + 2); // the alpha-mapped item goes: the hint with it
    if (check_list(s, r, v, "shortened", false, false)) return 1;
    v = all; v.pop_back();
    if (check_list(s, r, v, "last deleted", false, true)) return 1;
    v = all;
    v.push_back(make_item(900, 5, 0, 2, 2.0f, 1.0f, 2.0f, 3.0f)); // a second instance of a resident mesh
    v.push_back(make_item(901, -1, 1, 2, 50.0f, 0.0f, 0.0f, 0.0f)); // a ball
    v.back().trans_inv[3] = 0.25f;                                   // ... with a projective inverse: the other hint
    if (check_list(s, r, v, "lengthened", true, true)) return 1;
    v.insert(v.begin() + 4, make_item(902, 0, 0, 2, 1.0f, 0.0f, 9.0f, 0.0f)); v[6].visible = 0; v[7].flip_normals = 1;
    if (check_list(s, r, v, "inserted, hidden, flipped", true, true)) return 1;
    return 0;
}

// ---- keep or derive ------------------------------------------------------------------------------------------------------------
static int test_reuse() {
    Scene s = hand_made_scene();
    rr_flat_scene fs = s.flat();
    SceneRecords r;
    CHECK(validate_scene(&fs) == RR_OK && build_scene_records(&fs, &r) == RR_OK);
    std::vector<rr_item> v = s.items;          // old indices: 0 ball, 1 2 mesh 0, 3 .. 8 meshes 1 .. 6
    std::swap(v[1], v[8]);                     // moved: kept, from their old places
    v.erase(v.begin() + 4);                    // old 4 deleted
    // now: [0]=old 0, [1]=old 8, [2]=old 2, [3]=old 3, [4]=old 5, [5]=old 6, [6]=old 7, [7]=old 1
    float bumped = v[3].trans[12];
    uint32_t bits; memcpy(&bits, &bumped, 4); bits += 1u; memcpy(&bumped, &bits, 4);
    v[3].trans[12] = bumped;                   // one ulp in one matrix entry: derived
    v[4].visible = 0;                          // another flag word: derived
    v[6].mesh = 6;                             // another mesh under the old transform: derived
    v[2].id = 777; v[2].radius = 3.0f; v[2].bbox_max[1] = 99.0f; // id, radius and the declared box are no inputs of the derived data: kept
    v.push_back(make_item(900, 5, 0, 2, 2.0f, 1.0f, 2.0f, 3.0f)); // a new instance: derived
    v.push_back(s.items[7]);                   // a bitwise copy of old 7: kept
    ItemRecords got;
    CHECK(build_item_records(v.data(), (uint32_t)v.size(), s.materials.data(), r.meshes, r.tex_width, &got) == RR_OK);
    std::vector<int32_t> keep;
    plan_item_reuse(r.items, got.items, &keep);
    const int32_t want[10] = {0, 8, 2, -1, -1, 6, -1, 1, -1, 7};
    CHECK(keep.size() == 10);
    for (int i = 0; i < 10; i++) {
        if (keep[i] != want[i]) std::printf("item %d: keep_from %d, want %d\n", i, keep[i], want[i]);
        CHECK(keep[i] == want[i]);
    }
    // the kept items sit elsewhere in the new arena: what is compared is the input of the derived data, not its place
    CHECK(got.items[1].wn_base != r.items[8].wn_base && got.items[1].n_tris == r.items[8].n_tris);
    // no old list (a rebuilt mesh arena): everything is derived
    plan_item_reuse(std::vector<DItem>(), got.items, &keep);
    for (int32_t k : keep) CHECK(k == -1);
    // two old items alike: the first
    std::vector<DItem> twice = r.items;
    twice.push_back(r.items[3]);
    plan_item_reuse(twice, r.items, &keep);
    for (size_t i = 0; i < r.items.size(); i++) CHECK(keep[i] == (int32_t)i);
    // the chunk map: every item at least one chunk, RR_HOST_ITEM_CHUNK triangles each, consecutive per item
    std::vector<DItem> big = got.items;
    big[1].n_tris = 3 * RR_HOST_ITEM_CHUNK + 5;
    std::vector<uint2> chunks; std::vector<uint32_t> chunk_item;
    item_chunk_map(big, &chunks, &chunk_item);
    CHECK(chunks.size() == big.size() + 3 && chunk_item.size() == chunks.size());
    CHECK(chunks[1].x == 1 && chunks[1].y == 0 && chunks[4].x == 1 && chunks[4].y == 3 * RR_HOST_ITEM_CHUNK && chunks[5].x == 2 && chunks[0].x == 0);
    std::printf("keep or derive: 6 of 10 items kept, 4 derived\n");
    return 0;
}

// ---- rejections ----------------------------------------------------------------------------------------------------------------
static int test_rejections() {
    Scene s = hand_made_scene();
    rr_flat_scene fs = s.flat();
    SceneRecords r;
    CHECK(validate_scene(&fs) == RR_OK && build_scene_records(&fs, &r) == RR_OK);
    const uint32_t nm = (uint32_t)s.materials.size();
    auto items_rc = [&](std::vector<rr_item> v, const std::vector<rr_material>& mats, const char* message) {
        g_error.clear();
        const int rc = check_items(v.data(), (uint32_t)v.size(), mats.data(), (uint32_t)mats.size(), r.meshes.size());
        return g_error.find(message) != std::string::npos ? rc : 12345;
    };
    std::vector<rr_item> v = s.items;
    CHECK(items_rc(v, s.materials, "") == RR_OK);
    v[4].kind = 7; CHECK(items_rc(v, s.materials, "item 4: kind 7") == RR_ERR_INVALID_ARGUMENT); v = s.items;
    v[1].material = (int32_t)nm; CHECK(items_rc(v, s.materials, "item 1: material index") == RR_ERR_INVALID_ARGUMENT); v = s.items;
    v[1].material = -1; CHECK(items_rc(v, s.materials, "item 1: material index") == RR_ERR_INVALID_ARGUMENT); v = s.items;
    v[8].material_cache = (int32_t)nm; CHECK(items_rc(v, s.materials, "item 8: material index") == RR_ERR_INVALID_ARGUMENT); v = s.items;
    v[8].material_cache = -3; CHECK(items_rc(v, s.materials, "item 8: material index") == RR_ERR_INVALID_ARGUMENT); v = s.items;
    v[3].material_cache = 1; CHECK(items_rc(v, s.materials, "item 3: material_cache must not carry textures") == RR_ERR_INVALID_ARGUMENT); v = s.items;
    v[5].mesh = (int32_t)r.meshes.size(); CHECK(items_rc(v, s.materials, "item 5: mesh index 7") == RR_ERR_INVALID_ARGUMENT); v = s.items;
    v[5].mesh = -1; CHECK(items_rc(v, s.materials, "item 5: mesh index -1") == RR_ERR_INVALID_ARGUMENT); v = s.items;
    v[0].mesh = 99; CHECK(items_rc(v, s.materials, "") == RR_OK); v = s.items; // a ball names no mesh
    v[6].trans[13] = NAN; CHECK(items_rc(v, s.materials, "item 6: non-finite transform") == RR_ERR_INVALID_ARGUMENT); v = s.items;
    v[6].trans_inv[0] = INFINITY; CHECK(items_rc(v, s.materials, "item 6: non-finite transform") == RR_ERR_INVALID_ARGUMENT); v = s.items;
    g_error.clear(); // the item limits: refused before an item is read
    CHECK(check_items(v.data(), 1u << 27, s.materials.data(), nm, r.meshes.size()) == RR_ERR_UNSUPPORTED && g_error.find("27 bits") != std::string::npos);
    int tl = 0, bl = 0;
    CHECK(stack_shares(RR_MAX_ITEMS, &tl, &bl) == RR_OK && stack_shares(RR_MAX_ITEMS + 1u, &tl, &bl) == RR_ERR_UNSUPPORTED && g_error.find("RR_MAX_ITEMS") != std::string::npos);
    // materials that name a texture the scene does not hold
    std::vector<rr_material> mats = s.materials;
    mats[0].texture[3] = (int32_t)s.textures.size();
    CHECK(check_material_textures(mats.data(), nm, s.textures.size()) == RR_ERR_INVALID_ARGUMENT && g_error.find("material 0 texture slot 3") != std::string::npos);
    // 2^31 instanced triangles: 17 instances of a mesh of 2^27 triangles (a table entry is all the records take of it)
    std::vector<MeshDev> table = r.meshes;
    table[0].n_tris = 1u << 27;
    v.assign(17, s.items[1]);
    ItemRecords got;
    CHECK(build_item_records(v.data(), 15, s.materials.data(), table, r.tex_width, &got) == RR_OK && got.n_flat_normals == 15ull << 28);
    g_error.clear();
    CHECK(build_item_records(v.data(), 17, s.materials.data(), table, r.tex_width, &got) == RR_ERR_UNSUPPORTED && g_error.find("2^31 instanced triangles") != std::string::npos);
    // appended meshes: checked as rr_scene_create checks them, and named by their index in the scene's list
    auto mesh_rc = [&](rr_mesh m, const char* message) {
        g_error.clear();
        const int rc = check_meshes(&m, 1, 7);
        return g_error.find(message) != std::string::npos ? rc : 12345;
    };
    const rr_mesh good = s.mesh_data[1].view();
    CHECK(mesh_rc(good, "") == RR_OK);
    rr_mesh m = good; m.positions = nullptr; CHECK(mesh_rc(m, "mesh 7: missing positions") == RR_ERR_INVALID_ARGUMENT);
    m = good; m.uvs = nullptr; CHECK(mesh_rc(m, "mesh 7: attribute pointer") == RR_ERR_INVALID_ARGUMENT);
    m = good; m.n_vertices = 3; CHECK(mesh_rc(m, "mesh 7: vertex index") == RR_ERR_INVALID_ARGUMENT);
    m = good; m.n_uvs = 2; CHECK(mesh_rc(m, "mesh 7: uv index") == RR_ERR_INVALID_ARGUMENT);
    m = good; m.n_normals = 1; CHECK(mesh_rc(m, "mesh 7: normal index") == RR_ERR_INVALID_ARGUMENT);
    m = good; m.n_normal_faces = 1; CHECK(mesh_rc(m, "mesh 7: 1 normal faces") == RR_ERR_INVALID_ARGUMENT);
    m = good; m.n_triangles = 1u << 28; CHECK(mesh_rc(m, "mesh 7: 268435456 triangles") == RR_ERR_UNSUPPORTED);
    // a mesh that does not fit the levels left to it: refused by name, with the item count that took them
    MeshArenas a;
    const rr_mesh deep = s.mesh_data[5].view();
    g_error.clear();
    CHECK(append_mesh_records(&deep, 1, 2, 4242, &a) == RR_ERR_UNSUPPORTED && g_error.find("mesh 0") != std::string::npos && g_error.find("4242 items") != std::string::npos);
    std::printf("rejections: every check of an item list, a material list and an appended mesh refuses by name\n");
    return 0;
}

// ---- the stack share ------------------------------------------------------------------------------------------------------------
// The per-mesh trees get what the top level leaves of the RR_STACK_DEPTH entries.  By stack_shares the top level takes
// min(RR_TLAS_MAX_DEPTH, n - 1) levels (at least 1), and ceil(log2 n) above 2^RR_TLAS_MAX_DEPTH items: going from n to n + 1 items
// changes the share for n = 2 .. 12 and at every power of two from 4096 on, and nowhere else -- 0, 1 and 2 items share one level,
// and from 13 items on the top level has its 12.
static int test_shares() {
    auto blas = [](uint32_t n) { int t = 0, b = 0; return stack_shares(n, &t, &b) == RR_OK ? b : -1; };
    auto tlas = [](uint32_t n) { int t = 0, b = 0; return stack_shares(n, &t, &b) == RR_OK ? t : -1; };
    for (uint32_t n = 0; n <= 20; n++) {
        CHECK(tlas(n) + blas(n) == RR_STACK_DEPTH - 3);
        CHECK(tlas(n) == (int)std::min<uint32_t>(RR_TLAS_MAX_DEPTH, n > 1 ? n - 1 : 1u));
        const bool changes = blas(n) != blas(n + 1);
        CHECK(changes == (n >= 2 && n <= 12));
    }
    CHECK(blas(1) == blas(2) && blas(2) != blas(3) && blas(12) != blas(13) && blas(13) == blas(14));
    CHECK(blas(14) == blas(4096) && blas(4096) != blas(4097) && blas(4097) == blas(8192) && blas(8192) != blas(8193));
    CHECK(tlas(4097) == 13 && tlas(RR_MAX_ITEMS) == 20 && blas(RR_MAX_ITEMS) == RR_STACK_DEPTH - 3 - 20);
    // the records of the same meshes differ between shares where the budget binds, and a fresh scene of the other item count has
    // those of its own share: what an edit across the boundary must rebuild
    Scene s = hand_made_scene();
    s.items.resize(2);
    rr_flat_scene fs = s.flat();
    SceneRecords two, twelve;
    CHECK(validate_scene(&fs) == RR_OK && build_scene_records(&fs, &two) == RR_OK && two.blas_depth_limit == blas(2));
    s = hand_made_scene();
    for (int i = 9; i < 14; i++) s.items.push_back(make_item(100u + i, i % 7, 0, 2, 1.0f, 1.0f * i, 0.0f, 0.0f));
    fs = s.flat();
    CHECK(validate_scene(&fs) == RR_OK && build_scene_records(&fs, &twelve) == RR_OK && twelve.blas_depth_limit == blas(14));
    MeshArenas a;
    CHECK(append_mesh_records(fs.meshes, fs.n_meshes, blas(2), 2, &a) == RR_OK && same_arenas(a, two));
    MeshArenas b;
    CHECK(append_mesh_records(fs.meshes, fs.n_meshes, blas(14), 14, &b) == RR_OK && same_arenas(b, twelve));
    std::printf("stack share: changes from n to n + 1 items for n = 2 .. 12 and at 4096, 8192, ...; %d and %d levels for the meshes of 2 and 14 items\n", blas(2), blas(14));
    return 0;
}

int main() {
    if (test_split_append(hand_made_scene(), "hand-made scene")) return 1;
    {
        Scene s; // a dozen grids of growing size, some with attributes, and an empty mesh in the middle
        for (int m = 0; m < 12; m++) s.mesh_data.push_back(m == 5 ? MeshData() : grid_mesh(3 + 2 * m, m, m % 3 == 0));
        s.materials = {plain_material()};
        for (int i = 0; i < 30; i++) s.items.push_back(make_item(1u + i, i % 5 == 0 ? -1 : i % 12, 0, 0, 1.0f, 2.0f * i, 0.0f, 0.0f));
        if (test_split_append(s, "grids")) return 1;
    }
    if (test_item_lists() || test_reuse() || test_rejections() || test_shares()) return 1;
    std::printf("scene items test OK\n");
    return 0;
}
