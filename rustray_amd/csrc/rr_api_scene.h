// rr_api_scene.h — a scene's device state: created, pointed to by the view, edited in place and structurally.
// Offers: point_view; the top level (tlas_fits, tlas_capacity, reserve_tlas, copy_tlas, keep_tlas, upload_tlas) and its reach
//         (ensure_tlas_reach, ensure_camera_reach); derive_from_transforms; rr_test_host_build; rr_scene_create, rr_scene_destroy;
//         all_or_nothing; rr_scene_update_transforms / _materials / _lights / _item_flags; rr_scene_add_textures, rr_scene_add_meshes,
//         rr_scene_set_items.
// Needs:  rr_api_base.h, rr_api_handle.h (writes rr_scene::data and rr_scene::tlas; rr_scene_create has the frame parts set themselves up),
//         rr_scene_build.h (the records and trees this file uploads), the kernels k_world_normals, k_world_normals_edit, k_item_spans.

// ---------------------------------------------------------------------------
// the view
// ---------------------------------------------------------------------------
// THE place that points DSceneView at the scene's buffers: every pointer field from its DevBuf, and the counts that are sizes of host
// copies.  Every commit that moves a buffer calls it after its moves (rr_scene_create, keep_tlas, keep_mesh_buffers, the light and
// texture edits, rr_scene_set_items through the two keeps), so no pointer can be left behind.  The other words of the view stay where
// they are computed: compat, the two roots, general_w, any_alpha_occluder.
static void point_view(rr_scene* s) noexcept {
    const SceneData& d = s->data;
    DSceneView& v = s->data.view;
    v.items = d.items.as<DItem>(); v.nodes4 = d.nodes4.as<DNode4>(); v.tris = d.tris.as<DTri>(); v.trix = d.trix.as<DTriX>(); v.attrs = d.attrs.as<DTriAttr>();
    v.flat_normals = d.flat_normals.as<float4>();
    v.face_slot = d.face_slot.as<uint32_t>();
    v.materials = d.materials.as<DMaterial>(); v.textures = d.textures.as<DTexture>(); v.texels = d.texels.as<uint32_t>();
    v.lights = d.lights.as<DLight>();
    v.n_items = (uint32_t)d.h_items.size(); v.n_lights = (uint32_t)d.h_lights.size(); v.n_enabled_lights = d.n_enabled_lights;
    v.tnodes4 = d.tnodes4.as<DNode4>();
    v.tnodes4c = s->tlas.has_surface ? d.tnodes4.as<DNode4>() + s->tlas.node_capacity : d.tnodes4.as<DNode4>();
    v.item_boxes = d.item_boxes.as<float4>();
}

// ---------------------------------------------------------------------------
// top level: upload, and the reach it is padded for (the scene's records and trees are built by rr_scene_build.h)
// ---------------------------------------------------------------------------
// the nodes per tree a scene of n_items reserves for these trees: room for rebuilds after transform updates
static uint32_t tlas_capacity(const TlasTrees& t, uint32_t n_items) {
    return std::max<uint32_t>((uint32_t)std::max(t.corner.size(), t.surface.size()), n_items ? n_items : 1u);
}
// the device side of a top level of `capacity` nodes per tree: the zeroed node buffer for both trees, and the item boxes
static int reserve_tlas(DevBuf* tnodes4, DevBuf* item_boxes, const TlasTrees& t, uint32_t capacity) {
    HIP_TRY(tnodes4->reserve(2 * (size_t)capacity * sizeof(DNode4)));
    HIP_TRY(hipMemset(tnodes4->p, 0, 2 * (size_t)capacity * sizeof(DNode4)));
    HIP_TRY(item_boxes->reserve(std::max<size_t>((t.item_boxes.size() + t.item_groups.size()) * sizeof(float4), 16))); // (both sizes follow from n_items alone)
    return RR_OK;
}
// THE refusal of trees that do not fit a node buffer of `capacity` nodes per tree
static int tlas_fits(const TlasTrees& t, uint32_t capacity) {
    if (t.corner.size() > capacity || t.surface.size() > capacity)
        return fail(RR_ERR_DEVICE, "top-level rebuild needs %zu / %zu nodes, capacity %u", t.corner.size(), t.surface.size(), capacity);
    return RR_OK;
}
// The two trees into the scene's node buffer (the corner tree in its first half, the surface tree in the second: s->tlas.node_capacity
// nodes each) and the item boxes; then, and only then, the scene keeps what they were built for: the reach, the NaN-ball hint, the host
// copy of the boxes, which tree the closest-hit walks take and the roots in the view.  A failed copy leaves all of that as it was and
// marks the device trees stale.  Blocking copies.
// copy_tlas / keep_tlas: the two halves, which rr_scene_set_items runs on buffers built beside the scene's and at its commit.
static int copy_tlas(const TlasTrees& t, DNode4* tnodes4, uint32_t capacity, float4* item_boxes) {
    RR_TRY(tlas_fits(t, capacity));
    if (!t.corner.empty()) HIP_TRY(hipMemcpy(tnodes4, t.corner.data(), t.corner.size() * sizeof(DNode4), hipMemcpyHostToDevice));
    if (!t.surface.empty()) HIP_TRY(hipMemcpy(tnodes4 + capacity, t.surface.data(), t.surface.size() * sizeof(DNode4), hipMemcpyHostToDevice));
    if (!t.item_boxes.empty()) HIP_TRY(hipMemcpy(item_boxes, t.item_boxes.data(), t.item_boxes.size() * sizeof(float4), hipMemcpyHostToDevice));
    if (!t.item_groups.empty()) HIP_TRY(hipMemcpy(item_boxes + t.item_boxes.size(), t.item_groups.data(), t.item_groups.size() * sizeof(float4), hipMemcpyHostToDevice));
    return RR_OK;
}
static void keep_tlas(rr_scene* s, TlasTrees& t) noexcept {
    for (int c = 0; c < 3; c++) s->tlas.reach[c] = t.reach[c];
    s->data.view.compat = t.nan_balls ? (s->data.view.compat | RR_VIEW_NAN_BALLS) : (s->data.view.compat & ~RR_VIEW_NAN_BALLS);
    s->tlas.h_item_boxes.swap(t.item_boxes);
    s->tlas.has_surface = t.has_surface;
    s->data.view.tlas_root4 = t.root;
    s->data.view.tlas_root4c = t.has_surface ? t.root_surface : t.root;
    point_view(s);
}
static int upload_tlas(rr_scene* s, TlasTrees& t) {
    RR_TRY(tlas_fits(t, s->tlas.node_capacity)); // (before the trees are marked stale: a refusal writes nothing)
    s->tlas.stale = true;
    RR_TRY(copy_tlas(t, s->data.tnodes4.as<DNode4>(), s->tlas.node_capacity, s->data.item_boxes.as<float4>()));
    s->tlas.stale = false;
    keep_tlas(s, t);
    return RR_OK;
}

// Ray origins of the coming launch reach out to +-need: rebuilds the top level when its boxes were padded for less
// (a camera far outside the scene), or for more than 16x as much (the camera came back), or when an upload failed part-way.
// s->tlas.reach changes with the upload only (upload_tlas): after a failure the next frame from this camera rebuilds again.
static int ensure_tlas_reach(rr_scene* s, const double need[3]) {
    bool grow = false, shrink = s->tlas.stale;
    for (int c = 0; c < 3; c++) {
        if (need[c] > s->tlas.reach[c]) grow = true;
        if (s->tlas.reach[c] > 16.0 * std::max(need[c], s->tlas.floor[c])) shrink = true;
    }
    if (!grow && !shrink) return RR_OK;
    double want[3];
    for (int c = 0; c < 3; c++) want[c] = 2.0 * need[c]; // build_tlas raises it to the items' own extent
    TlasTrees trees;
    RR_TRY(build_tlas(s->data.h_items, s->data.h_spans, s->tlas.depth_limit, want, &trees));
    RR_FAULT_POINT("tlas_reach.upload");
    HIP_TRY(hipDeviceSynchronize());
    return upload_tlas(s, trees);
}
// the top level padded for the primary-ray origins of a camera: a bound on them (primary_ray: view_inv * (proj_inv * (sx, sy, -1, 1)).xyz1, |sx|, |sy| <= smax)
static int ensure_camera_reach(rr_scene* s, const rr_camera* cam, const rr_config* cfg) {
    double need[3];
    const double aperture = cfg ? std::max(1.0, (double)cfg->aperture_size) : 1.0;
    const double smax = 1.0 + 2.0 * (1.0 + aperture * cam->width / 800.0) * (2.0 / std::max(1u, std::min(cam->width, cam->height)));
    const double v[4] = {smax, smax, 1.0, 1.0};
    double pp[3];
    for (int k = 0; k < 3; k++) {
        pp[k] = 0.0;
        for (int j = 0; j < 4; j++) pp[k] += std::fabs((double)cam->projection_inverse[4 * j + k]) * v[j];
    }
    for (int c = 0; c < 3; c++) {
        double m = std::fabs((double)cam->view_inverse[12 + c]);
        for (int k = 0; k < 3; k++) m += std::fabs((double)cam->view_inverse[4 * k + c]) * pp[k];
        need[c] = m * 1.001;
    }
    return ensure_tlas_reach(s, need);
}

// DSceneView::flat_normals from the items and triangles on the device (k_world_normals); after every upload of the items' transforms
// ... and the extent of every item's surface along its transform's rows (k_item_spans -> s->data.h_spans, for the top level's surface boxes).
// Everything that depends on the transforms and on the meshes is derived HERE, on the device, where the meshes are resident: the one
// blocking copy of 72 B per item at the end is the call's only wait.
static_assert(RR_HOST_ITEM_CHUNK == RR_ITEM_CHUNK, "the host's chunk map is the kernels'");
// the spans of n items before any chunk is merged into them: what k_item_spans gives a ball or an empty mesh
static void empty_spans(uint32_t n, std::vector<double>* spans) {
    spans->resize(9 * (size_t)n);
    for (uint32_t i = 0; i < n; i++)
        for (int k = 0; k < 9; k++) (*spans)[9 * (size_t)i + k] = k < 3 ? std::numeric_limits<double>::infinity() : (k < 6 ? -std::numeric_limits<double>::infinity() : 0.0);
}
// one chunk's 9 doubles (k_item_spans) into its item's
static void merge_chunk_span(const double* q, double* d) {
    for (int k = 0; k < 9; k++) {
        if (q[k] != q[k]) d[k] = q[k];                       // a NaN chunk poisons the item (the corner box is kept for it)
        else if (d[k] == d[k]) d[k] = k < 3 ? std::min(d[k], q[k]) : std::max(d[k], q[k]);
    }
}
static int derive_from_transforms(rr_scene* s) {
    const uint32_t n = (uint32_t)s->data.h_items.size();
    s->data.h_spans.clear();
    if (n == 0) return RR_OK;
    if (s->data.h_chunk_item.empty()) { // the chunk map depends on the items' triangle counts only: laid out once
        std::vector<uint2> chunks;
        item_chunk_map(s->data.h_items, &chunks, &s->data.h_chunk_item);
        HIP_TRY(s->data.item_chunks.reserve(chunks.size() * sizeof(uint2)));
        HIP_TRY(hipMemcpy(s->data.item_chunks.p, chunks.data(), chunks.size() * sizeof(uint2), hipMemcpyHostToDevice));
        HIP_TRY(s->data.spans.reserve(9 * sizeof(double) * chunks.size()));
    }
    const size_t nc = s->data.h_chunk_item.size();
    if (nc > 0x7fffffffull) return fail(RR_ERR_UNSUPPORTED, "%zu chunks of instanced triangles", nc);
    hipLaunchKernelGGL(k_world_normals, dim3((uint32_t)nc), dim3(RR_BLOCK), 0, nullptr, s->data.items.as<DItem>(), s->data.item_chunks.as<uint2>(), s->data.tris.as<DTri>(), s->data.flat_normals.as<float4>());
    hipLaunchKernelGGL(k_item_spans, dim3((uint32_t)nc), dim3(RR_BLOCK), 0, nullptr, s->data.items.as<DItem>(), s->data.item_chunks.as<uint2>(), s->data.tris.as<DTri>(), s->data.spans.as<double>());
    HIP_TRY(hipGetLastError());
    std::vector<double> part(9 * nc);
    HIP_TRY(hipMemcpy(part.data(), s->data.spans.p, 9 * sizeof(double) * nc, hipMemcpyDeviceToHost)); // (waits for both kernels)
    empty_spans(n, &s->data.h_spans);
    for (size_t c = 0; c < nc; c++) merge_chunk_span(&part[9 * c], &s->data.h_spans[9 * (size_t)s->data.h_chunk_item[c]]);
    return RR_OK;
}

// Test-only (tests/test_abi.py; not in the header): the host half of rr_scene_create -- validation and the threaded mesh tree
// builds -- without a device, so that the no-throw guard and the worker net can be exercised on a CPU-only box.
extern "C" int rr_test_host_build(const rr_flat_scene* fs, uint64_t* n_nodes_out) try {
    int rc = validate_scene(fs);
    if (rc != RR_OK) return rc;
    RR_FAULT_POINT("scene_create.host");
    std::vector<rr::BvhResult> built(fs->n_meshes);
    std::vector<char> built_ok(fs->n_meshes, 0);
    build_mesh_trees(fs, RR_BLAS_MAX_DEPTH, &built, &built_ok);
    uint64_t n = 0;
    for (uint32_t mi = 0; mi < fs->n_meshes; mi++) {
        if (!built_ok[mi]) return fail(RR_ERR_UNSUPPORTED, "mesh %u: BVH depth limit exceeded", mi);
        n += built[mi].nodes.size();
    }
    if (n_nodes_out) *n_nodes_out = n;
    return RR_OK;
} RR_GUARD_END("rr_test_host_build")

// the images' texels into the RGBA8 pool, at the offsets their descriptors name (append_texture_layout)
static int upload_images(uint32_t* pool, const rr_texture* textures, uint32_t n, const DTexture* dtex) {
    for (uint32_t i = 0; i < n; i++) {
        const uint64_t texels = (uint64_t)dtex[i].width * dtex[i].height;
        if (texels) HIP_TRY(hipMemcpy(pool + dtex[i].offset, textures[i].rgba8, texels * 4, hipMemcpyHostToDevice));
    }
    return RR_OK;
}

extern "C" int rr_scene_create(const rr_flat_scene* fs, int device, rr_scene** out) try {
    if (!out) return fail(RR_ERR_INVALID_ARGUMENT, "out is NULL");
    *out = nullptr;
    RR_TRY(validate_scene(fs));
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(RR_ERR_NO_DEVICE, "no HIP device available");
    if (device < 0 || device >= ndev) return fail(RR_ERR_INVALID_ARGUMENT, "device %d of %d", device, ndev);
    HIP_TRY(hipSetDevice(device));
    std::unique_ptr<rr_scene> s(new rr_scene);
    RR_FAULT_POINT("scene_create.host");
    s->device = device;
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    s->n_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;

    // u8 -> f32 table, exactly (float)i / 255.0f
    float lut[256];
    for (int i = 0; i < 256; i++) lut[i] = (float)i / 255.0f;
    HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(c_u8_to_f32), lut, sizeof lut));

    // ---- the records, built on the host (rr_scene_build.h), then uploaded; an empty array still gets a buffer
    SceneRecords r;
    RR_TRY(build_scene_records(fs, &r));
    HIP_TRY(s->data.texels.reserve(std::max<uint64_t>(pool_texels(r.dtex), 1) * 4));
    RR_TRY(upload_images(s->data.texels.as<uint32_t>(), fs->textures, fs->n_textures, r.dtex.data()));
    HIP_TRY(s->data.textures.upload(r.dtex, sizeof(DTexture)));
    HIP_TRY(s->data.materials.upload(r.dmat, sizeof(DMaterial)));
    HIP_TRY(s->data.lights.upload(r.dlights, sizeof(DLight)));
    HIP_TRY(s->data.nodes4.upload(r.nodes4, 16));
    HIP_TRY(s->data.tris.upload(r.tris, 16));
    HIP_TRY(s->data.trix.upload(r.trix, 16));
    HIP_TRY(s->data.attrs.upload(r.attrs, 16));
    HIP_TRY(s->data.face_slot.upload(r.face_slot, 16));
    HIP_TRY(s->data.items.upload(r.items, 16));
    HIP_TRY(s->data.flat_normals.reserve(flat_normals_bytes(r.n_flat_normals)));
    // the host copies that the scene's edits and queries work from
    s->data.tex_width.swap(r.tex_width); s->data.h_textures.swap(r.dtex); s->data.h_dmat.swap(r.dmat); s->data.h_lights.swap(r.dlights);
    s->data.h_items.swap(r.items); s->data.item_host.swap(r.item_host);
    s->data.mesh_table.swap(r.meshes); s->data.n_nodes4 = r.nodes4.size(); s->data.n_mesh_tris = r.tris.size(); s->data.blas_depth_limit = r.blas_depth_limit;
    s->data.h_meshes.reserve(fs->n_meshes);
    for (uint32_t i = 0; i < fs->n_meshes; i++) s->data.h_meshes.emplace_back(fs->meshes[i]);
    s->data.n_materials = fs->n_materials;
    s->data.n_enabled_lights = r.n_enabled_lights;
    s->tlas.depth_limit = r.tlas_depth_limit;
    RR_TRY(derive_from_transforms(s.get())); // flat world normals; the extent of every item's surface, for the top level below

    // ---- top level: always present (even for one item), so the kernels have a single traversal path.
    // The reference's choice between "all items" and its scene BVH (src/raytracing.rs:434) only changes the
    // candidate set, never the result.
    {
        TlasTrees trees;
        const double none[3] = {0.0, 0.0, 0.0};
        RR_TRY(build_tlas(s->data.h_items, s->data.h_spans, s->tlas.depth_limit, none, &trees));
        for (int c = 0; c < 3; c++) s->tlas.floor[c] = trees.reach[c];
        s->tlas.node_capacity = tlas_capacity(trees, fs->n_items);
        RR_TRY(reserve_tlas(&s->data.tnodes4, &s->data.item_boxes, trees, s->tlas.node_capacity));
        RR_TRY(upload_tlas(s.get(), trees));
    }

    point_view(s.get());
    s->data.view.general_w = r.general_w ? 1u : 0u;
    s->data.view.any_alpha_occluder = r.any_alpha_occluder ? 1u : 0u;

    RR_TRY(s->frame.init());
    RR_TRY(s->timing.init());
    *out = s.release();
    return RR_OK;
} RR_GUARD_END("rr_scene_create")

extern "C" void rr_scene_destroy(rr_scene* s) {
    if (!s) return;
    try {
        (void)hipSetDevice(s->device);
        (void)hipDeviceSynchronize();
        delete s; // ~rr_scene: events, pinned memory; ~DevBuf: every device buffer
    } catch (...) { (void)guard_fail("rr_scene_destroy"); }
}

// ---------------------------------------------------------------------------
// scene edits: all or nothing
// ---------------------------------------------------------------------------
// Runs apply(); when it fails -- a status code or an exception -- runs restore(), which puts back everything apply may have written,
// and returns apply's status and message.  When restore fails as well the scene holds a mix of before and after: *broken is set, and
// frame calls refuse (check_intact) until an update of the same kind succeeds.
template <class Apply, class Restore>
static int all_or_nothing(const char* fn, bool* broken, Apply apply, Restore restore) {
    int rc;
    try { rc = apply(); } catch (...) { rc = guard_fail(fn); }
    if (rc == RR_OK) { *broken = false; return RR_OK; }
    std::string msg;
    try { msg = tl_error; } catch (...) { /* the code still says what happened */ }
    int rrc;
    try { rrc = restore(); } catch (...) { rrc = guard_fail(fn); }
    if (rrc != RR_OK) {
        *broken = true;
        return fail(rc, "%s; rolling back failed too (%s): the scene is broken until an update succeeds", msg.c_str(), tl_error.c_str());
    }
    try { tl_error = msg; } catch (...) {}
    return rc;
}
// The items' records to the device, then what derives from their transforms there: the update's way there and its way back.
static int upload_items_and_derive(rr_scene* s) {
    HIP_TRY(hipDeviceSynchronize()); // no frame may be in flight on the records that change (a caller that renders asynchronously through rr_render_region_device)
    HIP_TRY(hipMemcpyAsync(s->data.items.p, s->data.h_items.data(), s->data.h_items.size() * sizeof(DItem), hipMemcpyHostToDevice, nullptr));
    RR_FAULT_POINT("update_transforms.derive");
    return derive_from_transforms(s);
}

// All or nothing: every matrix is checked before anything is written, and a failure after the first write puts the items, their
// flat normals and spans, the top level and the view back as they were (derive_from_transforms and build_tlas are deterministic).
extern "C" int rr_scene_update_transforms(rr_scene* s, const float* trans, const float* trans_inv) try {
    if (!s || !trans || !trans_inv) return fail(RR_ERR_INVALID_ARGUMENT, "NULL argument");
    RR_TRY(not_in_pass(s, "rr_scene_update_transforms"));
    std::lock_guard<std::mutex> lk(s->mu);
    HIP_TRY(hipSetDevice(s->device));
    RR_FAULT_POINT("update_transforms.host");
    const uint32_t n = (uint32_t)s->data.h_items.size();
    bool general_w = false;
    for (uint32_t i = 0; i < n; i++) {
        const float *t = trans + 16 * (size_t)i, *ti = trans_inv + 16 * (size_t)i;
        RR_TRY(check_item_transform(i, t, ti));
        if (!affine_inverse(make_float4(ti[3], ti[7], ti[11], ti[15]))) general_w = true;
    }
    // what the update writes, for the way back
    const std::vector<DItem> items0 = s->data.h_items;
    const std::vector<double> spans0 = s->data.h_spans;
    const std::vector<float4> boxes0 = s->tlas.h_item_boxes;
    double reach0[3], floor0[3];
    memcpy(reach0, s->tlas.reach, sizeof reach0); memcpy(floor0, s->tlas.floor, sizeof floor0);
    const DSceneView view0 = s->data.view;
    const bool has_surface0 = s->tlas.has_surface; // (which tree view0.tnodes4c names)
    auto apply = [&]() -> int {
        for (uint32_t i = 0; i < n; i++) fill_item_matrices(s->data.h_items[i], trans + 16 * (size_t)i, trans_inv + 16 * (size_t)i);
        RR_TRY(upload_items_and_derive(s));
        s->data.view.general_w = general_w ? 1u : 0u;
        TlasTrees trees;
        const double none[3] = {0.0, 0.0, 0.0};
        RR_TRY(build_tlas(s->data.h_items, s->data.h_spans, s->tlas.depth_limit, none, &trees)); // the next frame's camera grows the reach again if it has to
        RR_FAULT_POINT("update_transforms.upload_tlas");
        RR_TRY(upload_tlas(s, trees));
        for (int c = 0; c < 3; c++) s->tlas.floor[c] = s->tlas.reach[c];
        return RR_OK;
    };
    auto restore = [&]() -> int {
        s->data.h_items = items0; s->data.h_spans = spans0; s->tlas.h_item_boxes = boxes0;
        memcpy(s->tlas.reach, reach0, sizeof reach0); memcpy(s->tlas.floor, floor0, sizeof floor0);
        s->data.view = view0; s->tlas.has_surface = has_surface0;
        RR_TRY(upload_items_and_derive(s)); // the flat normals and spans of before, bit for bit
        TlasTrees trees;
        RR_TRY(build_tlas(s->data.h_items, s->data.h_spans, s->tlas.depth_limit, reach0, &trees)); // reach0 already covers the items: the same reach, boxes and trees as before
        RR_TRY(upload_tlas(s, trees));
        s->data.view = view0; s->tlas.has_surface = has_surface0;
        return RR_OK;
    };
    return all_or_nothing("rr_scene_update_transforms", &s->broken_geometry, apply, restore);
} RR_GUARD_END("rr_scene_update_transforms")

// Records of an update to buffers that hold them already: the update's way there and its way back.  `point` (a test's fault point) is
// crossed after the first copy: between the two of a material update, behind the only one of the others.
struct RecordCopy { void* dst; const void* src; size_t bytes; };
static int copy_records(const char* point, std::initializer_list<RecordCopy> copies) {
    HIP_TRY(hipDeviceSynchronize()); // no frame enqueued through rr_render_region_device may still read the records
    for (const RecordCopy& c : copies) {
        if (c.bytes) HIP_TRY(hipMemcpy(c.dst, c.src, c.bytes, hipMemcpyHostToDevice));
        if (&c == copies.begin()) RR_FAULT_POINT(point);
    }
    return RR_OK;
}
template <class T> static RecordCopy records_to(const DevBuf& b, const std::vector<T>& v) { return RecordCopy{b.p, v.data(), v.size() * sizeof(T)}; }

// Material edits between frames (GUI sliders: reference src/run.rs:1132-1133 writes through Material::apply_diff,
// src/shape/mod.rs:182-242): every material record is replaced and the item flag words derived from the material
// caches are rebuilt; geometry, acceleration structures and texture images stay as uploaded.  All or nothing: after a failed copy the
// records of before are copied back.
extern "C" int rr_scene_update_materials(rr_scene* s, const rr_material* materials, uint32_t n_materials) try {
    if (!s || !materials) return fail(RR_ERR_INVALID_ARGUMENT, "NULL argument");
    RR_TRY(not_in_pass(s, "rr_scene_update_materials"));
    std::lock_guard<std::mutex> lk(s->mu);
    if (n_materials != s->data.n_materials) return fail(RR_ERR_INVALID_ARGUMENT, "%u materials, the scene was created with %u", n_materials, s->data.n_materials);
    RR_TRY(check_material_textures(materials, n_materials, s->data.tex_width.size()));
    for (const ItemHost& ih : s->data.item_host)
        if (carries_textures(materials[ih.material_cache]))
            return fail(RR_ERR_INVALID_ARGUMENT, "material %d is a material cache and must not carry textures (reference src/shape/mod.rs:769-772)", ih.material_cache);
    HIP_TRY(hipSetDevice(s->device));
    std::vector<DMaterial> dmat(n_materials);
    for (uint32_t i = 0; i < n_materials; i++) dmat[i] = make_dmaterial(materials[i], s->data.tex_width, s->data.h_textures);
    // the item flag words and the alpha-occluder hint of the new materials: the scene keeps them once both copies have succeeded
    std::vector<DItem> items = s->data.h_items;
    uint32_t any_alpha_occluder = 0u;
    for (size_t i = 0; i < s->data.item_host.size(); i++) {
        items[i].flags = item_flags(s->data.item_host[i], materials[s->data.item_host[i].material_cache], materials[s->data.item_host[i].material], s->data.tex_width);
        if (items[i].flags & RR_IF_OCCLUDER_ALPHA_TEX) any_alpha_occluder = 1u;
    }
    auto apply = [&]() -> int { return copy_records("update_materials.device", {records_to(s->data.materials, dmat), records_to(s->data.items, items)}); };
    auto restore = [&]() -> int { // the host copies still hold the records of before
        return copy_records("update_materials.device", {records_to(s->data.materials, s->data.h_dmat), records_to(s->data.items, s->data.h_items)});
    };
    RR_TRY(all_or_nothing("rr_scene_update_materials", &s->broken_materials, apply, restore));
    s->data.h_items.swap(items);
    s->data.h_dmat.swap(dmat);
    s->data.view.any_alpha_occluder = any_alpha_occluder;
    return RR_OK;
} RR_GUARD_END("rr_scene_update_materials")

// Light edits between frames (the GUI's light panel: reference src/run.rs:1294-1409 adds, edits and deletes `Scene::lights`): the
// whole list is replaced; its length may change.  A light's index is the RNG stream of its shadow jitter, so the list is taken in
// the caller's order, as rr_scene_create takes it.  A list longer than the buffer holds goes to a new buffer that replaces the old
// one only after the copy.  All or nothing: after a failed copy the records of before are copied back.
extern "C" int rr_scene_update_lights(rr_scene* s, const rr_light* lights, uint32_t n_lights) try {
    if (!s || (n_lights && !lights)) return fail(RR_ERR_INVALID_ARGUMENT, "NULL argument");
    RR_TRY(not_in_pass(s, "rr_scene_update_lights"));
    std::lock_guard<std::mutex> lk(s->mu);
    RR_TRY(check_lights(lights, n_lights));
    HIP_TRY(hipSetDevice(s->device));
    uint32_t n_enabled = 0;
    std::vector<DLight> dl = make_dlights(lights, n_lights, &n_enabled);
    DevBuf grown; // a list longer than the scene's buffer holds goes to a new one
    const bool grow = (size_t)n_lights * sizeof(DLight) > s->data.lights.bytes;
    if (grow) HIP_TRY(grown.reserve((size_t)n_lights * sizeof(DLight)));
    auto apply = [&]() -> int { return copy_records("update_lights.device", {records_to(grow ? grown : s->data.lights, dl)}); };
    auto restore = [&]() -> int { return copy_records("update_lights.device", {records_to(s->data.lights, s->data.h_lights)}); };
    RR_TRY(all_or_nothing("rr_scene_update_lights", &s->broken_lights, apply, restore));
    // the device holds the new records: the frame path reads the count, the enabled count (shadow-queue plan, fixed shadow slots) and the pointer together
    if (grow) s->data.lights = std::move(grown); // frees the old buffer: nothing reads it since the synchronisation in copy_records
    s->data.h_lights.swap(dl);
    s->data.n_enabled_lights = n_enabled;
    point_view(s);
    return RR_OK;
} RR_GUARD_END("rr_scene_update_lights")

// The GUI's "Visible" and "flip normals" checkboxes (reference src/run.rs:1464-1489, ShapeBasics::visible / flip_normals): only
// RR_IF_VISIBLE and RR_IF_FLIP_NORMALS of each item's flag word change.  The kernels read both per candidate and per hit
// (rr_kernels.hip), the flat world normals hold both signs, and hidden items keep their place in the top level: nothing is re-derived.
// item_host keeps the new values, from which rr_scene_update_materials rebuilds the flag words.  All or nothing, as the others.
extern "C" int rr_scene_update_item_flags(rr_scene* s, const uint8_t* visible, const uint8_t* flip_normals, uint32_t n_items) try {
    if (!s || !visible || !flip_normals) return fail(RR_ERR_INVALID_ARGUMENT, "NULL argument");
    RR_TRY(not_in_pass(s, "rr_scene_update_item_flags"));
    std::lock_guard<std::mutex> lk(s->mu);
    if (n_items != s->data.h_items.size()) return fail(RR_ERR_INVALID_ARGUMENT, "%u items, the scene was created with %zu", n_items, s->data.h_items.size());
    HIP_TRY(hipSetDevice(s->device));
    std::vector<DItem> items = s->data.h_items;
    for (uint32_t i = 0; i < n_items; i++)
        items[i].flags = (items[i].flags & ~(uint32_t)(RR_IF_VISIBLE | RR_IF_FLIP_NORMALS)) | (visible[i] ? (uint32_t)RR_IF_VISIBLE : 0u) |
                         (flip_normals[i] ? (uint32_t)RR_IF_FLIP_NORMALS : 0u);
    auto apply = [&]() -> int { return copy_records("update_item_flags.device", {records_to(s->data.items, items)}); };
    auto restore = [&]() -> int { return copy_records("update_item_flags.device", {records_to(s->data.items, s->data.h_items)}); };
    RR_TRY(all_or_nothing("rr_scene_update_item_flags", &s->broken_item_flags, apply, restore));
    s->data.h_items.swap(items);
    for (uint32_t i = 0; i < n_items; i++) { s->data.item_host[i].visible = visible[i] != 0; s->data.item_host[i].flip_normals = flip_normals[i] != 0; }
    return RR_OK;
} RR_GUARD_END("rr_scene_update_item_flags")

// A material's texture "+" (reference src/run.rs:936-947 loads a new image): the images are appended to the scene's texture list,
// in order, and *first_index is the index of the first.  rr_scene_create lays the RGBA8 pool out in list order, so the existing
// images keep their offsets and the new ones get those a scene created with the longer list gives them.  The grown pool and
// descriptor array are built aside (device-to-device copy of the old pool, upload of the new images) and replace the old ones only
// once complete: a failure leaves the scene as it was, with nothing to roll back.  Texture memory never shrinks.
extern "C" int rr_scene_add_textures(rr_scene* s, const rr_texture* textures, uint32_t n_textures, uint32_t* first_index) try {
    if (!s || !first_index || (n_textures && !textures)) return fail(RR_ERR_INVALID_ARGUMENT, "NULL argument");
    RR_TRY(not_in_pass(s, "rr_scene_add_textures"));
    std::lock_guard<std::mutex> lk(s->mu);
    RR_TRY(check_textures(textures, n_textures));
    const uint32_t first = (uint32_t)s->data.tex_width.size();
    if (n_textures == 0) { *first_index = first; return RR_OK; }
    HIP_TRY(hipSetDevice(s->device));
    std::vector<DTexture> dtex = s->data.h_textures;
    std::vector<uint32_t> widths = s->data.tex_width;
    const uint64_t old_texels = pool_texels(dtex);
    append_texture_layout(textures, n_textures, &dtex, &widths);
    DevBuf texels, descs;
    HIP_TRY(texels.reserve(std::max<uint64_t>(pool_texels(dtex), 1) * 4));
    if (old_texels) HIP_TRY(hipMemcpy(texels.p, s->data.texels.p, old_texels * 4, hipMemcpyDeviceToDevice)); // frames in flight only read the old pool
    RR_TRY(upload_images(texels.as<uint32_t>(), textures, n_textures, &dtex[first]));
    HIP_TRY(descs.upload(dtex, sizeof(DTexture)));
    RR_FAULT_POINT("add_textures.device");
    HIP_TRY(hipDeviceSynchronize()); // no frame enqueued through rr_render_region_device may still read the pool that is freed below
    // the pool and the descriptors of the longer list replace the old ones (frees them); material records keep their descriptors
    // (the old images did not move) and name the new images after a rr_scene_update_materials
    s->data.texels = std::move(texels);
    s->data.textures = std::move(descs);
    s->data.h_textures.swap(dtex);
    s->data.tex_width.swap(widths);
    point_view(s);
    *first_index = first;
    return RR_OK;
} RR_GUARD_END("rr_scene_add_textures")

// ---------------------------------------------------------------------------
// structural edits: meshes appended, the item list replaced
// ---------------------------------------------------------------------------
// Both build what changes BESIDE what the scene holds -- new device buffers, new host vectors -- and commit by moving buffers, host
// copies and the view last, after the device has finished every frame in flight.  Nothing the scene renders from is written before
// the commit and nothing in the commit can fail, so a failure leaves the scene exactly as it was: there is no way back to take and
// no "broken" state (check_intact has no flag for these).

// The device copies of the mesh arenas: `before` records of the scene's own buffers (device to device), then the host's records.
struct MeshBuffers { DevBuf nodes4, tris, trix, attrs, face_slot; };
template <class T> static int grown_copy(DevBuf* dst, const DevBuf& resident, size_t before, const std::vector<T>& more) {
    HIP_TRY(dst->reserve(std::max<size_t>((before + more.size()) * sizeof(T), 16)));
    if (before) HIP_TRY(hipMemcpy(dst->p, resident.p, before * sizeof(T), hipMemcpyDeviceToDevice)); // frames in flight only read the resident records
    if (!more.empty()) HIP_TRY(hipMemcpy(dst->as<T>() + before, more.data(), more.size() * sizeof(T), hipMemcpyHostToDevice));
    return RR_OK;
}
static int upload_mesh_arenas(const rr_scene* s, const MeshArenas& a, MeshBuffers* b) {
    RR_TRY(grown_copy(&b->nodes4, s->data.nodes4, a.nodes4_before, a.nodes4));
    RR_TRY(grown_copy(&b->tris, s->data.tris, a.tris_before, a.tris));
    RR_TRY(grown_copy(&b->trix, s->data.trix, a.tris_before, a.trix));
    RR_TRY(grown_copy(&b->attrs, s->data.attrs, a.tris_before, a.attrs));
    return grown_copy(&b->face_slot, s->data.face_slot, a.tris_before, a.face_slot);
}
// the commit's half for the meshes
static void keep_mesh_buffers(rr_scene* s, MeshBuffers& b) noexcept {
    s->data.nodes4 = std::move(b.nodes4); s->data.tris = std::move(b.tris); s->data.trix = std::move(b.trix); s->data.attrs = std::move(b.attrs); s->data.face_slot = std::move(b.face_slot);
    point_view(s);
}

// The GUI's "add ground plane" (reference src/scene.rs:1564-1578 loads a scene file with a mesh the scene does not hold yet): the
// meshes are appended to the scene's mesh list, in order, and *first_index is the index of the first.  A mesh's records name
// nothing outside the mesh (rr_scene_build.h: MeshArenas), so the resident meshes keep their records and the new ones get those a
// scene created with the longer list gives them; their trees are built for the scene's current share of the traversal stack.
// Nothing is rendered from them until rr_scene_set_items names them.  Mesh memory never shrinks.
extern "C" int rr_scene_add_meshes(rr_scene* s, const rr_mesh* meshes, uint32_t n_meshes, uint32_t* first_index) try {
    if (!s || !first_index || (n_meshes && !meshes)) return fail(RR_ERR_INVALID_ARGUMENT, "NULL argument");
    RR_TRY(not_in_pass(s, "rr_scene_add_meshes"));
    std::lock_guard<std::mutex> lk(s->mu);
    const uint32_t first = (uint32_t)s->data.mesh_table.size();
    RR_TRY(check_meshes(meshes, n_meshes, first));
    if (n_meshes == 0) { *first_index = first; return RR_OK; }
    if ((uint64_t)first + n_meshes > 0x7fffffffull) return fail(RR_ERR_UNSUPPORTED, "%u + %u meshes (rr_item::mesh is an int32_t)", first, n_meshes);
    HIP_TRY(hipSetDevice(s->device));
    MeshArenas a;
    a.meshes = s->data.mesh_table;
    a.tris_before = s->data.n_mesh_tris; a.nodes4_before = s->data.n_nodes4;
    RR_TRY(append_mesh_records(meshes, n_meshes, s->data.blas_depth_limit, (uint32_t)s->data.h_items.size(), &a));
    std::vector<HostMesh> h_meshes;
    h_meshes.reserve(s->data.h_meshes.size() + n_meshes);
    for (uint32_t i = 0; i < n_meshes; i++) h_meshes.emplace_back(meshes[i]);
    s->data.h_meshes.reserve(s->data.h_meshes.size() + n_meshes); // (capacity only: the commit's moves then cannot fail)
    MeshBuffers b;
    RR_TRY(upload_mesh_arenas(s, a, &b));
    RR_FAULT_POINT("add_meshes.device");
    HIP_TRY(hipDeviceSynchronize()); // no frame enqueued through rr_render_region_device may still read the arenas that are freed below
    // ---- commit
    keep_mesh_buffers(s, b);
    s->data.n_nodes4 = a.nodes4_before + a.nodes4.size(); s->data.n_mesh_tris = a.tris_before + a.tris.size();
    s->data.mesh_table.swap(a.meshes);
    for (HostMesh& m : h_meshes) s->data.h_meshes.push_back(std::move(m));
    *first_index = first;
    return RR_OK;
} RR_GUARD_END("rr_scene_add_meshes")

// The GUI's "delete" of an object, "add ground plane" and "add environment sphere" (reference src/scene.rs:1602-1620, :1564-1578):
// the whole item list and the whole material list are replaced, together -- items name materials by index, and a host that keeps
// the material caches behind the full materials moves every cache index when one item comes or goes.  Any item count, any order; an
// item may name any resident mesh, a material any resident texture; the checks and limits are rr_scene_create's.  Afterwards the
// handle renders, bit for bit, what a handle created from the flat scene (resident meshes and textures, current lights, these items
// and materials) renders.
//   Device work follows what changed: an item whose matrices, mesh and flag word are those of an item of the list before keeps that
// item's surface spans (host copy) and flat world normals (k_world_normals_edit copies its run into the new arena); only the other
// mesh items are derived.  The top level is rebuilt (host, items only).
//   The stack share: the top level's share of the traversal stack depends on the item count (stack_shares), and the per-mesh trees
// are built and collapsed for the rest.  An edit that changes the share rebuilds every mesh's records from the scene's host copies,
// as a fresh scene builds them (and derives every item: the leaf order changed); a mesh that no longer fits is RR_ERR_UNSUPPORTED.
extern "C" int rr_scene_set_items(rr_scene* s, const rr_item* items, uint32_t n_items, const rr_material* materials, uint32_t n_materials) try {
    if (!s || (n_items && !items) || (n_materials && !materials)) return fail(RR_ERR_INVALID_ARGUMENT, "NULL argument");
    RR_TRY(not_in_pass(s, "rr_scene_set_items"));
    std::lock_guard<std::mutex> lk(s->mu);
    RR_TRY(check_intact(s)); // (a scene that an earlier edit left mixed has no derived data worth keeping)
    RR_TRY(check_material_textures(materials, n_materials, s->data.tex_width.size()));
    int tlas_depth_limit = 0, blas_depth_limit = 0;
    if (n_items < (1u << 27)) RR_TRY(stack_shares(n_items, &tlas_depth_limit, &blas_depth_limit)); // the count's limits before an item is read
    RR_TRY(check_items(items, n_items, materials, n_materials, s->data.mesh_table.size()));
    HIP_TRY(hipSetDevice(s->device));

    // ---- the meshes, when their share of the stack changes: every record anew
    const bool rebuild_meshes = blas_depth_limit != s->data.blas_depth_limit && !s->data.h_meshes.empty();
    MeshArenas arenas;
    MeshBuffers mesh_buffers;
    if (rebuild_meshes) {
        std::vector<rr_mesh> views;
        views.reserve(s->data.h_meshes.size());
        for (const HostMesh& m : s->data.h_meshes) views.push_back(m.view());
        RR_TRY(append_mesh_records(views.data(), (uint32_t)views.size(), blas_depth_limit, n_items, &arenas));
        RR_TRY(upload_mesh_arenas(s, arenas, &mesh_buffers));
    }
    const std::vector<MeshDev>& mesh_table = rebuild_meshes ? arenas.meshes : s->data.mesh_table;
    const DTri* tris = rebuild_meshes ? mesh_buffers.tris.as<DTri>() : s->data.tris.as<DTri>();

    // ---- item and material records
    ItemRecords rec;
    RR_TRY(build_item_records(items, n_items, materials, mesh_table, s->data.tex_width, &rec));
    std::vector<DMaterial> dmat(n_materials);
    for (uint32_t i = 0; i < n_materials; i++) dmat[i] = make_dmaterial(materials[i], s->data.tex_width, s->data.h_textures);

    // ---- keep or derive, per chunk of the new chunk map
    std::vector<uint2> chunks;
    std::vector<uint32_t> chunk_item;
    item_chunk_map(rec.items, &chunks, &chunk_item);
    const size_t nc = chunks.size();
    if (nc > 0x7fffffffull) return fail(RR_ERR_UNSUPPORTED, "%zu chunks of instanced triangles", nc);
    std::vector<int32_t> keep_from;
    const bool old_spans = s->data.h_spans.size() == 9 * s->data.h_items.size();
    const std::vector<DItem> no_items;
    plan_item_reuse(rebuild_meshes || !old_spans ? no_items : s->data.h_items, rec.items, &keep_from);
    std::vector<uint32_t> chunk_src(nc, RR_CHUNK_DERIVE);
    std::vector<uint2> derive_chunks;
    std::vector<uint32_t> derive_item;
    for (size_t c = 0; c < nc; c++) {
        const uint32_t i = chunk_item[c];
        if (rec.items[i].flags & RR_IF_SPHERE) continue; // nothing is derived for a ball
        if (keep_from[i] >= 0) chunk_src[c] = s->data.h_items[keep_from[i]].wn_base;
        else { derive_chunks.push_back(chunks[c]); derive_item.push_back(i); }
    }
    const size_t nd = derive_chunks.size();

    // ---- the new device state, beside the old
    DevBuf d_items, d_materials, d_flat_normals, d_item_chunks, d_spans, d_chunk_src, d_derive_chunks, d_tnodes4, d_item_boxes;
    HIP_TRY(d_items.upload(rec.items, 16));
    HIP_TRY(d_materials.upload(dmat, sizeof(DMaterial)));
    HIP_TRY(d_flat_normals.reserve(flat_normals_bytes(rec.n_flat_normals)));
    HIP_TRY(d_item_chunks.upload(chunks, 16));
    HIP_TRY(d_spans.reserve(std::max<size_t>(9 * sizeof(double) * nc, 16))); // room for every chunk: a transform update derives them all
    HIP_TRY(d_chunk_src.upload(chunk_src, 16));
    HIP_TRY(d_derive_chunks.upload(derive_chunks, 16));
    std::vector<double> spans;
    empty_spans(n_items, &spans);
    for (uint32_t i = 0; i < n_items; i++)
        if (keep_from[i] >= 0) memcpy(&spans[9 * (size_t)i], &s->data.h_spans[9 * (size_t)keep_from[i]], 9 * sizeof(double));
    if (nc) hipLaunchKernelGGL(k_world_normals_edit, dim3((uint32_t)nc), dim3(RR_BLOCK), 0, nullptr, d_items.as<DItem>(), d_item_chunks.as<uint2>(), d_chunk_src.as<uint32_t>(),
                               tris, s->data.flat_normals.as<float4>(), d_flat_normals.as<float4>());
    if (nd) hipLaunchKernelGGL(k_item_spans, dim3((uint32_t)nd), dim3(RR_BLOCK), 0, nullptr, d_items.as<DItem>(), d_derive_chunks.as<uint2>(), tris, d_spans.as<double>());
    HIP_TRY(hipGetLastError());
    if (nd) {
        std::vector<double> part(9 * nd);
        HIP_TRY(hipMemcpy(part.data(), d_spans.p, 9 * sizeof(double) * nd, hipMemcpyDeviceToHost)); // (waits for both kernels)
        for (size_t c = 0; c < nd; c++) merge_chunk_span(&part[9 * c], &spans[9 * (size_t)derive_item[c]]);
    }

    // ---- the top level over the new items, as rr_scene_create builds it
    TlasTrees trees;
    const double none[3] = {0.0, 0.0, 0.0};
    RR_TRY(build_tlas(rec.items, spans, tlas_depth_limit, none, &trees));
    const uint32_t capacity = tlas_capacity(trees, n_items);
    RR_TRY(reserve_tlas(&d_tnodes4, &d_item_boxes, trees, capacity));
    RR_TRY(copy_tlas(trees, d_tnodes4.as<DNode4>(), capacity, d_item_boxes.as<float4>()));
    RR_FAULT_POINT("set_items.device");
    HIP_TRY(hipDeviceSynchronize()); // the kernels above; and no frame enqueued through rr_render_region_device may still read what is freed below

    // ---- commit: buffers, host copies, the view
    if (rebuild_meshes) {
        keep_mesh_buffers(s, mesh_buffers);
        s->data.mesh_table.swap(arenas.meshes);
        s->data.n_nodes4 = arenas.nodes4.size(); s->data.n_mesh_tris = arenas.tris.size();
    }
    s->data.blas_depth_limit = blas_depth_limit; s->tlas.depth_limit = tlas_depth_limit;
    s->data.items = std::move(d_items); s->data.materials = std::move(d_materials); s->data.flat_normals = std::move(d_flat_normals);
    s->data.item_chunks = std::move(d_item_chunks); s->data.spans = std::move(d_spans); s->data.tnodes4 = std::move(d_tnodes4); s->data.item_boxes = std::move(d_item_boxes);
    s->data.h_items.swap(rec.items); s->data.item_host.swap(rec.item_host); s->data.h_dmat.swap(dmat); s->data.h_spans.swap(spans); s->data.h_chunk_item.swap(chunk_item);
    s->data.n_materials = n_materials;
    s->tlas.node_capacity = capacity;
    s->data.view.general_w = rec.general_w ? 1u : 0u;
    s->data.view.any_alpha_occluder = rec.any_alpha_occluder ? 1u : 0u;
    for (int c = 0; c < 3; c++) s->tlas.floor[c] = trees.reach[c];
    keep_tlas(s, trees); // (and points the view at everything moved above)
    s->tlas.stale = false;
    return RR_OK;
} RR_GUARD_END("rr_scene_set_items")

