// rr_api_handle.h — the scene handle of the C ABI (rr_scene), in named parts: one per host layer of rr_api.hip.
// Offers: TimerKernel, TimedLaunch; POOL_WORDS; RAY_RECORD_BYTES; SceneData, TopLevel, FrameState, QueryState, AdaptiveState, DenoiseState, MotionState, RecordStage, MultiState, FrameTiming
//         and rr_scene, which holds one of each; HC_* (the words of FrameState::h_count); check_intact.
// Needs:  rr_api_base.h (fail, HIP_TRY, DevBuf), rr_scene_build.h (ItemHost, MeshDev, HostMesh), rr_device.h, rr_primary_setup.h, rr_motion.h (MoEntry).
// A layer that reads or borrows another layer's part says so in the spelling of the access (s->frame.h_count in a query).

enum TimerKernel { TK_CLOSEST, TK_SHADOW, TK_SHADE, TK_BINNING }; // what a timed launch ran (resolve_timers)
struct TimedLaunch { hipEvent_t a, b; TimerKernel kernel; bool level1; }; // level1: the kernel's level-1 build

static const uint32_t POOL_WORDS = 1u << 22; // per-batch counters (level sizes, fetch heads, shadow shard counts): 16 MB, zeroed per batch
// bytes per ray of the four record arrays r0, r1, r2, hit (DRayQueue): the frames' arena and the queries' records
static const size_t RAY_RECORD_BYTES[4] = {16, 16, 8, 16};

// ---- scene data: what the kernels read through the view, and the host copies the edits and queries work from.  Written by rr_api_scene.h.
struct SceneData {
    DevBuf items, nodes4, tnodes4, tris, trix, attrs, face_slot, materials, textures, texels, lights, flat_normals;
    DSceneView view{}; // its pointers and counts are set by point_view (rr_api_scene.h) after every move of a buffer above, and nowhere else
    std::vector<DItem> h_items;
    std::vector<ItemHost> item_host; // what rr_scene_update_materials needs to rebuild the item flag words
    // the meshes: where each one's records sit in the arenas (what an item takes from the mesh it names, rr_scene_set_items), how many
    // records the arenas hold (rr_scene_add_meshes appends behind them), the scene's own copy of the caller's arrays (the trees are
    // rebuilt from it when an edit of the item list changes their share of the traversal stack) and that share
    std::vector<MeshDev> mesh_table;
    std::vector<HostMesh> h_meshes;
    size_t n_nodes4 = 0, n_mesh_tris = 0;
    int blas_depth_limit = RR_BLAS_MAX_DEPTH;
    // per item: the extent of its surface along the rows of its transform (k_item_spans: minima, maxima, largest |local coordinate|; 9 doubles),
    // read back after every upload of the items' transforms; the top level's surface boxes are derived from it (exact_world_box)
    std::vector<double> h_spans;
    DevBuf spans, item_chunks;              // item_chunks: (item, first triangle) per workgroup of k_world_normals / k_item_spans (RR_ITEM_CHUNK triangles each)
    std::vector<uint32_t> h_chunk_item;     // the item of every chunk (chunks of one item are consecutive)
    std::vector<uint32_t> tex_width;
    std::vector<DTexture> h_textures; // descriptors of the uploaded images (copied into the material records, make_dmaterial)
    uint32_t n_materials = 0;
    uint32_t n_enabled_lights = 0;
    DevBuf item_boxes; // the top level's padded world boxes per item on the device (view.item_boxes); the trees themselves: tnodes4
    std::vector<DMaterial> h_dmat; // the material records on the device (rr_scene_update_materials puts them back after a failed update)
    std::vector<DLight> h_lights;  // the light records on the device (rr_scene_update_lights puts them back after a failed update)
};

// ---- the top level's host state (its device records are SceneData::tnodes4 and item_boxes).  Written by rr_api_scene.h.
struct TopLevel {
    uint32_t node_capacity = 0; // nodes per tree in SceneData::tnodes4: the corner tree in its first half, the surface tree in the second
    bool has_surface = false;   // the closest-hit walks take the surface tree (point_view: view.tnodes4c)
    std::vector<float4> h_item_boxes; // padded world boxes per item (lo, hi), built by build_tlas, kept by upload_tlas
    double reach[3] = {0.0, 0.0, 0.0}; // the top level's boxes are padded for ray origins within +-reach (build_tlas)
    double floor[3] = {0.0, 0.0, 0.0}; // ... and never for less than this: the items' own extent
    bool stale = false; // a top-level upload failed part-way: the device trees match no reach, the next frame rebuilds them
    int depth_limit = RR_TLAS_MAX_DEPTH; // the top level's share of the traversal stack (build_scene_records), for its rebuilds
};

// the words of FrameState::h_count.  HC_LIST_COUNT serves every list (rr_api_adaptive.h, rr_api_levels.h, rr_api_prefix.h): the calls are
// serialised by the scene's lock and each reads its count behind its own wait
enum : uint32_t {
    HC_LEVEL = 0,      // the next depth level's size (run_level)
    HC_REACH = 4,      // 4 words: the reach of a query's rays (await_reach, rr_api_query.h)
    HC_PIXEL_BAD = 8,  // the first entry of a pixel list outside the frame (fill_pixel_slots)
    HC_LIST_COUNT = 9, // the length of a refinement list (await_list_count, rr_api_adaptive.h)
};

// ---- frame state (grown on demand, reused across frames).  Written by rr_api_frame.h; the ray queries (rr_api_query.h) borrow h_count and
// last_stream, and rr_shade_rays the arena, the shadow queue, the accumulators and the counter pool (why that is safe: next to its body).
struct FrameState {
    DevBuf hit1;      // hit records of depth level 1 (the primary rays are derived from their index, not stored)
    DevBuf arena[4];  // ray records of the deeper live depth levels, SoA: r0 r1 r2 hit (RAY_RECORD_BYTES each)
    size_t arena_cap = 0; // rays
    uint32_t arena_factor = 2; // arena rays per primary ray of a batch; doubled after a frame that had to slice levels
    DevBuf sq[3];
    size_t sq_cap = 0;
    DevBuf sq3;         // rr_render_pixel_split: the diffuse part of every shadow ray's term, 16 B per ray of the queue; reserved by such a frame only
    DevBuf acc_diffuse; // ... and its three diffuse planes, 24 B per slot
    DevBuf sq_valid; // one 64-bit word per (enabled light, 64 shadow slots): which lanes hold a ray
    DevBuf acc_rgb, acc_normal, acc_depth, acc_id, acc_flags, shade_const;
    DevBuf region_xy, trace_order, pool, counters; // region_xy: pixel of each accumulator slot; trace_order: its output index
    // what primary_ray reads (rr_primary_setup.h): slot_c, the screen point of each slot's pixel centre, lives and dies with region_xy;
    // sample_tr, the screen offset of each sample, is uploaded when the sub-sample table or one of the frame constants in tr_key changes
    DevBuf slot_c, sample_tr;
    // rr_render_pixels with a list: the call's own slot table (the caller's entries and their centres, k_pixel_slots) and the first bad
    // index; the region's tables and their cache below are not touched, so the frame after a list call finds its map
    DevBuf pixel_xy, pixel_c, pixel_bad;
    std::vector<uint16_t> tr_table; PrimarySampleKey tr_key{}; bool tr_valid = false;
    std::vector<DevBuf> pool_more; // further segments of per-batch counters, for batches with very many launches (kept for the next frame)
    DevBuf tmp_out[4];
    DevBuf tmp_parts; // rr_render_pixel_parts, host form: the part records on the device (32 B per pixel and part)
    std::vector<uint32_t> h_region_xy;
    rr_region region_cached{0, 0, 0, 0};
    uint32_t region_w = 0, region_h = 0;
    hipEvent_t count_ready = nullptr;
    hipStream_t last_stream = nullptr; // frame state (queues, accumulators) is shared: frames on different streams are serialised
    // level 1 in stages (run_level1_stages): this handle's second non-blocking stream, created on first use on the handle's device, and per
    // shadow-queue buffer the event behind its shade launch (first stream) and behind its shadow launch (second stream)
    hipStream_t overlap_stream = nullptr;
    hipEvent_t stage_shaded[3] = {nullptr, nullptr, nullptr}, stage_traced[3] = {nullptr, nullptr, nullptr};
    // ... and the third one, which traces the closest hits of stage k + 1, k + 2, ... while stage k is shaded: it forks from the frame's stream
    // behind stage_fork, and stage_closest[k % 3] follows the closest-hit launch of stage k
    hipStream_t closest_stream = nullptr;
    hipEvent_t stage_fork = nullptr, stage_closest[3] = {nullptr, nullptr, nullptr};
    hipEvent_t stage_tail = nullptr; // behind the shadow launches of the last two stages: what the frame's stream joins late (rr_api_frame.h join_shadow)
    uint32_t overlap_stages = 0; // level-1 stages of the last frame that ran on the two streams (rr_scene_overlap_stages)
    uint32_t* h_count = nullptr; // pinned, 16 words, by HC_*: what the host waits for (every wait reads its word before the next one is issued)
    std::vector<uint16_t> table_cache; uint16_t table_samples = 0; // built-in sub-sample table of the last sample count
    // what every frame needs from the start (rr_scene_create, on the scene's device)
    int init() {
        HIP_TRY(pool.reserve(POOL_WORDS * 4));
        HIP_TRY(counters.reserve(RR_CNT_WORDS * 8));
        HIP_TRY(hipEventCreateWithFlags(&count_ready, hipEventDisableTiming));
        HIP_TRY(hipHostMalloc((void**)&h_count, 64, hipHostMallocDefault));
        return RR_OK;
    }
    ~FrameState() {
        if (count_ready) (void)hipEventDestroy(count_ready);
        if (h_count) (void)hipHostFree(h_count);
        for (hipEvent_t e : stage_shaded) if (e) (void)hipEventDestroy(e);
        for (hipEvent_t e : stage_traced) if (e) (void)hipEventDestroy(e);
        for (hipEvent_t e : stage_closest) if (e) (void)hipEventDestroy(e);
        if (stage_fork) (void)hipEventDestroy(stage_fork);
        if (stage_tail) (void)hipEventDestroy(stage_tail);
        if (overlap_stream) (void)hipStreamDestroy(overlap_stream);
        if (closest_stream) (void)hipStreamDestroy(closest_stream);
    }
};

// ---- ray queries (the host forms are the device forms behind a staging copy): what the launches of a device form read and write after the
// call has returned belongs to the handle, grows on demand and is never shrunk.  rec: the packed records r0, r1, r2 and the walks'
// raw hits (RAY_RECORD_BYTES: 16 + 16 + 8 + 16 = 56 B per ray of the largest closest-hit or shadow query, host or device form; a shadow
// query uses 48 of them); words: QW_* (rr_api_query.h); ids: the stream ids 0 .. n - 1 of rr_shade_rays_device without the caller's
// (4 B per result), or the slot -> output index map of a whole-frame rr_surface_pixels (4 B per pixel).  Written by rr_api_query.h and
// rr_api_surface_pixels.h.
struct QueryState {
    DevBuf rec[4], words, ids;
};

// ---- rr_refine_list_device and rr_render_adaptive (rr_api_adaptive.h): grown on demand, never shrunk.  scratch: per 8x8 block of the largest
// frame so far its 64-bit refine mask, then its count (after k_refine_scan: its offset), then one word, the list's length (12 B per
// block + 4).  The fused call keeps in addition the base frame's two part records per pixel (64 B), its list (4 B per pixel, padded)
// and the fine records of the largest padded list so far (32 B per entry).  Written by rr_api_adaptive.h.
// rr_refine_sublist_device and rr_render_adaptive_levels (rr_api_levels.h) use the same buffers -- scratch: 12 B per 64 entries of the list + 4;
// parts: the frame's part records and then every list's (64 B per pixel, rounded up to 64 pixels) -- and a second list buffer for the
// list made from a list (list2: 4 B per entry of the largest padded list so far).  Written by rr_api_levels.h as well.
// rr_render_adaptive_prefix (rr_api_prefix.h) uses scratch, list and list2 in the same way and keeps two sets of resident accumulators
// (acc_set: 64 B per slot, two slots per entry of the first padded list; rr_adaptive.h has the layout), written in turn level by level.
struct AdaptiveState {
    DevBuf scratch, parts, list, fine, list2, acc_set[2];
};

// ---- rr_denoise_records (rr_api_denoise.h): grown on demand, never shrunk.  work: the working colour (r, g, b, var), ping-pong, 16 B per
// pixel each; guide: normal and depth, 16 B; meta: object id and flags, 8 B -- 56 B per pixel of the largest frame so far.  Written by
// rr_api_denoise.h.  (rr_accumulate_records, rr_api_temporal.h, keeps nothing.)
struct DenoiseState {
    DevBuf work[2], guide, meta;
    DevBuf split[4]; // rr_denoise_split_records: the rest and direct record sets (32 B per pixel each) and their halves (64 B each)
};

// ---- rr_motion_records (rr_api_motion.h): grown on demand, never shrunk.  table: the call's table on the device, 112 B per entry of the
// largest list so far; slot: the same in pinned memory, what the copy on the caller's stream reads after the call has returned, four of
// them used in turn, each with the event behind its last copy (pending: there is one) -- a call waits for the copy of the fourth call
// before it, which reads the slot it is about to write, and for nothing else.  Written by rr_api_motion.h.
struct MotionSlot {
    MoEntry* h_table = nullptr; size_t entries = 0;
    hipEvent_t copied = nullptr; bool pending = false;
};
struct MotionState {
    DevBuf table;
    MotionSlot slot[4]; uint32_t next = 0;
    ~MotionState() {
        for (MotionSlot& m : slot) {
            if (m.copied) (void)hipEventDestroy(m.copied);
            if (m.h_table) (void)hipHostFree(m.h_table);
        }
    }
};

// ---- the host forms of the record calls (rr_denoise_records, rr_accumulate_records, rr_accumulate_split_records, rr_motion_records and
// the rest): the device's copies of the caller's arrays, argument k of a call in buf[k] (the most arguments: the sixteen of
// rr_accumulate_split_records), each only where the call has it; grown on demand, never shrunk, so a slot holds the largest argument any
// of the calls has put there.  One pool serves them all: a host form holds the scene's lock and returns with the null stream idle, on
// its failing paths as well (IdleOnExit), so no call finds another's copies in use.  Written by staged_host_call (rr_api_query.h).
struct RecordStage {
    DevBuf buf[16];
};

// ---- rr_render_multi (rr_api_multi.h)
struct MultiState {
    DevBuf part[4], cat[4]; // this device's compact buffers; on device slot 0 the concatenation of all
    hipStream_t stream = nullptr; // this handle's own non-blocking stream (created on first use)
    void* stage[4] = {nullptr, nullptr, nullptr, nullptr}; size_t stage_bytes[4] = {0, 0, 0, 0}; // pinned staging, devices without peer access
    ~MultiState() {
        if (stream) (void)hipStreamDestroy(stream);
        for (void* p : stage) if (p) (void)hipHostFree(p);
    }
};

// ---- what a frame cost: written by rr_api_frame.h; rr_render_multi adds its multi_* fields and rr_shade_rays counts its batches in `stats`
struct FrameTiming {
    rr_frame_stats stats{};
    bool stats_final = false; // stats already holds the sums over the passes of rr_render_progressive_tiles (nothing to collect from the device)
    // rr_render_adaptive: what its base pass cost, collected while the call waited for the list's length; added ONCE to what the device
    // reports for the fine pass when somebody asks (collect_stats_locked), so the call itself need not wait for its last launch.
    // rr_render_adaptive_levels: the sums over every pass but its last, in the same way
    rr_frame_stats carry{};
    bool has_carry = false;
    bool profiling = false;
    std::vector<TimedLaunch> timed;
    std::vector<hipEvent_t> event_pool;
    hipEvent_t frame_a = nullptr, frame_b = nullptr;
    int init() {
        HIP_TRY(hipEventCreate(&frame_a));
        HIP_TRY(hipEventCreate(&frame_b));
        return RR_OK;
    }
    ~FrameTiming() {
        for (hipEvent_t e : event_pool) (void)hipEventDestroy(e);
        for (auto& t : timed) { (void)hipEventDestroy(t.a); (void)hipEventDestroy(t.b); }
        if (frame_a) (void)hipEventDestroy(frame_a);
        if (frame_b) (void)hipEventDestroy(frame_b);
    }
};

struct rr_scene {
    int device = 0;
    int n_cus = 256;
    std::mutex mu;
    rr_tuning tuning{}; // rr_scene_set_tuning; all zero = automatic
    // An update that failed and could not be rolled back either (all_or_nothing): the device holds a mix of two scenes, and every
    // frame call refuses until an update of that kind succeeds.  geometry: items, flat normals, top level; materials: materials, item flags.
    // lights: the light records; item_flags: the items' records after a failed rr_scene_update_item_flags.
    bool broken_geometry = false, broken_materials = false, broken_lights = false, broken_item_flags = false;
    // one part per layer; each is written by its layer's file only (the exceptions are named at the part) and releases what it owns
    SceneData data;
    TopLevel tlas;
    FrameState frame;
    QueryState query;
    AdaptiveState adaptive;
    DenoiseState denoise;
    MotionState motion;
    RecordStage record_stage;
    MultiState multi;
    FrameTiming timing;
    ScheduleLog sched; // the schedule recorder (rr_schedule_log.h): off unless a test switches it on; written by rr_api_frame.h
    // Every release (hipFree in ~DevBuf, the events, streams and pinned memory in the parts' destructors) must run on the scene's
    // device.  A destructor's body runs before its class's members are destroyed, whatever their order of declaration: the
    // hipSetDevice here precedes every one of them, and `device` is a plain int that stays readable throughout.
    ~rr_scene() { (void)hipSetDevice(device); }
};

// every frame call on a scene: a scene that a failed update left mixed is not rendered
static int check_intact(const rr_scene* s) {
    if (s->broken_geometry || s->broken_materials || s->broken_lights || s->broken_item_flags)
        return fail(RR_ERR_DEVICE, "the scene is broken: a failed %s update could not be rolled back (update again, or create the scene anew)",
                    s->broken_geometry ? "transform" : s->broken_materials ? "material" : s->broken_lights ? "light" : "item flag");
    return RR_OK;
}

