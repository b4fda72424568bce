// rr_api_query.h — questions to a scene outside a frame: rr_pick, and the closest-hit, shadow, surface and radiance queries for rays of the caller's.
// Offers: rr_pick; check_query_pointer(s); launch_query_shadow; rr_trace_rays, rr_trace_shadow_rays, rr_surface_rays, rr_shade_rays,
//         rr_render_pixels and their *_device forms; for the list calls of the layers behind it: check_pixels_args, host_list_call,
//         render_pixels_locked; for the record calls (rr_api_denoise.h, rr_api_temporal.h, rr_api_motion.h, rr_api_surface_pixels.h):
//         check_arg_ranges, record_call, StageArg, stage_input, stage_output, staged_host_call (writes rr_scene::record_stage).
// Needs:  rr_arg_ranges.h, rr_api_base.h, rr_api_handle.h (writes rr_scene::query), rr_api_scene.h (ensure_tlas_reach, ensure_camera_reach; reads
//         rr_scene::data), rr_api_frame.h (launch_trace_closest, take_stream, make_frame; for rr_shade_rays the frame's own level walk:
//         make_frame_run, run_level, upload_shade_const, reset_accumulators, ALL_PLANES, grow_ray_queues, begin_frame_stats; for rr_render_pixels the whole frame:
//         check_frame_args, pixels_io, IdleOnExit, render_region_locked), rr_pixel_list.h, rr_api_multi.h (the peer
//         access it has enabled: g_peer_mu, g_peer_state), rr_query_pointers.h, rr_frame_plan.h.
// Borrowed from rr_scene::frame: h_count[HC_REACH ..] and last_stream by every query (await_reach, take_stream); the arena, the shadow
// queue, the accumulators and the counter pool by rr_shade_rays (why the next frame does not see it: above shade_rays_locked).

// ---------------------------------------------------------------------------
// pick (reference src/raytracing.rs:237-273): pixel-centre ray, one closest-hit query
// ---------------------------------------------------------------------------
extern "C" int rr_pick(rr_scene* s, const rr_camera* cam, int x, int y, rr_pick_result* out) try {
    if (!s || !cam || !out) return fail(RR_ERR_INVALID_ARGUMENT, "NULL argument");
    if (x < 0 || y < 0 || (uint32_t)x >= cam->width || (uint32_t)y >= cam->height) return fail(RR_ERR_INVALID_ARGUMENT, "pixel (%d,%d) outside %ux%u", x, y, cam->width, cam->height);
    RR_TRY(not_in_pass(s, "rr_pick"));
    std::lock_guard<std::mutex> lk(s->mu);
    RR_TRY(check_intact(s));
    HIP_TRY(hipSetDevice(s->device));
    RR_TRY(ensure_camera_reach(s, cam, nullptr));
    const rr_config none{}; // a pick has no frame config
    DFrame fr = make_frame(cam, &none);
    fr.samples = 1; fr.cell_size = 1; fr.n_region_pixels = 1;
    DevBuf scratch;
    HIP_TRY(scratch.reserve(256 + sizeof(DShadeConst)));
    // layout: [0] slot_c (the pixel's centre), [8] sample_tr (the one sample's offset), [64] hit, [96] count, [100] head, [128] counters, [256] scene view + frame constants
    char* b = scratch.as<char>();
    const uint32_t h_xy = (uint32_t)x | ((uint32_t)y << 16);
    const uint16_t h_sample[2] = {0, 0};
    float h_tables[4]; // the one-entry tables of a frame of one pixel and one sample: the launch takes the frames' code path
    primary_slot_centres(&h_xy, 1, fr.width, fr.height, h_tables);
    primary_sample_offsets(h_sample, PrimarySampleKey{fr.width, fr.height, fr.cell_size, fr.dof, fr.samples, fr.aperture_size}, h_tables + 2);
    HIP_TRY(hipMemset(b, 0, 256));
    HIP_TRY(hipMemcpy(b, h_tables, sizeof h_tables, hipMemcpyHostToDevice));
    DRayQueue q{nullptr, nullptr, nullptr, (uint4*)(b + 64)};
    DPrimary pr{(const float*)(b + 8), primary_launch(0, 1u, 1u), 1u};
    DShadeConst hc;
    hc.sc = s->data.view; hc.fr = fr; hc.ps = primary_frame((const float*)b, 1u, 1u);
    HIP_TRY(hipMemcpy(b + 256, &hc, sizeof hc, hipMemcpyHostToDevice));
    RR_TRY(launch_trace_closest(s, true, q, (uint32_t*)(b + 96), (uint32_t*)(b + 100), 1, (const DShadeConst*)(b + 256), pr, (unsigned long long*)(b + 128), nullptr, 0u, RR_ALL_PACKETS));
    uint32_t hit[4];
    HIP_TRY(hipMemcpy(hit, b + 64, 16, hipMemcpyDeviceToHost));
    scratch.release();
    memset(out, 0, sizeof *out);
    if ((int32_t)hit[1] >= 0) {
        out->hit = 1; out->item_index = hit[1]; out->object_id = s->data.h_items[hit[1]].id;
        memcpy(&out->distance, &hit[0], 4);
    }
    return RR_OK;
} RR_GUARD_END("rr_pick")

// ---------------------------------------------------------------------------
// ray queries: Raytracing::trace for caller-supplied rays (rr_pick generalised), closest-hit and shadow form, and
// Raytracing::get_color_depth_normal_id for them (rr_shade_rays).  Each query has ONE body, which works on buffers the scene's
// device can address and on a stream: the *_device entry points check the caller's pointers and run it in place; the host entry
// points are the device forms behind a staging copy -- the caller's arrays go into buffers of the call as they are, the body runs
// on the null stream, and the copy of the answers into `out` is the synchronisation.
// The streaming kernels of rr_kernels.hip (5d .. 5g) turn the caller's 12-byte rays into the walks' records and the walks' raw
// hits into the 20-byte records of the ABI; the walks and their launch sites are the frames' own.
// A closest-hit or shadow query waits ONCE for the device, for the 16 bytes of query.words[QW_REACH]: the largest finite |origin|
// per axis (the top level must be padded for it BEFORE the walk is enqueued: ensure_tlas_reach, * 1.001 in double) and the first
// bad max_distance.  A radiance query additionally waits where a frame's level walk does (the level sizes).
// Everything the launches of a device form touch after the call has returned is the caller's or the handle's (rr_scene::query,
// the arena): a scene edit waits for the device before it overwrites what they read, and rr_scene_destroy before it frees.
// ---------------------------------------------------------------------------
enum : size_t { QW_COUNT = 0, QW_HEAD = 4, QW_REACH = 64, QW_COUNTERS = 128, QW_CONST = 256 }; // byte offsets into rr_scene::query.words
static_assert(sizeof(rr_ray_hit) == 20 && sizeof(rr_shadow_hit) == 20, "k_unpack_hits writes five words per ray");
static_assert(sizeof(rr_surface_hit) == 128 && offsetof(rr_surface_hit, position) == 16 && offsetof(rr_surface_hit, normal) == 32 &&
              offsetof(rr_surface_hit, shading_normal) == 48 && offsetof(rr_surface_hit, base_color) == 64 && offsetof(rr_surface_hit, ambient_color) == 80 &&
              offsetof(rr_surface_hit, specular_color) == 96 && offsetof(rr_surface_hit, uv) == 112, "k_surface_hits writes rr_surface_hit as eight 16-byte rows");

// `p` (argument `arg` of `fn`) must be memory the scene's device can address: decided by query_pointer_ok (rr_query_pointers.h)
static int check_query_pointer(const rr_scene* s, const void* p, const char* fn, const char* arg) {
    hipPointerAttribute_t at;
    memset(&at, 0, sizeof at);
    QueryMemKind kind = RR_QMEM_UNREGISTERED;
    int owner = -1;
    if (hipPointerGetAttributes(&at, p) != hipSuccess) (void)hipGetLastError(); // a pointer the runtime has never seen
    else {
        switch (at.type) {
        case hipMemoryTypeHost: kind = RR_QMEM_HOST; break;
        case hipMemoryTypeDevice: kind = RR_QMEM_DEVICE; owner = at.device; break;
        case hipMemoryTypeManaged: case hipMemoryTypeUnified: kind = RR_QMEM_MANAGED; break;
        case hipMemoryTypeArray: kind = RR_QMEM_ARRAY; break;
        default: kind = RR_QMEM_UNREGISTERED; break;
        }
    }
    bool peer = false;
    if (kind == RR_QMEM_DEVICE && owner != s->device) { // only what this library has enabled itself (rr_render_multi) counts
        std::lock_guard<std::mutex> lk(g_peer_mu);
        const auto it = g_peer_state.find({s->device, owner});
        peer = it != g_peer_state.end() && it->second;
    }
    if (!query_pointer_ok(kind, owner, s->device, peer))
        return fail(RR_ERR_INVALID_ARGUMENT, "%s: %s is %s%s the scene's device %d cannot address", fn, arg, query_mem_kind_name(kind),
                    kind == RR_QMEM_DEVICE ? " of another device without peer access, which" : ", which", s->device);
    return RR_OK;
}
// every pointer of a device form in one call, in the order given; a NULL one is an optional the caller left out
struct QueryPointer { const void* p; const char* arg; };
static int check_query_pointers(const rr_scene* s, const char* fn, const QueryPointer* pointers, size_t n) {
    for (size_t k = 0; k < n; k++)
        if (pointers[k].p) RR_TRY(check_query_pointer(s, pointers[k].p, fn, pointers[k].arg));
    return RR_OK;
}
static int check_query_pointers(const rr_scene* s, const char* fn, std::initializer_list<QueryPointer> pointers) {
    return check_query_pointers(s, fn, pointers.begin(), pointers.size());
}

// The buffers of one call as a table (rr_arg_ranges.h has the rule): the first forbidden overlap, worded.  An output over an input is
// "<output> overlaps <input>" and `in_place_tail`; two outputs are "<earlier> overlaps <later>", or with `later_first` the other way
// round -- the two wordings the tests of the record calls pin.
static int check_arg_ranges(const char* fn, const ArgRange* t, int n, bool later_first, const char* in_place_tail) {
    const ArgConflict c = arg_ranges_first_conflict(t, n);
    if (c.a < 0) return RR_OK;
    if (c.a == c.b) return fail(RR_ERR_INVALID_ARGUMENT, "%s: %s ends beyond the address space", fn, t[c.a].name);
    if (!t[c.b].is_output) return fail(RR_ERR_INVALID_ARGUMENT, "%s: %s overlaps %s%s", fn, t[c.a].name, t[c.b].name, in_place_tail);
    return fail(RR_ERR_INVALID_ARGUMENT, "%s: %s overlaps %s", fn, t[later_first ? c.b : c.a].name, t[later_first ? c.a : c.b].name);
}

// The ONE place that launches the shadow-query kernel (rr_trace_shadow_rays), as launch_trace_closest (rr_api_frame.h): every pointer the kernel
// touches is checked here, on the host.  r0 / r1: n ray records each; out: n result records; head: the zeroed fetch word.
static int launch_query_shadow(rr_scene* s, const float4* r0, const float4* r1, uint64_t n, uint32_t* head, uint4* out, hipStream_t st) {
    if (!r0 || !r1 || !head || !out) return fail(RR_ERR_DEVICE, "internal: shadow-query launch with a NULL argument");
    if (!s->data.view.items || !s->data.view.tnodes4 || !s->data.view.item_boxes) return fail(RR_ERR_DEVICE, "internal: shadow-query launch on a scene without a top level");
    if (n == 0 || n > 0x7fffff00ull) return fail(RR_ERR_DEVICE, "internal: shadow-query launch of %llu rays", (unsigned long long)n);
    const int grid = (int)std::min<uint64_t>((n + RR_BLOCK - 1) / RR_BLOCK, (uint64_t)s->n_cus * RR_SHADOW_GRID_WG);
    hipLaunchKernelGGL(k_query_shadow, dim3(grid), dim3(RR_BLOCK), 0, st, s->data.view, r0, r1, (uint32_t)n, head, out);
    HIP_TRY(hipGetLastError());
    return RR_OK;
}

// the handle's record buffers for n rays (grow-only; a failed growth leaves an empty buffer that the next call allocates anew)
static int reserve_query_records(rr_scene* s, uint32_t n, bool shadow) {
    for (int k = 0; k < 4; k++)
        if (!(shadow && k == 2)) HIP_TRY(s->query.rec[k].reserve((size_t)n * RAY_RECORD_BYTES[k]));
    HIP_TRY(s->query.words.reserve(QW_CONST + sizeof(DShadeConst)));
    return RR_OK;
}

// the reach words, preset; the caller enqueues the kernel that merges into them and then calls await_reach
static int preset_reach(rr_scene* s, hipStream_t st) {
    char* w = s->query.words.as<char>();
    HIP_TRY(hipMemsetAsync(w, 0, QW_CONST, st));
    HIP_TRY(hipMemsetAsync(w + QW_REACH + 12, 0xff, 4, st));
    return RR_OK;
}
// THE wait of a query on device buffers: reads the reach words back (pinned, s->frame.h_count[HC_REACH ..]) and pads the top level for them.
// *first_bad = the first index with a bad limit, or 0xffffffff.
static int await_reach(rr_scene* s, hipStream_t st, uint32_t* first_bad) {
    uint32_t* h = s->frame.h_count + HC_REACH;
    HIP_TRY(hipMemcpyAsync(h, s->query.words.as<char>() + QW_REACH, 16, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    *first_bad = h[3];
    if (h[3] != 0xffffffffu) return RR_OK; // the caller refuses: nothing is rebuilt for a call that does nothing
    double need[3];
    for (int c = 0; c < 3; c++) {
        float a;
        memcpy(&a, &h[c], 4);
        need[c] = (double)a * 1.001;
    }
    return ensure_tlas_reach(s, need);
}

static int query_grid(const rr_scene* s, uint64_t n) { return (int)std::min<uint64_t>((n + RR_BLOCK - 1) / RR_BLOCK, (uint64_t)s->n_cus * 8u); }

// a host array of the caller's in a device buffer of the call (blocking)
static int stage_in(DevBuf* b, const void* src, size_t bytes) {
    HIP_TRY(b->reserve(bytes));
    HIP_TRY(hipMemcpy(b->p, src, bytes, hipMemcpyHostToDevice));
    return RR_OK;
}

// THE staging of a host form whose arguments are whole arrays (rr_denoise_records, rr_accumulate_records, rr_motion_records): argument k
// in pool[k], reserved only where the caller gave it; the inputs go up on the null stream, `body(dev)` runs on the device's copies
// (dev[k] NULL where host was), the outputs come back behind it and ONE wait ends the call: the caller's outputs are written by a
// finished call only.  The pool is the handle's (rr_scene::record_stage) or, for answers too large to stay resident, the call's own.
struct StageArg { void* host; size_t bytes; bool is_output; };
static StageArg stage_input(const void* host, size_t bytes) { return StageArg{const_cast<void*>(host), bytes, false}; } // (only read)
static StageArg stage_output(void* host, size_t bytes) { return StageArg{host, bytes, true}; }
template <int N, class Body>
static int staged_host_call(DevBuf* pool, const StageArg (&args)[N], Body body) {
    void* dev[N];
    for (int k = 0; k < N; k++) {
        if (args[k].host) HIP_TRY(pool[k].reserve(args[k].bytes));
        dev[k] = args[k].host ? pool[k].p : nullptr;
    }
    for (int k = 0; k < N; k++)
        if (args[k].host && !args[k].is_output) HIP_TRY(hipMemcpyAsync(dev[k], args[k].host, args[k].bytes, hipMemcpyHostToDevice, nullptr));
    RR_TRY(body(dev));
    for (int k = 0; k < N; k++)
        if (args[k].host && args[k].is_output) HIP_TRY(hipMemcpyAsync(args[k].host, dev[k], args[k].bytes, hipMemcpyDeviceToHost, nullptr));
    HIP_TRY(hipStreamSynchronize(nullptr));
    return RR_OK;
}

// THE entry of a record call, its arguments checked: `body()` under the scene's lock on stream st, which a call that ends early leaves
// idle.  `intact`: the call reads the scene (a call that only filters records works on a broken one too).  `pointers`: the caller's
// buffers of a device form, as a list or as a pointer and a count; a host form has none and runs on the null stream.  `prepare()` is
// what the call refuses from the scene's host state, before it waits for another stream or enqueues anything.
template <class Prepare, class Body>
static int record_call(rr_scene* s, const char* fn, bool intact, const QueryPointer* pointers, size_t n_pointers, hipStream_t st, Prepare prepare, Body body) {
    RR_TRY(not_in_pass(s, fn));
    std::lock_guard<std::mutex> lk(s->mu);
    if (intact) RR_TRY(check_intact(s));
    HIP_TRY(hipSetDevice(s->device));
    RR_TRY(check_query_pointers(s, fn, pointers, n_pointers));
    RR_TRY(prepare());
    RR_TRY(take_stream(s, st));
    IdleOnExit idle(st);
    return idle.done(body());
}
template <class Prepare, class Body>
static int record_call(rr_scene* s, const char* fn, bool intact, std::initializer_list<QueryPointer> pointers, hipStream_t st, Prepare prepare, Body body) {
    return record_call(s, fn, intact, pointers.begin(), pointers.size(), st, prepare, body);
}
template <class Body>
static int record_call(rr_scene* s, const char* fn, bool intact, std::initializer_list<QueryPointer> pointers, hipStream_t st, Body body) {
    return record_call(s, fn, intact, pointers, st, [] { return (int)RR_OK; }, body);
}

// ---- closest-hit and shadow queries
// Shadow queries: Raytracing::trace(ray, true, true, depth) and `in_light = toi > len` (reference src/raytracing.rs:429-490,
// :883-892) through the walk the frames' shadow kernel uses (k_query_shadow); closest-hit queries: the closest-hit kernel of the
// deeper levels on a queue that k_pack_rays fills.

// The argument checks of the four entry points, in the order the tests pin; `device`: the alignment rule of the device forms.
// n == 0 passes: the caller returns RR_OK before it touches anything.
static int check_trace_args(const char* fn, bool device, const rr_scene* s, const float* origins, const float* directions, const float* max_distance,
                            uint32_t n, uint32_t depth, const void* out, uintptr_t out_align = 4u) {
    if (!s || (n && (!origins || !directions || !out))) return fail(RR_ERR_INVALID_ARGUMENT, "NULL argument");
    if (depth == 0 || depth > 255u) return fail(RR_ERR_INVALID_ARGUMENT, "depth %u (1 .. 255)", depth);
    if (n == 0) return RR_OK;
    if (n > 0x7fffff00u) return fail(RR_ERR_UNSUPPORTED, "%u rays in one call", n);
    if (device && (((uintptr_t)origins | (uintptr_t)directions | (uintptr_t)max_distance | (uintptr_t)out) & 3u))
        return fail(RR_ERR_INVALID_ARGUMENT, "%s: a buffer is not 4-byte aligned", fn);
    if (device && ((uintptr_t)out & (out_align - 1u))) return fail(RR_ERR_INVALID_ARGUMENT, "%s: out_dev is not %u-byte aligned", fn, (unsigned)out_align);
    return RR_OK;
}

// One query on device buffers, in stream order (the caller holds the lock): Q_SHADOW = limits (or NULL) and the shadow walk into
// rr_shadow_hit records, else the closest-hit walk, whose raw hits end as rr_ray_hit records (Q_CLOSEST) or, with the packed rays
// they answer, as rr_surface_hit records (Q_SURFACE).  The only wait is await_reach.
enum QueryKind { Q_CLOSEST, Q_SHADOW, Q_SURFACE };
template <QueryKind KIND> struct QueryRecord { static const size_t bytes = 20; };
template <> struct QueryRecord<Q_SURFACE> { static const size_t bytes = sizeof(rr_surface_hit); };
template <QueryKind KIND>
static int trace_rays_locked(rr_scene* s, const float* origins, const float* directions, const float* max_distance, uint32_t n, uint32_t depth, void* out,
                             hipStream_t st) {
    constexpr bool SHADOW = KIND == Q_SHADOW;
    RR_TRY(take_stream(s, st));
    RR_TRY(reserve_query_records(s, n, SHADOW));
    char* w = s->query.words.as<char>();
    const DRayQueue q{s->query.rec[0].as<float4>(), s->query.rec[1].as<float4>(), SHADOW ? nullptr : s->query.rec[2].as<uint2>(), s->query.rec[3].as<uint4>()};
    RR_TRY(preset_reach(s, st));
    hipLaunchKernelGGL(k_pack_rays<SHADOW>, dim3(query_grid(s, n)), dim3(RR_BLOCK), 0, st, origins, directions, max_distance, n, depth, q.r0, q.r1, q.r2,
                       (uint32_t*)(w + QW_COUNT), (uint32_t*)(w + QW_REACH));
    HIP_TRY(hipGetLastError());
    uint32_t first_bad = 0;
    RR_TRY(await_reach(s, st, &first_bad));
    if (SHADOW && first_bad != 0xffffffffu) { // (the stream is idle: the value for the message comes with one more small copy)
        float v = 0.0f;
        HIP_TRY(hipMemcpy(&v, max_distance + first_bad, 4, hipMemcpyDefault));
        return fail(RR_ERR_INVALID_ARGUMENT, "max_distance[%u] = %g (a distance >= 0, or +inf for no limit)", first_bad, (double)v);
    }
    if (SHADOW) RR_TRY(launch_query_shadow(s, q.r0, q.r1, n, (uint32_t*)(w + QW_HEAD), q.hit, st));
    else { // (the <false> build reads neither the frame constants nor the work counters; both pointers name the handle's words all the same)
        const DPrimary pr{nullptr, PrimaryLaunch{0u, 0u, 0u, 6u}, 0u};
        RR_TRY(launch_trace_closest(s, false, q, (uint32_t*)(w + QW_COUNT), (uint32_t*)(w + QW_HEAD), n, (const DShadeConst*)(w + QW_CONST), pr,
                                    (unsigned long long*)(w + QW_COUNTERS), st, 0u, RR_ALL_PACKETS));
    }
    if (KIND == Q_SURFACE) hipLaunchKernelGGL(k_surface_hits, dim3(query_grid(s, n)), dim3(RR_BLOCK), 0, st, s->data.view, q.r0, q.r1, q.hit, n, (uint4*)out);
    else hipLaunchKernelGGL(k_unpack_hits<SHADOW>, dim3(query_grid(s, n)), dim3(RR_BLOCK), 0, st, q.hit, n, s->data.view.items, s->data.view.n_items, s->data.view.trix, (uint32_t*)out);
    HIP_TRY(hipGetLastError());
    return RR_OK;
}

// The host form: the caller's arrays as they are (12 + 12 B per ray, 4 B of limit) and the 20-byte (128-byte) answers in buffers of the
// call, freed on return (hipFree waits for what a failed call left in flight); trace_rays_locked on the null stream between them.
template <QueryKind KIND>
static int trace_rays_staged(rr_scene* s, const float* origins, const float* directions, const float* max_distance, uint32_t n, uint32_t depth, void* out) {
    DevBuf d_origins, d_dirs, d_limits, d_out;
    RR_TRY(stage_in(&d_origins, origins, 12ull * n));
    RR_TRY(stage_in(&d_dirs, directions, 12ull * n));
    if (max_distance) RR_TRY(stage_in(&d_limits, max_distance, 4ull * n));
    const size_t out_bytes = QueryRecord<KIND>::bytes * n;
    HIP_TRY(d_out.reserve(out_bytes));
    RR_TRY(trace_rays_locked<KIND>(s, d_origins.as<float>(), d_dirs.as<float>(), d_limits.as<float>(), n, depth, d_out.p, nullptr));
    HIP_TRY(hipMemcpy(out, d_out.p, out_bytes, hipMemcpyDeviceToHost)); // waits for the launches: `out` is written by a finished query only
    return RR_OK;
}

extern "C" int rr_trace_rays(rr_scene* s, const float* origins, const float* directions, uint32_t n, uint32_t depth, rr_ray_hit* out) try {
    RR_TRY(check_trace_args("rr_trace_rays", false, s, origins, directions, nullptr, n, depth, out));
    if (n == 0) return RR_OK;
    RR_TRY(not_in_pass(s, "rr_trace_rays"));
    std::lock_guard<std::mutex> lk(s->mu);
    RR_TRY(check_intact(s));
    HIP_TRY(hipSetDevice(s->device));
    RR_FAULT_POINT("trace_rays.host");
    return trace_rays_staged<Q_CLOSEST>(s, origins, directions, nullptr, n, depth, out);
} RR_GUARD_END("rr_trace_rays")

extern "C" int rr_trace_shadow_rays(rr_scene* s, const float* origins, const float* directions, const float* max_distance,
                                    uint32_t n, uint32_t depth, rr_shadow_hit* out) try {
    RR_TRY(check_trace_args("rr_trace_shadow_rays", false, s, origins, directions, max_distance, n, depth, out));
    if (n == 0) return RR_OK;
    if (max_distance) // (the body refuses the same limits; here the refusal costs no upload)
        for (uint32_t i = 0; i < n; i++)
            if (!(max_distance[i] >= 0.0f)) return fail(RR_ERR_INVALID_ARGUMENT, "max_distance[%u] = %g (a distance >= 0, or +inf for no limit)", i, (double)max_distance[i]);
    RR_TRY(not_in_pass(s, "rr_trace_shadow_rays"));
    std::lock_guard<std::mutex> lk(s->mu);
    RR_TRY(check_intact(s));
    HIP_TRY(hipSetDevice(s->device));
    RR_FAULT_POINT("trace_shadow_rays.host");
    return trace_rays_staged<Q_SHADOW>(s, origins, directions, max_distance, n, depth, out);
} RR_GUARD_END("rr_trace_shadow_rays")

extern "C" int rr_trace_rays_device(rr_scene* s, const float* origins, const float* directions, uint32_t n, uint32_t depth, rr_ray_hit* out,
                                    void* hip_stream) try {
    RR_TRY(check_trace_args("rr_trace_rays_device", true, s, origins, directions, nullptr, n, depth, out));
    if (n == 0) return RR_OK;
    RR_TRY(not_in_pass(s, "rr_trace_rays_device"));
    std::lock_guard<std::mutex> lk(s->mu);
    RR_TRY(check_intact(s));
    HIP_TRY(hipSetDevice(s->device));
    RR_FAULT_POINT("trace_rays_device.host");
    RR_TRY(check_query_pointers(s, "rr_trace_rays_device", {{origins, "origins_dev"}, {directions, "directions_dev"}, {out, "out_dev"}}));
    return trace_rays_locked<Q_CLOSEST>(s, origins, directions, nullptr, n, depth, out, (hipStream_t)hip_stream);
} RR_GUARD_END("rr_trace_rays_device")

extern "C" int rr_trace_shadow_rays_device(rr_scene* s, const float* origins, const float* directions, const float* max_distance, uint32_t n, uint32_t depth,
                                           rr_shadow_hit* out, void* hip_stream) try {
    RR_TRY(check_trace_args("rr_trace_shadow_rays_device", true, s, origins, directions, max_distance, n, depth, out));
    if (n == 0) return RR_OK;
    RR_TRY(not_in_pass(s, "rr_trace_shadow_rays_device"));
    std::lock_guard<std::mutex> lk(s->mu);
    RR_TRY(check_intact(s));
    HIP_TRY(hipSetDevice(s->device));
    RR_FAULT_POINT("trace_shadow_rays_device.host");
    RR_TRY(check_query_pointers(s, "rr_trace_shadow_rays_device", {{origins, "origins_dev"}, {directions, "directions_dev"}, {max_distance, "max_distance_dev"}, {out, "out_dev"}}));
    return trace_rays_locked<Q_SHADOW>(s, origins, directions, max_distance, n, depth, out, (hipStream_t)hip_stream);
} RR_GUARD_END("rr_trace_shadow_rays_device")

// ---- surface queries: the closest-hit query with its third ending (k_surface_hits): what get_color_depth_normal_id evaluates at the
// hit before its light loop.  No config, no generator, nothing of a frame's state is touched.
extern "C" int rr_surface_rays(rr_scene* s, const float* origins, const float* directions, uint32_t n, uint32_t depth, rr_surface_hit* out) try {
    RR_TRY(check_trace_args("rr_surface_rays", false, s, origins, directions, nullptr, n, depth, out));
    if (n == 0) return RR_OK;
    RR_TRY(not_in_pass(s, "rr_surface_rays"));
    std::lock_guard<std::mutex> lk(s->mu);
    RR_TRY(check_intact(s));
    HIP_TRY(hipSetDevice(s->device));
    RR_FAULT_POINT("surface_rays.host");
    return trace_rays_staged<Q_SURFACE>(s, origins, directions, nullptr, n, depth, out);
} RR_GUARD_END("rr_surface_rays")

extern "C" int rr_surface_rays_device(rr_scene* s, const float* origins, const float* directions, uint32_t n, uint32_t depth, rr_surface_hit* out,
                                      void* hip_stream) try {
    RR_TRY(check_trace_args("rr_surface_rays_device", true, s, origins, directions, nullptr, n, depth, out, 16u));
    if (n == 0) return RR_OK;
    RR_TRY(not_in_pass(s, "rr_surface_rays_device"));
    std::lock_guard<std::mutex> lk(s->mu);
    RR_TRY(check_intact(s));
    HIP_TRY(hipSetDevice(s->device));
    RR_FAULT_POINT("surface_rays_device.host");
    RR_TRY(check_query_pointers(s, "rr_surface_rays_device", {{origins, "origins_dev"}, {directions, "directions_dev"}, {out, "out_dev"}}));
    return trace_rays_locked<Q_SURFACE>(s, origins, directions, nullptr, n, depth, out, (hipStream_t)hip_stream);
} RR_GUARD_END("rr_surface_rays_device")

// ---- radiance queries: Raytracing::get_color_depth_normal_id(scene, ray, 1) (reference src/raytracing.rs:720-998) for caller-supplied
// rays -- what `render` calls per sample, without its pinhole / DOF camera.  The caller's rays are seeded as depth level 1 of the
// frame's own level walk (k_seed_rays, run_level's seeded form), batch by batch (rr_frame_plan.h plan_ray_batches), into one
// accumulator slot per result; k_resolve_rays returns what k_resolve computes before its clamp.
// Per-frame state of the handle this call shares with rr_render, and why the next frame does not see it: the shade constants, the
// accumulators and the counter pool are rewritten by every frame; the arena and the shadow queue only grow (a frame takes what it
// needs from the front); the slot -> pixel map is this call's own buffer (FrameRun::slot_xy), so the cached region map, the
// sub-sample table and arena_factor are not touched at all.
static_assert(sizeof(rr_radiance) == 32 && offsetof(rr_radiance, depth) == 12 && offsetof(rr_radiance, normal) == 16 && offsetof(rr_radiance, object_id) == 28,
              "k_resolve_rays writes rr_radiance as two float4");
static const uint32_t RESOLVE_RAYS_CHUNK = 1u << 22; // results per k_resolve_rays launch and, in the host form, read-back (128 MB of staging at most)

// Where the rays, the stream ids (or NULL) and the results of one radiance query live: `host` = the caller's host arrays, which
// shade_rays_locked stages batch by batch and chunk by chunk; else buffers the scene's device can address, used where they are.
struct RayIo { const float* origins; const float* directions; const uint32_t* stream_ids; rr_radiance* out; bool host; };

// The argument checks of the two entry points, in the order the tests pin; `device`: the alignment rule of the device form.
// n_results == 0 passes: the caller returns RR_OK before it touches anything.
static int check_shade_args(const char* fn, bool device, const rr_scene* s, const rr_config* cfg, const float* origins, const float* directions,
                            const uint32_t* stream_ids, const rr_radiance* out, uint32_t n_results, uint32_t rays_per_result) {
    if (!s || !cfg) return fail(RR_ERR_INVALID_ARGUMENT, "NULL argument");
    if (rays_per_result == 0) return fail(RR_ERR_INVALID_ARGUMENT, "rays_per_result must be >= 1");
    if (rays_per_result > RR_MAX_SAMPLES_WITH_TABLE) return fail(RR_ERR_UNSUPPORTED, "rays_per_result %u > %u", rays_per_result, RR_MAX_SAMPLES_WITH_TABLE);
    if (cfg->max_recursion > RR_MAX_RECURSION) return fail(RR_ERR_UNSUPPORTED, "max_recursion %u > %u", cfg->max_recursion, RR_MAX_RECURSION);
    if (n_results == 0) return RR_OK;
    if (n_results > 0x7fffff00u) return fail(RR_ERR_UNSUPPORTED, "%u results in one call", n_results);
    if (!origins || !directions || !out) return fail(RR_ERR_INVALID_ARGUMENT, "NULL argument");
    if (device && ((((uintptr_t)origins | (uintptr_t)directions | (uintptr_t)stream_ids) & 3u) || ((uintptr_t)out & 15u)))
        return fail(RR_ERR_INVALID_ARGUMENT, "%s: the ray buffers must be 4-byte aligned and out_dev 16-byte aligned", fn);
    return RR_OK;
}

// the top level padded for host origins (n_words = 3 x rays): what k_ray_reach and await_reach do for rays on the device
static int ensure_host_ray_reach(rr_scene* s, const float* origins, uint64_t n_words) {
    double need[3] = {0.0, 0.0, 0.0};
    for (uint64_t g = 0; g < n_words; g++) {
        const double a = std::fabs((double)origins[g]) * 1.001;
        if (std::isfinite(a)) need[g % 3] = std::max(need[g % 3], a);
    }
    return ensure_tlas_reach(s, need);
}

// the frame constants k_shade reads: `samples` decides which ray of a result carries its object id; a width of 65536 makes
// k_shade's RNG pixel (xy >> 16) * width + (xy & 0xffff) the 32-bit id itself
static DFrame make_ray_frame(const rr_config* cfg, uint32_t rays_per_result, uint32_t n_results) {
    DFrame fr;
    memset(&fr, 0, sizeof fr);
    fr.width = 65536u; fr.height = 65536u; fr.samples = rays_per_result; fr.cell_size = 1u;
    fr.max_recursion = cfg->max_recursion; fr.monte_carlo = cfg->monte_carlo ? 1u : 0u;
    fr.fog_density = cfg->fog_density;
    for (int k = 0; k < 3; k++) fr.fog_color[k] = cfg->fog_color[k];
    fr.seed_lo = (uint32_t)cfg->seed; fr.seed_hi = (uint32_t)(cfg->seed >> 32);
    fr.n_region_pixels = n_results;
    return fr;
}

// the batches of one call, in order; d_origins / d_dirs: the host form's staging for one batch (plan.B rays)
static int run_ray_batches(FrameRun& f, const RayIo& io, uint32_t rays_per_result, float* d_origins, float* d_dirs) {
    rr_scene* s = f.s;
    const uint64_t B = f.plan.B, n_rays = f.plan.total_primary;
    for (uint64_t first = 0; first < n_rays; first += B) {
        if (f.cancel && *f.cancel) return fail(RR_ERR_CANCELLED, "cancelled");
        const uint32_t nb = (uint32_t)std::min<uint64_t>(B, n_rays - first);
        RR_TRY(f.pool.start_batch());
        uint32_t* level1_count = f.pool.take(1);
        if (!level1_count) return counters_exhausted();
        const float *origins = io.origins + 3ull * first, *dirs = io.directions + 3ull * first;
        if (io.host) { // (stream-ordered: the copies wait for the kernels of the batch before, which read the same staging buffers)
            HIP_TRY(hipMemcpyAsync(d_origins, origins, 12ull * nb, hipMemcpyHostToDevice, f.st));
            HIP_TRY(hipMemcpyAsync(d_dirs, dirs, 12ull * nb, hipMemcpyHostToDevice, f.st));
            origins = d_origins; dirs = d_dirs;
        }
        hipLaunchKernelGGL(k_seed_rays, dim3((nb + RR_BLOCK - 1) / RR_BLOCK), dim3(RR_BLOCK), 0, f.st, origins, dirs, (unsigned long long)first, nb, rays_per_result,
                           f.queue_at(0), level1_count, s->frame.counters.as<unsigned long long>());
        HIP_TRY(hipGetLastError());
        s->timing.stats.batches++;
        RR_TRY(run_level(f, 1, 0, nb, level1_count));
        HIP_TRY(hipGetLastError());
        if (f.cancel && first + B < n_rays) { // only a caller that can cancel needs the host to keep pace
            if (io.host) HIP_TRY(hipStreamSynchronize(f.st));
            else if (hipStreamSynchronize(f.st) != hipSuccess) return fail(RR_ERR_DEVICE, "rr_shade_rays_device: the stream failed");
        }
    }
    return RR_OK;
}

// One radiance query (the caller holds the lock).  Host rays: staging of the call, bounded by plan.B rays and RESOLVE_RAYS_CHUNK
// results, and the stream is idle when the call returns, whatever ended it (the staging goes, `out` is the caller's to read).
// Device rays: nothing is the call's own, so nothing is freed behind launches in flight, and only a call that ends early waits.
static int shade_rays_locked(rr_scene* s, const rr_config* cfg, const RayIo& io, uint32_t n_results, uint32_t rays_per_result, hipStream_t st,
                             const volatile int* cancel) {
    RR_TRY(take_stream(s, st));
    begin_frame_stats(s);
    const uint64_t n_rays = (uint64_t)n_results * rays_per_result;
    if (io.host) RR_TRY(ensure_host_ray_reach(s, io.origins, 3ull * n_rays));
    else {
        HIP_TRY(s->query.words.reserve(QW_CONST + sizeof(DShadeConst)));
        RR_TRY(preset_reach(s, st));
        hipLaunchKernelGGL(k_ray_reach, dim3(query_grid(s, 3ull * n_rays)), dim3(RR_BLOCK), 0, st, io.origins, (unsigned long long)(3ull * n_rays),
                           (uint32_t*)(s->query.words.as<char>() + QW_REACH));
        HIP_TRY(hipGetLastError());
        uint32_t first_bad = 0;
        RR_TRY(await_reach(s, st, &first_bad));
    }
    RR_TRY(upload_shade_const(s, make_ray_frame(cfg, rays_per_result, n_results), PrimaryFrame{}, st)); // (level 1 is ray records here: nothing is derived)
    DevBuf d_ids, d_origins, d_dirs, d_out; // the host form's staging
    const uint32_t* ids = io.stream_ids;
    if (io.host || !ids) { // the caller's host ids uploaded, or 0 .. n - 1: into the call's buffer (host form) or the handle's
        DevBuf& b = io.host ? d_ids : s->query.ids;
        HIP_TRY(b.reserve((size_t)n_results * 4));
        if (ids) HIP_TRY(hipMemcpy(b.p, ids, (size_t)n_results * 4, hipMemcpyHostToDevice));
        else {
            hipLaunchKernelGGL(k_iota, dim3((n_results + RR_BLOCK - 1) / RR_BLOCK), dim3(RR_BLOCK), 0, st, b.as<uint32_t>(), n_results);
            HIP_TRY(hipGetLastError());
        }
        ids = b.as<uint32_t>();
    }
    DAccum acc;
    RR_TRY(reset_accumulators(s, n_results, ALL_PLANES, st, &acc));
    uint64_t budget = 0;
    RR_TRY(queue_budget(s, &budget));
    const FramePlan plan = plan_ray_batches(n_rays, cfg->max_recursion, budget, s->data.n_enabled_lights, s->tuning.shade_chunk_rays);
    RR_TRY(grow_ray_queues(s, plan.M, plan.sq_need, 0));
    if (io.host) {
        HIP_TRY(d_origins.reserve(12ull * plan.B));
        HIP_TRY(d_dirs.reserve(12ull * plan.B));
        HIP_TRY(d_out.reserve(32ull * std::min<uint32_t>(n_results, RESOLVE_RAYS_CHUNK)));
    }
    FrameRun f = make_frame_run(s, st, plan, cfg->max_recursion, false, acc, DPrimary{nullptr, PrimaryLaunch{0u, 0u, 0u, 6u}, 0u}, ids, cancel);
    f.seeded = true;
    HIP_TRY(hipEventRecord(s->timing.frame_a, st));
    int rc = run_ray_batches(f, io, rays_per_result, d_origins.as<float>(), d_dirs.as<float>());
    for (uint32_t r0 = 0; r0 < n_results && rc == RR_OK; r0 += RESOLVE_RAYS_CHUNK) {
        const uint32_t n = std::min<uint32_t>(RESOLVE_RAYS_CHUNK, n_results - r0);
        hipLaunchKernelGGL(k_resolve_rays, dim3((n + RR_BLOCK - 1) / RR_BLOCK), dim3(RR_BLOCK), 0, st, acc, r0, n, rays_per_result,
                           io.host ? d_out.as<float4>() : (float4*)(io.out + r0));
        if (!io.host) continue;
        const hipError_t e = hipMemcpyAsync(io.out + r0, d_out.p, 32ull * n, hipMemcpyDeviceToHost, st);
        if (e != hipSuccess) rc = fail(RR_ERR_DEVICE, "rr_shade_rays: %s", hipGetErrorString(e));
    }
    (void)hipEventRecord(s->timing.frame_b, st);
    const hipError_t e = (io.host || rc != RR_OK) ? hipStreamSynchronize(st) : hipSuccess;
    if (rc != RR_OK) return rc;
    HIP_TRY(e);
    HIP_TRY(hipGetLastError());
    return RR_OK;
}

extern "C" int rr_shade_rays(rr_scene* s, const rr_config* cfg, const float* origins, const float* directions, uint32_t n_results, uint32_t rays_per_result,
                             const uint32_t* stream_ids, rr_radiance* out, const volatile int* cancel) try {
    RR_TRY(check_shade_args("rr_shade_rays", false, s, cfg, origins, directions, stream_ids, out, n_results, rays_per_result));
    if (n_results == 0) return RR_OK;
    RR_TRY(not_in_pass(s, "rr_shade_rays"));
    std::lock_guard<std::mutex> lk(s->mu);
    RR_TRY(check_intact(s));
    HIP_TRY(hipSetDevice(s->device));
    RR_FAULT_POINT("shade_rays.host");
    return shade_rays_locked(s, cfg, RayIo{origins, directions, stream_ids, out, true}, n_results, rays_per_result, nullptr, cancel);
} RR_GUARD_END("rr_shade_rays")

extern "C" int rr_shade_rays_device(rr_scene* s, const rr_config* cfg, const float* origins, const float* directions, uint32_t n_results, uint32_t rays_per_result,
                                    const uint32_t* stream_ids, rr_radiance* out, void* hip_stream, const volatile int* cancel) try {
    RR_TRY(check_shade_args("rr_shade_rays_device", true, s, cfg, origins, directions, stream_ids, out, n_results, rays_per_result));
    if (n_results == 0) return RR_OK;
    RR_TRY(not_in_pass(s, "rr_shade_rays_device"));
    std::lock_guard<std::mutex> lk(s->mu);
    RR_TRY(check_intact(s));
    HIP_TRY(hipSetDevice(s->device));
    RR_FAULT_POINT("shade_rays_device.host");
    RR_TRY(check_query_pointers(s, "rr_shade_rays_device", {{origins, "origins_dev"}, {directions, "directions_dev"}, {stream_ids, "stream_ids_dev"}, {out, "out_dev"}}));
    return shade_rays_locked(s, cfg, RayIo{origins, directions, stream_ids, out, false}, n_results, rays_per_result, (hipStream_t)hip_stream, cancel);
} RR_GUARD_END("rr_shade_rays_device")

// ---- pixel queries: rr_render_pixels, Raytracing::render(x, y) (reference src/raytracing.rs:275-427) for pixels of the caller's choice, or for every
// pixel of the frame, ending in what `render` holds before its clamp (rr_radiance, as rr_shade_rays defines it) and, on request, in the
// frame's own bytes.  The body is render_region_locked: the frame's batches, level walk, stages and plan; only the slot table
// (fill_pixel_slots) and the last kernel (k_resolve_pixels) differ.  The device form works on buffers the scene's device can address, in
// stream order; the host form is the device form behind a staging copy (the list, 32 + 4 B per pixel of answers, the null stream).
static_assert(sizeof(rr_radiance) == 32, "k_resolve_pixels writes rr_radiance as two float4");

// The argument checks of the two entry points; `device`: the alignment rule of the device form.  n_pixels == 0 passes: the caller returns
// RR_OK before it touches anything.
static int check_pixels_args(const char* fn, bool device, const rr_scene* s, const rr_camera* cam, const rr_config* cfg, const uint16_t* sample_xy,
                             const uint32_t* pixel_xy, uint32_t n_pixels, const rr_radiance* out, const uint8_t* rgba8) {
    RR_TRY(check_frame_args(s, cam, cfg, sample_xy));
    if (!out) return fail(RR_ERR_INVALID_ARGUMENT, "%s: out is required", fn);
    if (n_pixels > (1u << 30)) return fail(RR_ERR_UNSUPPORTED, "%u pixels in one call", n_pixels);
    if (n_pixels == 0) return RR_OK;
    if (!pixel_xy && (uint64_t)n_pixels != (uint64_t)cam->width * cam->height)
        return fail(RR_ERR_INVALID_ARGUMENT, "%s: %u pixels without a list, the frame of %ux%u has %llu", fn, n_pixels, cam->width, cam->height,
                    (unsigned long long)cam->width * cam->height);
    if (device && ((((uintptr_t)pixel_xy | (uintptr_t)rgba8) & 3u) || ((uintptr_t)out & 15u)))
        return fail(RR_ERR_INVALID_ARGUMENT, "%s: pixel_xy_dev and rgba8_out_dev must be 4-byte aligned and out_dev 16-byte aligned", fn);
    return RR_OK;
}

// THE host form of a list call (rr_render_pixels, rr_render_pixel_parts, rr_render_pixel_prefix), its arguments checked and n_pixels > 0:
// the device form behind a staging copy.  The list is checked here (the body refuses the same entries; here the refusal costs no
// upload), the scene is locked, and `body(list, out, parts, rgba8)` runs on the null stream on buffers of the handle -- s->frame.tmp_out
// (grown, kept, used by host forms only, which return with the stream idle): the bytes where rr_render stages its bytes, the records and
// the list in the buffers of the next two outputs, the part records (parts_per_pixel of them, where parts_out is given) in tmp_parts; no
// allocation per call.  The caller's outputs are written by a finished call only: `out` is copied last and waits for the launches.
template <class Body>
static int host_list_call(rr_scene* s, const char* fn, const rr_camera* cam, const uint32_t* pixel_xy, uint32_t n_pixels, uint32_t parts_per_pixel,
                          rr_radiance* out, rr_radiance* parts_out, uint8_t* rgba8_out, Body body) {
    if (pixel_xy) {
        const uint32_t bad = pixel_list_first_bad(pixel_xy, n_pixels, cam->width, cam->height);
        if (bad != RR_PIXEL_LIST_OK)
            return fail(RR_ERR_INVALID_ARGUMENT, "pixel_xy[%u] = (%u, %u) lies outside the frame of %ux%u pixels", bad, pixel_xy[bad] & 0xffffu, pixel_xy[bad] >> 16,
                        cam->width, cam->height);
    }
    RR_TRY(not_in_pass(s, fn));
    std::lock_guard<std::mutex> lk(s->mu);
    RR_TRY(check_intact(s));
    HIP_TRY(hipSetDevice(s->device));
    DevBuf &d_rgba = s->frame.tmp_out[0], &d_out = s->frame.tmp_out[1], &d_list = s->frame.tmp_out[2], &d_parts = s->frame.tmp_parts;
    const size_t parts_bytes = 32ull * n_pixels * parts_per_pixel;
    if (pixel_xy) {
        HIP_TRY(d_list.reserve(4ull * n_pixels));
        HIP_TRY(hipMemcpy(d_list.p, pixel_xy, 4ull * n_pixels, hipMemcpyHostToDevice));
    }
    HIP_TRY(d_out.reserve(32ull * n_pixels));
    if (parts_out) HIP_TRY(d_parts.reserve(parts_bytes));
    if (rgba8_out) HIP_TRY(d_rgba.reserve(4ull * n_pixels));
    RR_TRY(body(pixel_xy ? d_list.as<uint32_t>() : nullptr, d_out.as<rr_radiance>(), parts_out ? d_parts.as<rr_radiance>() : nullptr,
                rgba8_out ? d_rgba.as<uint8_t>() : nullptr));
    if (parts_out) HIP_TRY(hipMemcpyAsync(parts_out, d_parts.p, parts_bytes, hipMemcpyDeviceToHost, nullptr));
    if (rgba8_out) HIP_TRY(hipMemcpyAsync(rgba8_out, d_rgba.p, 4ull * n_pixels, hipMemcpyDeviceToHost, nullptr));
    HIP_TRY(hipMemcpy(out, d_out.p, 32ull * n_pixels, hipMemcpyDeviceToHost));
    HIP_TRY(hipStreamSynchronize(nullptr));
    return RR_OK;
}

// one call on buffers the device can address (the caller holds the lock); a call that ends early leaves the stream idle
static int render_pixels_locked(rr_scene* s, const rr_camera* cam, const rr_config* cfg, const uint16_t* sample_xy, const uint32_t* pixel_xy,
                                uint32_t n_pixels, rr_radiance* out, uint8_t* rgba8, hipStream_t st, const volatile int* cancel) {
    IdleOnExit idle(st);
    return idle.done(render_region_locked(s, cam, cfg, sample_xy, pixels_io(pixel_xy, n_pixels, out, rgba8), st, cancel));
}

// (the two entry points of this family share one linkage block; tests/test_pixel_list.py holds each to the guard every entry point has)
extern "C" {
int rr_render_pixels_device(rr_scene* s, const rr_camera* cam, const rr_config* cfg, const uint16_t* sample_xy, const uint32_t* pixel_xy,
                                       uint32_t n_pixels, rr_radiance* out, uint8_t* rgba8_out, void* hip_stream, const volatile int* cancel) try {
    RR_TRY(check_pixels_args("rr_render_pixels_device", true, s, cam, cfg, sample_xy, pixel_xy, n_pixels, out, rgba8_out));
    if (n_pixels == 0) return RR_OK;
    RR_TRY(not_in_pass(s, "rr_render_pixels_device"));
    std::lock_guard<std::mutex> lk(s->mu);
    RR_TRY(check_intact(s));
    HIP_TRY(hipSetDevice(s->device));
    RR_TRY(check_query_pointers(s, "rr_render_pixels_device", {{pixel_xy, "pixel_xy_dev"}, {out, "out_dev"}, {rgba8_out, "rgba8_out_dev"}}));
    return render_pixels_locked(s, cam, cfg, sample_xy, pixel_xy, n_pixels, out, rgba8_out, (hipStream_t)hip_stream, cancel);
} RR_GUARD_END("rr_render_pixels_device")

int rr_render_pixels(rr_scene* s, const rr_camera* cam, const rr_config* cfg, const uint16_t* sample_xy, const uint32_t* pixel_xy,
                                uint32_t n_pixels, rr_radiance* out, uint8_t* rgba8_out, const volatile int* cancel) try {
    RR_TRY(check_pixels_args("rr_render_pixels", false, s, cam, cfg, sample_xy, pixel_xy, n_pixels, out, rgba8_out));
    if (n_pixels == 0) return RR_OK;
    return host_list_call(s, "rr_render_pixels", cam, pixel_xy, n_pixels, 0u, out, nullptr, rgba8_out,
                          [&](const uint32_t* d_list, rr_radiance* d_out, rr_radiance*, uint8_t* d_rgba) {
                              return render_pixels_locked(s, cam, cfg, sample_xy, d_list, n_pixels, d_out, d_rgba, nullptr, cancel);
                          });
} RR_GUARD_END("rr_render_pixels")
} // extern "C"
