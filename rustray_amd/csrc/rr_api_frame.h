// rr_api_frame.h — one frame on one device: the batches of primary rays, the level walk behind them, what the frame cost.
// Offers: check_frame_args; ScopedTimer, resolve_timers; OUT_ELEM, out_buffer, stage_outputs, copy_outputs; PassHook;
//         launch_trace_closest; FrameEnd, FrameIo and its makers frame_io and pixels_io, frame_end_plan (what an ending implies),
//         ALL_PLANES; make_frame, upload_shade_const, reset_accumulators, queue_budget, grow_ray_queues; CounterPool, FrameRun and its maker
//         make_frame_run; launch_shade and launch_shadow (THE launch sites of k_shade and k_trace_shadow), read_back_level_size;
//         join_shadow, join_shadow_for, FrameStreamsIdle (the staged level 1's last shadow launches stay pending while the frame's stream goes on;
//         a frame that ends early, by code or by exception, leaves its three streams idle);
//         run_level (with level 1 in stages on three streams; with FrameEnd::ALBEDO level 1 ends in k_albedo_level1: rr_api_albedo_pixels.h;
//         with FrameEnd::RECORD_SPLIT level 1 runs the SPLIT builds of the two kernels, serially: rr_api_pixel_split.h); pick_build;
//         take_stream, begin_frame_stats;
//         WHOLE_FRAME, IdleOnExit, fill_pixel_slots, render_region_locked (the pixel queries and the adaptive calls are its other callers);
//         rr_render_region_device, rr_render, rr_render_progressive, rr_render_progressive_tiles; add_pass_stats, PassSums,
//         collect_stats_locked, rr_scene_last_stats, rr_scene_overlap_stages;
//         rr_scene_set_compat, rr_scene_set_tuning, rr_scene_get_tuning.
// Needs:  rr_api_base.h, rr_sample_table.h (rr_sample_table, cell_size_of, fill_region, check_region), rr_api_handle.h (writes
//         rr_scene::frame and rr_scene::timing), rr_api_scene.h (ensure_camera_reach; reads rr_scene::data), rr_frame_plan.h (plan_frame,
//         plan_level1_stages, plan_shade_chunk, level1_tail, chunk_clear_of_tail, level_slice, batch_group),
//         rr_primary_setup.h, rr_pixel_list.h, the frame kernels of rr_kernels.hip.

// ---------------------------------------------------------------------------
// frame
// ---------------------------------------------------------------------------
static int check_frame_args(const rr_scene* s, const rr_camera* cam, const rr_config* cfg, const uint16_t* sample_xy) {
    if (!s || !cam || !cfg) return fail(RR_ERR_INVALID_ARGUMENT, "NULL argument");
    if (cfg->samples == 0) return fail(RR_ERR_INVALID_ARGUMENT, "samples must be >= 1");
    // with the caller's table the reference's own u16 limit applies; the built-in table stops where its shuffle stays affordable
    if (cfg->samples > (sample_xy ? RR_MAX_SAMPLES_WITH_TABLE : RR_MAX_SAMPLES))
        return fail(RR_ERR_UNSUPPORTED, "samples %u > %u%s", (unsigned)cfg->samples, sample_xy ? RR_MAX_SAMPLES_WITH_TABLE : RR_MAX_SAMPLES,
                    sample_xy ? "" : " (the built-in sub-sample table; pass sample_xy for up to 32766)");
    if (cfg->max_recursion > RR_MAX_RECURSION) return fail(RR_ERR_UNSUPPORTED, "max_recursion %u > %u", cfg->max_recursion, RR_MAX_RECURSION);
    if (cam->width == 0 || cam->height == 0 || cam->width > 65535u || cam->height > 65535u) return fail(RR_ERR_INVALID_ARGUMENT, "bad frame size %ux%u", cam->width, cam->height);
    if (!finite16(cam->projection_inverse) || !finite16(cam->view_inverse)) return fail(RR_ERR_INVALID_ARGUMENT, "non-finite camera matrix");
    return RR_OK;
}

static hipEvent_t take_event(rr_scene* s) {
    if (!s->timing.event_pool.empty()) { hipEvent_t e = s->timing.event_pool.back(); s->timing.event_pool.pop_back(); return e; }
    hipEvent_t e = nullptr;
    (void)hipEventCreate(&e);
    return e;
}
struct ScopedTimer {
    rr_scene* s; hipStream_t st; TimerKernel kernel; bool level1; hipEvent_t a = nullptr, b = nullptr;
    ScopedTimer(rr_scene* s_, hipStream_t st_, TimerKernel kernel_, bool level1_) : s(s_), st(st_), kernel(kernel_), level1(level1_) {
        if (s->timing.profiling) { a = take_event(s); b = take_event(s); (void)sched_record(s->sched, a, st, "timer"); }
    }
    ~ScopedTimer() { if (s->timing.profiling) { (void)sched_record(s->sched, b, st, "timer"); s->timing.timed.push_back(TimedLaunch{a, b, kernel, level1}); } }
};

// the rr_frame_stats fields of each TimerKernel: every launch, and the launches of its level-1 build (binning: time only)
static const struct {
    double rr_frame_stats::*ms; uint64_t rr_frame_stats::*launches;
    double rr_frame_stats::*ms_level1; uint64_t rr_frame_stats::*launches_level1;
} k_timer_fields[] = {
    {&rr_frame_stats::ms_trace_closest, &rr_frame_stats::launches_trace_closest, &rr_frame_stats::ms_trace_closest_level1, &rr_frame_stats::launches_trace_closest_level1},
    {&rr_frame_stats::ms_trace_shadow, &rr_frame_stats::launches_trace_shadow, &rr_frame_stats::ms_trace_shadow_level1, &rr_frame_stats::launches_trace_shadow_level1},
    {&rr_frame_stats::ms_shade, &rr_frame_stats::launches_shade, &rr_frame_stats::ms_shade_level1, &rr_frame_stats::launches_shade_level1},
    {&rr_frame_stats::ms_binning, nullptr, nullptr, nullptr},
};

static void resolve_timers(rr_scene* s) {
    for (auto& t : s->timing.timed) {
        float ms = 0.0f;
        if (sched_sync_event(s->sched, t.b, "timer") == hipSuccess && hipEventElapsedTime(&ms, t.a, t.b) == hipSuccess) {
            const auto& f = k_timer_fields[t.kernel];
            s->timing.stats.*f.ms += ms;
            if (f.launches) s->timing.stats.*f.launches += 1;
            if (t.level1) { s->timing.stats.*f.ms_level1 += ms; s->timing.stats.*f.launches_level1 += 1; }
        }
        s->timing.event_pool.push_back(t.a); s->timing.event_pool.push_back(t.b);
    }
    s->timing.timed.clear();
}

// ---- the output buffers of a frame, in rr_frame order, and their bytes per pixel: rgba8, normal (3 x f32), depth, object_id
static const size_t OUT_ELEM[4] = {4, 12, 4, 4};
static void* out_buffer(const rr_frame& f, int k) {
    void* const b[4] = {f.rgba8, f.normal, f.depth, f.object_id};
    return b[k];
}
// The device frame behind a frame for the host: s->frame.tmp_out[k] of np pixels for every buffer `host` asks for, zeroed on request.
static int stage_outputs(rr_scene* s, const rr_frame& host, size_t np, bool zero, rr_frame* dev) {
    void* p[4] = {nullptr, nullptr, nullptr, nullptr};
    for (int k = 0; k < 4; k++) {
        if (!out_buffer(host, k)) continue;
        HIP_TRY(s->frame.tmp_out[k].reserve(np * OUT_ELEM[k]));
        p[k] = s->frame.tmp_out[k].p;
        if (zero) HIP_TRY(hipMemsetAsync(p[k], 0, np * OUT_ELEM[k], nullptr));
    }
    *dev = rr_frame{(uint8_t*)p[0], (float*)p[1], (float*)p[2], (uint32_t*)p[3]};
    return RR_OK;
}
// dev -> host for every buffer both have (np pixels each), on stream st; returns when they are on the host
static int copy_outputs(ScheduleLog& log, const rr_frame& host, const rr_frame& dev, size_t np, hipStream_t st) {
    for (int k = 0; k < 4; k++)
        if (out_buffer(host, k) && out_buffer(dev, k))
            HIP_TRY(sched_copy(log, out_buffer(host, k), out_buffer(dev, k), np * OUT_ELEM[k], hipMemcpyDeviceToHost, st, "frame -> host"));
    HIP_TRY(sched_sync_stream(log, st, "copy_outputs"));
    return RR_OK;
}

// Progressive preview (rr_render_progressive): after every device batch that ends on a whole slice of samples the
// accumulators are resolved over the samples finished so far and handed to the caller (the device frame -> `host`).
struct PassHook { rr_pass_fn fn; void* user; uint32_t min_passes; const rr_frame* host; };

// The ONE place that launches the closest-hit kernel: the frame path (run_level), rr_pick and rr_trace_rays all come through here, so a
// change to the kernel's arguments cannot leave one caller behind.  Every pointer the kernel may touch is checked here, on the host,
// before the launch: a NULL one would be a write to address 16 * i on the device.  Level 1 reads no ray records (the rays are
// derived from their index), so its queue carries the hit records only and its ray pointers are passed as NULL.
// The launch walks the packets [p0, p0 + np) of the level's n rays with `head` as its own head word (0, RR_ALL_PACKETS: the whole level) on at
// most wg_per_cu workgroups per CU: RR_CLOSEST_WAVES, the resident ones, for a launch that has the GPU to itself.
static int launch_trace_closest(rr_scene* s, bool primary, DRayQueue q, uint32_t* count, uint32_t* head, uint64_t n, const DShadeConst* kc,
                                const DPrimary& pr, unsigned long long* counters, hipStream_t st, uint32_t p0, uint32_t np,
                                uint32_t wg_per_cu = RR_CLOSEST_WAVES) {
    if (!count || !head || !q.hit || !kc || !counters) return fail(RR_ERR_DEVICE, "internal: closest-hit launch with a NULL argument");
    if (primary && (!pr.sample_tr || pr.n != n)) return fail(RR_ERR_DEVICE, "internal: level-1 closest-hit launch without its ray table");
    if (!primary && (!q.r0 || !q.r1 || !q.r2)) return fail(RR_ERR_DEVICE, "internal: closest-hit launch without ray records");
    if (n == 0 || n > 0x7fffff00ull) return fail(RR_ERR_DEVICE, "internal: closest-hit launch of %llu rays", (unsigned long long)n);
    const uint64_t level_packets = (n + RR_WAVE - 1) / RR_WAVE;
    if (np == 0 || p0 >= level_packets || wg_per_cu == 0) return fail(RR_ERR_DEVICE, "internal: closest-hit launch of packets %u + %u of %llu", p0, np, (unsigned long long)level_packets);
    const uint64_t packets = std::min<uint64_t>(np, level_packets - p0); // a hit record is written only for a ray below n, whatever the range
    const int grid = (int)std::min<uint64_t>((packets * RR_WAVE + RR_BLOCK - 1) / RR_BLOCK, (uint64_t)s->n_cus * wg_per_cu);
    if (s->sched.on) {
        // k_trace_closest: a hit record for every ray of its packets that the level has; the <true> build derives the rays (frame constants, sample
        // offsets, slot centres), stores the level's size plainly and counts its rays; the <false> build reads the size and the ray records
        const uint64_t i0 = (uint64_t)p0 * RR_WAVE, i1 = std::min<uint64_t>(n, i0 + packets * RR_WAVE);
        if (primary)
            sched_launch(s->sched, st, "k_trace_closest<true>", {sa_r(kc, sizeof(DShadeConst), "shade_const"), sa_r(pr.sample_tr, s->frame.sample_tr.bytes, "sample_tr"),
                                                               sa_r(s->frame.slot_c.p, s->frame.slot_c.bytes, "slot_c"), sa_r(s->frame.pixel_c.p, s->frame.pixel_c.bytes, "pixel_c"),
                                                               sa_w(count, 4, "level count"), sa_w(q.hit + i0, (i1 - i0) * 16, "hit records"), sa_a(head, 4, "closest head"),
                                                               sa_a(counters, RR_CNT_WORDS * 8, "counters")});
        else
            sched_launch(s->sched, st, "k_trace_closest<false>", {sa_r(count, 4, "level count"), sa_r(q.r0, n * 16, "ray r0"), sa_r(q.r1, n * 16, "ray r1"), sa_r(q.r2, n * 8, "ray r2"),
                                                                sa_w(q.hit, n * 16, "hit records"), sa_a(head, 4, "closest head")});
    }
    if (primary) {
        q.r0 = nullptr; q.r1 = nullptr; q.r2 = nullptr;
        hipLaunchKernelGGL(k_trace_closest<true>, dim3(grid), dim3(RR_BLOCK), 0, st, s->data.view, q, count, head, kc, pr, counters, p0, np);
    } else {
        hipLaunchKernelGGL(k_trace_closest<false>, dim3(grid), dim3(RR_BLOCK), 0, st, s->data.view, q, count, head, kc, pr, counters, p0, np);
    }
    HIP_TRY(hipGetLastError());
    return RR_OK;
}


// ---- the steps of a frame (render_region_locked)

// the region's accumulator slots on the device (slot -> pixel, slot -> output index), uploaded when the region changes
static int update_region_map(rr_scene* s, uint32_t W, uint32_t H, const rr_region& rg, hipStream_t st) {
    if (memcmp(&s->frame.region_cached, &rg, sizeof rg) == 0 && s->frame.region_w == W && s->frame.region_h == H) return RR_OK;
    std::vector<uint32_t> order;
    fill_region(W, H, rg, &s->frame.h_region_xy, &order);
    HIP_TRY(sched_sync_stream(s->sched, st, "update_region_map"));
    HIP_TRY(s->frame.region_xy.reserve(std::max<size_t>(s->frame.h_region_xy.size(), 1) * 4));
    HIP_TRY(s->frame.slot_c.reserve(std::max<size_t>(s->frame.h_region_xy.size(), 1) * 8));
    HIP_TRY(s->frame.trace_order.reserve(std::max<size_t>(order.size(), 1) * 4));
    if (!s->frame.h_region_xy.empty()) {
        // slot_xy[j] = pixel of accumulator slot j; slot_out[j] = its index in the compact output order
        std::vector<uint32_t> slot_xy(order.size());
        for (size_t j = 0; j < order.size(); j++) slot_xy[j] = s->frame.h_region_xy[order[j]];
        HIP_TRY(sched_copy_blocking(s->sched, s->frame.region_xy.p, slot_xy.data(), slot_xy.size() * 4, hipMemcpyHostToDevice, "region_xy"));
        std::vector<float> slot_c(slot_xy.size() * 2); // the pixel centres on the screen, as primary_ray adds the sample's offset to them
        primary_slot_centres(slot_xy.data(), slot_xy.size(), W, H, slot_c.data());
        HIP_TRY(sched_copy_blocking(s->sched, s->frame.slot_c.p, slot_c.data(), slot_c.size() * 4, hipMemcpyHostToDevice, "slot_c"));
        HIP_TRY(sched_copy_blocking(s->sched, s->frame.trace_order.p, order.data(), order.size() * 4, hipMemcpyHostToDevice, "trace_order"));
    }
    s->frame.region_cached = rg; s->frame.region_w = W; s->frame.region_h = H;
    return RR_OK;
}

// How a frame ends, by name.  What an ending implies is stated once, in frame_end_plan; its last kernel is launch_resolve's.
enum class FrameEnd {
    REGION_BYTES, // k_resolve into the device frame `out` (frame_layout: at the pixel's place in the whole frame, else compact; `hook`: the progressive preview)
    RECORDS,      // k_resolve_pixels into `radiance` records and, on request, the frame's bytes in `rgba8`
    RECORD_PARTS, // k_resolve_pixel_parts (rr_api_parts.h): `parts` gets the K part records of every pixel, `radiance` the pixel's full record
    ALBEDO,       // rr_albedo_pixels (rr_api_albedo_pixels.h): level 1 ends in k_albedo_level1 instead of the shade and shadow kernels, nothing spawns,
                  // only the colour planes are accumulated, and k_resolve_albedo writes three floats per pixel to `albedo`
    RECORD_SPLIT, // rr_render_pixel_split (rr_api_pixel_split.h): level 1 runs the SPLIT builds of k_shade and k_trace_shadow, which sum the direct
                  // diffuse light of the primary hits in three planes of their own; k_resolve_pixel_parts<true> writes RECORD_PARTS' outputs (`parts` only
                  // with lg_parts > 0) and the planes as floats to `diffuse` and `diffuse_parts`
    NONE,         // no resolve: the caller reads the accumulators itself (every plane: rr_api_prefix.h)
};
// Where the accumulator slots of a frame come from and how the frame ends, by value (render_region_locked):
//   slots: a region's map (update_region_map), or `n_pixels` entries x | y << 16 the scene's device can address, entry i = slot i;
//   end:   `end` and the outputs it names; what is per pixel goes to the entry's index for a list, to y * width + x for a region.
// Built by name: a maker below, then assignments of the fields that differ; every field left alone is null / 0 / false.
struct FrameIo {
    const rr_region* region = nullptr; const uint32_t* pixel_xy = nullptr; uint32_t n_pixels = 0u;
    FrameEnd end = FrameEnd::REGION_BYTES;
    const rr_frame* out = nullptr; bool frame_layout = false; const PassHook* hook = nullptr;
    rr_radiance* radiance = nullptr; uint8_t* rgba8 = nullptr; float* albedo = nullptr;
    float* diffuse = nullptr; float* diffuse_parts = nullptr; // RECORD_SPLIT: 3 floats per pixel, and per part where lg_parts > 0
    // rr_render_pixel_parts (rr_api_parts.h): 2^lg_parts accumulator slots per pixel, slot i * K + h = part h of entry i
    uint32_t lg_parts = 0u; rr_radiance* parts = nullptr;
    // rr_render_pixel_prefix and rr_render_adaptive_prefix (rr_api_prefix.h): the samples [samples_from, samples_used) of the frame of
    // config->samples samples, both multiples of K; samples_used == 0 = all of them.  The table, the cell size and the generator's keys
    // stay the whole frame's; the object-id rule and the resolve take samples_used as the frame's count.
    uint32_t samples_used = 0u, samples_from = 0u;
    // ... its level passes: `resident` = accumulators that already hold the samples before samples_from (not cleared, n = the call's slots);
    // own_list = the list is the library's own, made from pixels it has checked (no wait for a first bad entry)
    const DAccum* resident = nullptr; bool own_list = false;
};
static FrameIo frame_io(const rr_region* rg, const rr_frame* out, bool frame_layout, const PassHook* hook = nullptr) {
    FrameIo io;
    io.region = rg; io.out = out; io.frame_layout = frame_layout; io.hook = hook;
    return io;
}
static const rr_region WHOLE_FRAME{8, 8, 1, 0}; // rr_render's slot order: 8x8 tiles, one wave = one tile of primary rays
// records (and, on request, the frame's bytes) of a list's pixels, or of the whole frame where there is no list; a caller with another
// ending names it and its output afterwards
static FrameIo pixels_io(const uint32_t* pixel_xy, uint32_t n_pixels, rr_radiance* radiance, uint8_t* rgba8) {
    FrameIo io;
    io.region = pixel_xy ? nullptr : &WHOLE_FRAME; io.pixel_xy = pixel_xy; io.n_pixels = n_pixels; io.end = FrameEnd::RECORDS; io.radiance = radiance; io.rgba8 = rgba8;
    return io;
}

// What an ending implies, stated once: the accumulator planes (aux: the three aux planes are reserved and zeroed; normal, depth, id:
// handed to the kernels -- an aux output nobody asked for is not accumulated at all) and whether level 1 ends every path (no arena, no
// shadow queue, R = 0).  Records hold all three aux means.
// split: three diffuse planes and the fourth shadow-queue array are reserved, and level 1 runs the SPLIT builds, serially.
struct FrameEndPlan { bool aux, normal, depth, id, level1_only, split; };
static const FrameEndPlan ALL_PLANES{true, true, true, true, false, false}; // (also what rr_shade_rays, which resolves its own way, accumulates)
static FrameEndPlan frame_end_plan(const FrameIo& io) {
    if (io.end == FrameEnd::ALBEDO) return FrameEndPlan{false, false, false, false, true, false};
    if (io.end == FrameEnd::REGION_BYTES) return FrameEndPlan{true, io.out->normal != nullptr, io.out->depth != nullptr, io.out->object_id != nullptr, false, false};
    if (io.end == FrameEnd::RECORD_SPLIT) return FrameEndPlan{true, true, true, true, false, true};
    return ALL_PLANES;
}

// "A call that ends early leaves the stream idle", by construction: armed at the top of a *_locked body, it waits for the stream on every
// way out but `return idle.done(RR_OK)` -- a refusal, a failed launch or reservation, the cancel flag, whatever was launched before it.
struct IdleOnExit {
    hipStream_t st; bool armed = true;
    explicit IdleOnExit(hipStream_t st_) : st(st_) {}
    ~IdleOnExit() { if (armed) (void)hipStreamSynchronize(st); }
    int done(int rc) { armed = rc != RR_OK; return rc; }
    IdleOnExit(const IdleOnExit&) = delete;
    IdleOnExit& operator=(const IdleOnExit&) = delete;
};

// The caller's pixel list as the slot table of this call: buffers of the handle's own (pixel_xy, pixel_c), so the launches read nothing
// of the caller's after the return and the cached region map (region_xy, slot_c, trace_order) is what it was for the next frame.
// THE wait of a list call: 4 bytes, the first index outside the frame (pinned, h_count[HC_PIXEL_BAD]); such a call is refused before any walk.
// With parts every entry becomes 2^lg_parts slots (k_pixel_slots); `pixel_xy` may then be the region's own map (the whole frame in parts).
// trusted: a list the library made itself from pixels of the frame; nothing is read back and the call does not wait.
static int fill_pixel_slots(rr_scene* s, uint32_t W, uint32_t H, const uint32_t* pixel_xy, uint32_t n_entries, uint32_t lg_parts, hipStream_t st, bool trusted = false) {
    const uint64_t n = (uint64_t)n_entries << lg_parts; // slots
    HIP_TRY(s->frame.pixel_xy.reserve((size_t)n * 4));
    HIP_TRY(s->frame.pixel_c.reserve((size_t)n * 8));
    HIP_TRY(s->frame.pixel_bad.reserve(4));
    HIP_TRY(sched_memset(s->sched, s->frame.pixel_bad.p, 0xff, 4, st, "pixel_bad"));
    const int grid = (int)std::min<uint64_t>((n + RR_BLOCK - 1) / RR_BLOCK, (uint64_t)s->n_cus * 8u);
    // (k_pixel_slots: entry j >> lg_parts read, slot j of both tables written, one atomicMin on the first bad index)
    if (s->sched.on) sched_launch(s->sched, st, "k_pixel_slots", {sa_r(pixel_xy, (size_t)n_entries * 4, "pixel list"), sa_w(s->frame.pixel_xy.p, (size_t)n * 4, "pixel_xy"),
                                                                  sa_w(s->frame.pixel_c.p, (size_t)n * 8, "pixel_c"), sa_a(s->frame.pixel_bad.p, 4, "pixel_bad")});
    hipLaunchKernelGGL(k_pixel_slots, dim3(grid), dim3(RR_BLOCK), 0, st, pixel_xy, n_entries, lg_parts, W, H, s->frame.pixel_xy.as<uint32_t>(), s->frame.pixel_c.as<float2>(),
                       s->frame.pixel_bad.as<uint32_t>());
    HIP_TRY(hipGetLastError());
    if (trusted) return RR_OK;
    uint32_t* h = s->frame.h_count + HC_PIXEL_BAD;
    HIP_TRY(sched_copy(s->sched, h, s->frame.pixel_bad.p, 4, hipMemcpyDeviceToHost, st, "pixel_bad -> h_count"));
    HIP_TRY(sched_sync_stream(s->sched, st, "fill_pixel_slots"));
    sched_host_read(s->sched, h, 4, "h_count[HC_PIXEL_BAD]");
    const uint32_t bad = *h;
    if (bad == RR_PIXEL_LIST_OK) return RR_OK;
    uint32_t xy = 0; // (the stream is idle: the entry for the message comes with one more small copy)
    HIP_TRY(sched_copy_blocking(s->sched, &xy, s->frame.pixel_xy.as<uint32_t>() + ((size_t)bad << lg_parts), 4, hipMemcpyDeviceToHost, "pixel_xy[bad]"));
    return fail(RR_ERR_INVALID_ARGUMENT, "pixel_xy[%u] = (%u, %u) lies outside the frame of %ux%u pixels", bad, xy & 0xffffu, xy >> 16, W, H);
}

// the frame constants of a camera and config (n_region_pixels is the caller's)
static DFrame make_frame(const rr_camera* cam, const rr_config* cfg) {
    DFrame fr;
    memset(&fr, 0, sizeof fr);
    memcpy(fr.proj_inv, cam->projection_inverse, 64);
    memcpy(fr.view_inv, cam->view_inverse, 64);
    fr.width = cam->width; fr.height = cam->height; fr.samples = cfg->samples; fr.cell_size = cell_size_of(cfg->samples);
    fr.max_recursion = cfg->max_recursion; fr.monte_carlo = cfg->monte_carlo ? 1u : 0u; fr.gamma = cfg->gamma_correction ? 1u : 0u;
    fr.dof = (cfg->aperture_size > 1.0f && cfg->focal_length > 1.0f) ? 1u : 0u;
    fr.focal_length = cfg->focal_length; fr.aperture_size = cfg->aperture_size; fr.fog_density = cfg->fog_density;
    for (int k = 0; k < 3; k++) fr.fog_color[k] = cfg->fog_color[k];
    fr.seed_lo = (uint32_t)cfg->seed; fr.seed_hi = (uint32_t)(cfg->seed >> 32);
    return fr;
}

// the shade kernel's constants (scene view + frame), read from device memory
static int upload_shade_const(rr_scene* s, const DFrame& fr, const PrimaryFrame& ps, hipStream_t st) {
    DShadeConst hc;
    hc.sc = s->data.view; hc.fr = fr; hc.ps = ps;
    HIP_TRY(s->frame.shade_const.reserve(sizeof hc));
    HIP_TRY(sched_copy(s->sched, s->frame.shade_const.p, &hc, sizeof hc, hipMemcpyHostToDevice, st, "shade_const"));
    HIP_TRY(sched_sync_stream(s->sched, st, "upload_shade_const")); // `hc` is a stack local
    return RR_OK;
}

// sample_tr on the device: the screen offset of every sample of this frame (primary_sample_offsets), uploaded only when the
// sub-sample table or a frame constant it depends on differs from what the buffer holds
static int upload_sample_table(rr_scene* s, const DFrame& fr, const uint16_t* sample_xy, hipStream_t st) {
    const uint32_t samples = fr.samples;
    if (!sample_xy) { // the built-in table depends on the sample count only: built once per count, not once per frame
        if (s->frame.table_samples != samples) {
            s->frame.table_samples = 0; // the cache names a sample count only once its table is complete
            try { s->frame.table_cache.resize((size_t)samples * 2); }
            catch (const std::exception&) { return fail(RR_ERR_OUT_OF_MEMORY, "no host memory for the sub-sample table"); }
            RR_TRY(rr_sample_table((uint16_t)samples, s->frame.table_cache.data(), nullptr));
            s->frame.table_samples = (uint16_t)samples;
        }
        sample_xy = s->frame.table_cache.data();
    }
    const PrimarySampleKey key{fr.width, fr.height, fr.cell_size, fr.dof, samples, fr.aperture_size};
    if (s->frame.tr_valid && same_key(s->frame.tr_key, key) && s->frame.tr_table.size() == (size_t)samples * 2 &&
        memcmp(s->frame.tr_table.data(), sample_xy, (size_t)samples * 4) == 0) return RR_OK;
    s->frame.tr_valid = false;
    std::vector<float> tr;
    try { s->frame.tr_table.assign(sample_xy, sample_xy + (size_t)samples * 2); tr.resize((size_t)samples * 2); }
    catch (const std::exception&) { return fail(RR_ERR_OUT_OF_MEMORY, "no host memory for the sample offsets"); }
    primary_sample_offsets(sample_xy, key, tr.data());
    HIP_TRY(sched_sync_stream(s->sched, st, "upload_sample_table")); // an earlier frame on this stream may still read the buffer
    HIP_TRY(s->frame.sample_tr.reserve((size_t)samples * 8));
    HIP_TRY(sched_copy(s->sched, s->frame.sample_tr.p, tr.data(), (size_t)samples * 8, hipMemcpyHostToDevice, st, "sample_tr"));
    HIP_TRY(sched_sync_stream(s->sched, st, "upload_sample_table")); // `tr` is a local
    s->frame.tr_key = key; s->frame.tr_valid = true;
    return RR_OK;
}

// zeroed accumulators (and work counters) for npix slots: the planes `want` names (a call that sums colours only reserves and touches no
// aux plane; an aux plane that is reserved is zeroed whether or not the kernels are handed it).
// resident: the set to go on with instead, as it is (every plane present, n == npix); the work counters are zeroed all the same.
// want.split: the three diffuse planes of rr_render_pixel_split as well, to *diffuse (never with resident accumulators).
static int reset_accumulators(rr_scene* s, uint32_t npix, const FrameEndPlan& want, hipStream_t st, DAccum* acc, const DAccum* resident = nullptr,
                              long long** diffuse = nullptr) {
    if (want.split) {
        if (resident || !diffuse) return fail(RR_ERR_DEVICE, "internal: a split frame on resident accumulators");
        HIP_TRY(s->frame.acc_diffuse.reserve((size_t)npix * 24));
        HIP_TRY(sched_memset(s->sched, s->frame.acc_diffuse.p, 0, (size_t)npix * 24, st, "acc_diffuse"));
        *diffuse = s->frame.acc_diffuse.as<long long>();
    }
    if (resident) {
        if (resident->n != npix || !resident->rgb || !resident->normal || !resident->depth || !resident->object_id || !resident->flags)
            return fail(RR_ERR_DEVICE, "internal: resident accumulators of %llu slots for a pass of %u", resident->n, npix);
        HIP_TRY(sched_memset(s->sched, s->frame.counters.p, 0, RR_CNT_WORDS * 8, st, "counters"));
        *acc = *resident;
        return RR_OK;
    }
    // (flags, colour, normal, depth, id, counters: the order the memsets have always been enqueued in)
    DevBuf* const plane[5] = {&s->frame.acc_flags, &s->frame.acc_rgb, &s->frame.acc_normal, &s->frame.acc_depth, &s->frame.acc_id};
    const size_t bytes[5] = {4, 24, 24, 8, 4};
    static const char* const plane_name[5] = {"acc_flags", "acc_rgb", "acc_normal", "acc_depth", "acc_id"};
    const int n_planes = want.aux ? 5 : 2;
    for (int k = 0; k < n_planes; k++) HIP_TRY(plane[k]->reserve((size_t)npix * bytes[k]));
    for (int k = 0; k < n_planes; k++) HIP_TRY(sched_memset(s->sched, plane[k]->p, 0, (size_t)npix * bytes[k], st, plane_name[k]));
    HIP_TRY(sched_memset(s->sched, s->frame.counters.p, 0, RR_CNT_WORDS * 8, st, "counters"));
    *acc = DAccum{s->frame.acc_rgb.as<long long>(), want.normal ? s->frame.acc_normal.as<long long>() : nullptr, want.depth ? s->frame.acc_depth.as<long long>() : nullptr,
                  want.id ? s->frame.acc_id.as<uint32_t>() : nullptr, (unsigned long long)npix, s->frame.acc_flags.as<uint32_t>()};
    return RR_OK;
}

// Ray memory (rr_frame_plan.h): a quarter of what is free on the device, at most 64 GB (MI355X has 288 GB of HBM3E),
// unless rr_tuning::queue_budget_bytes says otherwise.  Memory already held by this scene's arena counts as free.
static int queue_budget(rr_scene* s, uint64_t* budget) {
    if (s->tuning.queue_budget_bytes) { *budget = s->tuning.queue_budget_bytes; return RR_OK; }
    size_t free_b = 0, total_b = 0;
    HIP_TRY(hipMemGetInfo(&free_b, &total_b));
    *budget = std::min<uint64_t>((free_b + 56ull * s->frame.arena_cap + s->frame.hit1.bytes) / 4, 64ull << 30);
    return RR_OK;
}

// how n hits of level 1 are cut into stages for the two-stream path (rr_frame_plan.h; the knobs: rr_kernels.hip)
static bool level1_stages_wanted(const rr_scene* s) { return RR_L1_OVERLAP >= 2 || (RR_L1_OVERLAP == 1 && s->tuning.shade_chunk_rays != 0); }
static Level1Stages level1_stages(const rr_scene* s, uint64_t n) {
    return plan_level1_stages(Level1StageInputs{n, s->data.n_enabled_lights, s->tuning.shade_chunk_rays, RR_L1_STAGE_RAYS, RR_L1_BUFFERS});
}

// the ray arena for M rays and the shadow queue for sq_need rays, with at least valid_need words of lane masks (grown, never shrunk)
// split: the fourth queue array of rr_render_pixel_split as well (16 B per ray; no other frame reserves it)
static int grow_ray_queues(rr_scene* s, uint64_t M, uint64_t sq_need, uint64_t valid_need, bool split = false) {
    if (split) HIP_TRY(s->frame.sq3.reserve(std::max<uint64_t>(sq_need, s->frame.sq_cap) * 16)); // (as many rays as sq[2] holds after this call)
    if (M > s->frame.arena_cap) {
        for (int k = 0; k < 4; k++) HIP_TRY(s->frame.arena[k].reserve(M * RAY_RECORD_BYTES[k]));
        s->frame.arena_cap = M;
    }
    if (sq_need > s->frame.sq_cap) { // (one word of sq_valid per 64 rays of the queue)
        for (int k = 0; k < 3; k++) HIP_TRY(s->frame.sq[k].reserve(sq_need * 16));
        HIP_TRY(s->frame.sq_valid.reserve(std::max<uint64_t>(sq_need / RR_WAVE + 1, valid_need) * 8));
        s->frame.sq_cap = sq_need;
    }
    return RR_OK;
}

// Per-batch counters (level sizes, fetch heads, shadow shard counts) come out of zeroed segments of POOL_WORDS words.  A segment
// is never recycled inside a batch (launches still in flight and the levels above in the recursion hold pointers into it); a
// batch with more launches than one segment serves (a deeply branching scene in a very small ray arena) gets another one.
struct CounterPool {
    rr_scene* s; hipStream_t st;
    uint32_t* pool = nullptr;
    uint32_t next_word = 0;
    size_t pool_segment = 0; // 0 = s->frame.pool, k = s->frame.pool_more[k - 1]
    int start_batch() {
        pool = s->frame.pool.as<uint32_t>(); pool_segment = 0;
        HIP_TRY(sched_memset(s->sched, pool, 0, POOL_WORDS * 4, st, "counter pool"));
        next_word = 0;
        return RR_OK;
    }
    // n zeroed words; nullptr = no memory for another segment
    uint32_t* take(uint32_t n) {
        if (next_word + n > POOL_WORDS) {
            if (pool_segment == s->frame.pool_more.size()) {
                if (s->frame.pool_more.size() >= 255) return nullptr; // 4 GB of counters: something else is wrong
                s->frame.pool_more.emplace_back();
                if (s->frame.pool_more.back().reserve(POOL_WORDS * 4) != hipSuccess) { s->frame.pool_more.pop_back(); return nullptr; }
            }
            pool = s->frame.pool_more[pool_segment++].as<uint32_t>();
            if (sched_memset(s->sched, pool, 0, POOL_WORDS * 4, st, "counter pool segment") != hipSuccess) return nullptr;
            next_word = 0;
        }
        uint32_t* p = pool + next_word; next_word += n; return p;
    }
    void align_line() { next_word = (next_word + 31u) & ~31u; } // the next words start on a 128-B line
};
static int counters_exhausted() { return fail(RR_ERR_UNSUPPORTED, "out of memory for the per-launch counters of a batch"); }

// what the depth levels of a frame share
struct FrameRun {
    rr_scene* s; hipStream_t st;
    FramePlan plan; uint32_t R;
    DShadowQueue SQ; DAccum acc;
    CounterPool pool;
    DPrimary pr; // the batch being traced: depth level 1
    const volatile int* cancel;
    int shadow_grid, shade_grid_max;
    const uint32_t* slot_xy = nullptr; // accumulator slot -> RNG pixel as (x | y << 16): the region's map, the pixel list of rr_render_pixels, or the stream ids of rr_shade_rays
    bool seeded = false;               // rr_shade_rays: depth level 1 is ray RECORDS at the front of the arena (k_seed_rays), not derived from its index
    bool level1_only = false;          // FrameEnd::ALBEDO: level 1 ends in k_albedo_level1 (R = 0: the level spawns nothing; never in stages)
    // FrameEnd::RECORD_SPLIT: the diffuse planes (3 x acc.n words) and the fourth shadow-queue array; level 1 runs the SPLIT builds, never in stages
    long long* diffuse = nullptr; float4* sq_s3 = nullptr;
    // the event behind the shadow launches that still run on the handle's other streams while `st` goes on, and the rays of the shadow-queue
    // allocation they read (join_shadow); nullptr = none.  shadow_rest: while they are pending, the event behind the shadow launch that last
    // read the buffer in front of theirs, until `st` has waited for it (join_shadow_for); nullptr = no such launch, or waited for
    hipEvent_t shadow_pending = nullptr, shadow_rest = nullptr; Level1Tail shadow_tail{0, 0, -1, -1};
    DRayQueue queue_at(uint64_t base) const {
        return DRayQueue{s->frame.arena[0].as<float4>() + base, s->frame.arena[1].as<float4>() + base, s->frame.arena[2].as<uint2>() + base, s->frame.arena[3].as<uint4>() + base};
    }
};
// THE maker (render_region_locked, rr_shade_rays): the handle's shadow queue and the launch sizes of a kernel that has the GPU to itself
static FrameRun make_frame_run(rr_scene* s, hipStream_t st, const FramePlan& plan, uint32_t R, bool level1_only, const DAccum& acc, const DPrimary& pr,
                               const uint32_t* slot_xy, const volatile int* cancel) {
    return FrameRun{s, st, plan, R, DShadowQueue{s->frame.sq[0].as<float4>(), s->frame.sq[1].as<float4>(), s->frame.sq[2].as<float4>()}, acc, CounterPool{s, st}, pr, cancel,
                    s->n_cus * RR_SHADOW_GRID_WG, // RR_STACK_DEPTH KB of LDS stack per 256-thread workgroup
                    s->n_cus * RR_SHADE_GRID_WG, slot_xy, false, level1_only};
}

// THE deferred join.  The staged level 1 leaves the shadow launches of its last two stages running on the handle's second and third streams
// (FrameRun::shadow_pending, the event behind both) so that the next level runs beside them on `st`: its closest-hit launch shares nothing
// with them but integer atomics.  This makes `st` wait for them and clears the flag.  It stands in front of everything on `st` that may
// touch what those launches read (their buffers of the shadow queue, the validity words, their counters and head words) or what the frame
// returns: every launch_shade of the serial loop (with the take_chunk_shadow in front of it) unless the chunk's queue keeps clear of the
// buffers (join_shadow_for: `st` then waits for the earlier stage's shadow launch that read the buffer it writes, long over as a rule, and
// the chunk's shade and shadow launches run beside the two as well), the staged path's entry (its fork of the third stream
// and its first shade launch), start_batch of the next batch, the pass hook's resolve, and the frame's resolve and end event.
// A frame that ends early is drained by FrameStreamsIdle instead.
static int join_shadow(FrameRun& f) {
    if (!f.shadow_pending) return RR_OK;
    HIP_TRY(sched_wait(f.s->sched, f.st, f.shadow_pending, "stage_tail")); // (stage_tail follows every shadow launch of the level: the one shadow_rest names too)
    f.shadow_pending = nullptr; f.shadow_rest = nullptr;
    return RR_OK;
}
// In front of the shade launch of the chunk `g` of the serial loop, whose queue starts at ray 0 of the allocation.  A chunk that keeps clear
// of the two buffers in use (rr_frame_plan.h chunk_clear_of_tail) writes the buffer in front of them, which the shadow launch of an earlier
// stage read (Level1Tail::rest_stage) and for which no shade launch of the level has waited: `st` waits for THAT launch, once -- every
// later chunk follows this one on `st` -- instead of for the two that still run.
static int join_shadow_for(FrameRun& f, const ShadeChunk& g) {
    if (!f.shadow_pending || !chunk_clear_of_tail(g, f.shadow_tail)) return join_shadow(f);
    if (f.shadow_rest) {
        HIP_TRY(sched_wait(f.s->sched, f.st, f.shadow_rest, "shadow_rest"));
        f.shadow_rest = nullptr;
    }
    return RR_OK;
}
// ... and THE way out of a frame that ends early -- an error code (cancel flag, HIP error, counters_exhausted, arena too small, a join that
// failed) or an exception on its way to the ABI guard (CounterPool::take grows a std::vector inside the stage loop) -- with launches pending
// on any of the three streams: armed at the top of render_region_locked, it waits for the third stream, the second and then `st` on every way
// out but done(RR_OK).  FrameRun::shadow_pending is a local and is lost on unwinding; the streams are the handle's and are not.
// (What is waited for is complete, valid launches: nothing is cancelled.  The log's own allocation must not throw out of a destructor.)
struct FrameStreamsIdle {
    rr_scene* s; hipStream_t st; bool armed = true;
    FrameStreamsIdle(rr_scene* s_, hipStream_t st_) : s(s_), st(st_) {}
    void drain() noexcept {
        const hipStream_t order[3] = {s->frame.closest_stream, s->frame.overlap_stream, st};
        for (int k = 0; k < 3; k++) {
            if (k < 2 && !order[k]) continue; // (never created: no staged frame on this handle yet)
            try { (void)sched_sync_stream(s->sched, order[k], "frame left early"); }
            catch (...) { (void)hipStreamSynchronize(order[k]); }
        }
    }
    int done(int rc) { if (rc != RR_OK) drain(); armed = false; return rc; }
    ~FrameStreamsIdle() { if (armed) drain(); }
    FrameStreamsIdle(const FrameStreamsIdle&) = delete;
    FrameStreamsIdle& operator=(const FrameStreamsIdle&) = delete;
};

// Where the shadow rays of one shade chunk go: the queue and its validity words (the handle's, from `ray_offset` / `valid_offset` on: a
// stage's buffer) and, from the batch's pool, the chunk's own append counters (on a 128-B line) and the shadow launch's head word.
// counts or head NULL = the pool has no memory for another segment: launch_shade refuses the chunk.
struct ChunkShadow { DShadowQueue SQ; unsigned long long* valid; uint32_t* counts; uint32_t* head; };
static ChunkShadow take_chunk_shadow(FrameRun& f, uint64_t ray_offset, uint64_t valid_offset) {
    f.pool.align_line();
    return ChunkShadow{DShadowQueue{f.SQ.s0 + ray_offset, f.SQ.s1 + ray_offset, f.SQ.s2 + ray_offset}, f.s->frame.sq_valid.as<unsigned long long>() + valid_offset,
                       f.pool.take(RR_SQ_SHARDS * RR_SQ_STRIDE), f.pool.take(1)}; // (a braced list is evaluated in order: the counters, then the head word)
}

// The ONE place that launches the shade kernel, and the one that launches the shadow kernel behind it: the serial loop of run_level and the
// staged path come through here with the chunk's geometry (rr_frame_plan.h plan_shade_chunk) and its queue, so the two launches of a chunk
// cannot disagree about where the shadow rays are.  As in launch_trace_closest, every pointer the build in question dereferences is checked
// on the host, and so is that the geometry fits the kernels' 32-bit arguments.  max_wg: the caller's cap on the grid.
// (A template's builds are emitted in the order they are first named.  This line names the four in the order the code object has always
// held them, level 1's pair before the deeper levels', so the library's device assembly stays byte for byte what it was and a diff of it
// remains a usable check of a change to the host code.)
// `first` where FIRST, else `other`: the kernel of a launch whose SPLIT build is another function type than the builds it stands beside
template <bool FIRST, class A, class B> static auto pick_build(A first, B other) {
    if constexpr (FIRST) return first;
    else return other;
}
[[maybe_unused]] static const void* const k_chunk_kernel_order[4] = {(const void*)k_shade<true>, (const void*)k_trace_shadow<true>, (const void*)k_shade<false>,
                                                                     (const void*)k_trace_shadow<false>};
// level1 = the <true> build (rays derived from their index: no ray records, and only it may have fixed shadow slots); the hits [c0, c1) of
// qin, children to qout
static int launch_shade(FrameRun& f, bool level1, const DRayQueue& qin, const uint32_t* count, uint64_t c0, uint64_t c1, const DRayQueue& qout, uint32_t* child_count,
                        const ShadeChunk& g, const ChunkShadow& q, uint64_t max_wg, hipStream_t st) {
    rr_scene* s = f.s;
    if (!q.counts || !q.head) return counters_exhausted();
    if (!qin.hit || !count || !child_count || !f.acc.rgb || !f.acc.flags || !s->frame.shade_const.p || (!level1 && (!qin.r0 || !qin.r1 || !qin.r2)) ||
        (s->data.n_enabled_lights > 0 && (!q.SQ.s0 || !q.SQ.s1 || !q.SQ.s2)) || (g.fixed && (!level1 || !q.valid)) || c1 <= c0 || c1 > 0xffffffffull ||
        g.segcap > 0xffffffffull || g.sq_cap > 0xffffffffull || max_wg == 0)
        return fail(RR_ERR_DEVICE, "internal: shade launch of hits %llu .. %llu with a NULL or out-of-range argument", (unsigned long long)c0, (unsigned long long)c1);
    // a split frame's level 1 (serial loop only: the queue starts at the handle's, where sq_s3 starts too); its deeper levels add nothing to the planes
    const bool split = level1 && f.diffuse != nullptr;
    if (split && ((s->data.n_enabled_lights > 0 && !f.sq_s3) || q.SQ.s0 != f.SQ.s0))
        return fail(RR_ERR_DEVICE, "internal: split shade launch without its queue array, or in a stage buffer");
    ScopedTimer t(s, st, TK_SHADE, level1);
    if (s->sched.on) {
        // k_shade reads the hits [c0, c1) (and, below level 1, their ray records; on level 1 what primary_ray reads) and the slot -> pixel map; appends
        // children ANYWHERE in [child_base, M) behind one atomic counter (declared whether or not this level spawns); writes the chunk's shadow rays --
        // fixed slots: sq_cap per light and the validity words; dense: RR_SQ_SHARDS shards of segcap behind their append counters; adds to the
        // colour, normal and depth planes, ORs the flags, STORES the object id plainly, counts its work
        const uint32_t L = s->data.n_enabled_lights;
        const size_t n_acc = (size_t)f.acc.n, sq_rays = (size_t)(g.fixed ? g.sq_cap * L : (L ? g.segcap * RR_SQ_SHARDS : 0ull));
        const size_t room = f.plan.M - (size_t)(qout.r0 - s->frame.arena[0].as<float4>()); // rays from child_base to the arena's end
        sched_launch(s->sched, st, level1 ? (split ? "k_shade<true, SPLIT>" : "k_shade<true>") : "k_shade<false>",
                     {sa_r(s->frame.shade_const.p, sizeof(DShadeConst), "shade_const"), sa_r(f.slot_xy, n_acc * 4, "slot_xy"),
                      sa_r(level1 ? f.pr.sample_tr : nullptr, s->frame.sample_tr.bytes, "sample_tr"), sa_r(level1 ? s->frame.slot_c.p : nullptr, s->frame.slot_c.bytes, "slot_c"),
                      sa_r(level1 ? s->frame.pixel_c.p : nullptr, s->frame.pixel_c.bytes, "pixel_c"), sa_r(count, 4, "level count"), sa_r(qin.hit + c0, (size_t)(c1 - c0) * 16, "hit records"),
                      sa_r(level1 ? nullptr : qin.r0 + c0, (size_t)(c1 - c0) * 16, "ray r0"), sa_r(level1 ? nullptr : qin.r1 + c0, (size_t)(c1 - c0) * 16, "ray r1"),
                      sa_r(level1 ? nullptr : qin.r2 + c0, (size_t)(c1 - c0) * 8, "ray r2"), sa_w(qout.r0, room * 16, "child r0"), sa_w(qout.r1, room * 16, "child r1"),
                      sa_w(qout.r2, room * 8, "child r2"), sa_a(child_count, 4, "child_count"), sa_w(q.SQ.s0, sq_rays * 16, "shadow s0"), sa_w(q.SQ.s1, sq_rays * 16, "shadow s1"),
                      sa_w(q.SQ.s2, sq_rays * 16, "shadow s2"), sa_w(split ? f.sq_s3 : nullptr, sq_rays * 16, "shadow s3"),
                      sa_w(g.fixed ? q.valid : nullptr, (size_t)g.sq_packets * 8, "sq_valid"), sa_a(g.fixed || !L ? nullptr : q.counts, RR_SQ_SHARDS * RR_SQ_STRIDE * 4, "shard counts"),
                      sa_a(f.acc.rgb, n_acc * 24, "acc_rgb"), sa_a(f.acc.normal, n_acc * 24, "acc_normal"), sa_a(f.acc.depth, n_acc * 8, "acc_depth"),
                      sa_w(f.acc.object_id, n_acc * 4, "acc_id"), sa_a(f.acc.flags, n_acc * 4, "acc_flags"), sa_a(split ? f.diffuse : nullptr, n_acc * 24, "acc_diffuse"),
                      sa_a(s->frame.counters.p, RR_CNT_WORDS * 8, "counters")});
    }
    // ONE launch for every build: `extra` is empty, or the two pointers only the SPLIT build takes behind the arguments all builds share
    const auto launch = [&](auto... extra) {
        constexpr bool SP = sizeof...(extra) != 0;
        hipLaunchKernelGGL((pick_build<SP>(k_shade<true, SP, decltype(extra)...>, level1 ? k_shade<true> : k_shade<false>)), dim3((uint32_t)std::min<uint64_t>(g.groups, max_wg)),
                           dim3(RR_BLOCK), 0, st, s->frame.shade_const.as<DShadeConst>(), f.slot_xy, f.pr, qin, count, (uint32_t)c0, (uint32_t)c1, qout, child_count, q.SQ, q.counts,
                           (uint32_t)g.segcap, q.valid, (uint32_t)g.sq_cap, f.acc, s->frame.counters.as<unsigned long long>(), extra...);
    };
    if (split) launch(f.diffuse, f.sq_s3);
    else launch();
    HIP_TRY(hipGetLastError());
    return RR_OK;
}
// (the timer's level-1 flag is by kernel BUILD: level 1 of a scene without fixed shadow slots runs k_trace_shadow<false>)
// split: the launch behind k_shade<true, true> (level 1 of a split frame)
static int launch_shadow(FrameRun& f, const ShadeChunk& g, const ChunkShadow& q, uint64_t max_wg, hipStream_t st, bool split = false) {
    if (split && (!f.diffuse || !f.sq_s3 || q.SQ.s0 != f.SQ.s0)) return fail(RR_ERR_DEVICE, "internal: split shadow launch without its planes or queue array");
    if (!q.counts || !q.head || !f.acc.rgb || !f.acc.flags || !q.SQ.s0 || !q.SQ.s1 || !q.SQ.s2 || (g.fixed && !q.valid) || g.segcap > 0xffffffffull ||
        g.sq_packets > 0xffffffffull || g.shadow_wg == 0 || max_wg == 0)
        return fail(RR_ERR_DEVICE, "internal: shadow launch of %llu workgroups with a NULL or out-of-range argument", (unsigned long long)g.shadow_wg);
    ScopedTimer t(f.s, st, TK_SHADOW, g.fixed);
    if (f.s->sched.on) {
        // k_trace_shadow reads the chunk's rays as far as launch_shade declares them written (fixed: by the validity words; dense: by the shard counts),
        // deals its packets behind its own head word, adds to the colour planes and ORs the flags; no other plane, no counter
        const uint32_t L = f.s->data.n_enabled_lights;
        const size_t n_acc = (size_t)f.acc.n, sq_rays = (size_t)(g.fixed ? g.sq_cap * L : g.segcap * RR_SQ_SHARDS);
        sched_launch(f.s->sched, st, g.fixed ? "k_trace_shadow<true>" : (split ? "k_trace_shadow<false, SPLIT>" : "k_trace_shadow<false>"),
                     {sa_r(q.SQ.s0, sq_rays * 16, "shadow s0"), sa_r(q.SQ.s1, sq_rays * 16, "shadow s1"), sa_r(q.SQ.s2, sq_rays * 16, "shadow s2"),
                      sa_r(split ? f.sq_s3 : nullptr, sq_rays * 16, "shadow s3"), sa_r(g.fixed ? q.valid : nullptr, (size_t)g.sq_packets * 8, "sq_valid"),
                      sa_r(g.fixed ? nullptr : q.counts, RR_SQ_SHARDS * RR_SQ_STRIDE * 4, "shard counts"), sa_a(q.head, 4, "shadow head"), sa_a(f.acc.rgb, n_acc * 24, "acc_rgb"),
                      sa_a(f.acc.flags, n_acc * 4, "acc_flags"), sa_a(split ? f.diffuse : nullptr, n_acc * 24, "acc_diffuse")});
    }
    const auto launch = [&](auto... extra) { // (as in launch_shade: empty, or the SPLIT builds' two pointers)
        constexpr bool SP = sizeof...(extra) != 0;
        hipLaunchKernelGGL((pick_build<SP>(g.fixed ? k_trace_shadow<true, SP, decltype(extra)...> : k_trace_shadow<false, SP, decltype(extra)...>,
                                           g.fixed ? k_trace_shadow<true> : k_trace_shadow<false>)),
                           dim3((uint32_t)std::min<uint64_t>(g.shadow_wg, max_wg)), dim3(RR_BLOCK), 0, st, f.s->data.view, q.SQ, q.counts, (uint32_t)g.segcap, q.valid,
                           (uint32_t)g.sq_packets, q.head, f.acc, extra...);
    };
    if (split) launch(f.diffuse, (const float4*)f.sq_s3);
    else launch();
    HIP_TRY(hipGetLastError());
    return RR_OK;
}
// The size of the next level, final once the last shade launch of a slice has run, on its way to the host (run_level waits for count_ready)
static int read_back_level_size(FrameRun& f, const uint32_t* child_count) {
    HIP_TRY(sched_copy(f.s->sched, f.s->frame.h_count + HC_LEVEL, child_count, 4, hipMemcpyDeviceToHost, f.st, "child_count -> h_count"));
    HIP_TRY(sched_record(f.s->sched, f.s->frame.count_ready, f.st, "count_ready"));
    return RR_OK;
}

// On request (rr_tuning::bin_min_rays) a deeper level of m rays at child_base is traced in bins of (origin cell, direction octant)
// when the sorted copy fits behind the unsorted one (rr_kernels.hip: ray binning; off by default, it does not pay).
// *level_base = child_base + m (the sorted copy) when the level was binned.
static int bin_level(FrameRun& f, uint64_t child_base, uint64_t m, uint64_t* level_base) {
    rr_scene* s = f.s;
    const uint64_t bin_min = s->tuning.bin_min_rays;
    if (bin_min == 0 || m < bin_min || f.plan.M - child_base < 3 * m + 2ull * RR_BLOCK * (f.R + 1)) return RR_OK;
    f.pool.align_line();
    int* bounds = (int*)f.pool.take(8);
    uint32_t* hist = f.pool.take(RR_BIN_COUNT);
    if (!bounds || !hist) return RR_OK;
    const int init[8] = {0x7f7fffff, 0x7f7fffff, 0x7f7fffff, (int)0x80800000, (int)0x80800000, (int)0x80800000, 0, 0}; // ordered(+FLT_MAX) x3, ordered(-FLT_MAX) x3
    HIP_TRY(sched_copy(s->sched, bounds, init, sizeof init, hipMemcpyHostToDevice, f.st, "bin bounds"));
    const DRayQueue qsrc = f.queue_at(child_base), qdst = f.queue_at(child_base + m);
    const int g = (int)std::min<uint64_t>((m + RR_BLOCK - 1) / RR_BLOCK, (uint64_t)s->n_cus * 8);
    ScopedTimer t(s, f.st, TK_BINNING, false);
    if (s->sched.on) { // (atomicMin / atomicMax on the bounds: A; the prefix sum rewrites the histogram in place: W)
        sched_launch(s->sched, f.st, "k_bin_bounds", {sa_r(qsrc.r0, m * 16, "ray r0"), sa_a(bounds, 24, "bin bounds")});
        sched_launch(s->sched, f.st, "k_bin_count", {sa_r(qsrc.r0, m * 16, "ray r0"), sa_r(qsrc.r1, m * 16, "ray r1"), sa_r(bounds, 24, "bin bounds"), sa_w(qsrc.hit, m * 16, "bin keys"),
                                                    sa_a(hist, RR_BIN_COUNT * 4, "bin histogram")});
        sched_launch(s->sched, f.st, "k_bin_prefix", {sa_w(hist, RR_BIN_COUNT * 4, "bin histogram")});
        sched_launch(s->sched, f.st, "k_bin_scatter", {sa_r(qsrc.hit, m * 16, "bin keys"), sa_r(qsrc.r0, m * 16, "ray r0"), sa_r(qsrc.r1, m * 16, "ray r1"), sa_r(qsrc.r2, m * 8, "ray r2"),
                                                      sa_w(qdst.r0, m * 16, "sorted r0"), sa_w(qdst.r1, m * 16, "sorted r1"), sa_w(qdst.r2, m * 8, "sorted r2"),
                                                      sa_a(hist, RR_BIN_COUNT * 4, "bin histogram")});
    }
    hipLaunchKernelGGL(k_bin_bounds, dim3(g), dim3(RR_BLOCK), 0, f.st, qsrc, (uint32_t)m, bounds);
    hipLaunchKernelGGL(k_bin_count, dim3(g), dim3(RR_BLOCK), 0, f.st, qsrc, (uint32_t)m, bounds, hist);
    hipLaunchKernelGGL(k_bin_prefix, dim3(1), dim3(1024), 0, f.st, hist);
    hipLaunchKernelGGL(k_bin_scatter, dim3(g), dim3(RR_BLOCK), 0, f.st, qsrc, qdst, (uint32_t)m, hist);
    *level_base = child_base + m;
    s->timing.stats.binned_rays += m;
    return RR_OK;
}

// ---- level 1 in stages on three streams -------------------------------------------------------------------------------------------
// k_shade<true> is bound by instruction issue and k_trace_shadow<true> by memory latency; one after the other, each has the whole
// GPU in turn.  Here the hits [s0, s1) are cut into stages (rr_frame_plan.h, plan_level1_stages): stage k is shaded on the frame's
// stream `st` into shadow buffer k % n_buf, and its shadow rays are traced on the handle's second stream behind an event that
// follows the shade launch, while `st` already shades stage k + 1.  Shade k + n_buf waits for the event behind shadow k, so a
// buffer is never rewritten while it is read.  `st` may be the legacy null stream and the second stream is non-blocking: all
// ordering is by these events.  The frame cannot change: the kernels are the serial loop's, every write they share is an integer
// atomic, and all else goes to the stage's own buffer.  Which frames take this path, and the sizes of the grids: RR_L1_OVERLAP
// and the knobs after it (rr_kernels.hip), with what was measured.
// Where the stages cover the whole level (trace_closest: one slice), its closest hits are traced stage by stage as well, on the handle's third
// stream: k_trace_closest<true> over the packets of stage k (launch_trace_closest with a range; a stage is whole packets), each launch with
// its own head word.  The stream forks from `st` where the path begins -- behind the frame's uploads and memsets, the zeroing of the counter
// pool and the previous batch's last shade launch, which reads hit1 -- and nothing else orders its launches: hit1 covers the level, so they
// run ahead as far as the CUs allow.  Shade k waits for the event behind closest-hit launch k; the wait of the last stage joins the stream into `st`.
// The second stream is NOT joined into `st` where the path ends.  When the last stage has been shaded, the shadow launch of the stage before it
// has only just begun (shadow k trails shade k + 1) and the last stage's would follow it, alone; then level 2, one small launch at a time.
// Instead the last stage's shadow launch goes to the third stream, beside its predecessor, and both stay pending (join_shadow) while `st`
// goes on with level 2.
static int ensure_overlap_stream(rr_scene* s) {
    if (!s->frame.overlap_stream) HIP_TRY(hipStreamCreateWithFlags(&s->frame.overlap_stream, hipStreamNonBlocking));
    if (!s->frame.closest_stream) HIP_TRY(hipStreamCreateWithFlags(&s->frame.closest_stream, hipStreamNonBlocking));
    if (!s->frame.stage_fork) HIP_TRY(hipEventCreateWithFlags(&s->frame.stage_fork, hipEventDisableTiming));
    if (!s->frame.stage_tail) HIP_TRY(hipEventCreateWithFlags(&s->frame.stage_tail, hipEventDisableTiming));
    for (int b = 0; b < 3; b++) {
        if (!s->frame.stage_shaded[b]) HIP_TRY(hipEventCreateWithFlags(&s->frame.stage_shaded[b], hipEventDisableTiming));
        if (!s->frame.stage_traced[b]) HIP_TRY(hipEventCreateWithFlags(&s->frame.stage_traced[b], hipEventDisableTiming));
        if (!s->frame.stage_closest[b]) HIP_TRY(hipEventCreateWithFlags(&s->frame.stage_closest[b], hipEventDisableTiming));
    }
    return RR_OK;
}

// enqueues every stage; on any error or exception the frame's FrameStreamsIdle waits for all three streams
static int enqueue_level1_stages(FrameRun& f, const Level1Stages& sp, const DRayQueue& qin, uint32_t* count, uint64_t s0, uint64_t s1,
                                 const DRayQueue& qout, uint32_t* child_count, bool spawns, bool trace_closest) {
    rr_scene* s = f.s;
    const hipStream_t st = f.st, st2 = s->frame.overlap_stream, st3 = s->frame.closest_stream;
    unsigned long long* counters = s->frame.counters.as<unsigned long long>();
    if (sp.sq_need > s->frame.sq_cap || sp.valid_need * 8 > s->frame.sq_valid.bytes) return fail(RR_ERR_DEVICE, "internal: shadow queue smaller than its stage buffers");
    RR_TRY(join_shadow(f)); // (a level in several slices: the previous slice's last shadow stage reads the buffers and events this one reuses)
    uint32_t* closest_heads = nullptr; // one per closest-hit launch, RR_SQ_STRIDE words apart, zeroed on `st` before the fork
    if (trace_closest) {
        if (s0 != 0 || s1 != f.pr.n || sp.stage % RR_WAVE != 0) return fail(RR_ERR_DEVICE, "internal: closest-hit stages over a part of level 1");
        f.pool.align_line();
        closest_heads = f.pool.take(sp.n_stages * RR_SQ_STRIDE);
        if (!closest_heads) return counters_exhausted();
        HIP_TRY(sched_record(s->sched, s->frame.stage_fork, st, "stage_fork"));
        HIP_TRY(sched_wait(s->sched, st3, s->frame.stage_fork, "stage_fork"));
    }
    for (uint32_t k = 0; k < sp.n_stages; k++) {
        if (f.cancel && *f.cancel) return fail(RR_ERR_CANCELLED, "cancelled");
        RR_FAULT_POINT("level1_stages.stage"); // (tests: an exception between two stages, with launches of the earlier ones on all three streams)
        const uint64_t c0 = s0 + sp.begin_of(k), c1 = std::min<uint64_t>(c0 + sp.stage, s1);
        const uint32_t b = sp.buffer_of(k);
        const bool first = k == 0, last = k + 1 == sp.n_stages;
        const ShadeChunk g = plan_shade_chunk(c0, c1, s->data.n_enabled_lights, true); // (sq_cap <= sp.stage: lights x this many slots fit the buffer)
        const ChunkShadow q = take_chunk_shadow(f, sp.ray_offset[b], sp.valid_offset[b]); // (its head word is zeroed on `st` before the event the second stream waits for)
        // the first stage's shade runs alone: the serial loop's grid.  After it the launches share the CUs, the last stage's shadow launch too:
        // it runs beside the one before it and beside level 2 (rr_kernels.hip, RR_L1_SHADOW_WG: what was measured)
        const uint64_t shade_wg = first ? (uint64_t)f.shade_grid_max : (RR_L1_SHADE_WG ? (uint64_t)s->n_cus * RR_L1_SHADE_WG : g.groups);
        const uint64_t shadow_wg = (uint64_t)s->n_cus * RR_L1_SHADOW_WG;
        if (trace_closest) { // the host is stages ahead of the device: launch k is enqueued long before launch k - 1 ends
            {
                // Every launch of k_trace_closest<true> STORES the level's size (*q_count = n, a plain store of the same value).  Launch 0 stores it where
                // the shade launches read it; launch k > 0 runs beside shade launches that read that word, ordered against them by nothing, so it
                // is handed the word behind its own head word instead (zeroed with the pool, read by nobody): no store beside a load of one word.
                static_assert(RR_SQ_STRIDE >= 2, "a closest-hit launch's head word and its copy of the level's size share the launch's stride");
                uint32_t* const count_k = first ? count : closest_heads + (size_t)k * RR_SQ_STRIDE + 1;
                ScopedTimer t(s, st3, TK_CLOSEST, true);
                RR_TRY(launch_trace_closest(s, true, qin, count_k, closest_heads + (size_t)k * RR_SQ_STRIDE, f.pr.n, s->frame.shade_const.as<DShadeConst>(), f.pr, counters, st3,
                                            (uint32_t)(c0 / RR_WAVE), (uint32_t)(sp.stage / RR_WAVE), first ? RR_L1_CLOSEST_FIRST_WG : RR_L1_CLOSEST_WG));
            }
            HIP_TRY(sched_record(s->sched, s->frame.stage_closest[k % 3u], st3, "stage_closest", (int)(k % 3u)));
            HIP_TRY(sched_wait(s->sched, st, s->frame.stage_closest[k % 3u], "stage_closest", (int)(k % 3u)));
        }
        if (k >= sp.n_buf) HIP_TRY(sched_wait(s->sched, st, s->frame.stage_traced[b], "stage_traced", (int)b));
        RR_TRY(launch_shade(f, true, qin, count, c0, c1, qout, child_count, g, q, shade_wg, st));
        if (spawns && last) RR_TRY(read_back_level_size(f, child_count)); // behind the last shade stage
        HIP_TRY(sched_record(s->sched, s->frame.stage_shaded[b], st, "stage_shaded", (int)b));
        // The last stage's shadow launch goes to the third stream, idle by now (its last closest-hit launch ended before this stage was shaded):
        // on the second stream it would start only when the stage before it has been traced, and run alone.  It reads its own buffer and counters.
        const hipStream_t st_shadow = last ? st3 : st2;
        HIP_TRY(sched_wait(s->sched, st_shadow, s->frame.stage_shaded[b], "stage_shaded", (int)b));
        RR_TRY(launch_shadow(f, g, q, shadow_wg, st_shadow));
        HIP_TRY(sched_record(s->sched, s->frame.stage_traced[b], st_shadow, "stage_traced", (int)b));
    }
    // the second stream joins `st` later (join_shadow): before the deeper levels reuse the shadow queue, before k_resolve and before the frame's end event
    // ... and the third stream through it: stage_tail, on the second stream, follows the shadow launches of the last two stages
    HIP_TRY(sched_wait(s->sched, st2, s->frame.stage_traced[sp.buffer_of(sp.n_stages - 1)], "stage_traced", (int)sp.buffer_of(sp.n_stages - 1)));
    HIP_TRY(sched_record(s->sched, s->frame.stage_tail, st2, "stage_tail"));
    f.shadow_pending = s->frame.stage_tail;
    f.shadow_tail = level1_tail(sp);
    // (stage_traced[rest_buffer] was last recorded behind the shadow launch of rest_stage: the two stages after it use the other buffers)
    f.shadow_rest = f.shadow_tail.rest_stage >= 0 ? s->frame.stage_traced[f.shadow_tail.rest_buffer] : nullptr;
    return RR_OK;
}

// THE one way into the staged path.  Whatever ends it early (cancel flag, HIP error, counter pool exhausted, an exception) leaves launches on
// all three streams: the frame's FrameStreamsIdle (render_region_locked) waits for them, so the handle stays usable and the next frame cannot race a straggler.
static int run_level1_stages(FrameRun& f, const Level1Stages& sp, const DRayQueue& qin, uint32_t* count, uint64_t s0, uint64_t s1,
                             const DRayQueue& qout, uint32_t* child_count, bool spawns, bool trace_closest) {
    rr_scene* s = f.s;
    RR_TRY(ensure_overlap_stream(s));
    RR_TRY(enqueue_level1_stages(f, sp, qin, count, s0, s1, qout, child_count, spawns, trace_closest));
    s->frame.overlap_stages += sp.n_stages;
    return RR_OK;
}

// One depth level: rays [base, base + n) of the arena, their count also in the device word `count`.
// The size of the next level is read back once per slice (4 bytes + stream sync), so launches are sized by the
// rays that exist and empty levels are never launched.
// depth level 1 = the batch's primary rays [pr.first, pr.first + pr.n): only hit records (hit1); its children start the arena
// SEEDED (rr_shade_rays): depth level 1 is n ray records at the front of the arena like any deeper level -- arena hit records, the
// <false> builds of the three kernels (a path is a root where its record says depth 1 and carries the id bit), children behind
// the level, the dense shadow queue, no stages.
static int run_level(FrameRun& f, uint32_t d, uint64_t base, uint64_t n, uint32_t* count) {
    rr_scene* s = f.s;
    const hipStream_t st = f.st;
    const uint32_t L = s->data.n_enabled_lights;
    unsigned long long* counters = s->frame.counters.as<unsigned long long>();
    const bool l1 = d == 1 && !f.seeded; // the level-1 builds: rays derived from their index
    DRayQueue qin = f.queue_at(base);
    if (l1) { qin.r0 = nullptr; qin.r1 = nullptr; qin.r2 = nullptr; qin.hit = s->frame.hit1.as<uint4>(); }
    const bool spawns = d <= f.R; // the deepest level spawns nothing (k_shade: depth <= max_recursion)
    const uint64_t M = f.plan.M, child_base = l1 ? 0 : base + n;
    const uint64_t slice = level_slice(M, child_base, n, d, f.R);
    // level 1 keeps fixed shadow slots per chunk (rr_frame_plan.h plan_shade_chunk), only where the shadow kernel's packet form applies
    // (rr_kernels.hip, RR_BEAM_MIN_ITEMS .. RR_BEAM_MAX_ITEMS) and up to RR_FIXED_SLOT_LIGHTS enabled lights: k_shade keeps one bit per
    // light and lane for the validity words; more lights take the dense queue of the deeper levels, which has no such limit
    const bool sq_fixed = l1 && s->data.view.n_items >= RR_BEAM_MIN_ITEMS && s->data.view.n_items <= RR_BEAM_MAX_ITEMS && L <= RR_FIXED_SLOT_LIGHTS;
    // ... and with at least one light and two stages: shade and shadow launches side by side on two streams (per slice of the level)
    // (a split frame leaves the staged schedule out and runs the serial loop: integer adds commute, so its bits do not depend on the schedule)
    const auto staged = [&](uint64_t hits) { return !f.level1_only && !f.diffuse && level1_stages_wanted(s) && sq_fixed && L >= 1 && level1_stages(s, hits).overlapped(); };
    // ... and where the level is ONE slice, its closest hits stage by stage on a third stream; every other level in one launch, here
    const bool closest_staged = slice == n && staged(n);
    if (!closest_staged) {
        uint32_t* head = f.pool.take(1);
        if (!head) return counters_exhausted();
        ScopedTimer t(s, st, TK_CLOSEST, l1);
        RR_TRY(launch_trace_closest(s, l1, qin, count, head, n, s->frame.shade_const.as<DShadeConst>(), f.pr, counters, st, 0u, RR_ALL_PACKETS));
    }
    if (slice == 0) return fail(RR_ERR_OUT_OF_MEMORY, "ray arena of %llu rays is too small for depth level %u", (unsigned long long)M, d);
    if (slice < n) s->timing.stats.sliced_levels++;
    for (uint64_t s0 = 0; s0 < n; s0 += slice) {
        const uint64_t s1 = std::min<uint64_t>(s0 + slice, n);
        uint32_t* child_count = f.pool.take(1);
        if (!child_count) return counters_exhausted();
        const DRayQueue qout = f.queue_at(child_base);
        const bool in_stages = staged(s1 - s0);
        if (in_stages) RR_TRY(run_level1_stages(f, level1_stages(s, s1 - s0), qin, count, s0, s1, qout, child_count, spawns, closest_staged));
        for (uint64_t c0 = s0; c0 < s1 && !in_stages; c0 += f.plan.chunk) {
            if (f.cancel && *f.cancel) { (void)sched_sync_stream(s->sched, st, "cancelled"); return fail(RR_ERR_CANCELLED, "cancelled"); }
            const uint64_t c1 = std::min<uint64_t>(c0 + f.plan.chunk, s1);
            const ShadeChunk g = plan_shade_chunk(c0, c1, L, sq_fixed);
            if (f.level1_only) { // the ending of level 1 of rr_albedo_pixels: no shadow slots, no children, no counters of its own
                if (!l1 || spawns || !f.acc.rgb || !f.acc.flags) return fail(RR_ERR_DEVICE, "internal: albedo launch outside a level 1 that ends its paths");
                ScopedTimer t(s, st, TK_SHADE, true);
                if (s->sched.on) // (k_albedo_level1: the hits and what primary_ray reads; colour planes and flags only)
                    sched_launch(s->sched, st, "k_albedo_level1", {sa_r(s->frame.shade_const.p, sizeof(DShadeConst), "shade_const"), sa_r(f.pr.sample_tr, s->frame.sample_tr.bytes, "sample_tr"),
                                                                  sa_r(s->frame.slot_c.p, s->frame.slot_c.bytes, "slot_c"), sa_r(s->frame.pixel_c.p, s->frame.pixel_c.bytes, "pixel_c"),
                                                                  sa_r(count, 4, "level count"), sa_r(qin.hit + c0, (size_t)(c1 - c0) * 16, "hit records"),
                                                                  sa_a(f.acc.rgb, (size_t)f.acc.n * 24, "acc_rgb"), sa_a(f.acc.flags, (size_t)f.acc.n * 4, "acc_flags")});
                hipLaunchKernelGGL(k_albedo_level1, dim3((uint32_t)std::min<uint64_t>(g.groups, (uint64_t)f.shade_grid_max)), dim3(RR_BLOCK), 0, st, s->frame.shade_const.as<DShadeConst>(),
                                   f.pr, qin.hit, count, (uint32_t)c0, (uint32_t)c1, f.acc);
                continue;
            }
            RR_TRY(join_shadow_for(f, g)); // the chunk's queue starts where the staged level 1 keeps its first buffer
            const ChunkShadow q = take_chunk_shadow(f, 0, 0);
            RR_TRY(launch_shade(f, l1, qin, count, c0, c1, qout, child_count, g, q, (uint64_t)f.shade_grid_max, st));
            // The size of the next level is final once the slice's last shade chunk has run: its read-back is enqueued
            // BEFORE that chunk's shadow kernel, so the host learns it (and enqueues the next level) while the shadow
            // rays are still being traced, instead of leaving the device idle for a host round trip per level.
            if (spawns && c1 == s1) RR_TRY(read_back_level_size(f, child_count));
            if (L) RR_TRY(launch_shadow(f, g, q, (uint64_t)f.shadow_grid, st, l1 && f.diffuse != nullptr));
        }
        if (!spawns) continue;
        HIP_TRY(sched_sync_event(s->sched, s->frame.count_ready, "count_ready"));
        sched_host_read(s->sched, s->frame.h_count + HC_LEVEL, 4, "h_count[HC_LEVEL]");
        const uint64_t m = s->frame.h_count[HC_LEVEL];
        if (m > M - child_base) return fail(RR_ERR_DEVICE, "internal: level %u holds %llu rays, room for %llu", d + 1, (unsigned long long)m, (unsigned long long)(M - child_base));
        if (m == 0) continue;
        uint64_t level_base = child_base;
        // (no join in front of bin_level: its kernels read and write the arena and fresh words of the counter pool, nothing a pending shadow launch touches)
        RR_TRY(bin_level(f, child_base, m, &level_base));
        RR_TRY(run_level(f, d + 1, level_base, m, child_count));
    }
    return RR_OK;
}

static void launch_resolve(const FrameRun& f, const DFrame& fr, const FrameIo& io) {
    const dim3 grid((fr.n_region_pixels + RR_BLOCK - 1) / RR_BLOCK), block(RR_BLOCK);
    const uint32_t by_pixel = io.pixel_xy ? 0u : 1u; // a region's answers go to y * width + x, a list's to the entry's index
    if (f.s->sched.on && io.end != FrameEnd::NONE) {
        // every resolve reads the planes of its n slots and the slot -> pixel map and writes one answer per pixel: at y * width + x anywhere in the
        // frame, or at the slot's (the entry's) index; with parts a pixel is K slots and has K part records more
        ScheduleLog& log = f.s->sched;
        const size_t n = fr.n_region_pixels, K = (size_t)1 << io.lg_parts, frame_px = (size_t)fr.width * fr.height;
        const size_t px = io.end == FrameEnd::REGION_BYTES ? (io.frame_layout ? frame_px : n) : (by_pixel ? frame_px : n >> io.lg_parts);
        const bool split = io.end == FrameEnd::RECORD_SPLIT, parts = io.end == FrameEnd::RECORD_PARTS || split, region = io.end == FrameEnd::REGION_BYTES;
        const bool records = io.end == FrameEnd::RECORDS || parts;
        static const char* const name[6] = {"k_resolve", "k_resolve_pixels", "k_resolve_pixel_parts", "k_resolve_albedo", "k_resolve_pixel_split", ""};
        sched_launch(log, f.st, name[(int)io.end],
                     {sa_r(f.acc.rgb, n * 24, "acc_rgb"), sa_r(f.acc.normal, n * 24, "acc_normal"), sa_r(f.acc.depth, n * 8, "acc_depth"), sa_r(f.acc.object_id, n * 4, "acc_id"),
                      sa_r(f.acc.flags, n * 4, "acc_flags"), sa_r(split ? f.diffuse : nullptr, n * 24, "acc_diffuse"), sa_r(region ? nullptr : f.slot_xy, n * 4, "slot_xy"),
                      sa_r(region ? f.s->frame.region_xy.p : nullptr, n * 4, "region_xy"), sa_r(region ? f.s->frame.trace_order.p : nullptr, n * 4, "trace_order"),
                      sa_w(region ? io.out->rgba8 : nullptr, px * 4, "out rgba8"), sa_w(region ? io.out->normal : nullptr, px * 12, "out normal"),
                      sa_w(region ? io.out->depth : nullptr, px * 4, "out depth"), sa_w(region ? io.out->object_id : nullptr, px * 4, "out object_id"),
                      sa_w(records ? io.radiance : nullptr, px * 32, "out records"), sa_w(io.end == FrameEnd::RECORDS ? io.rgba8 : nullptr, px * 4, "out rgba8"),
                      sa_w(parts ? io.parts : nullptr, px * K * 32, "out part records"), sa_w(split ? io.diffuse : nullptr, px * 12, "out diffuse"),
                      sa_w(split ? io.diffuse_parts : nullptr, px * K * 12, "out diffuse parts"), sa_w(io.end == FrameEnd::ALBEDO ? io.albedo : nullptr, px * 12, "out albedo")});
    }
    switch (io.end) {
    case FrameEnd::NONE: break;
    case FrameEnd::ALBEDO: hipLaunchKernelGGL(k_resolve_albedo, grid, block, 0, f.st, fr, f.slot_xy, f.acc, by_pixel, (uint32_t*)io.albedo); break;
    case FrameEnd::RECORD_PARTS:
        hipLaunchKernelGGL(k_resolve_pixel_parts<false>, grid, block, 0, f.st, fr, f.slot_xy, f.acc, (const long long*)nullptr, io.lg_parts, by_pixel, (float4*)io.radiance,
                           (float4*)io.parts, (float*)nullptr, (float*)nullptr);
        break;
    case FrameEnd::RECORD_SPLIT:
        hipLaunchKernelGGL(k_resolve_pixel_parts<true>, grid, block, 0, f.st, fr, f.slot_xy, f.acc, (const long long*)f.diffuse, io.lg_parts, by_pixel, (float4*)io.radiance,
                           (float4*)io.parts, io.diffuse, io.diffuse_parts);
        break;
    case FrameEnd::RECORDS: hipLaunchKernelGGL(k_resolve_pixels, grid, block, 0, f.st, fr, f.slot_xy, f.acc, by_pixel, (float4*)io.radiance, (uint32_t*)io.rgba8); break;
    case FrameEnd::REGION_BYTES:
        hipLaunchKernelGGL(k_resolve, grid, block, 0, f.st, fr, f.s->frame.region_xy.as<uint32_t>(), f.s->frame.trace_order.as<uint32_t>(), f.acc, io.out->rgba8, io.out->normal,
                           io.out->depth, io.out->object_id, io.frame_layout ? 1u : 0u);
        break;
    }
}

// The frame's batches of primary rays, in order.  After a batch that ends on a whole slice of samples the pass hook
// (if any) gets the frame resolved over the samples finished so far.  first0: the primary index the batches start at, a whole number
// of sample slices (a pass that goes on where resident accumulators stopped); the plan's total_primary indices follow it.
static int run_batches(FrameRun& f, const DFrame& fr, const FrameIo& io, uint64_t first0 = 0) {
    rr_scene* s = f.s;
    const uint32_t npix = fr.n_region_pixels;
    const uint64_t B = f.plan.B, total_primary = first0 + f.plan.total_primary;
    const PassHook* hook = io.hook;
    for (uint64_t first = first0; first < total_primary; first += B) {
        if (f.cancel && *f.cancel) { (void)sched_sync_stream(s->sched, f.st, "cancelled"); return fail(RR_ERR_CANCELLED, "cancelled"); }
        const uint32_t n_batch = (uint32_t)std::min<uint64_t>(B, total_primary - first);
        RR_TRY(join_shadow(f)); // the previous batch's last shadow launch reads counters of the pool that start_batch zeroes
        RR_TRY(f.pool.start_batch());
        uint32_t* level1_count = f.pool.take(1);
        // The batch covers primary indices [first, first + n_batch): index i -> sample i / npix, pixel i % npix.
        f.pr.at = primary_launch(first, npix, batch_group(f.plan, npix, first, n_batch)); f.pr.n = n_batch;
        s->timing.stats.batches++;
        RR_TRY(run_level(f, 1, 0, n_batch, level1_count));
        HIP_TRY(hipGetLastError());
        // batches are stream-ordered; only a caller that can cancel needs the host to keep pace with the device
        if (f.cancel && first + B < total_primary) HIP_TRY(sched_sync_stream(s->sched, f.st, "keep pace with a cancellable frame"));
        const uint64_t done = first + n_batch;
        if (hook && hook->fn && done < total_primary && done % npix == 0) {
            DFrame pf = fr;
            pf.samples = (uint32_t)(done / npix); // the mean over the sample slices finished so far
            RR_TRY(join_shadow(f));
            launch_resolve(f, pf, io);
            RR_TRY(copy_outputs(s->sched, *hook->host, *io.out, (size_t)fr.width * fr.height, f.st));
            InPass in_pass(s);
            if (hook->fn(hook->user, done, total_primary) != 0) return fail(RR_ERR_CANCELLED, "stopped by the pass callback");
        }
    }
    return RR_OK;
}

// The handle's frame and query buffers are shared: frames and queries on different streams are serialised.
static int take_stream(rr_scene* s, hipStream_t st) {
    if (st != s->frame.last_stream) { HIP_TRY(sched_sync_stream(s->sched, s->frame.last_stream, "take_stream")); s->frame.last_stream = st; }
    return RR_OK;
}
// a frame's (or a radiance query's) statistics start from nothing
static void begin_frame_stats(rr_scene* s) {
    resolve_timers(s); // launches of an earlier frame nobody asked about must not leak into this frame's stats
    memset(&s->timing.stats, 0, sizeof s->timing.stats);
    s->timing.stats_final = false; s->timing.has_carry = false;
    s->frame.overlap_stages = 0;
}

static int render_region_body(rr_scene* s, const rr_camera* cam, const rr_config* cfg, const uint16_t* sample_xy,
                              const FrameIo& io, hipStream_t st, const volatile int* cancel) {
    RR_TRY(check_intact(s));
    HIP_TRY(hipSetDevice(s->device));
    RR_TRY(take_stream(s, st));
    const uint32_t W = cam->width, H = cam->height;
    if ((uint64_t)W * H > (1ull << 30)) return fail(RR_ERR_UNSUPPORTED, "frame of %ux%u pixels", W, H);
    uint32_t npix;
    const uint32_t* slot_xy; // accumulator slot -> pixel, and the screen point of its centre: the list's own tables or the region's
    const float* slot_c;
    if (io.pixel_xy) {
        RR_TRY(fill_pixel_slots(s, W, H, io.pixel_xy, io.n_pixels, io.lg_parts, st, io.own_list));
        npix = io.n_pixels << io.lg_parts; slot_xy = s->frame.pixel_xy.as<uint32_t>(); slot_c = s->frame.pixel_c.as<float>();
    } else {
        RR_TRY(update_region_map(s, W, H, *io.region, st));
        npix = (uint32_t)s->frame.h_region_xy.size(); slot_xy = s->frame.region_xy.as<uint32_t>(); slot_c = s->frame.slot_c.as<float>();
        if (io.lg_parts && npix) { // the region's slots, in their order, as the entries of a list: K slots each, in the list's own tables
            RR_TRY(fill_pixel_slots(s, W, H, slot_xy, npix, io.lg_parts, st));
            npix <<= io.lg_parts; slot_xy = s->frame.pixel_xy.as<uint32_t>(); slot_c = s->frame.pixel_c.as<float>();
        }
    }
    begin_frame_stats(s);
    if (npix == 0) return RR_OK;
    RR_TRY(ensure_camera_reach(s, cam, cfg)); // the top level's boxes must be padded for this camera's distance from the origin
    DFrame fr = make_frame(cam, cfg);
    fr.n_region_pixels = npix;
    RR_TRY(upload_sample_table(s, fr, sample_xy, st));
    // a prefix: samples [samples_from, used) of the frame.  The table above and the cell size are the whole frame's; from here on the frame's
    // count is `used` (k_shade: the id is that of sample used - 1, as the oracle's samples_used has it; the resolve divides by it)
    const uint32_t used = io.samples_used ? io.samples_used : cfg->samples;
    fr.samples = used;
    const FrameEndPlan end = frame_end_plan(io);
    const uint32_t R = end.level1_only ? 0u : cfg->max_recursion;
    DAccum acc;
    long long* diffuse = nullptr; // (a split frame's planes)
    RR_TRY(reset_accumulators(s, npix, end, st, &acc, io.resident, &diffuse));
    // The frame's plan (rr_frame_plan.h), and its level-1 hit records, ray arena and shadow queue.  With parts the plan sees K x the slots
    // and 1 / K of the samples (a sample group must divide THIS range: plan_frame); the frame constants keep the frame's S.
    uint64_t budget = 0;
    RR_TRY(queue_budget(s, &budget));
    const FramePlan plan = plan_frame(FramePlanInputs{npix, (used - io.samples_from) >> io.lg_parts, R, budget, s->tuning.sample_group, io.hook ? io.hook->min_passes : 0u,
                                                      s->frame.arena_factor, s->data.n_enabled_lights, s->tuning.shade_chunk_rays});
    HIP_TRY(s->frame.hit1.reserve(plan.B * 16));
    if (!end.level1_only) { // the shadow queue serves the serial loop and, where level 1 runs in stages, the stage buffers (their layout is the same for every batch)
        const Level1Stages sp = level1_stages(s, plan.B);
        RR_TRY(grow_ray_queues(s, plan.M, std::max<uint64_t>(plan.sq_need, level1_stages_wanted(s) ? sp.sq_need : 0ull), sp.valid_need, end.split));
    }
    RR_TRY(upload_shade_const(s, fr, primary_frame(slot_c, npix, plan.G), st)); // (after the plan: the index constants follow its sample group)
    FrameRun f = make_frame_run(s, st, plan, R, end.level1_only, acc, DPrimary{s->frame.sample_tr.as<float>(), primary_launch(0, npix, 1u), 0u, io.lg_parts}, slot_xy, cancel);
    if (end.split) { f.diffuse = diffuse; f.sq_s3 = s->frame.sq3.as<float4>(); }
    HIP_TRY(sched_record(s->sched, s->timing.frame_a, st, "frame_a"));
    int rc = run_batches(f, fr, io, (uint64_t)(io.samples_from >> io.lg_parts) * npix);
    if (rc == RR_OK) rc = join_shadow(f); // level 2 empty, or a level 1 that spawns nothing: the join falls here
    if (rc != RR_OK) return rc; // (FrameStreamsIdle waits for whatever is pending)
    launch_resolve(f, fr, io);
    HIP_TRY(sched_record(s->sched, s->timing.frame_b, st, "frame_b"));
    HIP_TRY(hipGetLastError());
    // a scene that branches more than the arena was sized for gets a larger one for its next frame (within the budget)
    if (s->timing.stats.sliced_levels > 0 && s->frame.arena_factor < 128) s->frame.arena_factor *= 2;
    return RR_OK;
}

// (the recorder's scope: the log holds what was enqueued between this function's entry and its return, whichever way it is left)
static int render_region_locked(rr_scene* s, const rr_camera* cam, const rr_config* cfg, const uint16_t* sample_xy,
                                const FrameIo io, hipStream_t st, const volatile int* cancel) {
    ScheduleScope scope(s->sched, st);
    FrameStreamsIdle idle(s, st); // (destroyed before `scope`: on unwinding its waits stand in front of the log's end marker, as on an error code)
    return scope.done(idle.done(render_region_body(s, cam, cfg, sample_xy, io, st, cancel)));
}

extern "C" int rr_render_region_device(rr_scene* s, const rr_camera* cam, const rr_config* cfg, const uint16_t* sample_xy,
                                       const rr_region* rg, const rr_frame* out, void* hip_stream, const volatile int* cancel) try {
    RR_TRY(check_frame_args(s, cam, cfg, sample_xy));
    RR_TRY(check_region(cam->width, cam->height, rg));
    if (!out || !out->rgba8) return fail(RR_ERR_INVALID_ARGUMENT, "out->rgba8 is required");
    RR_TRY(not_in_pass(s, "rr_render_region_device"));
    std::lock_guard<std::mutex> lk(s->mu);
    return render_region_locked(s, cam, cfg, sample_xy, frame_io(rg, out, false), (hipStream_t)hip_stream, cancel);
} RR_GUARD_END("rr_render_region_device")

static int render_to_host(rr_scene* s, const rr_camera* cam, const rr_config* cfg, const uint16_t* sample_xy, const rr_frame* out,
                          const volatile int* cancel, rr_pass_fn fn, void* user, uint32_t min_passes) {
    RR_TRY(check_frame_args(s, cam, cfg, sample_xy));
    if (!out || !out->rgba8) return fail(RR_ERR_INVALID_ARGUMENT, "out->rgba8 is required");
    RR_TRY(not_in_pass(s, fn ? "rr_render_progressive" : "rr_render"));
    std::lock_guard<std::mutex> lk(s->mu);
    HIP_TRY(hipSetDevice(s->device));
    const size_t np = (size_t)cam->width * cam->height;
    rr_frame dev{};
    RR_TRY(stage_outputs(s, *out, np, false, &dev));
    PassHook hook{fn, user, min_passes, out};
    RR_TRY(render_region_locked(s, cam, cfg, sample_xy, frame_io(&WHOLE_FRAME, &dev, true, fn ? &hook : nullptr), nullptr, cancel));
    HIP_TRY(hipStreamSynchronize(nullptr));
    return copy_outputs(s->sched, *out, dev, np, nullptr);
}

extern "C" int rr_render(rr_scene* s, const rr_camera* cam, const rr_config* cfg, const uint16_t* sample_xy, const rr_frame* out,
                         const volatile int* cancel) try {
    return render_to_host(s, cam, cfg, sample_xy, out, cancel, nullptr, nullptr, 0);
} RR_GUARD_END("rr_render")

extern "C" int rr_render_progressive(rr_scene* s, const rr_camera* cam, const rr_config* cfg, const uint16_t* sample_xy, const rr_frame* out,
                                     uint32_t min_passes, rr_pass_fn on_pass, void* user, const volatile int* cancel) try {
    if (!on_pass) return fail(RR_ERR_INVALID_ARGUMENT, "on_pass is required (use rr_render for a one-shot frame)");
    return render_to_host(s, cam, cfg, sample_xy, out, cancel, on_pass, user, min_passes);
} RR_GUARD_END("rr_render_progressive")

// the device's work counters of the frame (or pass) that ran last, or of the batches so far inside on_pass
static int read_counters(const rr_scene* s, rr_frame_stats* st) {
    unsigned long long c[RR_CNT_WORDS];
    HIP_TRY(hipMemcpy(c, s->frame.counters.p, sizeof c, hipMemcpyDeviceToHost));
    st->primary_rays = c[RR_CNT_PRIMARY]; st->secondary_rays = c[RR_CNT_SECONDARY];
    st->shadow_rays = c[RR_CNT_SHADOW]; st->shaded_hits = c[RR_CNT_SHADED];
    return RR_OK;
}
// sum += a, field by field: the statistics of a frame made of several passes (rr_render_progressive_tiles, rr_render_adaptive, rr_render_adaptive_levels)
static void add_pass_stats(rr_frame_stats* sum_, const rr_frame_stats& a) {
    rr_frame_stats& sum = *sum_;
    sum.primary_rays += a.primary_rays; sum.secondary_rays += a.secondary_rays; sum.shadow_rays += a.shadow_rays; sum.shaded_hits += a.shaded_hits;
    sum.ms_total += a.ms_total; sum.ms_trace_closest += a.ms_trace_closest; sum.ms_trace_shadow += a.ms_trace_shadow; sum.ms_shade += a.ms_shade;
    sum.launches_trace_closest += a.launches_trace_closest; sum.launches_trace_shadow += a.launches_trace_shadow; sum.launches_shade += a.launches_shade;
    sum.batches += a.batches; sum.sliced_levels += a.sliced_levels; sum.binned_rays += a.binned_rays; sum.ms_binning += a.ms_binning;
    sum.ms_trace_closest_level1 += a.ms_trace_closest_level1; sum.launches_trace_closest_level1 += a.launches_trace_closest_level1;
    sum.ms_shade_level1 += a.ms_shade_level1; sum.launches_shade_level1 += a.launches_shade_level1;
    sum.ms_trace_shadow_level1 += a.ms_trace_shadow_level1; sum.launches_trace_shadow_level1 += a.launches_trace_shadow_level1;
}
// The statistics of a call made of several passes are the sums over them.  add: the pass that was just collected (collect_stats_locked, the
// stream idle).  carry: the last pass is still in flight -- the device reports it when somebody asks and the sums so far are added to it,
// once (FrameTiming::carry), so the call need not wait for its last launch.  close: unless carried, no pass is in flight and the sums are final.
struct PassSums {
    rr_scene* s; rr_frame_stats sum{}; bool carried = false;
    void add() { add_pass_stats(&sum, s->timing.stats); }
    void carry() { s->timing.carry = sum; s->timing.has_carry = true; carried = true; }
    void close() { if (!carried) { s->timing.stats = sum; s->timing.has_carry = false; s->timing.stats_final = true; } }
};
// the device counters and launch timers of the frame (or pass) that ran last, into s->timing.stats; behind a pass that carries the sums
// of the passes before it (PassSums::carry) these are added, once, and the sums are final
static int collect_stats_locked(rr_scene* s) {
    float ms = 0.0f;
    if (hipEventSynchronize(s->timing.frame_b) == hipSuccess && hipEventElapsedTime(&ms, s->timing.frame_a, s->timing.frame_b) == hipSuccess) s->timing.stats.ms_total = ms;
    resolve_timers(s);
    RR_TRY(read_counters(s, &s->timing.stats));
    if (s->timing.has_carry) {
        add_pass_stats(&s->timing.stats, s->timing.carry);
        s->timing.has_carry = false; s->timing.stats_final = true;
    }
    return RR_OK;
}
extern "C" int rr_scene_overlap_stages(const rr_scene* cs, uint32_t* out) try {
    if (!cs || !out) return fail(RR_ERR_INVALID_ARGUMENT, "NULL argument");
    *out = cs->frame.overlap_stages;
    return RR_OK;
} RR_GUARD_END("rr_scene_overlap_stages")

extern "C" int rr_scene_last_stats(const rr_scene* cs, rr_frame_stats* out) try {
    if (!cs || !out) return fail(RR_ERR_INVALID_ARGUMENT, "NULL argument");
    if (tl_in_pass == cs) { // inside on_pass of this scene: its frame holds s->mu on this thread and the stream is idle -- the passes so far
        rr_frame_stats st = cs->timing.stats;
        if (!cs->timing.stats_final) RR_TRY(read_counters(cs, &st));
        *out = st;
        return RR_OK;
    }
    rr_scene* s = const_cast<rr_scene*>(cs);
    std::lock_guard<std::mutex> lk(s->mu);
    HIP_TRY(hipSetDevice(s->device));
    if (!s->timing.stats_final) { const int rc = collect_stats_locked(s); if (rc != RR_OK) return rc; }
    *out = s->timing.stats;
    return RR_OK;
} RR_GUARD_END("rr_scene_last_stats")

// The frame filled in TILE BY TILE, every pixel final when it appears: what the reference's GUI shows (shuffled 2x2 cells, each rendered with all of
// its samples: src/renderer.rs:125-172, drained by Run::apply_pixels, src/run.rs:506-545).  Pass k of n_passes renders the 32x8-pixel tiles with
// tile_index % n_passes == k -- an interleaved subset, like the shuffled cell list -- straight into their places in the frame.
extern "C" int rr_render_progressive_tiles(rr_scene* s, const rr_camera* cam, const rr_config* cfg, const uint16_t* sample_xy, const rr_frame* out,
                                           uint32_t n_passes, rr_pass_fn on_pass, void* user, const volatile int* cancel) try {
    if (!on_pass) return fail(RR_ERR_INVALID_ARGUMENT, "on_pass is required (use rr_render for a one-shot frame)");
    RR_TRY(check_frame_args(s, cam, cfg, sample_xy));
    if (!out || !out->rgba8) return fail(RR_ERR_INVALID_ARGUMENT, "out->rgba8 is required");
    RR_TRY(not_in_pass(s, "rr_render_progressive_tiles"));
    std::lock_guard<std::mutex> lk(s->mu);
    HIP_TRY(hipSetDevice(s->device));
    const uint32_t W = cam->width, H = cam->height, TW = 32, TH = 8;
    const size_t np = (size_t)W * H;
    for (int k = 0; k < 4; k++) // pixels not rendered yet are zero, also when the frame stops before its first pass
        if (out_buffer(*out, k)) memset(out_buffer(*out, k), 0, np * OUT_ELEM[k]);
    rr_frame dev{};
    RR_TRY(stage_outputs(s, *out, np, true, &dev));
    const uint32_t n_tiles = ((W + TW - 1) / TW) * ((H + TH - 1) / TH);
    const uint32_t P = std::max(1u, std::min(n_passes ? n_passes : 16u, n_tiles));
    PassSums sums{s};
    uint64_t done = 0;
    for (uint32_t k = 0; k < P; k++) {
        if (cancel && *cancel) return fail(RR_ERR_CANCELLED, "cancelled");
        const rr_region rg{TW, TH, P, k};
        RR_TRY(render_region_locked(s, cam, cfg, sample_xy, frame_io(&rg, &dev, true), nullptr, cancel));
        HIP_TRY(hipStreamSynchronize(nullptr));
        RR_TRY(collect_stats_locked(s));
        sums.add(); // the frame's statistics are the sums over its passes
        RR_TRY(copy_outputs(s->sched, *out, dev, np, nullptr));
        done += rr_region_pixel_count(W, H, &rg);
        sums.close();
        if (k + 1 < P) {
            InPass in_pass(s);
            if (on_pass(user, done * cfg->samples, (uint64_t)np * cfg->samples) != 0) return fail(RR_ERR_CANCELLED, "stopped by the pass callback");
        }
    }
    return RR_OK;
} RR_GUARD_END("rr_render_progressive_tiles")

extern "C" int rr_scene_set_compat(rr_scene* s, uint32_t flags) try {
    if (!s) return fail(RR_ERR_INVALID_ARGUMENT, "NULL argument");
    if (flags & ~RR_COMPAT_OCCLUDER_ALPHA_SHADOWS) return fail(RR_ERR_INVALID_ARGUMENT, "unknown compatibility flags 0x%x", flags);
    RR_TRY(not_in_pass(s, "rr_scene_set_compat"));
    std::lock_guard<std::mutex> lk(s->mu);
    s->data.view.compat = (s->data.view.compat & RR_VIEW_NAN_BALLS) | flags; // the scene view is passed to the kernels by value with every launch
    return RR_OK;
} RR_GUARD_END("rr_scene_set_compat")

extern "C" int rr_scene_set_tuning(rr_scene* s, const rr_tuning* t) try {
    if (!s || !t) return fail(RR_ERR_INVALID_ARGUMENT, "NULL argument");
    if (t->struct_size != sizeof(rr_tuning)) return fail(RR_ERR_INVALID_ARGUMENT, "rr_tuning::struct_size %u, library expects %zu", t->struct_size, sizeof(rr_tuning));
    if (t->sample_group > 64u || (t->sample_group & (t->sample_group - 1u))) return fail(RR_ERR_INVALID_ARGUMENT, "sample_group %u is not 0 or a power of two <= 64", t->sample_group);
    RR_TRY(not_in_pass(s, "rr_scene_set_tuning"));
    std::lock_guard<std::mutex> lk(s->mu);
    s->tuning = *t;
    s->timing.profiling = t->kernel_timing != 0;
    return RR_OK;
} RR_GUARD_END("rr_scene_set_tuning")
extern "C" int rr_scene_get_tuning(const rr_scene* s, rr_tuning* t) try {
    if (!s || !t) return fail(RR_ERR_INVALID_ARGUMENT, "NULL argument");
    *t = s->tuning;
    t->struct_size = (uint32_t)sizeof(rr_tuning);
    return RR_OK;
} RR_GUARD_END("rr_scene_get_tuning")

