// rr_api_prefix.h — the first samples of a frame as records, and a frame refined level by level whose pixels KEEP their samples: every
// level is a prefix of ONE frame of config->samples samples, and a pixel that climbs is given only the samples it does not have yet.
// Offers: rr_render_pixel_prefix, rr_render_pixel_prefix_device, rr_render_adaptive_prefix, rr_render_adaptive_prefix_device.
// Needs:  rr_api_frame.h (FrameIo: samples_used, samples_from, resident, own_list, FrameEnd::NONE and RECORD_PARTS; pixels_io, render_region_locked, ScopedTimer,
//         IdleOnExit, PassSums, collect_stats_locked), rr_api_query.h (check_pixels_args, host_list_call, check_query_pointers),
//         rr_api_adaptive.h (list_scratch, await_list_count; FusedOut, check_fused_outputs, device_fused_call, host_fused_call,
//         launch_record_bytes, finish_fused), rr_api_levels.h (check_ladder), rr_adaptive.h (the sets of resident accumulators), kernels 5m,
//         5p, 5t and 5u of rr_kernels.hip.
//
// The prefix is the frame driver with its batch loop ending at samples_used / K * slots and its resolve dividing by samples_used.  The
// fused call is: the whole frame in two halves over [0, P0) WITHOUT a resolve; then per level k_prefix_masks (records, error and refine
// masks straight from the integer sums), k_refine_scan, the wait for the 4 bytes of the count, k_prefix_compact (the survivors' pixels
// into the next list, their sums into the next set) and the frame driver over that list for samples [P(l-1), Pl) on the set as it is;
// k_record_bytes at the end.  The host forms are the device forms behind the staging copies of every list call and every fused call
// (host_list_call, rr_api_query.h; host_fused_call, rr_api_adaptive.h).

static int check_prefix_args(const char* fn, bool device, const rr_scene* s, const rr_camera* cam, const rr_config* cfg, const uint16_t* sample_xy,
                             const uint32_t* pixel_xy, uint32_t n_pixels, uint32_t samples_used, const rr_radiance* out, const rr_radiance* halves,
                             const uint8_t* rgba8) {
    RR_TRY(check_pixels_args(fn, device, s, cam, cfg, sample_xy, pixel_xy, n_pixels, out, rgba8));
    if (samples_used == 0u || samples_used > cfg->samples)
        return fail(RR_ERR_INVALID_ARGUMENT, "%s: samples_used %u must be from 1 to samples %u", fn, samples_used, (unsigned)cfg->samples);
    if (halves && (samples_used & 1u))
        return fail(RR_ERR_INVALID_ARGUMENT, "%s: samples_used %u is odd; with halves_out it must be even: the two halves of a pixel must be equal", fn, samples_used);
    if (halves && (uint64_t)n_pixels * 2u > (1ull << 30)) return fail(RR_ERR_UNSUPPORTED, "%s: %u pixels x 2 halves are more than 2^30 accumulator slots", fn, n_pixels);
    if (device && ((uintptr_t)halves & 15u)) return fail(RR_ERR_INVALID_ARGUMENT, "%s: out_dev and halves_out_dev must be 16-byte aligned", fn);
    return RR_OK;
}

// one call on buffers the device can address (the caller holds the lock); a call that ends early leaves the stream idle
static int render_pixel_prefix_locked(rr_scene* s, const rr_camera* cam, const rr_config* cfg, const uint16_t* sample_xy, const uint32_t* pixel_xy,
                                      uint32_t n_pixels, uint32_t samples_used, rr_radiance* out, rr_radiance* halves, uint8_t* rgba8, hipStream_t st,
                                      const volatile int* cancel) {
    IdleOnExit idle(st);
    // (k_resolve_pixel_parts has no byte output: with halves the bytes come from the finished records, as rr_render_adaptive makes its own)
    FrameIo io = pixels_io(pixel_xy, n_pixels, out, halves ? nullptr : rgba8);
    if (halves) { io.end = FrameEnd::RECORD_PARTS; io.lg_parts = 1u; io.parts = halves; }
    io.samples_used = samples_used;
    RR_TRY(render_region_locked(s, cam, cfg, sample_xy, io, st, cancel));
    if (halves && rgba8) {
        launch_record_bytes(s, cfg, out, n_pixels, rgba8, st);
        if (hipGetLastError() != hipSuccess) return fail(RR_ERR_DEVICE, "rr_render_pixel_prefix: a launch failed");
    }
    return idle.done(RR_OK);
}

// (C linkage: the entry points of this layer are declared in include/rustray_hip.h, inside its extern "C" block, and a definition keeps the
// linkage of its declaration; tests/test_adaptive_prefix_host.py holds each to the guard every entry point has)
int rr_render_pixel_prefix_device(rr_scene* s, const rr_camera* cam, const rr_config* cfg, const uint16_t* sample_xy, const uint32_t* pixel_xy,
                                  uint32_t n_pixels, uint32_t samples_used, rr_radiance* out, rr_radiance* halves_out, uint8_t* rgba8_out, void* hip_stream,
                                  const volatile int* cancel) try {
    RR_TRY(check_prefix_args("rr_render_pixel_prefix_device", true, s, cam, cfg, sample_xy, pixel_xy, n_pixels, samples_used, out, halves_out, rgba8_out));
    if (n_pixels == 0) return RR_OK;
    RR_TRY(not_in_pass(s, "rr_render_pixel_prefix_device"));
    std::lock_guard<std::mutex> lk(s->mu);
    RR_TRY(check_intact(s));
    HIP_TRY(hipSetDevice(s->device));
    RR_TRY(check_query_pointers(s, "rr_render_pixel_prefix_device",
                                {{pixel_xy, "pixel_xy_dev"}, {out, "out_dev"}, {halves_out, "halves_out_dev"}, {rgba8_out, "rgba8_out_dev"}}));
    return render_pixel_prefix_locked(s, cam, cfg, sample_xy, pixel_xy, n_pixels, samples_used, out, halves_out, rgba8_out, (hipStream_t)hip_stream, cancel);
} RR_GUARD_END("rr_render_pixel_prefix_device")

int rr_render_pixel_prefix(rr_scene* s, const rr_camera* cam, const rr_config* cfg, const uint16_t* sample_xy, const uint32_t* pixel_xy, uint32_t n_pixels,
                           uint32_t samples_used, rr_radiance* out, rr_radiance* halves_out, uint8_t* rgba8_out, const volatile int* cancel) try {
    RR_TRY(check_prefix_args("rr_render_pixel_prefix", false, s, cam, cfg, sample_xy, pixel_xy, n_pixels, samples_used, out, halves_out, rgba8_out));
    if (n_pixels == 0) return RR_OK;
    return host_list_call(s, "rr_render_pixel_prefix", cam, pixel_xy, n_pixels, 2u, out, halves_out, rgba8_out,
                          [&](const uint32_t* d_list, rr_radiance* d_out, rr_radiance* d_halves, uint8_t* d_rgba) {
                              return render_pixel_prefix_locked(s, cam, cfg, sample_xy, d_list, n_pixels, samples_used, d_out, d_halves, d_rgba, nullptr, cancel);
                          });
} RR_GUARD_END("rr_render_pixel_prefix")

// ---- the fused ladder

// what both forms check before the scene is looked at
static int check_adaptive_prefix_args(const char* fn, bool device, const rr_scene* s, const rr_camera* cam, const rr_config* cfg, const uint16_t* sample_xy,
                                      const uint16_t* prefix_samples, uint32_t n_levels, float threshold, const FusedOut& o) {
    RR_TRY(check_frame_args(s, cam, cfg, sample_xy));
    RR_TRY(check_ladder(fn, "prefix_samples", "prefixes", prefix_samples, n_levels, [](uint32_t) { return RR_OK; }));
    if (prefix_samples[n_levels - 1] != cfg->samples)
        return fail(RR_ERR_INVALID_ARGUMENT, "%s: prefix_samples[%u] = %u is not samples %u: the last prefix must be the whole frame", fn, n_levels - 1,
                    (unsigned)prefix_samples[n_levels - 1], (unsigned)cfg->samples);
    return check_fused_outputs(fn, device, cam, threshold, o);
}

// a set of n slots at `base` as the accumulators of a pass (rr_adaptive.h: the layout)
static DAccum prefix_set_accum(const DevBuf& b, uint64_t n) {
    char* base = (char*)b.p;
    return DAccum{(long long*)(base + prefix_plane_offset(0u, n)), (long long*)(base + prefix_plane_offset(3u, n)), (long long*)(base + prefix_plane_offset(6u, n)),
                  (uint32_t*)(base + prefix_id_offset(n)), (unsigned long long)n, (uint32_t*)(base + prefix_flags_offset(n))};
}

// One call on buffers the device can address (the caller holds the lock); a call that ends early leaves the stream idle.  Statistics as in
// rr_render_adaptive_levels: behind every count's wait the stream is idle and the finished pass is collected (PassSums); the last level's
// pass is reported by the device when somebody asks, with the sums carried.
static int render_adaptive_prefix_locked(rr_scene* s, const rr_camera* cam, const rr_config* cfg, const uint16_t* sample_xy, const uint16_t* prefix_samples,
                                         uint32_t n_levels, float threshold, const FusedOut& o, hipStream_t st, const volatile int* cancel) {
    IdleOnExit idle(st);
    const uint32_t W = cam->width, H = cam->height, N = W * H;
    uint32_t level_pixels[RR_MAX_ADAPTIVE_LEVELS] = {N, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
    // every level's pass: two halves per entry, its samples added to accumulators nobody resolves but k_prefix_masks
    FrameIo io = pixels_io(nullptr, N, nullptr, nullptr);
    io.end = FrameEnd::NONE; io.lg_parts = 1u;
    // level 0: the whole frame over [0, P0); its sums stay in the frame's own accumulators, in the region's slot order
    io.samples_used = prefix_samples[0];
    RR_TRY(render_region_locked(s, cam, cfg, sample_xy, io, st, cancel));
    DAccum acc{s->frame.acc_rgb.as<long long>(), s->frame.acc_normal.as<long long>(), s->frame.acc_depth.as<long long>(), s->frame.acc_id.as<uint32_t>(), 2ull * N,
               s->frame.acc_flags.as<uint32_t>()};
    const uint32_t* xy = s->frame.pixel_xy.as<uint32_t>(); // the slot table: entry i at word 2 i
    uint32_t xy_stride = 2u, count = N;
    DevBuf* const lists[2] = {&s->adaptive.list, &s->adaptive.list2};
    PassSums sums{s};
    for (uint32_t l = 0;; l++) {
        const bool last = l + 1 == n_levels;
        const uint32_t nw = sublist_waves(count);
        ListScratch ls;
        RR_TRY(list_scratch(s, nw, &ls));
        {
            ScopedTimer t(s, st, TK_BINNING, false);
            hipLaunchKernelGGL(k_prefix_masks, dim3(ls.grid), dim3(RR_BLOCK), 0, st, acc, xy, xy_stride, count, (uint32_t)prefix_samples[l], threshold, W, (float4*)o.out, o.samples,
                               o.error, ls.masks, ls.counts);
            if (!last) hipLaunchKernelGGL(k_refine_scan, dim3(1), dim3(1024), 0, st, ls.counts, nw, ls.total);
        }
        if (hipGetLastError() != hipSuccess) return fail(RR_ERR_DEVICE, "rr_render_adaptive_prefix: a launch failed");
        if (last) {
            sums.carry(); // rr_scene_last_stats: the sums over all passes
            break;
        }
        uint32_t taken = 0;
        RR_TRY(await_list_count(s, ls.total, st, &taken));
        RR_TRY(collect_stats_locked(s)); // the stream is idle: what the pass cost, and the list's launches with it
        sums.add();
        if (taken > count) return fail(RR_ERR_DEVICE, "internal: %u of %u entries taken", taken, count);
        if (taken == 0u) break;
        if (cancel && *cancel) return fail(RR_ERR_CANCELLED, "cancelled");
        // the survivors: their pixels into the other list, their sums into the other set; both sets are sized by the FIRST list
        const uint32_t padded = refine_padded(taken);
        const uint64_t n_next = prefix_set_slots(taken);
        DevBuf& set = s->adaptive.acc_set[l & 1u];
        DevBuf& next_list = *lists[l & 1u]; // (level l + 1's; level l's own, if any, is the other one)
        HIP_TRY(set.reserve(prefix_set_bytes(n_next)));
        HIP_TRY(next_list.reserve(4ull * padded));
        const DAccum next = prefix_set_accum(set, n_next);
        {
            ScopedTimer t(s, st, TK_BINNING, false);
            hipLaunchKernelGGL(k_prefix_compact, dim3(ls.grid), dim3(RR_BLOCK), 0, st, acc, xy, xy_stride, count, ls.masks, ls.counts, ls.total, next_list.as<uint32_t>(), next);
        }
        if (hipGetLastError() != hipSuccess) return fail(RR_ERR_DEVICE, "rr_render_adaptive_prefix: a launch failed");
        // (the pass below starts its statistics from nothing: the compaction's timer is kept aside and counted with that pass)
        std::vector<TimedLaunch> held;
        held.swap(s->timing.timed);
        // level l + 1: the survivors' list, the library's own, over [Pl, P(l+1)) on the set as it is
        io.region = nullptr; io.pixel_xy = next_list.as<uint32_t>(); io.n_pixels = padded; io.own_list = true;
        io.samples_used = prefix_samples[l + 1]; io.samples_from = prefix_samples[l]; io.resident = &next;
        const int rc = render_region_locked(s, cam, cfg, sample_xy, io, st, cancel);
        s->timing.timed.insert(s->timing.timed.end(), held.begin(), held.end());
        RR_TRY(rc);
        acc = next; xy = next_list.as<uint32_t>(); xy_stride = 1u; count = taken;
        level_pixels[l + 1] = taken;
    }
    sums.close();
    return idle.done(finish_fused(s, "rr_render_adaptive_prefix", cfg, N, o, level_pixels, n_levels, st));
}

int rr_render_adaptive_prefix_device(rr_scene* s, const rr_camera* cam, const rr_config* cfg, const uint16_t* sample_xy, const uint16_t* prefix_samples,
                                     uint32_t n_levels, float threshold, rr_radiance* out, uint8_t* rgba8_out, uint16_t* samples_out, float* error_out,
                                     uint32_t* level_pixels_out, void* hip_stream, const volatile int* cancel) try {
    const FusedOut o{out, rgba8_out, samples_out, error_out, level_pixels_out};
    RR_TRY(check_adaptive_prefix_args("rr_render_adaptive_prefix_device", true, s, cam, cfg, sample_xy, prefix_samples, n_levels, threshold, o));
    return device_fused_call(s, "rr_render_adaptive_prefix_device", o, [&](const FusedOut& d) {
        return render_adaptive_prefix_locked(s, cam, cfg, sample_xy, prefix_samples, n_levels, threshold, d, (hipStream_t)hip_stream, cancel);
    });
} RR_GUARD_END("rr_render_adaptive_prefix_device")

int rr_render_adaptive_prefix(rr_scene* s, const rr_camera* cam, const rr_config* cfg, const uint16_t* sample_xy, const uint16_t* prefix_samples, uint32_t n_levels,
                              float threshold, rr_radiance* out, uint8_t* rgba8_out, uint16_t* samples_out, float* error_out, uint32_t* level_pixels_out,
                              const volatile int* cancel) try {
    const FusedOut o{out, rgba8_out, samples_out, error_out, level_pixels_out};
    RR_TRY(check_adaptive_prefix_args("rr_render_adaptive_prefix", false, s, cam, cfg, sample_xy, prefix_samples, n_levels, threshold, o));
    return host_fused_call(s, "rr_render_adaptive_prefix", cam, o, n_levels, [&](const FusedOut& d) {
        return render_adaptive_prefix_locked(s, cam, cfg, sample_xy, prefix_samples, n_levels, threshold, d, nullptr, cancel);
    });
} RR_GUARD_END("rr_render_adaptive_prefix")
