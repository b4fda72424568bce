// rr_api_prefix.h — the first samples of a frame as records, and a frame refined level by level whose pixels KEEP their samples: every
// level is a prefix of ONE frame of config->samples samples, and a pixel that climbs is given only the samples it does not have yet.
// Offers: rr_render_pixel_prefix, rr_render_pixel_prefix_device, rr_render_adaptive_prefix, rr_render_adaptive_prefix_device.
// Needs:  rr_api_frame.h (FrameIo: samples_used, samples_from, resident, own_list, no_resolve; render_region_locked, ScopedTimer,
//         add_pass_stats, collect_stats_locked), rr_api_query.h (check_pixels_args, WHOLE_FRAME, check_query_pointers), rr_api_adaptive.h
//         (check_refine_frame), rr_adaptive.h (the sets of resident accumulators), kernels 5m, 5p, 5t and 5u of rr_kernels.hip.
//
// The prefix is the frame driver with its batch loop ending at samples_used / K * slots and its resolve dividing by samples_used.  The
// fused call is: the whole frame in two halves over [0, P0) WITHOUT a resolve; then per level k_prefix_masks (records, error and refine
// masks straight from the integer sums), k_refine_scan, the wait for the 4 bytes of the count, k_prefix_compact (the survivors' pixels
// into the next list, their sums into the next set) and the frame driver over that list for samples [P(l-1), Pl) on the set as it is;
// k_record_bytes at the end.  The host forms are the device forms behind a staging copy in buffers of the handle.

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
    // (k_resolve_pixel_parts has no byte output: with halves the bytes come from the finished records, as rr_render_adaptive makes its own)
    int rc = render_region_locked(s, cam, cfg, sample_xy,
                                  FrameIo{pixel_xy ? nullptr : &WHOLE_FRAME, pixel_xy, n_pixels, nullptr, false, nullptr, out, halves ? nullptr : rgba8, halves ? 1u : 0u,
                                          halves, samples_used, 0u, nullptr, false, false},
                                  st, cancel);
    if (rc == RR_OK && halves && rgba8) {
        const int grid = (int)std::min<uint64_t>((n_pixels + RR_BLOCK - 1) / RR_BLOCK, (uint64_t)s->n_cus * 8u);
        hipLaunchKernelGGL(k_record_bytes, dim3(grid), dim3(RR_BLOCK), 0, st, (const float4*)out, n_pixels, cfg->gamma_correction ? 1u : 0u, (uint32_t*)rgba8);
        if (hipGetLastError() != hipSuccess) rc = fail(RR_ERR_DEVICE, "rr_render_pixel_prefix: a launch failed");
    }
    if (rc != RR_OK) (void)hipStreamSynchronize(st);
    return rc;
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
    if (pixel_xy) { // (the body refuses the same entries; here the refusal costs no upload)
        const uint32_t bad = pixel_list_first_bad(pixel_xy, n_pixels, cam->width, cam->height);
        if (bad != RR_PIXEL_LIST_OK)
            return fail(RR_ERR_INVALID_ARGUMENT, "pixel_xy[%u] = (%u, %u) lies outside the frame of %ux%u pixels", bad, pixel_xy[bad] & 0xffffu, pixel_xy[bad] >> 16,
                        cam->width, cam->height);
    }
    RR_TRY(not_in_pass(s, "rr_render_pixel_prefix"));
    std::lock_guard<std::mutex> lk(s->mu);
    RR_TRY(check_intact(s));
    HIP_TRY(hipSetDevice(s->device));
    // the staging is the handle's, where rr_render_pixels and rr_render_pixel_parts stage their own: no allocation per call
    DevBuf &d_rgba = s->frame.tmp_out[0], &d_out = s->frame.tmp_out[1], &d_list = s->frame.tmp_out[2], &d_halves = s->frame.tmp_parts;
    if (pixel_xy) {
        HIP_TRY(d_list.reserve(4ull * n_pixels));
        HIP_TRY(hipMemcpy(d_list.p, pixel_xy, 4ull * n_pixels, hipMemcpyHostToDevice));
    }
    HIP_TRY(d_out.reserve(32ull * n_pixels));
    if (halves_out) HIP_TRY(d_halves.reserve(64ull * n_pixels));
    if (rgba8_out) HIP_TRY(d_rgba.reserve(4ull * n_pixels));
    RR_TRY(render_pixel_prefix_locked(s, cam, cfg, sample_xy, pixel_xy ? d_list.as<uint32_t>() : nullptr, n_pixels, samples_used, d_out.as<rr_radiance>(),
                                      halves_out ? d_halves.as<rr_radiance>() : nullptr, rgba8_out ? d_rgba.as<uint8_t>() : nullptr, nullptr, cancel));
    if (halves_out) HIP_TRY(hipMemcpyAsync(halves_out, d_halves.p, 64ull * n_pixels, hipMemcpyDeviceToHost, nullptr));
    if (rgba8_out) HIP_TRY(hipMemcpyAsync(rgba8_out, d_rgba.p, 4ull * n_pixels, hipMemcpyDeviceToHost, nullptr));
    HIP_TRY(hipMemcpy(out, d_out.p, 32ull * n_pixels, hipMemcpyDeviceToHost)); // waits for the launches: the outputs are written by a finished call only
    HIP_TRY(hipStreamSynchronize(nullptr));
    return RR_OK;
} RR_GUARD_END("rr_render_pixel_prefix")

// ---- the fused ladder

// what both forms check before the scene is looked at; `device`: the alignment rule of the device form
static int check_adaptive_prefix_args(const char* fn, bool device, const rr_scene* s, const rr_camera* cam, const rr_config* cfg, const uint16_t* sample_xy,
                                      const uint16_t* prefix_samples, uint32_t n_levels, float threshold, const rr_radiance* out, const uint8_t* rgba8,
                                      const uint16_t* samples_out, const float* error_out) {
    RR_TRY(check_frame_args(s, cam, cfg, sample_xy));
    if (n_levels < 2u || n_levels > RR_MAX_ADAPTIVE_LEVELS)
        return fail(RR_ERR_INVALID_ARGUMENT, "%s: n_levels %u must be from 2 to %u", fn, n_levels, RR_MAX_ADAPTIVE_LEVELS);
    if (!prefix_samples) return fail(RR_ERR_INVALID_ARGUMENT, "%s: prefix_samples is NULL", fn);
    for (uint32_t l = 0; l < n_levels; l++) {
        const unsigned P = prefix_samples[l];
        if (P < 2u || (P & 1u))
            return fail(RR_ERR_INVALID_ARGUMENT, "%s: prefix_samples[%u] = %u must be even and at least 2: the two halves of a pixel must be equal", fn, l, P);
        if (l && P <= prefix_samples[l - 1])
            return fail(RR_ERR_INVALID_ARGUMENT, "%s: prefix_samples[%u] = %u is not above prefix_samples[%u] = %u: the prefixes must increase strictly", fn, l, P, l - 1,
                        (unsigned)prefix_samples[l - 1]);
    }
    if (prefix_samples[n_levels - 1] != cfg->samples)
        return fail(RR_ERR_INVALID_ARGUMENT, "%s: prefix_samples[%u] = %u is not samples %u: the last prefix must be the whole frame", fn, n_levels - 1,
                    (unsigned)prefix_samples[n_levels - 1], (unsigned)cfg->samples);
    RR_TRY(check_refine_frame(fn, cam->width, cam->height, threshold));
    if (!out) return fail(RR_ERR_INVALID_ARGUMENT, "%s: out is required", fn);
    if (device && (((uintptr_t)out & 15u) || ((uintptr_t)samples_out & 1u) || (((uintptr_t)rgba8 | (uintptr_t)error_out) & 3u)))
        return fail(RR_ERR_INVALID_ARGUMENT, "%s: out_dev must be 16-byte aligned, rgba8_out_dev and error_out_dev 4-byte aligned and samples_out_dev 2-byte aligned", fn);
    return RR_OK;
}

// a set of n slots at `base` as the accumulators of a pass (rr_adaptive.h: the layout)
static DAccum prefix_set_accum(const DevBuf& b, uint64_t n) {
    char* base = (char*)b.p;
    return DAccum{(long long*)(base + prefix_plane_offset(0u, n)), (long long*)(base + prefix_plane_offset(3u, n)), (long long*)(base + prefix_plane_offset(6u, n)),
                  (uint32_t*)(base + prefix_id_offset(n)), (unsigned long long)n, (uint32_t*)(base + prefix_flags_offset(n))};
}

// One call on buffers the device can address (the caller holds the lock); a call that ends early leaves the stream idle.  Statistics as in
// rr_render_adaptive_levels: behind every count's wait the stream is idle and the finished pass is collected into `sum`; the last level's
// pass is reported by the device when somebody asks, with `sum` carried.
static int render_adaptive_prefix_locked(rr_scene* s, const rr_camera* cam, const rr_config* cfg, const uint16_t* sample_xy, const uint16_t* prefix_samples,
                                         uint32_t n_levels, float threshold, rr_radiance* out, uint8_t* rgba8, uint16_t* samples_out, float* error_out,
                                         uint32_t* level_pixels_out, hipStream_t st, const volatile int* cancel) {
    const uint32_t W = cam->width, H = cam->height, N = W * H;
    uint32_t level_pixels[RR_MAX_ADAPTIVE_LEVELS] = {N, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
    // level 0: the whole frame in two halves over [0, P0); its sums stay in the frame's own accumulators, in the region's slot order
    int rc = render_region_locked(s, cam, cfg, sample_xy,
                                  FrameIo{&WHOLE_FRAME, nullptr, N, nullptr, false, nullptr, out, nullptr, 1u, nullptr, prefix_samples[0], 0u, nullptr, false, true}, st,
                                  cancel);
    if (rc != RR_OK) { (void)hipStreamSynchronize(st); return rc; }
    DAccum acc{s->frame.acc_rgb.as<long long>(), s->frame.acc_normal.as<long long>(), s->frame.acc_depth.as<long long>(), s->frame.acc_id.as<uint32_t>(), 2ull * N,
               s->frame.acc_flags.as<uint32_t>()};
    const uint32_t* xy = s->frame.pixel_xy.as<uint32_t>(); // the slot table: entry i at word 2 i
    uint32_t xy_stride = 2u, count = N;
    DevBuf* const lists[2] = {&s->adaptive.list, &s->adaptive.list2};
    rr_frame_stats sum{};
    bool carried = false;
    for (uint32_t l = 0;; l++) {
        const bool last = l + 1 == n_levels;
        const uint32_t nw = sublist_waves(count);
        HIP_TRY(s->adaptive.scratch.reserve(12ull * nw + 4u));
        unsigned long long* masks = s->adaptive.scratch.as<unsigned long long>();
        uint32_t* counts = (uint32_t*)(masks + nw);
        uint32_t* total = counts + nw;
        const int grid = (int)std::min<uint64_t>((nw + RR_BLOCK / RR_WAVE - 1) / (RR_BLOCK / RR_WAVE), (uint64_t)s->n_cus * 8u);
        {
            ScopedTimer t(s, st, TK_BINNING, false);
            hipLaunchKernelGGL(k_prefix_masks, dim3(grid), dim3(RR_BLOCK), 0, st, acc, xy, xy_stride, count, (uint32_t)prefix_samples[l], threshold, W, (float4*)out, samples_out,
                               error_out, masks, counts);
            if (!last) hipLaunchKernelGGL(k_refine_scan, dim3(1), dim3(1024), 0, st, counts, nw, total);
        }
        if (hipGetLastError() != hipSuccess) { (void)hipStreamSynchronize(st); return fail(RR_ERR_DEVICE, "rr_render_adaptive_prefix: a launch failed"); }
        if (last) {
            s->timing.carry = sum; s->timing.has_carry = true; // rr_scene_last_stats: the sums over all passes
            carried = true;
            break;
        }
        uint32_t* h = s->frame.h_count + 11;
        rc = hipMemcpyAsync(h, total, 4, hipMemcpyDeviceToHost, st) == hipSuccess && hipStreamSynchronize(st) == hipSuccess ? RR_OK : fail(RR_ERR_DEVICE, "rr_render_adaptive_prefix: the count's copy failed");
        if (rc == RR_OK) rc = collect_stats_locked(s); // the stream is idle: what the pass cost, and the list's launches with it
        if (rc != RR_OK) { (void)hipStreamSynchronize(st); return rc; }
        if (l == 0) sum = s->timing.stats; else add_pass_stats(&sum, s->timing.stats);
        const uint32_t taken = *h;
        if (taken > count) return fail(RR_ERR_DEVICE, "internal: %u of %u entries taken", taken, count);
        if (taken == 0u) break;
        if (cancel && *cancel) return fail(RR_ERR_CANCELLED, "cancelled"); // (between levels the stream is idle)
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
            hipLaunchKernelGGL(k_prefix_compact, dim3(grid), dim3(RR_BLOCK), 0, st, acc, xy, xy_stride, count, masks, counts, total, next_list.as<uint32_t>(), next);
        }
        if (hipGetLastError() != hipSuccess) { (void)hipStreamSynchronize(st); return fail(RR_ERR_DEVICE, "rr_render_adaptive_prefix: a launch failed"); }
        // (the pass below starts its statistics from nothing: the compaction's timer is kept aside and counted with that pass)
        std::vector<TimedLaunch> held;
        held.swap(s->timing.timed);
        rc = render_region_locked(s, cam, cfg, sample_xy,
                                  FrameIo{nullptr, next_list.as<uint32_t>(), padded, nullptr, false, nullptr, out, nullptr, 1u, nullptr, prefix_samples[l + 1], prefix_samples[l],
                                          &next, true, true},
                                  st, cancel);
        s->timing.timed.insert(s->timing.timed.end(), held.begin(), held.end());
        if (rc != RR_OK) { (void)hipStreamSynchronize(st); return rc; }
        acc = next; xy = next_list.as<uint32_t>(); xy_stride = 1u; count = taken;
        level_pixels[l + 1] = taken;
    }
    if (!carried) { s->timing.stats = sum; s->timing.has_carry = false; s->timing.stats_final = true; }
    if (rgba8) {
        const int grid = (int)std::min<uint64_t>((N + RR_BLOCK - 1) / RR_BLOCK, (uint64_t)s->n_cus * 8u);
        hipLaunchKernelGGL(k_record_bytes, dim3(grid), dim3(RR_BLOCK), 0, st, (const float4*)out, N, cfg->gamma_correction ? 1u : 0u, (uint32_t*)rgba8);
    }
    if (hipGetLastError() != hipSuccess) { (void)hipStreamSynchronize(st); return fail(RR_ERR_DEVICE, "rr_render_adaptive_prefix: a launch failed"); }
    if (level_pixels_out) memcpy(level_pixels_out, level_pixels, 4ull * n_levels);
    return RR_OK;
}

int rr_render_adaptive_prefix_device(rr_scene* s, const rr_camera* cam, const rr_config* cfg, const uint16_t* sample_xy, const uint16_t* prefix_samples,
                                     uint32_t n_levels, float threshold, rr_radiance* out, uint8_t* rgba8_out, uint16_t* samples_out, float* error_out,
                                     uint32_t* level_pixels_out, void* hip_stream, const volatile int* cancel) try {
    RR_TRY(check_adaptive_prefix_args("rr_render_adaptive_prefix_device", true, s, cam, cfg, sample_xy, prefix_samples, n_levels, threshold, out, rgba8_out, samples_out,
                                      error_out));
    RR_TRY(not_in_pass(s, "rr_render_adaptive_prefix_device"));
    std::lock_guard<std::mutex> lk(s->mu);
    RR_TRY(check_intact(s));
    HIP_TRY(hipSetDevice(s->device));
    RR_TRY(check_query_pointers(s, "rr_render_adaptive_prefix_device",
                                {{out, "out_dev"}, {rgba8_out, "rgba8_out_dev"}, {samples_out, "samples_out_dev"}, {error_out, "error_out_dev"}}));
    return render_adaptive_prefix_locked(s, cam, cfg, sample_xy, prefix_samples, n_levels, threshold, out, rgba8_out, samples_out, error_out, level_pixels_out,
                                         (hipStream_t)hip_stream, cancel);
} RR_GUARD_END("rr_render_adaptive_prefix_device")

int rr_render_adaptive_prefix(rr_scene* s, const rr_camera* cam, const rr_config* cfg, const uint16_t* sample_xy, const uint16_t* prefix_samples, uint32_t n_levels,
                              float threshold, rr_radiance* out, uint8_t* rgba8_out, uint16_t* samples_out, float* error_out, uint32_t* level_pixels_out,
                              const volatile int* cancel) try {
    RR_TRY(check_adaptive_prefix_args("rr_render_adaptive_prefix", false, s, cam, cfg, sample_xy, prefix_samples, n_levels, threshold, out, rgba8_out, samples_out,
                                      error_out));
    RR_TRY(not_in_pass(s, "rr_render_adaptive_prefix"));
    std::lock_guard<std::mutex> lk(s->mu);
    RR_TRY(check_intact(s));
    HIP_TRY(hipSetDevice(s->device));
    // the staging is the handle's, where rr_render_adaptive_levels stages its own (s->frame.tmp_out: grown, kept, used by host forms only)
    const size_t n = (size_t)cam->width * cam->height;
    DevBuf &d_rgba = s->frame.tmp_out[0], &d_out = s->frame.tmp_out[1], &d_samples = s->frame.tmp_out[2], &d_error = s->frame.tmp_out[3];
    HIP_TRY(d_out.reserve(32ull * n));
    if (rgba8_out) HIP_TRY(d_rgba.reserve(4ull * n));
    if (samples_out) HIP_TRY(d_samples.reserve(2ull * n));
    if (error_out) HIP_TRY(d_error.reserve(4ull * n));
    uint32_t level_pixels[RR_MAX_ADAPTIVE_LEVELS] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u}; // (the caller's words are written by a finished call only)
    RR_TRY(render_adaptive_prefix_locked(s, cam, cfg, sample_xy, prefix_samples, n_levels, threshold, d_out.as<rr_radiance>(), rgba8_out ? d_rgba.as<uint8_t>() : nullptr,
                                         samples_out ? d_samples.as<uint16_t>() : nullptr, error_out ? d_error.as<float>() : nullptr, level_pixels, nullptr, cancel));
    if (rgba8_out) HIP_TRY(hipMemcpyAsync(rgba8_out, d_rgba.p, 4ull * n, hipMemcpyDeviceToHost, nullptr));
    if (samples_out) HIP_TRY(hipMemcpyAsync(samples_out, d_samples.p, 2ull * n, hipMemcpyDeviceToHost, nullptr));
    if (error_out) HIP_TRY(hipMemcpyAsync(error_out, d_error.p, 4ull * n, hipMemcpyDeviceToHost, nullptr));
    HIP_TRY(hipMemcpy(out, d_out.p, 32ull * n, hipMemcpyDeviceToHost)); // waits for the launches: the outputs are written by a finished call only
    HIP_TRY(hipStreamSynchronize(nullptr));
    if (level_pixels_out) memcpy(level_pixels_out, level_pixels, 4ull * n_levels);
    return RR_OK;
} RR_GUARD_END("rr_render_adaptive_prefix")
