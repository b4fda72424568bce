// rr_api_levels.h — refine the noisy pixels of a frame level by level, on the device: the list made from a list (adaptive.refine_sublist
// of rustray_amd/adaptive.py) and a frame at up to RR_MAX_ADAPTIVE_LEVELS sample counts as ONE call under one hold of the scene's lock.
// Offers: rr_refine_sublist_device, rr_render_adaptive_levels, rr_render_adaptive_levels_device.
// Needs:  rr_api_adaptive.h (refine_list_locked, check_refine_frame), rr_api_parts.h (render_pixel_parts_locked: the whole frame and every
//         list in two parts), rr_api_query.h (check_query_pointers), rr_api_frame.h (check_frame_args, take_stream, ScopedTimer, add_pass_stats,
//         collect_stats_locked), rr_adaptive.h, kernels 5m, 5p and 5q .. 5s of rr_kernels.hip.
//
// The sublist is three launches (k_sublist_masks, k_refine_scan, k_sublist_scatter) and one wait, for the 4 bytes of its length.  The
// fused call is: the frame in parts at level_samples[0] (records straight into `out`) and its list as rr_render_adaptive makes it; then
// per level, while the list is not empty, the padded list in parts at the level's count, k_scatter_level, and -- unless the level is
// the last -- the sublist for the next one; k_record_bytes at the end.  The host form is the device form behind a staging copy in
// buffers of the handle.

// The sublist of `count` > 0 entries on stream st, into list_out (refine_padded(count) entries) and *count_out (host); the caller holds the
// lock and has taken the stream.  THE wait of the call: 4 bytes (pinned, h_count[10]).  With kernel_timing the three launches are timed as
// one re-ordering (rr_frame_stats::ms_binning).  Scratch: per 64 entries a mask and a count, then the total (12 B per wave + 4).
static int refine_sublist_locked(rr_scene* s, const uint32_t* list, uint32_t count, const rr_radiance* parts, float threshold, float* error_out,
                                 uint32_t* list_out, uint32_t* count_out, hipStream_t st) {
    const uint32_t nw = sublist_waves(count);
    HIP_TRY(s->adaptive.scratch.reserve(12ull * nw + 4u));
    unsigned long long* masks = s->adaptive.scratch.as<unsigned long long>();
    uint32_t* counts = (uint32_t*)(masks + nw);
    uint32_t* total = counts + nw;
    const int grid = (int)std::min<uint64_t>((nw + RR_BLOCK / RR_WAVE - 1) / (RR_BLOCK / RR_WAVE), (uint64_t)s->n_cus * 8u);
    {
        ScopedTimer t(s, st, TK_BINNING, false);
        hipLaunchKernelGGL(k_sublist_masks, dim3(grid), dim3(RR_BLOCK), 0, st, (const float4*)parts, count, threshold, error_out, masks, counts);
        hipLaunchKernelGGL(k_refine_scan, dim3(1), dim3(1024), 0, st, counts, nw, total);
        hipLaunchKernelGGL(k_sublist_scatter, dim3(grid), dim3(RR_BLOCK), 0, st, list, count, masks, counts, total, list_out);
    }
    HIP_TRY(hipGetLastError());
    uint32_t* h = s->frame.h_count + 10;
    HIP_TRY(hipMemcpyAsync(h, total, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    *count_out = *h;
    return RR_OK;
}

// (C linkage: the entry points of this layer are declared in include/rustray_hip.h, inside its extern "C" block, and a definition keeps the
// linkage of its declaration; tests/test_adaptive_levels_host.py holds each to the guard every entry point has)
int rr_refine_sublist_device(rr_scene* s, const uint32_t* list, uint32_t count, const rr_radiance* parts, float threshold, float* error_out,
                             uint32_t* list_out, uint32_t* count_out, void* hip_stream) try {
    if (!s || !count_out) return fail(RR_ERR_INVALID_ARGUMENT, "rr_refine_sublist_device: NULL argument");
    if (threshold != threshold) return fail(RR_ERR_INVALID_ARGUMENT, "rr_refine_sublist_device: threshold is NaN");
    if (count > (1u << 29)) return fail(RR_ERR_UNSUPPORTED, "rr_refine_sublist_device: a list of %u entries is longer than 2^29", count);
    if (count == 0) { *count_out = 0; return RR_OK; } // nothing is read, written or launched
    if (!list || !parts || !list_out)
        return fail(RR_ERR_INVALID_ARGUMENT, "rr_refine_sublist_device: %s is NULL", !list ? "list_dev" : !parts ? "parts_dev" : "list_out_dev");
    if (((uintptr_t)parts & 15u) || (((uintptr_t)list | (uintptr_t)error_out | (uintptr_t)list_out) & 3u))
        return fail(RR_ERR_INVALID_ARGUMENT, "rr_refine_sublist_device: parts_dev must be 16-byte aligned, list_dev, error_out_dev and list_out_dev 4-byte aligned");
    const uintptr_t in_a = (uintptr_t)list, in_b = in_a + 4ull * count, out_a = (uintptr_t)list_out, out_b = out_a + 4ull * refine_padded(count);
    if (in_a < out_b && out_a < in_b)
        return fail(RR_ERR_INVALID_ARGUMENT, "rr_refine_sublist_device: list_out_dev (%u entries) overlaps list_dev (%u entries)", refine_padded(count), count);
    RR_TRY(not_in_pass(s, "rr_refine_sublist_device"));
    std::lock_guard<std::mutex> lk(s->mu);
    HIP_TRY(hipSetDevice(s->device));
    RR_TRY(check_query_pointers(s, "rr_refine_sublist_device",
                                {{list, "list_dev"}, {parts, "parts_dev"}, {error_out, "error_out_dev"}, {list_out, "list_out_dev"}}));
    const hipStream_t st = (hipStream_t)hip_stream;
    RR_TRY(take_stream(s, st));
    const bool profiling = s->timing.profiling; // nothing of a frame's stats is touched: the launches are not timed here
    s->timing.profiling = false;
    const int rc = refine_sublist_locked(s, list, count, parts, threshold, error_out, list_out, count_out, st);
    s->timing.profiling = profiling;
    if (rc != RR_OK) (void)hipStreamSynchronize(st);
    return rc;
} RR_GUARD_END("rr_refine_sublist_device")

// what both forms check before the scene is looked at; `device`: the alignment rule of the device form
static int check_levels_args(const char* fn, bool device, const rr_scene* s, const rr_camera* cam, const rr_config* cfg, const uint16_t* level_samples, uint32_t n_levels,
                             float threshold, const uint16_t* const* tables, const rr_radiance* out, const uint8_t* rgba8, const uint16_t* samples_out,
                             const float* error_out) {
    if (!s || !cam || !cfg) return fail(RR_ERR_INVALID_ARGUMENT, "NULL argument");
    if (n_levels < 2u || n_levels > RR_MAX_ADAPTIVE_LEVELS)
        return fail(RR_ERR_INVALID_ARGUMENT, "%s: n_levels %u must be from 2 to %u", fn, n_levels, RR_MAX_ADAPTIVE_LEVELS);
    if (!level_samples) return fail(RR_ERR_INVALID_ARGUMENT, "%s: level_samples is NULL", fn);
    rr_config c = *cfg; // (config->samples is ignored)
    for (uint32_t l = 0; l < n_levels; l++) {
        const unsigned S = level_samples[l];
        if (S < 2u || (S & 1u))
            return fail(RR_ERR_INVALID_ARGUMENT, "%s: level_samples[%u] = %u must be even and at least 2: the two halves of a pixel must be equal", fn, l, S);
        if (l && S <= level_samples[l - 1])
            return fail(RR_ERR_INVALID_ARGUMENT, "%s: level_samples[%u] = %u is not above level_samples[%u] = %u: the counts must increase strictly", fn, l, S, l - 1,
                        (unsigned)level_samples[l - 1]);
        c.samples = level_samples[l];
        RR_TRY(check_frame_args(s, cam, &c, tables ? tables[l] : nullptr));
    }
    RR_TRY(check_refine_frame(fn, cam->width, cam->height, threshold));
    if (!out) return fail(RR_ERR_INVALID_ARGUMENT, "%s: out is required", fn);
    if (device && (((uintptr_t)out & 15u) || ((uintptr_t)samples_out & 1u) || (((uintptr_t)rgba8 | (uintptr_t)error_out) & 3u)))
        return fail(RR_ERR_INVALID_ARGUMENT, "%s: out_dev must be 16-byte aligned, rgba8_out_dev and error_out_dev 4-byte aligned and samples_out_dev 2-byte aligned", fn);
    return RR_OK;
}

// One call on buffers the device can address (the caller holds the lock); a call that ends early leaves the stream idle.  The stream is
// idle behind every list's wait: there the finished passes' statistics are collected into `sum`.  The last level has no list behind it,
// so its pass is reported by the device when somebody asks, with `sum` carried (FrameTiming::carry); the call returns without that wait.
static int render_adaptive_levels_locked(rr_scene* s, const rr_camera* cam, const rr_config* cfg, const uint16_t* level_samples, uint32_t n_levels, float threshold,
                                         const uint16_t* const* tables, rr_radiance* out, uint8_t* rgba8, uint16_t* samples_out, float* error_out,
                                         uint32_t* level_pixels_out, hipStream_t st, const volatile int* cancel) {
    const uint32_t W = cam->width, H = cam->height, N = W * H;
    const uint64_t cap = refine_capacity(W, H);
    HIP_TRY(s->adaptive.parts.reserve(64ull * cap)); // the frame's part records; then those of every list, none longer than `cap`
    HIP_TRY(s->adaptive.list.reserve(4ull * cap));
    rr_radiance* parts = s->adaptive.parts.as<rr_radiance>();
    uint32_t* lists[2] = {s->adaptive.list.as<uint32_t>(), nullptr};
    uint32_t level_pixels[RR_MAX_ADAPTIVE_LEVELS] = {N, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
    rr_config c = *cfg;
    c.samples = level_samples[0];
    RR_TRY(render_pixel_parts_locked(s, cam, &c, tables ? tables[0] : nullptr, nullptr, N, 1u, out, parts, st, cancel));
    uint32_t count = 0;
    int rc = RR_OK;
    if (samples_out && hipMemsetD16Async((hipDeviceptr_t)samples_out, level_samples[0], N, st) != hipSuccess) rc = fail(RR_ERR_DEVICE, "hipMemsetD16Async(samples_out) failed");
    if (rc == RR_OK) rc = refine_list_locked(s, W, H, parts, threshold, error_out, lists[0], &count, st);
    if (rc == RR_OK) rc = collect_stats_locked(s); // the stream is idle: what the pass cost, and the list's launches with it
    if (rc != RR_OK) { (void)hipStreamSynchronize(st); return rc; }
    rr_frame_stats sum = s->timing.stats;
    bool carried = false; // the last pass is still in flight and `sum` is its carry
    uint32_t cur = 0;
    for (uint32_t l = 1; l < n_levels && count; l++) {
        if (cancel && *cancel) return fail(RR_ERR_CANCELLED, "cancelled"); // (between levels the stream is idle)
        const uint32_t padded = refine_padded(count);
        HIP_TRY(s->adaptive.fine.reserve(32ull * padded));
        float4* fine = s->adaptive.fine.as<float4>();
        c.samples = level_samples[l];
        RR_TRY(render_pixel_parts_locked(s, cam, &c, tables ? tables[l] : nullptr, lists[cur], padded, 1u, (rr_radiance*)fine, parts, st, cancel));
        level_pixels[l] = count;
        const int grid = (int)std::min<uint64_t>((count + RR_BLOCK - 1) / RR_BLOCK, (uint64_t)s->n_cus * 8u);
        hipLaunchKernelGGL(k_scatter_level, dim3(grid), dim3(RR_BLOCK), 0, st, lists[cur], count, fine, (const float4*)parts, W, level_samples[l], (float4*)out, samples_out,
                           error_out);
        if (l + 1 == n_levels) {
            s->timing.carry = sum; s->timing.has_carry = true; // rr_scene_last_stats: the sums over all passes
            carried = true;
            break;
        }
        if (!lists[1]) { // the second list buffer: no list made from a list is longer than the first one made
            HIP_TRY(s->adaptive.list2.reserve(4ull * padded));
            lists[1] = s->adaptive.list2.as<uint32_t>();
        }
        rc = refine_sublist_locked(s, lists[cur], count, parts, threshold, nullptr, lists[cur ^ 1u], &count, st);
        if (rc == RR_OK) rc = collect_stats_locked(s);
        if (rc != RR_OK) { (void)hipStreamSynchronize(st); return rc; }
        add_pass_stats(&sum, s->timing.stats);
        cur ^= 1u;
    }
    if (!carried) { s->timing.stats = sum; s->timing.has_carry = false; s->timing.stats_final = true; }
    if (rgba8) {
        const int grid = (int)std::min<uint64_t>((N + RR_BLOCK - 1) / RR_BLOCK, (uint64_t)s->n_cus * 8u);
        hipLaunchKernelGGL(k_record_bytes, dim3(grid), dim3(RR_BLOCK), 0, st, (const float4*)out, N, cfg->gamma_correction ? 1u : 0u, (uint32_t*)rgba8);
    }
    if (hipGetLastError() != hipSuccess) { (void)hipStreamSynchronize(st); return fail(RR_ERR_DEVICE, "rr_render_adaptive_levels: a launch failed"); }
    if (level_pixels_out) memcpy(level_pixels_out, level_pixels, 4ull * n_levels);
    return RR_OK;
}

int rr_render_adaptive_levels_device(rr_scene* s, const rr_camera* cam, const rr_config* cfg, const uint16_t* level_samples, uint32_t n_levels, float threshold,
                                     const uint16_t* const* sample_xy_levels, rr_radiance* out, uint8_t* rgba8_out, uint16_t* samples_out, float* error_out,
                                     uint32_t* level_pixels_out, void* hip_stream, const volatile int* cancel) try {
    RR_TRY(check_levels_args("rr_render_adaptive_levels_device", true, s, cam, cfg, level_samples, n_levels, threshold, sample_xy_levels, out, rgba8_out, samples_out,
                             error_out));
    RR_TRY(not_in_pass(s, "rr_render_adaptive_levels_device"));
    std::lock_guard<std::mutex> lk(s->mu);
    RR_TRY(check_intact(s));
    HIP_TRY(hipSetDevice(s->device));
    RR_TRY(check_query_pointers(s, "rr_render_adaptive_levels_device",
                                {{out, "out_dev"}, {rgba8_out, "rgba8_out_dev"}, {samples_out, "samples_out_dev"}, {error_out, "error_out_dev"}}));
    return render_adaptive_levels_locked(s, cam, cfg, level_samples, n_levels, threshold, sample_xy_levels, out, rgba8_out, samples_out, error_out, level_pixels_out,
                                         (hipStream_t)hip_stream, cancel);
} RR_GUARD_END("rr_render_adaptive_levels_device")

int rr_render_adaptive_levels(rr_scene* s, const rr_camera* cam, const rr_config* cfg, const uint16_t* level_samples, uint32_t n_levels, float threshold,
                              const uint16_t* const* sample_xy_levels, rr_radiance* out, uint8_t* rgba8_out, uint16_t* samples_out, float* error_out,
                              uint32_t* level_pixels_out, const volatile int* cancel) try {
    RR_TRY(check_levels_args("rr_render_adaptive_levels", false, s, cam, cfg, level_samples, n_levels, threshold, sample_xy_levels, out, rgba8_out, samples_out, error_out));
    RR_TRY(not_in_pass(s, "rr_render_adaptive_levels"));
    std::lock_guard<std::mutex> lk(s->mu);
    RR_TRY(check_intact(s));
    HIP_TRY(hipSetDevice(s->device));
    // the staging is the handle's, where rr_render_adaptive stages its own (s->frame.tmp_out: grown, kept, used by host forms only)
    const size_t n = (size_t)cam->width * cam->height;
    DevBuf &d_rgba = s->frame.tmp_out[0], &d_out = s->frame.tmp_out[1], &d_samples = s->frame.tmp_out[2], &d_error = s->frame.tmp_out[3];
    HIP_TRY(d_out.reserve(32ull * n));
    if (rgba8_out) HIP_TRY(d_rgba.reserve(4ull * n));
    if (samples_out) HIP_TRY(d_samples.reserve(2ull * n));
    if (error_out) HIP_TRY(d_error.reserve(4ull * n));
    uint32_t level_pixels[RR_MAX_ADAPTIVE_LEVELS] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u}; // (the caller's words are written by a finished call only)
    RR_TRY(render_adaptive_levels_locked(s, cam, cfg, level_samples, n_levels, threshold, sample_xy_levels, d_out.as<rr_radiance>(),
                                         rgba8_out ? d_rgba.as<uint8_t>() : nullptr, samples_out ? d_samples.as<uint16_t>() : nullptr,
                                         error_out ? d_error.as<float>() : nullptr, level_pixels, nullptr, cancel));
    if (rgba8_out) HIP_TRY(hipMemcpyAsync(rgba8_out, d_rgba.p, 4ull * n, hipMemcpyDeviceToHost, nullptr));
    if (samples_out) HIP_TRY(hipMemcpyAsync(samples_out, d_samples.p, 2ull * n, hipMemcpyDeviceToHost, nullptr));
    if (error_out) HIP_TRY(hipMemcpyAsync(error_out, d_error.p, 4ull * n, hipMemcpyDeviceToHost, nullptr));
    HIP_TRY(hipMemcpy(out, d_out.p, 32ull * n, hipMemcpyDeviceToHost)); // waits for the launches: the outputs are written by a finished call only
    HIP_TRY(hipStreamSynchronize(nullptr));
    if (level_pixels_out) memcpy(level_pixels_out, level_pixels, 4ull * n_levels);
    return RR_OK;
} RR_GUARD_END("rr_render_adaptive_levels")
