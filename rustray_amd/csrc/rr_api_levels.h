// rr_api_levels.h — refine the noisy pixels of a frame level by level, on the device: the list made from a list (adaptive.refine_sublist
// of rustray_amd/adaptive.py) and a frame at up to RR_MAX_ADAPTIVE_LEVELS sample counts as ONE call under one hold of the scene's lock.
// Offers: rr_refine_sublist_device, rr_render_adaptive_levels, rr_render_adaptive_levels_device.
//         For rr_api_prefix.h: check_ladder.
// Needs:  rr_api_adaptive.h (refine_list_locked, compact_list_locked; FusedOut, check_fused_outputs, device_fused_call,
//         host_fused_call, finish_fused), rr_api_parts.h (render_pixel_parts_locked: the whole frame and every list in two parts),
//         rr_api_query.h (check_query_pointers), rr_api_frame.h (check_frame_args, take_stream, IdleOnExit, PassSums,
//         collect_stats_locked), rr_adaptive.h (ListSource, ladder_fault), kernels 5l .. 5p of rr_kernels.hip.
//
// The sublist is the list of rr_api_adaptive.h over a ListSource (k_refine_masks, k_refine_scan, k_refine_scatter and one wait).  The
// fused call is: the frame in parts at level_samples[0] (records straight into `out`) and its list as rr_render_adaptive makes it; then
// per level, while the list is not empty, the padded list in parts at the level's count, k_scatter_level, and -- unless the level is
// the last -- the sublist for the next one; k_record_bytes at the end.  The host form is the device form behind the staging copy of
// every fused call (host_fused_call, rr_api_adaptive.h).

// The sublist of `count` > 0 entries on stream st, into list_out (refine_padded(count) entries) and *count_out (host); the caller holds the
// lock and has taken the stream.  With kernel_timing the three launches are timed as one re-ordering (rr_frame_stats::ms_binning).
// Scratch: per 64 entries a mask and a count, then the total (list_scratch over the list's waves).
static int refine_sublist_locked(rr_scene* s, const uint32_t* list, uint32_t count, const rr_radiance* parts, float threshold, float* error_out,
                                 uint32_t* list_out, uint32_t* count_out, hipStream_t st) {
    return compact_list_locked(s, ListSource{list, count}, parts, threshold, error_out, list_out, count_out, st);
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
    IdleOnExit idle(st);
    const bool profiling = s->timing.profiling; // nothing of a frame's stats is touched: the launches are not timed here
    s->timing.profiling = false;
    const int rc = refine_sublist_locked(s, list, count, parts, threshold, error_out, list_out, count_out, st);
    s->timing.profiling = profiling;
    return idle.done(rc);
} RR_GUARD_END("rr_refine_sublist_device")

// THE ladder rule of the calls that refine level by level (rr_adaptive.h: ladder_fault), as their refusals: `array` is the ladder's name
// (level_samples, prefix_samples) and `noun` what its entries are (counts, prefixes).  Faults are reported in the ladder's order:
// per_level(l) -- this call's own check of level l, or nothing -- runs for the levels before the first entry that breaks the rule.
template <class PerLevel>
static int check_ladder(const char* fn, const char* array, const char* noun, const uint16_t* ladder, uint32_t n_levels, PerLevel per_level) {
    unsigned int at = 0;
    const LadderFault f = ladder_fault(ladder, n_levels, RR_MAX_ADAPTIVE_LEVELS, &at);
    if (f == LADDER_LEVELS) return fail(RR_ERR_INVALID_ARGUMENT, "%s: n_levels %u must be from 2 to %u", fn, n_levels, RR_MAX_ADAPTIVE_LEVELS);
    if (f == LADDER_NULL) return fail(RR_ERR_INVALID_ARGUMENT, "%s: %s is NULL", fn, array);
    for (uint32_t l = 0; l < (f == LADDER_OK ? n_levels : at); l++) RR_TRY(per_level(l));
    if (f == LADDER_ENTRY)
        return fail(RR_ERR_INVALID_ARGUMENT, "%s: %s[%u] = %u must be even and at least 2: the two halves of a pixel must be equal", fn, array, at, (unsigned)ladder[at]);
    if (f == LADDER_ORDER)
        return fail(RR_ERR_INVALID_ARGUMENT, "%s: %s[%u] = %u is not above %s[%u] = %u: the %s must increase strictly", fn, array, at, (unsigned)ladder[at], array, at - 1,
                    (unsigned)ladder[at - 1], noun);
    return RR_OK;
}

// what both forms check before the scene is looked at
static int check_levels_args(const char* fn, bool device, const rr_scene* s, const rr_camera* cam, const rr_config* cfg, const uint16_t* level_samples, uint32_t n_levels,
                             float threshold, const uint16_t* const* tables, const FusedOut& o) {
    if (!s || !cam || !cfg) return fail(RR_ERR_INVALID_ARGUMENT, "NULL argument");
    RR_TRY(check_ladder(fn, "level_samples", "counts", level_samples, n_levels, [&](uint32_t l) {
        rr_config c = *cfg; // (config->samples is ignored)
        c.samples = level_samples[l];
        return check_frame_args(s, cam, &c, tables ? tables[l] : nullptr);
    }));
    return check_fused_outputs(fn, device, cam, threshold, o);
}

// One call on buffers the device can address (the caller holds the lock); a call that ends early leaves the stream idle.  The stream is
// idle behind every list's wait: there the finished passes' statistics are collected (PassSums).  The last level has no list behind it,
// so its pass is reported by the device when somebody asks, with the sums carried; the call returns without that wait.
static int render_adaptive_levels_locked(rr_scene* s, const rr_camera* cam, const rr_config* cfg, const uint16_t* level_samples, uint32_t n_levels, float threshold,
                                         const uint16_t* const* tables, const FusedOut& o, hipStream_t st, const volatile int* cancel) {
    IdleOnExit idle(st);
    const uint32_t W = cam->width, H = cam->height, N = W * H;
    const uint64_t cap = refine_capacity(W, H);
    HIP_TRY(s->adaptive.parts.reserve(64ull * cap)); // the frame's part records; then those of every list, none longer than `cap`
    HIP_TRY(s->adaptive.list.reserve(4ull * cap));
    rr_radiance* parts = s->adaptive.parts.as<rr_radiance>();
    uint32_t* lists[2] = {s->adaptive.list.as<uint32_t>(), nullptr};
    uint32_t level_pixels[RR_MAX_ADAPTIVE_LEVELS] = {N, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
    rr_config c = *cfg;
    c.samples = level_samples[0];
    RR_TRY(render_pixel_parts_locked(s, cam, &c, tables ? tables[0] : nullptr, nullptr, N, 1u, o.out, parts, st, cancel));
    uint32_t count = 0;
    if (o.samples && hipMemsetD16Async((hipDeviceptr_t)o.samples, level_samples[0], N, st) != hipSuccess) return fail(RR_ERR_DEVICE, "hipMemsetD16Async(samples_out) failed");
    RR_TRY(refine_list_locked(s, W, H, parts, threshold, o.error, lists[0], &count, st));
    RR_TRY(collect_stats_locked(s)); // the stream is idle: what the pass cost, and the list's launches with it
    PassSums sums{s};
    sums.add();
    uint32_t cur = 0;
    for (uint32_t l = 1; l < n_levels && count; l++) {
        if (cancel && *cancel) return fail(RR_ERR_CANCELLED, "cancelled");
        const uint32_t padded = refine_padded(count);
        HIP_TRY(s->adaptive.fine.reserve(32ull * padded));
        float4* fine = s->adaptive.fine.as<float4>();
        c.samples = level_samples[l];
        RR_TRY(render_pixel_parts_locked(s, cam, &c, tables ? tables[l] : nullptr, lists[cur], padded, 1u, (rr_radiance*)fine, parts, st, cancel));
        level_pixels[l] = count;
        const int grid = (int)std::min<uint64_t>((count + RR_BLOCK - 1) / RR_BLOCK, (uint64_t)s->n_cus * 8u);
        hipLaunchKernelGGL(k_scatter_level, dim3(grid), dim3(RR_BLOCK), 0, st, lists[cur], count, fine, (const float4*)parts, W, level_samples[l], (float4*)o.out, o.samples,
                           o.error);
        if (l + 1 == n_levels) {
            sums.carry(); // rr_scene_last_stats: the sums over all passes
            break;
        }
        if (!lists[1]) { // the second list buffer: no list made from a list is longer than the first one made
            HIP_TRY(s->adaptive.list2.reserve(4ull * padded));
            lists[1] = s->adaptive.list2.as<uint32_t>();
        }
        RR_TRY(refine_sublist_locked(s, lists[cur], count, parts, threshold, nullptr, lists[cur ^ 1u], &count, st));
        RR_TRY(collect_stats_locked(s));
        sums.add();
        cur ^= 1u;
    }
    sums.close();
    return idle.done(finish_fused(s, "rr_render_adaptive_levels", cfg, N, o, level_pixels, n_levels, st));
}

int rr_render_adaptive_levels_device(rr_scene* s, const rr_camera* cam, const rr_config* cfg, const uint16_t* level_samples, uint32_t n_levels, float threshold,
                                     const uint16_t* const* sample_xy_levels, rr_radiance* out, uint8_t* rgba8_out, uint16_t* samples_out, float* error_out,
                                     uint32_t* level_pixels_out, void* hip_stream, const volatile int* cancel) try {
    const FusedOut o{out, rgba8_out, samples_out, error_out, level_pixels_out};
    RR_TRY(check_levels_args("rr_render_adaptive_levels_device", true, s, cam, cfg, level_samples, n_levels, threshold, sample_xy_levels, o));
    return device_fused_call(s, "rr_render_adaptive_levels_device", o, [&](const FusedOut& d) {
        return render_adaptive_levels_locked(s, cam, cfg, level_samples, n_levels, threshold, sample_xy_levels, d, (hipStream_t)hip_stream, cancel);
    });
} RR_GUARD_END("rr_render_adaptive_levels_device")

int rr_render_adaptive_levels(rr_scene* s, const rr_camera* cam, const rr_config* cfg, const uint16_t* level_samples, uint32_t n_levels, float threshold,
                              const uint16_t* const* sample_xy_levels, rr_radiance* out, uint8_t* rgba8_out, uint16_t* samples_out, float* error_out,
                              uint32_t* level_pixels_out, const volatile int* cancel) try {
    const FusedOut o{out, rgba8_out, samples_out, error_out, level_pixels_out};
    RR_TRY(check_levels_args("rr_render_adaptive_levels", false, s, cam, cfg, level_samples, n_levels, threshold, sample_xy_levels, o));
    return host_fused_call(s, "rr_render_adaptive_levels", cam, o, n_levels, [&](const FusedOut& d) {
        return render_adaptive_levels_locked(s, cam, cfg, level_samples, n_levels, threshold, sample_xy_levels, d, nullptr, cancel);
    });
} RR_GUARD_END("rr_render_adaptive_levels")
