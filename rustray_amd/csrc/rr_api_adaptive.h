// rr_api_adaptive.h — find the noisy pixels of a frame and refine them, on the device: the list of rustray_amd/adaptive.py (half_error,
// refine_list) from part records that already lie there, and a frame at two sample counts as ONE call under one hold of the scene's lock.
// Offers: rr_refine_list_capacity, rr_refine_list_device, rr_render_adaptive, rr_render_adaptive_device; for the fused calls of the layers
//         behind it: check_refine_frame; ListScratch, list_scratch, await_list_count; compact_list_locked, refine_list_locked; FusedOut,
//         check_fused_outputs, device_fused_call, host_fused_call, launch_record_bytes, finish_fused.
// Needs:  rr_api_parts.h (render_pixel_parts_locked: the whole frame in parts), rr_api_query.h (render_pixels_locked, check_query_pointers),
//         rr_api_frame.h (check_frame_args, take_stream, ScopedTimer, IdleOnExit, PassSums, collect_stats_locked), rr_adaptive.h (FrameSource),
//         kernels 5l .. 5p of rr_kernels.hip.
//
// A list is three launches (k_refine_masks, k_refine_scan, k_refine_scatter over the list's entry source) and one wait, for the 4 bytes of
// its length.  The fused call is: the frame in parts at base_samples (records straight into `out`), the list, that wait, the padded list
// through the body of rr_render_pixels at max_samples, k_scatter_level without an error, k_record_bytes.  The host form is the device form
// behind the staging copy of every fused call (host_fused_call).

// width x height as a frame whose two part records per pixel fit the accumulator slots of a call
static int check_refine_frame(const char* fn, uint32_t width, uint32_t height, float threshold) {
    if (width == 0 || height == 0 || width > 65535u || height > 65535u) return fail(RR_ERR_INVALID_ARGUMENT, "%s: bad frame size %ux%u", fn, width, height);
    if ((uint64_t)width * height * 2u > (1ull << 30))
        return fail(RR_ERR_UNSUPPORTED, "%s: %ux%u pixels x 2 parts are more than 2^30 accumulator slots", fn, width, height);
    if (threshold != threshold) return fail(RR_ERR_INVALID_ARGUMENT, "%s: threshold is NaN", fn);
    return RR_OK;
}

// ---- what every list has in common (this layer's, the sublist of rr_api_levels.h, the compaction of rr_api_prefix.h)
// The scratch of a list over n slots (8x8 blocks of a frame, or waves of 64 entries of a list): per slot a 64-bit mask, then its count
// (after k_refine_scan: its offset), then one word, the list's length; and the grid of the kernels that work a slot per wave.
struct ListScratch { unsigned long long* masks; uint32_t* counts; uint32_t* total; int grid; };
static int list_scratch(rr_scene* s, uint32_t n, ListScratch* ls) {
    HIP_TRY(s->adaptive.scratch.reserve(12ull * n + 4u));
    ls->masks = s->adaptive.scratch.as<unsigned long long>();
    ls->counts = (uint32_t*)(ls->masks + n);
    ls->total = ls->counts + n;
    ls->grid = (int)std::min<uint64_t>((n + RR_BLOCK / RR_WAVE - 1) / (RR_BLOCK / RR_WAVE), (uint64_t)s->n_cus * 8u);
    return RR_OK;
}
// THE wait of a list: the 4 bytes of its length (pinned, h_count[HC_LIST_COUNT]); behind it the stream is idle
static int await_list_count(rr_scene* s, const uint32_t* total, hipStream_t st, uint32_t* count) {
    uint32_t* h = s->frame.h_count + HC_LIST_COUNT;
    HIP_TRY(hipMemcpyAsync(h, total, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    *count = *h;
    return RR_OK;
}

// THE list of an entry source (rr_adaptive.h: a frame's blocks, or a list's entries) from its part records, on stream st, into list_out and
// *count_out (host): three launches and one wait.  The caller holds the lock and has taken the stream.  With kernel_timing the three
// launches are timed as one re-ordering (rr_frame_stats::ms_binning).  Scratch: list_scratch over the source's waves.
template <class Source>
static int compact_list_locked(rr_scene* s, const Source& src, const rr_radiance* parts, float threshold, float* error_out, uint32_t* list_out, uint32_t* count_out,
                               hipStream_t st) {
    const uint32_t nw = src.waves();
    ListScratch ls;
    RR_TRY(list_scratch(s, nw, &ls));
    {
        ScopedTimer t(s, st, TK_BINNING, false);
        hipLaunchKernelGGL(k_refine_masks<Source>, dim3(ls.grid), dim3(RR_BLOCK), 0, st, src, (const float4*)parts, threshold, error_out, ls.masks, ls.counts);
        hipLaunchKernelGGL(k_refine_scan, dim3(1), dim3(1024), 0, st, ls.counts, nw, ls.total);
        hipLaunchKernelGGL(k_refine_scatter<Source>, dim3(ls.grid), dim3(RR_BLOCK), 0, st, src, ls.masks, ls.counts, ls.total, list_out);
    }
    HIP_TRY(hipGetLastError());
    return await_list_count(s, ls.total, st, count_out);
}
// the list of a frame's parts: list_out has refine_capacity entries
static int refine_list_locked(rr_scene* s, uint32_t W, uint32_t H, const rr_radiance* parts, float threshold, float* error_out, uint32_t* list_out,
                              uint32_t* count_out, hipStream_t st) {
    return compact_list_locked(s, FrameSource{W, H}, parts, threshold, error_out, list_out, count_out, st);
}

uint64_t rr_refine_list_capacity(uint32_t width, uint32_t height) { return refine_capacity(width, height); }

// (C linkage: the entry points of this layer are declared in include/rustray_hip.h, inside its extern "C" block, and a definition keeps the
// linkage of its declaration; tests/test_adaptive_device_host.py holds each to the guard every entry point has)
int rr_refine_list_device(rr_scene* s, uint32_t width, uint32_t height, const rr_radiance* parts, float threshold, float* error_out, uint32_t* list_out,
                          uint32_t* count_out, void* hip_stream) try {
    if (!s || !parts || !list_out || !count_out) return fail(RR_ERR_INVALID_ARGUMENT, "rr_refine_list_device: NULL argument");
    RR_TRY(check_refine_frame("rr_refine_list_device", width, height, threshold));
    if (((uintptr_t)parts & 15u) || (((uintptr_t)error_out | (uintptr_t)list_out) & 3u))
        return fail(RR_ERR_INVALID_ARGUMENT, "rr_refine_list_device: parts_dev must be 16-byte aligned, error_out_dev and list_out_dev 4-byte aligned");
    RR_TRY(not_in_pass(s, "rr_refine_list_device"));
    std::lock_guard<std::mutex> lk(s->mu);
    HIP_TRY(hipSetDevice(s->device));
    RR_TRY(check_query_pointers(s, "rr_refine_list_device", {{parts, "parts_dev"}, {error_out, "error_out_dev"}, {list_out, "list_out_dev"}}));
    const hipStream_t st = (hipStream_t)hip_stream;
    RR_TRY(take_stream(s, st));
    IdleOnExit idle(st);
    const bool profiling = s->timing.profiling; // nothing of a frame's stats is touched: the launches are not timed here
    s->timing.profiling = false;
    const int rc = refine_list_locked(s, width, height, parts, threshold, error_out, list_out, count_out, st);
    s->timing.profiling = profiling;
    return idle.done(rc);
} RR_GUARD_END("rr_refine_list_device")

// ---- what every fused call has in common (rr_render_adaptive, rr_render_adaptive_levels, rr_render_adaptive_prefix)
// The outputs of a fused call: the records, and on request the frame's bytes, the samples and the error of every pixel, and the call's
// counts (n_refined, or level_pixels: host words, written by a finished call only).
struct FusedOut { rr_radiance* out; uint8_t* rgba8; uint16_t* samples; float* error; uint32_t* counts; };

// what both forms check of them, and of the frame they are for; `device`: the alignment rule of the device form
static int check_fused_outputs(const char* fn, bool device, const rr_camera* cam, float threshold, const FusedOut& o) {
    RR_TRY(check_refine_frame(fn, cam->width, cam->height, threshold));
    if (!o.out) return fail(RR_ERR_INVALID_ARGUMENT, "%s: out is required", fn);
    if (device && (((uintptr_t)o.out & 15u) || ((uintptr_t)o.samples & 1u) || (((uintptr_t)o.rgba8 | (uintptr_t)o.error) & 3u)))
        return fail(RR_ERR_INVALID_ARGUMENT, "%s: out_dev must be 16-byte aligned, rgba8_out_dev and error_out_dev 4-byte aligned and samples_out_dev 2-byte aligned", fn);
    return RR_OK;
}

// THE device form of a fused call, its arguments checked: `body(o)` under the scene's lock, on outputs the scene's device can address
template <class Body>
static int device_fused_call(rr_scene* s, const char* fn, const FusedOut& o, Body body) {
    RR_TRY(not_in_pass(s, fn));
    std::lock_guard<std::mutex> lk(s->mu);
    RR_TRY(check_intact(s));
    HIP_TRY(hipSetDevice(s->device));
    RR_TRY(check_query_pointers(s, fn, {{o.out, "out_dev"}, {o.rgba8, "rgba8_out_dev"}, {o.samples, "samples_out_dev"}, {o.error, "error_out_dev"}}));
    return body(o);
}

// THE host form of a fused call, its arguments checked: the device form on the null stream behind a staging copy.  The staging is the
// handle's (s->frame.tmp_out: grown, kept, used by host forms only, which return with the stream idle): the bytes and the records where
// rr_render_pixels stages its own, the sample counts and the errors in the buffers of the next two outputs.  The caller's outputs are
// written by a finished call only: `out` is copied last and waits for the launches, and the n_counts words of `counts` are the body's
// private ones until then.
template <class Body>
static int host_fused_call(rr_scene* s, const char* fn, const rr_camera* cam, const FusedOut& host, uint32_t n_counts, Body body) {
    RR_TRY(not_in_pass(s, fn));
    std::lock_guard<std::mutex> lk(s->mu);
    RR_TRY(check_intact(s));
    HIP_TRY(hipSetDevice(s->device));
    const size_t n = (size_t)cam->width * cam->height;
    DevBuf &d_rgba = s->frame.tmp_out[0], &d_out = s->frame.tmp_out[1], &d_samples = s->frame.tmp_out[2], &d_error = s->frame.tmp_out[3];
    HIP_TRY(d_out.reserve(32ull * n));
    if (host.rgba8) HIP_TRY(d_rgba.reserve(4ull * n));
    if (host.samples) HIP_TRY(d_samples.reserve(2ull * n));
    if (host.error) HIP_TRY(d_error.reserve(4ull * n));
    uint32_t counts[RR_MAX_ADAPTIVE_LEVELS] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
    RR_TRY(body(FusedOut{d_out.as<rr_radiance>(), host.rgba8 ? d_rgba.as<uint8_t>() : nullptr, host.samples ? d_samples.as<uint16_t>() : nullptr,
                         host.error ? d_error.as<float>() : nullptr, counts}));
    if (host.rgba8) HIP_TRY(hipMemcpyAsync(host.rgba8, d_rgba.p, 4ull * n, hipMemcpyDeviceToHost, nullptr));
    if (host.samples) HIP_TRY(hipMemcpyAsync(host.samples, d_samples.p, 2ull * n, hipMemcpyDeviceToHost, nullptr));
    if (host.error) HIP_TRY(hipMemcpyAsync(host.error, d_error.p, 4ull * n, hipMemcpyDeviceToHost, nullptr));
    HIP_TRY(hipMemcpy(host.out, d_out.p, 32ull * n, hipMemcpyDeviceToHost));
    HIP_TRY(hipStreamSynchronize(nullptr));
    if (host.counts) memcpy(host.counts, counts, 4ull * n_counts);
    return RR_OK;
}

// the frame's bytes of n finished records (k_record_bytes)
static void launch_record_bytes(rr_scene* s, const rr_config* cfg, const rr_radiance* records, uint32_t n, uint8_t* rgba8, hipStream_t st) {
    const int grid = (int)std::min<uint64_t>((n + RR_BLOCK - 1) / RR_BLOCK, (uint64_t)s->n_cus * 8u);
    hipLaunchKernelGGL(k_record_bytes, dim3(grid), dim3(RR_BLOCK), 0, st, (const float4*)records, n, cfg->gamma_correction ? 1u : 0u, (uint32_t*)rgba8);
}
// THE tail of a fused body: the bytes of the whole frame where they are asked for, the check of every launch not checked yet (`fn`: the
// call's name in the message), and the body's counts to where the call wants them
static int finish_fused(rr_scene* s, const char* fn, const rr_config* cfg, uint32_t N, const FusedOut& o, const uint32_t* counts, uint32_t n_counts, hipStream_t st) {
    if (o.rgba8) launch_record_bytes(s, cfg, o.out, N, o.rgba8, st);
    if (hipGetLastError() != hipSuccess) return fail(RR_ERR_DEVICE, "%s: a launch failed", fn);
    if (o.counts) memcpy(o.counts, counts, 4ull * n_counts);
    return RR_OK;
}

// what both forms check before the scene is looked at
static int check_adaptive_args(const char* fn, bool device, const rr_scene* s, const rr_camera* cam, const rr_config* cfg, uint16_t base_samples, uint16_t max_samples,
                               float threshold, const uint16_t* sample_xy_base, const uint16_t* sample_xy_max, const FusedOut& o) {
    if (!s || !cam || !cfg) return fail(RR_ERR_INVALID_ARGUMENT, "NULL argument");
    if (base_samples < 2u || (base_samples & 1u))
        return fail(RR_ERR_INVALID_ARGUMENT, "%s: base_samples %u must be even and at least 2: the two halves of a pixel must be equal", fn, (unsigned)base_samples);
    rr_config c = *cfg; // (config->samples is ignored)
    c.samples = base_samples;
    RR_TRY(check_frame_args(s, cam, &c, sample_xy_base));
    c.samples = max_samples;
    RR_TRY(check_frame_args(s, cam, &c, sample_xy_max));
    return check_fused_outputs(fn, device, cam, threshold, o);
}

// one call on buffers the device can address (the caller holds the lock); a call that ends early leaves the stream idle
static int render_adaptive_locked(rr_scene* s, const rr_camera* cam, const rr_config* cfg, uint16_t base_samples, uint16_t max_samples, float threshold,
                                  const uint16_t* sample_xy_base, const uint16_t* sample_xy_max, const FusedOut& o, hipStream_t st, const volatile int* cancel) {
    IdleOnExit idle(st);
    const uint32_t W = cam->width, H = cam->height, N = W * H;
    HIP_TRY(s->adaptive.parts.reserve(64ull * N));
    HIP_TRY(s->adaptive.list.reserve(4ull * refine_capacity(W, H)));
    rr_radiance* parts = s->adaptive.parts.as<rr_radiance>();
    uint32_t* list = s->adaptive.list.as<uint32_t>();
    rr_config c = *cfg;
    c.samples = base_samples;
    RR_TRY(render_pixel_parts_locked(s, cam, &c, sample_xy_base, nullptr, N, 1u, o.out, parts, st, cancel));
    uint32_t count = 0;
    if (o.samples && hipMemsetD16Async((hipDeviceptr_t)o.samples, base_samples, N, st) != hipSuccess) return fail(RR_ERR_DEVICE, "hipMemsetD16Async(samples_out) failed");
    RR_TRY(refine_list_locked(s, W, H, parts, threshold, o.error, list, &count, st));
    RR_TRY(collect_stats_locked(s)); // the stream is idle: what the base pass cost, and the list's launches with it
    PassSums sums{s};
    sums.add();
    if (count) {
        if (cancel && *cancel) return fail(RR_ERR_CANCELLED, "cancelled");
        const uint32_t padded = refine_padded(count);
        HIP_TRY(s->adaptive.fine.reserve(32ull * padded));
        float4* fine = s->adaptive.fine.as<float4>();
        c.samples = max_samples;
        RR_TRY(render_pixels_locked(s, cam, &c, sample_xy_max, list, padded, (rr_radiance*)fine, nullptr, st, cancel));
        const int grid = (int)std::min<uint64_t>((count + RR_BLOCK - 1) / RR_BLOCK, (uint64_t)s->n_cus * 8u);
        hipLaunchKernelGGL(k_scatter_level, dim3(grid), dim3(RR_BLOCK), 0, st, list, count, fine, (const float4*)nullptr, W, max_samples, (float4*)o.out, o.samples,
                           (float*)nullptr); // (no error at max_samples: there are no halves)
        sums.carry(); // rr_scene_last_stats: the sums over the two passes
    }
    sums.close();
    return idle.done(finish_fused(s, "rr_render_adaptive", cfg, N, o, &count, 1u, st));
}

int rr_render_adaptive_device(rr_scene* s, const rr_camera* cam, const rr_config* cfg, uint16_t base_samples, uint16_t max_samples, float threshold,
                              const uint16_t* sample_xy_base, const uint16_t* sample_xy_max, rr_radiance* out, uint8_t* rgba8_out, uint16_t* samples_out,
                              float* error_out, uint32_t* n_refined_out, void* hip_stream, const volatile int* cancel) try {
    const FusedOut o{out, rgba8_out, samples_out, error_out, n_refined_out};
    RR_TRY(check_adaptive_args("rr_render_adaptive_device", true, s, cam, cfg, base_samples, max_samples, threshold, sample_xy_base, sample_xy_max, o));
    return device_fused_call(s, "rr_render_adaptive_device", o, [&](const FusedOut& d) {
        return render_adaptive_locked(s, cam, cfg, base_samples, max_samples, threshold, sample_xy_base, sample_xy_max, d, (hipStream_t)hip_stream, cancel);
    });
} RR_GUARD_END("rr_render_adaptive_device")

int rr_render_adaptive(rr_scene* s, const rr_camera* cam, const rr_config* cfg, uint16_t base_samples, uint16_t max_samples, float threshold,
                       const uint16_t* sample_xy_base, const uint16_t* sample_xy_max, rr_radiance* out, uint8_t* rgba8_out, uint16_t* samples_out,
                       float* error_out, uint32_t* n_refined_out, const volatile int* cancel) try {
    const FusedOut o{out, rgba8_out, samples_out, error_out, n_refined_out};
    RR_TRY(check_adaptive_args("rr_render_adaptive", false, s, cam, cfg, base_samples, max_samples, threshold, sample_xy_base, sample_xy_max, o));
    return host_fused_call(s, "rr_render_adaptive", cam, o, 1u, [&](const FusedOut& d) {
        return render_adaptive_locked(s, cam, cfg, base_samples, max_samples, threshold, sample_xy_base, sample_xy_max, d, nullptr, cancel);
    });
} RR_GUARD_END("rr_render_adaptive")
