// rr_api_parts.h — rr_render_pixel_parts and its device form: the samples of a pixel as K interleaved means (part h = the frame samples
// s with s mod K == h) next to the pixel's full record, from the rays rr_render_pixels traces.
// Offers: rr_render_pixel_parts, rr_render_pixel_parts_device.
// Needs:  rr_api_frame.h (FrameIo, pixels_io, IdleOnExit, render_region_locked: K slots per pixel, k_pixel_slots and k_resolve_pixel_parts at
//         its two ends), rr_api_query.h (check_pixels_args, host_list_call, check_query_pointers).
//
// The body is the frame's: batches, level walk, stages and plan, over n_pixels * K accumulator slots of samples / K samples each.  The
// device form works on buffers the scene's device can address, in stream order; the host form is the device form behind the staging
// copy of every list call (host_list_call, rr_api_query.h).

// n_parts as log2, or why it is refused.  `out`, `parts_out`: both required; `device`: the alignment rule of the device form.
static int check_parts_args(const char* fn, bool device, const rr_scene* s, const rr_camera* cam, const rr_config* cfg, const uint16_t* sample_xy,
                            const uint32_t* pixel_xy, uint32_t n_pixels, uint32_t n_parts, const rr_radiance* out, const rr_radiance* parts_out,
                            uint32_t* lg_parts) {
    RR_TRY(check_pixels_args(fn, device, s, cam, cfg, sample_xy, pixel_xy, n_pixels, out, nullptr));
    if (!parts_out) return fail(RR_ERR_INVALID_ARGUMENT, "%s: parts_out is required", fn);
    if (n_parts < 2u || n_parts > 64u || (n_parts & (n_parts - 1u)) != 0u)
        return fail(RR_ERR_INVALID_ARGUMENT, "%s: n_parts %u is not a power of two from 2 to 64", fn, n_parts);
    if (cfg->samples % n_parts != 0u) return fail(RR_ERR_INVALID_ARGUMENT, "%s: n_parts %u does not divide samples %u", fn, n_parts, (unsigned)cfg->samples);
    if ((uint64_t)n_pixels * n_parts > (1ull << 30))
        return fail(RR_ERR_UNSUPPORTED, "%s: %u pixels x %u parts are more than 2^30 accumulator slots", fn, n_pixels, n_parts);
    if (device && ((uintptr_t)parts_out & 15u)) return fail(RR_ERR_INVALID_ARGUMENT, "%s: out_dev and parts_out_dev must be 16-byte aligned", fn);
    uint32_t lg = 0;
    while ((n_parts >> lg) > 1u) lg++;
    *lg_parts = lg;
    return RR_OK;
}

// one call on buffers the device can address (the caller holds the lock); a call that ends early leaves the stream idle
static int render_pixel_parts_locked(rr_scene* s, const rr_camera* cam, const rr_config* cfg, const uint16_t* sample_xy, const uint32_t* pixel_xy,
                                     uint32_t n_pixels, uint32_t lg_parts, rr_radiance* out, rr_radiance* parts_out, hipStream_t st, const volatile int* cancel) {
    IdleOnExit idle(st);
    FrameIo io = pixels_io(pixel_xy, n_pixels, out, nullptr);
    io.end = FrameEnd::RECORD_PARTS; io.lg_parts = lg_parts; io.parts = parts_out;
    return idle.done(render_region_locked(s, cam, cfg, sample_xy, io, st, cancel));
}

// (C linkage: both are declared in include/rustray_hip.h, inside its extern "C" block, and a definition keeps the linkage of its declaration;
// tests/test_pixel_parts.py holds each to the guard every entry point has and to its unmangled name in the library)
int rr_render_pixel_parts_device(rr_scene* s, const rr_camera* cam, const rr_config* cfg, const uint16_t* sample_xy, const uint32_t* pixel_xy,
                                 uint32_t n_pixels, uint32_t n_parts, rr_radiance* out, rr_radiance* parts_out, void* hip_stream,
                                 const volatile int* cancel) try {
    uint32_t lg_parts = 0;
    RR_TRY(check_parts_args("rr_render_pixel_parts_device", true, s, cam, cfg, sample_xy, pixel_xy, n_pixels, n_parts, out, parts_out, &lg_parts));
    if (n_pixels == 0) return RR_OK;
    RR_TRY(not_in_pass(s, "rr_render_pixel_parts_device"));
    std::lock_guard<std::mutex> lk(s->mu);
    RR_TRY(check_intact(s));
    HIP_TRY(hipSetDevice(s->device));
    RR_TRY(check_query_pointers(s, "rr_render_pixel_parts_device", {{pixel_xy, "pixel_xy_dev"}, {out, "out_dev"}, {parts_out, "parts_out_dev"}}));
    return render_pixel_parts_locked(s, cam, cfg, sample_xy, pixel_xy, n_pixels, lg_parts, out, parts_out, (hipStream_t)hip_stream, cancel);
} RR_GUARD_END("rr_render_pixel_parts_device")

int rr_render_pixel_parts(rr_scene* s, const rr_camera* cam, const rr_config* cfg, const uint16_t* sample_xy, const uint32_t* pixel_xy,
                          uint32_t n_pixels, uint32_t n_parts, rr_radiance* out, rr_radiance* parts_out, const volatile int* cancel) try {
    uint32_t lg_parts = 0;
    RR_TRY(check_parts_args("rr_render_pixel_parts", false, s, cam, cfg, sample_xy, pixel_xy, n_pixels, n_parts, out, parts_out, &lg_parts));
    if (n_pixels == 0) return RR_OK;
    return host_list_call(s, "rr_render_pixel_parts", cam, pixel_xy, n_pixels, n_parts, out, parts_out, nullptr,
                          [&](const uint32_t* d_list, rr_radiance* d_out, rr_radiance* d_parts, uint8_t*) {
                              return render_pixel_parts_locked(s, cam, cfg, sample_xy, d_list, n_pixels, lg_parts, d_out, d_parts, nullptr, cancel);
                          });
} RR_GUARD_END("rr_render_pixel_parts")
