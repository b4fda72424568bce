// rr_api_pixel_split.h — rr_render_pixel_split and its device form: the records (and, on request, the halves) rr_render_pixel_parts gives at
// K = 2, and next to them the frame's DIRECT DIFFUSE light of the primary hits as a sum of its own -- the part of a pixel's colour the base
// texture modulates, which rr_denoise_split_records demodulates alone.
// Offers: rr_render_pixel_split_device, rr_render_pixel_split.
// Needs:  rr_api_frame.h (check_frame_args, FrameEnd::RECORD_SPLIT, pixels_io, render_region_locked: level 1 through k_shade<true, true> and
//         k_trace_shadow<*, true>, ending in k_resolve_pixel_parts<true>), rr_api_query.h (check_arg_ranges, record_call, staged_host_call, StageArg),
//         rr_pixel_list.h (pixel_list_first_bad).
//
// The body is the frame's: slot table, sample table, batches, level walk and plan, over n_pixels * K accumulator slots (K = 2 with halves,
// else 1).  Level 1 runs serially (no stages on three streams); the deeper levels run the frame's own kernels.  The device form works on
// buffers the scene's device can address, in stream order; the host form is the device form behind the staging of every record call, in
// buffers of the call's own.

struct PixelSplitIo {
    rr_radiance* out; rr_radiance* halves; float* diffuse; float* diffuse_halves;
};

// what both forms check before the scene is looked at; `device`: the rules of the device form.  n_pixels == 0 passes: the caller returns
// RR_OK before it touches anything.
static int check_pixel_split_args(const char* fn, bool device, const rr_scene* s, const rr_camera* cam, const rr_config* cfg, const uint16_t* sample_xy,
                                  const uint32_t* pixel_xy, uint32_t n_pixels, const PixelSplitIo& io) {
    RR_TRY(check_frame_args(s, cam, cfg, sample_xy));
    if (!io.out) return fail(RR_ERR_INVALID_ARGUMENT, "%s: out is required", fn);
    if (!io.diffuse) return fail(RR_ERR_INVALID_ARGUMENT, "%s: diffuse_out is required", fn);
    if ((io.halves != nullptr) != (io.diffuse_halves != nullptr))
        return fail(RR_ERR_INVALID_ARGUMENT, "%s: halves_out and diffuse_halves_out are given together or not at all", fn);
    if (io.halves && cfg->samples % 2u != 0u) return fail(RR_ERR_INVALID_ARGUMENT, "%s: n_parts 2 does not divide samples %u", fn, (unsigned)cfg->samples);
    if ((uint64_t)n_pixels * (io.halves ? 2u : 1u) > (1ull << 30))
        return fail(RR_ERR_UNSUPPORTED, "%s: %u pixels%s are more than 2^30 accumulator slots", fn, n_pixels, io.halves ? " x 2 halves" : "");
    if (n_pixels == 0) return RR_OK;
    if (!pixel_xy && (uint64_t)n_pixels != (uint64_t)cam->width * cam->height)
        return fail(RR_ERR_INVALID_ARGUMENT, "%s: %u pixels without a list, the frame of %ux%u has %llu", fn, n_pixels, cam->width, cam->height,
                    (unsigned long long)cam->width * cam->height);
    if (!device) return RR_OK;
    if (((uintptr_t)io.out | (uintptr_t)io.halves) & 15u) return fail(RR_ERR_INVALID_ARGUMENT, "%s: out_dev and halves_out_dev must be 16-byte aligned", fn);
    if (((uintptr_t)pixel_xy | (uintptr_t)io.diffuse | (uintptr_t)io.diffuse_halves) & 3u)
        return fail(RR_ERR_INVALID_ARGUMENT, "%s: pixel_xy_dev, diffuse_out_dev and diffuse_halves_out_dev must be 4-byte aligned", fn);
    const uint64_t n = n_pixels;
    const ArgRange t[5] = {{pixel_xy, 4u * n, "pixel_xy_dev", false, -1}, {io.out, 32u * n, "out_dev", true, -1}, {io.halves, 64u * n, "halves_out_dev", true, -1},
                           {io.diffuse, 12u * n, "diffuse_out_dev", true, -1}, {io.diffuse_halves, 24u * n, "diffuse_halves_out_dev", true, -1}};
    return check_arg_ranges(fn, t, 5, true, "");
}

// One call on buffers the scene's device can address, in stream order (the caller holds the lock and leaves the stream idle on an early end).
// `trusted`: the list was checked on the host (the host form): nothing is read back.
static int render_pixel_split_locked(rr_scene* s, const rr_camera* cam, const rr_config* cfg, const uint16_t* sample_xy, const uint32_t* pixel_xy, uint32_t n,
                                     const PixelSplitIo& out, hipStream_t st, bool trusted, const volatile int* cancel) {
    FrameIo io = pixels_io(pixel_xy, n, out.out, nullptr);
    io.end = FrameEnd::RECORD_SPLIT; io.lg_parts = out.halves ? 1u : 0u; io.parts = out.halves; io.diffuse = out.diffuse; io.diffuse_parts = out.diffuse_halves;
    io.own_list = trusted;
    return render_region_locked(s, cam, cfg, sample_xy, io, st, cancel);
}

// (defined under the C linkage of their declarations in include/rustray_hip.h, as rr_api_albedo_pixels.h does)
int rr_render_pixel_split_device(rr_scene* s, const rr_camera* camera, const rr_config* config, const uint16_t* sample_xy, const uint32_t* pixel_xy, uint32_t n_pixels,
                                 rr_radiance* out, rr_radiance* halves_out, float* diffuse_out, float* diffuse_halves_out, void* hip_stream,
                                 const volatile int* cancel) try {
    const char* fn = "rr_render_pixel_split_device";
    const PixelSplitIo io{out, halves_out, diffuse_out, diffuse_halves_out};
    RR_TRY(check_pixel_split_args(fn, true, s, camera, config, sample_xy, pixel_xy, n_pixels, io));
    if (n_pixels == 0) return RR_OK;
    const hipStream_t st = (hipStream_t)hip_stream;
    return record_call(s, fn, true, {{pixel_xy, "pixel_xy_dev"}, {out, "out_dev"}, {halves_out, "halves_out_dev"}, {diffuse_out, "diffuse_out_dev"},
                                     {diffuse_halves_out, "diffuse_halves_out_dev"}}, st,
                       [&] { return render_pixel_split_locked(s, camera, config, sample_xy, pixel_xy, n_pixels, io, st, false, cancel); });
} RR_GUARD_END("rr_render_pixel_split_device")

// The host form: the device form behind the staging of every record call, in buffers of the call's own, freed on return, on the null
// stream.  The list is checked here, before anything is uploaded; the caller's outputs are written by a finished call only.
int rr_render_pixel_split(rr_scene* s, const rr_camera* camera, const rr_config* config, const uint16_t* sample_xy, const uint32_t* pixel_xy, uint32_t n_pixels,
                          rr_radiance* out, rr_radiance* halves_out, float* diffuse_out, float* diffuse_halves_out, const volatile int* cancel) try {
    const char* fn = "rr_render_pixel_split";
    RR_TRY(check_pixel_split_args(fn, false, s, camera, config, sample_xy, pixel_xy, n_pixels, PixelSplitIo{out, halves_out, diffuse_out, diffuse_halves_out}));
    if (n_pixels == 0) return RR_OK;
    if (pixel_xy) {
        const uint32_t bad = pixel_list_first_bad(pixel_xy, n_pixels, camera->width, camera->height);
        if (bad != RR_PIXEL_LIST_OK)
            return fail(RR_ERR_INVALID_ARGUMENT, "pixel_xy[%u] = (%u, %u) lies outside the frame of %ux%u pixels", bad, pixel_xy[bad] & 0xffffu, pixel_xy[bad] >> 16,
                        camera->width, camera->height);
    }
    const size_t n = n_pixels;
    const StageArg args[5] = {stage_input(pixel_xy, 4 * n), stage_output(out, 32 * n), stage_output(halves_out, 64 * n), stage_output(diffuse_out, 12 * n),
                              stage_output(diffuse_halves_out, 24 * n)};
    return record_call(s, fn, true, {}, nullptr, [&] {
        DevBuf own[5];
        return staged_host_call(own, args, [&](void* const* d) {
            return render_pixel_split_locked(s, camera, config, sample_xy, (const uint32_t*)d[0], n_pixels,
                                             PixelSplitIo{(rr_radiance*)d[1], (rr_radiance*)d[2], (float*)d[3], (float*)d[4]}, nullptr, true, cancel);
        });
    });
} RR_GUARD_END("rr_render_pixel_split")
