// rr_api_albedo_pixels.h — the frame's albedo per pixel: the mean, over the primary rays rr_render_pixels traces for the pixel, of the base
// colour at each ray's first hit -- the albedo a pixel's colour was actually modulated by, what rr_denoise_records takes at an edge pixel.
// Offers: rr_albedo_pixels_device, rr_albedo_pixels.
// Needs:  rr_api_frame.h (check_frame_args, FrameEnd::ALBEDO, pixels_io, render_region_locked: level 1 alone, ending in k_albedo_level1 and
//         k_resolve_albedo, kernels 5x and 5y of rr_kernels.hip), rr_api_query.h (check_arg_ranges, record_call, staged_host_call, StageArg),
//         rr_pixel_list.h (pixel_list_first_bad).
//
// The body is the frame's: slot table, sample table, batches, sample groups and the closest-hit launch of level 1; where a frame shades, the
// hits' base colours are summed in the colour planes of the frame's accumulators, nothing spawns, and the resolve writes three floats per
// pixel.  The device form works on buffers the scene's device can address, in stream order; the host form is the device form behind the
// staging of every record call, in buffers of the call's own.

// what both forms check before the scene is looked at, in the order the header states; `device`: the rules of the device form.
// n_pixels == 0 passes: the caller returns RR_OK before it touches anything.
static int check_albedo_pixels_args(const char* fn, bool device, const rr_scene* s, const rr_camera* cam, const rr_config* cfg, const uint16_t* sample_xy,
                                    const uint32_t* pixel_xy, uint32_t n_pixels, const float* albedo) {
    RR_TRY(check_frame_args(s, cam, cfg, sample_xy));
    if (!albedo) return fail(RR_ERR_INVALID_ARGUMENT, "%s: albedo_out is required", fn);
    if (n_pixels > (1u << 30)) return fail(RR_ERR_UNSUPPORTED, "%s: %u pixels in one call", fn, n_pixels);
    if (n_pixels == 0) return RR_OK;
    if (!pixel_xy && (uint64_t)n_pixels != (uint64_t)cam->width * cam->height)
        return fail(RR_ERR_INVALID_ARGUMENT, "%s: %u pixels without a list, the frame of %ux%u has %llu", fn, n_pixels, cam->width, cam->height,
                    (unsigned long long)cam->width * cam->height);
    if (!device) return RR_OK;
    if ((uintptr_t)albedo & 3u) return fail(RR_ERR_INVALID_ARGUMENT, "%s: albedo_out_dev is not 4-byte aligned", fn);
    if ((uintptr_t)pixel_xy & 3u) return fail(RR_ERR_INVALID_ARGUMENT, "%s: pixel_xy_dev is not 4-byte aligned", fn);
    const ArgRange t[2] = {{pixel_xy, 4ull * n_pixels, "pixel_xy_dev", false, -1}, {albedo, 12ull * n_pixels, "albedo_out_dev", true, -1}};
    return check_arg_ranges(fn, t, 2, true, "");
}

// One call on buffers the scene's device can address, in stream order (the caller holds the lock and leaves the stream idle on an early end).
// `trusted`: the list was checked on the host (the host form): nothing is read back.
static int albedo_pixels_locked(rr_scene* s, const rr_camera* cam, const rr_config* cfg, const uint16_t* sample_xy, const uint32_t* pixel_xy, uint32_t n,
                                float* albedo, hipStream_t st, bool trusted, const volatile int* cancel) {
    FrameIo io = pixels_io(pixel_xy, n, nullptr, nullptr);
    io.end = FrameEnd::ALBEDO; io.albedo = albedo; io.own_list = trusted;
    return render_region_locked(s, cam, cfg, sample_xy, io, st, cancel);
}

// (defined under the C linkage of their declarations in include/rustray_hip.h, as rr_api_surface_pixels.h does)
int rr_albedo_pixels_device(rr_scene* s, const rr_camera* camera, const rr_config* config, const uint16_t* sample_xy, const uint32_t* pixel_xy, uint32_t n_pixels,
                            float* albedo_out, void* hip_stream, const volatile int* cancel) try {
    const char* fn = "rr_albedo_pixels_device";
    RR_TRY(check_albedo_pixels_args(fn, true, s, camera, config, sample_xy, pixel_xy, n_pixels, albedo_out));
    if (n_pixels == 0) return RR_OK;
    const hipStream_t st = (hipStream_t)hip_stream;
    return record_call(s, fn, true, {{pixel_xy, "pixel_xy_dev"}, {albedo_out, "albedo_out_dev"}}, st,
                       [&] { return albedo_pixels_locked(s, camera, config, sample_xy, pixel_xy, n_pixels, albedo_out, st, false, cancel); });
} RR_GUARD_END("rr_albedo_pixels_device")

// The host form: the device form behind the staging of every record call, in buffers of the call's own, freed on return, on the null
// stream.  The list is checked here, before anything is uploaded; the caller's output is written by a finished call only.
int rr_albedo_pixels(rr_scene* s, const rr_camera* camera, const rr_config* config, const uint16_t* sample_xy, const uint32_t* pixel_xy, uint32_t n_pixels,
                     float* albedo_out, const volatile int* cancel) try {
    const char* fn = "rr_albedo_pixels";
    RR_TRY(check_albedo_pixels_args(fn, false, s, camera, config, sample_xy, pixel_xy, n_pixels, albedo_out));
    if (n_pixels == 0) return RR_OK;
    if (pixel_xy) {
        const uint32_t bad = pixel_list_first_bad(pixel_xy, n_pixels, camera->width, camera->height);
        if (bad != RR_PIXEL_LIST_OK)
            return fail(RR_ERR_INVALID_ARGUMENT, "pixel_xy[%u] = (%u, %u) lies outside the frame of %ux%u pixels", bad, pixel_xy[bad] & 0xffffu, pixel_xy[bad] >> 16,
                        camera->width, camera->height);
    }
    const StageArg args[2] = {stage_input(pixel_xy, 4ull * n_pixels), stage_output(albedo_out, 12ull * n_pixels)};
    return record_call(s, fn, true, {}, nullptr, [&] {
        DevBuf own[2];
        return staged_host_call(own, args, [&](void* const* d) {
            return albedo_pixels_locked(s, camera, config, sample_xy, (const uint32_t*)d[0], n_pixels, (float*)d[1], nullptr, true, cancel);
        });
    });
} RR_GUARD_END("rr_albedo_pixels")
