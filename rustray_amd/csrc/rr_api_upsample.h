// rr_api_upsample.h — a frame traced at a low resolution raised to the full one by the full-resolution G-buffer, on the device: the
// joint-bilateral upsampler between rr_render_pixel_parts on a small camera and rr_denoise_records / rr_accumulate_records at full size.
// Offers: rr_upsample_default_params, rr_upsample_records_device, rr_upsample_records, rr_upsample_albedo_records_device,
//         rr_upsample_albedo_records (the first pair is the second with no albedo planes).
// Needs:  rr_api_query.h (check_arg_ranges, record_call, staged_host_call), rr_api_adaptive.h (launch_record_bytes), rr_upsample.h,
//         kernel 7g of rr_kernels.hip.
//
// The call is ONE launch of k_upsample_records and, for the bytes, k_record_bytes, on the caller's stream, not waited for.  It keeps no
// working memory.  The host form is the device form behind the staging of every record call (staged_host_call, in the handle's pool).

int rr_upsample_default_params(rr_upsample_params* out) try {
    if (!out) return fail(RR_ERR_INVALID_ARGUMENT, "rr_upsample_default_params: out is NULL");
    out->struct_size = (uint32_t)sizeof(rr_upsample_params);
    out->normal_power_log2 = 5u;
    out->sigma_depth = 0.05f;
    out->use_albedo = 1u;
    out->gamma_correction = 0u;
    return RR_OK;
} RR_GUARD_END("rr_upsample_default_params")

struct UpsampleIo {
    const rr_radiance* low; const rr_radiance* halves_low; const rr_surface_hit* guide_low; const rr_surface_hit* guide;
    rr_radiance* out; rr_radiance* halves_out; uint8_t* rgba8; float* weight;
    const float* albedo_low; const float* albedo;   // the caller's albedo planes (12 B a pixel), each or NULL: the guides' base_color serves
};

// what both forms check before the scene is looked at, in the order include/rustray_hip.h states; `device`: the alignment rule of the device form
static int check_upsample_args(const char* fn, bool device, const rr_scene* s, uint32_t lw, uint32_t lh, uint32_t width, uint32_t height, const rr_upsample_params* prm,
                               const UpsampleIo& io) {
    if (!s) return fail(RR_ERR_INVALID_ARGUMENT, "%s: scene is NULL", fn);
    if (!prm) return fail(RR_ERR_INVALID_ARGUMENT, "%s: params is NULL", fn);
    if (!io.low) return fail(RR_ERR_INVALID_ARGUMENT, "%s: low is NULL", fn);
    if (!io.guide_low) return fail(RR_ERR_INVALID_ARGUMENT, "%s: guide_low is NULL", fn);
    if (!io.guide) return fail(RR_ERR_INVALID_ARGUMENT, "%s: guide is NULL", fn);
    if (!io.out) return fail(RR_ERR_INVALID_ARGUMENT, "%s: out is NULL", fn);
    if (width == 0 || height == 0 || width > 65535u || height > 65535u) return fail(RR_ERR_INVALID_ARGUMENT, "%s: bad frame size %ux%u", fn, width, height);
    if (lw == 0 || lh == 0 || lw > width || lh > height)
        return fail(RR_ERR_INVALID_ARGUMENT, "%s: bad low frame size %ux%u for a frame of %ux%u (1 .. the frame's)", fn, lw, lh, width, height);
    if (prm->struct_size != sizeof(rr_upsample_params))
        return fail(RR_ERR_INVALID_ARGUMENT, "%s: params->struct_size %u, expected %u", fn, prm->struct_size, (unsigned)sizeof(rr_upsample_params));
    if (prm->normal_power_log2 > 7u) return fail(RR_ERR_INVALID_ARGUMENT, "%s: normal_power_log2 %u (0 .. 7)", fn, prm->normal_power_log2);
    if (!(prm->sigma_depth > 0.0f) || !denoise_is_finite(prm->sigma_depth)) return fail(RR_ERR_INVALID_ARGUMENT, "%s: sigma_depth must be finite and above 0", fn);
    if ((io.halves_low != nullptr) != (io.halves_out != nullptr))
        return fail(RR_ERR_INVALID_ARGUMENT, "%s: halves_low and halves_out are given together or not at all", fn);
    if (device && (((uintptr_t)io.low | (uintptr_t)io.halves_low | (uintptr_t)io.guide_low | (uintptr_t)io.guide | (uintptr_t)io.out | (uintptr_t)io.halves_out) & 15u))
        return fail(RR_ERR_INVALID_ARGUMENT, "%s: low_dev, halves_low_dev, guide_low_dev, guide_dev, out_dev and halves_out_dev must be 16-byte aligned", fn);
    if (device && (((uintptr_t)io.rgba8 | (uintptr_t)io.weight | (uintptr_t)io.albedo_low | (uintptr_t)io.albedo) & 3u))
        return fail(RR_ERR_INVALID_ARGUMENT, "%s: rgba8_out_dev, weight_out_dev, albedo_low_dev and albedo_dev must be 4-byte aligned", fn);
    // overlaps: an output with an input or with another output; nothing is in place
    const uint64_t nl = (uint64_t)lw * lh, n = (uint64_t)width * height;
    const ArgRange t[10] = {{io.low, 32u * nl, "low", false, -1}, {io.halves_low, 64u * nl, "halves_low", false, -1}, {io.guide_low, 128u * nl, "guide_low", false, -1},
                            {io.guide, 128u * n, "guide", false, -1}, {io.albedo_low, 12u * nl, "albedo_low", false, -1}, {io.albedo, 12u * n, "albedo", false, -1},
                            {io.out, 32u * n, "out", true, -1}, {io.halves_out, 64u * n, "halves_out", true, -1},
                            {io.rgba8, 4u * n, "rgba8_out", true, -1}, {io.weight, 4u * n, "weight_out", true, -1}};
    RR_TRY(check_arg_ranges(fn, t, 10, false, ""));
    if (n * 2u > (1ull << 30)) return fail(RR_ERR_UNSUPPORTED, "%s: %ux%u pixels x 2 halves are more than 2^30 records", fn, width, height);
    return RR_OK;
}

// the launches of one call on stream st, on buffers the device can address; the caller holds the lock and has taken the stream
template <bool HALVES, bool PLANES>
static void launch_upsample(const dim3 grid, const UpCall& call, uint32_t lw, uint32_t lh, uint32_t W, uint32_t H, const UpsampleIo& io, hipStream_t st) {
    hipLaunchKernelGGL((k_upsample_records<HALVES, PLANES>), grid, dim3(RR_BLOCK), 0, st, (const float4*)io.low, (const float4*)io.halves_low, (const uint4*)io.guide_low,
                       (const uint4*)io.guide, io.albedo_low, io.albedo, lw, lh, W, H, call, (float4*)io.out, (float4*)io.halves_out, io.weight);
}
static int upsample_locked(rr_scene* s, uint32_t lw, uint32_t lh, uint32_t W, uint32_t H, const rr_upsample_params* prm, const UpsampleIo& io_in, hipStream_t st) {
    const UpCall call{prm->sigma_depth, upsample_ratio(W, H, lw, lh), prm->normal_power_log2, prm->use_albedo ? 1u : 0u};
    const dim3 grid((W + UP_TILE_W - 1) / UP_TILE_W, (H + UP_TILE_H - 1) / UP_TILE_H);
    UpsampleIo io = io_in;
    if (!call.use_albedo) io.albedo_low = io.albedo = nullptr;   // without use_albedo the planes are not read: the builds without them run
    if (io.albedo_low || io.albedo) {                            // the planes builds: either plane may still be NULL, a test uniform over the launch
        if (io.halves_low) launch_upsample<true, true>(grid, call, lw, lh, W, H, io, st);
        else launch_upsample<false, true>(grid, call, lw, lh, W, H, io, st);
    } else {
        if (io.halves_low) launch_upsample<true, false>(grid, call, lw, lh, W, H, io, st);
        else launch_upsample<false, false>(grid, call, lw, lh, W, H, io, st);
    }
    if (io.rgba8) {
        rr_config cfg{};
        cfg.gamma_correction = prm->gamma_correction ? 1 : 0;
        launch_record_bytes(s, &cfg, io.out, (uint32_t)((uint64_t)W * H), io.rgba8, st);
    }
    if (hipGetLastError() != hipSuccess) return fail(RR_ERR_DEVICE, "rr_upsample_records: a launch failed");
    return RR_OK;
}

// the two forms of the call under the name `fn`; rr_upsample_records(_device) are these with both planes NULL
static int upsample_device_call(const char* fn, rr_scene* s, uint32_t lw, uint32_t lh, uint32_t W, uint32_t H, const rr_upsample_params* prm, const UpsampleIo& io,
                                void* hip_stream) {
    RR_TRY(check_upsample_args(fn, true, s, lw, lh, W, H, prm, io));
    const hipStream_t st = (hipStream_t)hip_stream;
    return record_call(s, fn, false, {{io.low, "low_dev"}, {io.halves_low, "halves_low_dev"}, {io.guide_low, "guide_low_dev"}, {io.guide, "guide_dev"},
                                      {io.albedo_low, "albedo_low_dev"}, {io.albedo, "albedo_dev"}, {io.out, "out_dev"}, {io.halves_out, "halves_out_dev"},
                                      {io.rgba8, "rgba8_out_dev"}, {io.weight, "weight_out_dev"}}, st,
                       [&] { return upsample_locked(s, lw, lh, W, H, prm, io, st); });
}
static int upsample_host_call(const char* fn, rr_scene* s, uint32_t lw, uint32_t lh, uint32_t W, uint32_t H, const rr_upsample_params* prm, const UpsampleIo& io) {
    RR_TRY(check_upsample_args(fn, false, s, lw, lh, W, H, prm, io));
    const size_t nl = (size_t)lw * lh, n = (size_t)W * H;
    const StageArg args[10] = {stage_input(io.low, 32 * nl), stage_input(io.halves_low, 64 * nl), stage_input(io.guide_low, 128 * nl), stage_input(io.guide, 128 * n),
                               stage_input(io.albedo_low, 12 * nl), stage_input(io.albedo, 12 * n), stage_output(io.out, 32 * n), stage_output(io.halves_out, 64 * n),
                               stage_output(io.rgba8, 4 * n), stage_output(io.weight, 4 * n)};
    return record_call(s, fn, false, {}, nullptr, [&] {
        return staged_host_call(s->record_stage.buf, args, [&](void* const* d) {
            const UpsampleIo dev{(const rr_radiance*)d[0], (const rr_radiance*)d[1], (const rr_surface_hit*)d[2], (const rr_surface_hit*)d[3], (rr_radiance*)d[6],
                                 (rr_radiance*)d[7], (uint8_t*)d[8], (float*)d[9], (const float*)d[4], (const float*)d[5]};
            return upsample_locked(s, lw, lh, W, H, prm, dev, nullptr);
        });
    });
}

// (defined under the C linkage of their declarations in include/rustray_hip.h)
int rr_upsample_albedo_records_device(rr_scene* s, uint32_t low_width, uint32_t low_height, uint32_t width, uint32_t height, const rr_upsample_params* prm,
                                      const rr_radiance* low, const rr_radiance* halves_low, const rr_surface_hit* guide_low, const rr_surface_hit* guide,
                                      const float* albedo_low, const float* albedo, rr_radiance* out, rr_radiance* halves_out, uint8_t* rgba8_out, float* weight_out,
                                      void* hip_stream) try {
    return upsample_device_call("rr_upsample_albedo_records_device", s, low_width, low_height, width, height, prm,
                                UpsampleIo{low, halves_low, guide_low, guide, out, halves_out, rgba8_out, weight_out, albedo_low, albedo}, hip_stream);
} RR_GUARD_END("rr_upsample_albedo_records_device")

int rr_upsample_albedo_records(rr_scene* s, uint32_t low_width, uint32_t low_height, uint32_t width, uint32_t height, const rr_upsample_params* prm, const rr_radiance* low,
                               const rr_radiance* halves_low, const rr_surface_hit* guide_low, const rr_surface_hit* guide, const float* albedo_low, const float* albedo,
                               rr_radiance* out, rr_radiance* halves_out, uint8_t* rgba8_out, float* weight_out) try {
    return upsample_host_call("rr_upsample_albedo_records", s, low_width, low_height, width, height, prm,
                              UpsampleIo{low, halves_low, guide_low, guide, out, halves_out, rgba8_out, weight_out, albedo_low, albedo});
} RR_GUARD_END("rr_upsample_albedo_records")

int rr_upsample_records_device(rr_scene* s, uint32_t low_width, uint32_t low_height, uint32_t width, uint32_t height, const rr_upsample_params* prm,
                               const rr_radiance* low, const rr_radiance* halves_low, const rr_surface_hit* guide_low, const rr_surface_hit* guide, rr_radiance* out,
                               rr_radiance* halves_out, uint8_t* rgba8_out, float* weight_out, void* hip_stream) try {
    return upsample_device_call("rr_upsample_records_device", s, low_width, low_height, width, height, prm,
                                UpsampleIo{low, halves_low, guide_low, guide, out, halves_out, rgba8_out, weight_out, nullptr, nullptr}, hip_stream);
} RR_GUARD_END("rr_upsample_records_device")

int rr_upsample_records(rr_scene* s, uint32_t low_width, uint32_t low_height, uint32_t width, uint32_t height, const rr_upsample_params* prm, const rr_radiance* low,
                        const rr_radiance* halves_low, const rr_surface_hit* guide_low, const rr_surface_hit* guide, rr_radiance* out, rr_radiance* halves_out,
                        uint8_t* rgba8_out, float* weight_out) try {
    return upsample_host_call("rr_upsample_records", s, low_width, low_height, width, height, prm,
                              UpsampleIo{low, halves_low, guide_low, guide, out, halves_out, rgba8_out, weight_out, nullptr, nullptr});
} RR_GUARD_END("rr_upsample_records")
