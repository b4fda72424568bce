// rr_api_temporal.h — temporal reprojection of a frame of records on the device: the previous call's result is gathered into the
// current frame and the current records are blended into it, the step before rr_denoise_records in a frame-after-frame loop.
// Offers: rr_accumulate_default_params, rr_accumulate_records_device, rr_accumulate_records, rr_accumulate_split_records_device,
//         rr_accumulate_split_records, rr_history_clamp_default_params, rr_accumulate_clamped_records_device,
//         rr_accumulate_clamped_records, rr_accumulate_clamped_split_records_device, rr_accumulate_clamped_split_records; tp_frame (for
//         rr_api_motion.h).
// Needs:  rr_api_query.h (check_arg_ranges, record_call, staged_host_call), rr_api_adaptive.h (launch_record_bytes), rr_temporal.h,
//         rr_history_clamp.h, kernels 7e, 7e', 7e'' and 7e''' of rr_kernels.hip.
//
// The call is ONE launch of k_accumulate_records (with or without halves; the split call: of k_accumulate_split_records; the clamped
// call: of k_accumulate_clamped_records; the clamped split call: of k_accumulate_clamped_split_records) and, for the
// bytes, k_record_bytes, on the caller's stream, not waited for.  It keeps no working data.  The host form is the device form behind the staging of every record call
// (staged_host_call, in the handle's pool).

int rr_accumulate_default_params(rr_accumulate_params* out) try {
    if (!out) return fail(RR_ERR_INVALID_ARGUMENT, "rr_accumulate_default_params: out is NULL");
    memset(out, 0, sizeof *out);
    out->struct_size = (uint32_t)sizeof(rr_accumulate_params);
    for (int k = 0; k < 4; k++) out->prev_world_to_clip[5 * k] = 1.0f;
    out->max_history = 32.0f;
    out->normal_min = 0.9f;
    out->sigma_depth = 0.05f;
    out->snap = 0.015625f;
    return RR_OK;
} RR_GUARD_END("rr_accumulate_default_params")

struct AccumulateIo {
    const rr_radiance* records; const rr_radiance* halves; const rr_radiance* history; const rr_radiance* history_halves;
    const float* history_length; const float* motion;
    rr_radiance* out; rr_radiance* halves_out; float* length_out; uint8_t* rgba8;
};

// what both forms of both calls check before the scene is looked at, up to the overlaps; `device`: the alignment rule of the device form
static int check_accumulate_basics(const char* fn, bool device, const rr_scene* s, const rr_camera* cam, const rr_accumulate_params* prm, const AccumulateIo& io) {
    if (!s) return fail(RR_ERR_INVALID_ARGUMENT, "%s: scene is NULL", fn);
    if (!cam) return fail(RR_ERR_INVALID_ARGUMENT, "%s: camera is NULL", fn);
    if (!prm) return fail(RR_ERR_INVALID_ARGUMENT, "%s: params is NULL", fn);
    if (!io.records) return fail(RR_ERR_INVALID_ARGUMENT, "%s: records is NULL", fn);
    if (!io.out) return fail(RR_ERR_INVALID_ARGUMENT, "%s: out is NULL", fn);
    if (!io.length_out) return fail(RR_ERR_INVALID_ARGUMENT, "%s: length_out is NULL", fn);
    const uint32_t width = cam->width, height = cam->height;
    if (width == 0 || height == 0 || width > 65535u || height > 65535u) return fail(RR_ERR_INVALID_ARGUMENT, "%s: bad frame size %ux%u", fn, width, height);
    if (prm->struct_size != sizeof(rr_accumulate_params))
        return fail(RR_ERR_INVALID_ARGUMENT, "%s: params->struct_size %u, expected %u", fn, prm->struct_size, (unsigned)sizeof(rr_accumulate_params));
    if (!(prm->max_history >= 1.0f && prm->max_history <= 65536.0f)) return fail(RR_ERR_INVALID_ARGUMENT, "%s: max_history must lie in 1 .. 65536", fn);
    if (!(prm->normal_min >= -1.0f && prm->normal_min <= 1.0f)) return fail(RR_ERR_INVALID_ARGUMENT, "%s: normal_min must lie in -1 .. 1", fn);
    if (!(prm->sigma_depth > 0.0f) || !denoise_is_finite(prm->sigma_depth)) return fail(RR_ERR_INVALID_ARGUMENT, "%s: sigma_depth must be finite and above 0", fn);
    if (!(prm->snap >= 0.0f && prm->snap < 0.5f)) return fail(RR_ERR_INVALID_ARGUMENT, "%s: snap must lie in [0, 0.5)", fn);
    if ((uint64_t)width * height * 2u > (1ull << 30))
        return fail(RR_ERR_UNSUPPORTED, "%s: %ux%u pixels x 2 halves are more than 2^30 records", fn, width, height);
    // what comes with what
    if ((io.history == nullptr) != (io.history_length == nullptr))
        return fail(RR_ERR_INVALID_ARGUMENT, "%s: history and history_length come together (both NULL: the first frame)", fn);
    if (io.history ? (io.history_halves != nullptr) != (io.halves != nullptr) : io.history_halves != nullptr)
        return fail(RR_ERR_INVALID_ARGUMENT, "%s: history_halves is required exactly when history and halves are given", fn);
    if ((io.halves_out != nullptr) != (io.halves != nullptr)) return fail(RR_ERR_INVALID_ARGUMENT, "%s: halves_out is required exactly when halves is given", fn);
    if (device && (((uintptr_t)io.records | (uintptr_t)io.halves | (uintptr_t)io.history | (uintptr_t)io.history_halves | (uintptr_t)io.out | (uintptr_t)io.halves_out) & 15u))
        return fail(RR_ERR_INVALID_ARGUMENT, "%s: records_dev, halves_dev, history_dev, history_halves_dev, out_dev and halves_out_dev must be 16-byte aligned", fn);
    if (device && (((uintptr_t)io.history_length | (uintptr_t)io.motion | (uintptr_t)io.length_out | (uintptr_t)io.rgba8) & 3u))
        return fail(RR_ERR_INVALID_ARGUMENT, "%s: history_length_dev, motion_dev, length_out_dev and rgba8_out_dev must be 4-byte aligned", fn);
    return RR_OK;
}

static int check_accumulate_args(const char* fn, bool device, const rr_scene* s, const rr_camera* cam, const rr_accumulate_params* prm, const AccumulateIo& io) {
    RR_TRY(check_accumulate_basics(fn, device, s, cam, prm, io));
    const uint32_t width = cam->width, height = cam->height;
    // overlaps: an output with an input or with another output; out == records and halves_out == halves exactly are the in-place call
    const uint64_t n = (uint64_t)width * height;
    const ArgRange t[10] = {{io.records, 32u * n, "records", false, -1}, {io.halves, 64u * n, "halves", false, -1}, {io.history, 32u * n, "history", false, -1},
                            {io.history_halves, 64u * n, "history_halves", false, -1}, {io.history_length, 4u * n, "history_length", false, -1},
                            {io.motion, 12u * n, "motion", false, -1}, {io.out, 32u * n, "out", true, 0}, {io.halves_out, 64u * n, "halves_out", true, 1},
                            {io.length_out, 4u * n, "length_out", true, -1}, {io.rgba8, 4u * n, "rgba8_out", true, -1}};
    return check_arg_ranges(fn, t, 10, false, " (only out == records and halves_out == halves, in place, are allowed)");
}

// the camera and the frame size as the frame constants of the kernels that turn a record's depth into a world position (k_accumulate_records,
// k_motion_records); what else a kernel reads of them is its caller's to fill
static TpFrame tp_frame(const rr_camera* cam) {
    TpFrame f{};
    memcpy(f.proj_inv, cam->projection_inverse, sizeof f.proj_inv);
    memcpy(f.view_inv, cam->view_inverse, sizeof f.view_inv);
    f.w = (float)cam->width; f.h = (float)cam->height;
    f.width = (int)cam->width; f.height = (int)cam->height;
    return f;
}

// the kernel argument of the three accumulation kernels: the camera, the previous view and the scalars of the call; and their grid of 32x8 tiles
static TpFrame accumulate_frame(const rr_camera* cam, const rr_accumulate_params* prm) {
    TpFrame f = tp_frame(cam);
    memcpy(f.prev_clip, prm->prev_world_to_clip, sizeof f.prev_clip);
    memcpy(f.prev_eye, prm->prev_eye, sizeof f.prev_eye);
    f.max_history = prm->max_history; f.normal_min = prm->normal_min; f.sigma_depth = prm->sigma_depth; f.snap = prm->snap;
    return f;
}
static dim3 accumulate_grid(const rr_camera* cam) { return dim3((cam->width + DN_TILE_W - 1) / DN_TILE_W, (cam->height + DN_TILE_H - 1) / DN_TILE_H); }

// the launches of one call on stream st, on buffers the device can address; the caller holds the lock and has taken the stream
// split: the diffuse layers of rr_accumulate_split_records (then the SPLIT build of the kernel runs), or NULL
static int accumulate_locked(rr_scene* s, const rr_camera* cam, const rr_accumulate_params* prm, const AccumulateIo& io, hipStream_t st, const TpSplitIo* split = nullptr) {
    const uint32_t W = cam->width, H = cam->height;
    const TpFrame f = accumulate_frame(cam, prm);
    const dim3 grid = accumulate_grid(cam), block(RR_BLOCK);
    if (split) {
        if (io.halves)
            hipLaunchKernelGGL(k_accumulate_split_records<true>, grid, block, 0, st, f, (const float4*)io.records, (const float4*)io.halves, (const float4*)io.history,
                               (const float4*)io.history_halves, io.history_length, io.motion, (float4*)io.out, (float4*)io.halves_out, io.length_out, *split);
        else
            hipLaunchKernelGGL(k_accumulate_split_records<false>, grid, block, 0, st, f, (const float4*)io.records, (const float4*)nullptr, (const float4*)io.history,
                               (const float4*)nullptr, io.history_length, io.motion, (float4*)io.out, (float4*)nullptr, io.length_out, *split);
    } else if (io.halves)
        hipLaunchKernelGGL(k_accumulate_records<true>, grid, block, 0, st, f, (const float4*)io.records, (const float4*)io.halves, (const float4*)io.history,
                           (const float4*)io.history_halves, io.history_length, io.motion, (float4*)io.out, (float4*)io.halves_out, io.length_out);
    else
        hipLaunchKernelGGL(k_accumulate_records<false>, grid, block, 0, st, f, (const float4*)io.records, (const float4*)nullptr, (const float4*)io.history,
                           (const float4*)nullptr, io.history_length, io.motion, (float4*)io.out, (float4*)nullptr, io.length_out);
    if (io.rgba8) {
        rr_config cfg{};
        cfg.gamma_correction = prm->gamma_correction ? 1 : 0;
        launch_record_bytes(s, &cfg, io.out, W * H, io.rgba8, st);
    }
    if (hipGetLastError() != hipSuccess) return fail(RR_ERR_DEVICE, "rr_accumulate_records: a launch failed");
    return RR_OK;
}

int rr_accumulate_records_device(rr_scene* s, const rr_camera* camera, const rr_accumulate_params* prm, const rr_radiance* records, const rr_radiance* halves,
                                 const rr_radiance* history, const rr_radiance* history_halves, const float* history_length, const float* motion,
                                 rr_radiance* out, rr_radiance* halves_out, float* length_out, uint8_t* rgba8_out, void* hip_stream) try {
    const char* fn = "rr_accumulate_records_device";
    const AccumulateIo io{records, halves, history, history_halves, history_length, motion, out, halves_out, length_out, rgba8_out};
    RR_TRY(check_accumulate_args(fn, true, s, camera, prm, io));
    const hipStream_t st = (hipStream_t)hip_stream;
    return record_call(s, fn, false, {{records, "records_dev"}, {halves, "halves_dev"}, {history, "history_dev"}, {history_halves, "history_halves_dev"},
                                      {history_length, "history_length_dev"}, {motion, "motion_dev"}, {out, "out_dev"}, {halves_out, "halves_out_dev"},
                                      {length_out, "length_out_dev"}, {rgba8_out, "rgba8_out_dev"}}, st, [&] { return accumulate_locked(s, camera, prm, io, st); });
} RR_GUARD_END("rr_accumulate_records_device")

int rr_accumulate_records(rr_scene* s, const rr_camera* camera, const rr_accumulate_params* prm, const rr_radiance* records, const rr_radiance* halves,
                          const rr_radiance* history, const rr_radiance* history_halves, const float* history_length, const float* motion, rr_radiance* out,
                          rr_radiance* halves_out, float* length_out, uint8_t* rgba8_out) try {
    const char* fn = "rr_accumulate_records";
    RR_TRY(check_accumulate_args(fn, false, s, camera, prm, AccumulateIo{records, halves, history, history_halves, history_length, motion, out, halves_out, length_out, rgba8_out}));
    const size_t n = (size_t)camera->width * camera->height;
    const StageArg args[10] = {stage_input(records, 32 * n), stage_input(halves, 64 * n), stage_input(history, 32 * n), stage_input(history_halves, 64 * n),
                               stage_input(history_length, 4 * n), stage_input(motion, 12 * n), stage_output(out, 32 * n), stage_output(halves_out, 64 * n),
                               stage_output(length_out, 4 * n), stage_output(rgba8_out, 4 * n)};
    return record_call(s, fn, false, {}, nullptr, [&] {
        return staged_host_call(s->record_stage.buf, args, [&](void* const* d) {
            const AccumulateIo dev{(const rr_radiance*)d[0], (const rr_radiance*)d[1], (const rr_radiance*)d[2], (const rr_radiance*)d[3], (const float*)d[4],
                                   (const float*)d[5], (rr_radiance*)d[6], (rr_radiance*)d[7], (float*)d[8], (uint8_t*)d[9]};
            return accumulate_locked(s, camera, prm, dev, nullptr);
        });
    });
} RR_GUARD_END("rr_accumulate_records")

// ---- rr_accumulate_split_records: the same call with the diffuse layers of rr_render_pixel_split riding on the taps of the records
// what the split call checks beyond check_accumulate_basics: what comes with what, the float alignment and all sixteen ranges
static int check_accumulate_split_args(const char* fn, bool device, const rr_scene* s, const rr_camera* cam, const rr_accumulate_params* prm, const AccumulateIo& io,
                                       const TpSplitIo& d) {
    RR_TRY(check_accumulate_basics(fn, device, s, cam, prm, io));
    if (!d.diffuse) return fail(RR_ERR_INVALID_ARGUMENT, "%s: diffuse is NULL", fn);
    if (!d.diffuse_out) return fail(RR_ERR_INVALID_ARGUMENT, "%s: diffuse_out is NULL", fn);
    if ((d.dif_halves != nullptr) != (io.halves != nullptr)) return fail(RR_ERR_INVALID_ARGUMENT, "%s: diffuse_halves is required exactly when halves is given", fn);
    if ((d.dif_halves_out != nullptr) != (io.halves != nullptr)) return fail(RR_ERR_INVALID_ARGUMENT, "%s: diffuse_halves_out is required exactly when halves is given", fn);
    if ((d.history_diffuse != nullptr) != (io.history != nullptr)) return fail(RR_ERR_INVALID_ARGUMENT, "%s: history_diffuse is required exactly when history is given", fn);
    if ((d.history_dif_halves != nullptr) != (io.history_halves != nullptr))
        return fail(RR_ERR_INVALID_ARGUMENT, "%s: history_diffuse_halves is required exactly when history_halves is given", fn);
    if (device && (((uintptr_t)d.diffuse | (uintptr_t)d.dif_halves | (uintptr_t)d.history_diffuse | (uintptr_t)d.history_dif_halves | (uintptr_t)d.diffuse_out |
                    (uintptr_t)d.dif_halves_out) & 3u))
        return fail(RR_ERR_INVALID_ARGUMENT, "%s: diffuse_dev, diffuse_halves_dev, history_diffuse_dev, history_diffuse_halves_dev, diffuse_out_dev and diffuse_halves_out_dev must be 4-byte aligned", fn);
    const uint64_t n = (uint64_t)cam->width * cam->height;
    const ArgRange t[16] = {{io.records, 32u * n, "records", false, -1}, {io.halves, 64u * n, "halves", false, -1}, {d.diffuse, 12u * n, "diffuse", false, -1},
                            {d.dif_halves, 24u * n, "diffuse_halves", false, -1}, {io.history, 32u * n, "history", false, -1},
                            {io.history_halves, 64u * n, "history_halves", false, -1}, {d.history_diffuse, 12u * n, "history_diffuse", false, -1},
                            {d.history_dif_halves, 24u * n, "history_diffuse_halves", false, -1}, {io.history_length, 4u * n, "history_length", false, -1},
                            {io.motion, 12u * n, "motion", false, -1}, {io.out, 32u * n, "out", true, 0}, {io.halves_out, 64u * n, "halves_out", true, 1},
                            {d.diffuse_out, 12u * n, "diffuse_out", true, 2}, {d.dif_halves_out, 24u * n, "diffuse_halves_out", true, 3},
                            {io.length_out, 4u * n, "length_out", true, -1}, {io.rgba8, 4u * n, "rgba8_out", true, -1}};
    return check_arg_ranges(fn, t, 16, false,
                            " (only out == records, halves_out == halves, diffuse_out == diffuse and diffuse_halves_out == diffuse_halves, in place, are allowed)");
}

int rr_accumulate_split_records_device(rr_scene* s, const rr_camera* camera, const rr_accumulate_params* prm, const rr_radiance* records, const rr_radiance* halves,
                                       const float* diffuse, const float* diffuse_halves, const rr_radiance* history, const rr_radiance* history_halves,
                                       const float* history_diffuse, const float* history_diffuse_halves, const float* history_length, const float* motion,
                                       rr_radiance* out, rr_radiance* halves_out, float* diffuse_out, float* diffuse_halves_out, float* length_out, uint8_t* rgba8_out,
                                       void* hip_stream) try {
    const char* fn = "rr_accumulate_split_records_device";
    const AccumulateIo io{records, halves, history, history_halves, history_length, motion, out, halves_out, length_out, rgba8_out};
    const TpSplitIo split{diffuse, diffuse_halves, history_diffuse, history_diffuse_halves, diffuse_out, diffuse_halves_out};
    RR_TRY(check_accumulate_split_args(fn, true, s, camera, prm, io, split));
    const hipStream_t st = (hipStream_t)hip_stream;
    return record_call(s, fn, false, {{records, "records_dev"}, {halves, "halves_dev"}, {diffuse, "diffuse_dev"}, {diffuse_halves, "diffuse_halves_dev"},
                                      {history, "history_dev"}, {history_halves, "history_halves_dev"}, {history_diffuse, "history_diffuse_dev"},
                                      {history_diffuse_halves, "history_diffuse_halves_dev"}, {history_length, "history_length_dev"}, {motion, "motion_dev"},
                                      {out, "out_dev"}, {halves_out, "halves_out_dev"}, {diffuse_out, "diffuse_out_dev"}, {diffuse_halves_out, "diffuse_halves_out_dev"},
                                      {length_out, "length_out_dev"}, {rgba8_out, "rgba8_out_dev"}}, st, [&] { return accumulate_locked(s, camera, prm, io, st, &split); });
} RR_GUARD_END("rr_accumulate_split_records_device")

int rr_accumulate_split_records(rr_scene* s, const rr_camera* camera, const rr_accumulate_params* prm, const rr_radiance* records, const rr_radiance* halves,
                                const float* diffuse, const float* diffuse_halves, const rr_radiance* history, const rr_radiance* history_halves,
                                const float* history_diffuse, const float* history_diffuse_halves, const float* history_length, const float* motion, rr_radiance* out,
                                rr_radiance* halves_out, float* diffuse_out, float* diffuse_halves_out, float* length_out, uint8_t* rgba8_out) try {
    const char* fn = "rr_accumulate_split_records";
    RR_TRY(check_accumulate_split_args(fn, false, s, camera, prm, AccumulateIo{records, halves, history, history_halves, history_length, motion, out, halves_out, length_out, rgba8_out},
                                       TpSplitIo{diffuse, diffuse_halves, history_diffuse, history_diffuse_halves, diffuse_out, diffuse_halves_out}));
    const size_t n = (size_t)camera->width * camera->height;
    const StageArg args[16] = {stage_input(records, 32 * n), stage_input(halves, 64 * n), stage_input(diffuse, 12 * n), stage_input(diffuse_halves, 24 * n),
                               stage_input(history, 32 * n), stage_input(history_halves, 64 * n), stage_input(history_diffuse, 12 * n),
                               stage_input(history_diffuse_halves, 24 * n), stage_input(history_length, 4 * n), stage_input(motion, 12 * n),
                               stage_output(out, 32 * n), stage_output(halves_out, 64 * n), stage_output(diffuse_out, 12 * n), stage_output(diffuse_halves_out, 24 * n),
                               stage_output(length_out, 4 * n), stage_output(rgba8_out, 4 * n)};
    return record_call(s, fn, false, {}, nullptr, [&] {
        return staged_host_call(s->record_stage.buf, args, [&](void* const* d) {
            const AccumulateIo dev{(const rr_radiance*)d[0], (const rr_radiance*)d[1], (const rr_radiance*)d[4], (const rr_radiance*)d[5], (const float*)d[8],
                                   (const float*)d[9], (rr_radiance*)d[10], (rr_radiance*)d[11], (float*)d[14], (uint8_t*)d[15]};
            const TpSplitIo split{(const float*)d[2], (const float*)d[3], (const float*)d[6], (const float*)d[7], (float*)d[12], (float*)d[13]};
            return accumulate_locked(s, camera, prm, dev, nullptr, &split);
        });
    });
} RR_GUARD_END("rr_accumulate_split_records")

// ---- rr_accumulate_clamped_records: the same call with the history held to the box of the current frame's colours around each pixel
int rr_history_clamp_default_params(rr_history_clamp_params* out) try {
    if (!out) return fail(RR_ERR_INVALID_ARGUMENT, "rr_history_clamp_default_params: out is NULL");
    memset(out, 0, sizeof *out);
    out->struct_size = (uint32_t)sizeof(rr_history_clamp_params);
    out->radius = 1u;        // chosen by measurement: DESIGN.md section 8, item 24
    out->sigma_scale = 0.5f;
    return RR_OK;
} RR_GUARD_END("rr_history_clamp_default_params")

// what the clamped call checks: rr_accumulate_records' rules with `out` allowed nowhere on `records` (the window reads other pixels'
// records, which another workgroup may already have overwritten), and the clamp's own parameters
static int check_accumulate_clamped_args(const char* fn, bool device, const rr_scene* s, const rr_camera* cam, const rr_accumulate_params* prm,
                                         const rr_history_clamp_params* clamp, const AccumulateIo& io) {
    RR_TRY(check_accumulate_basics(fn, device, s, cam, prm, io));
    if (!clamp) return fail(RR_ERR_INVALID_ARGUMENT, "%s: clamp is NULL", fn);
    if (clamp->struct_size != sizeof(rr_history_clamp_params))
        return fail(RR_ERR_INVALID_ARGUMENT, "%s: clamp->struct_size %u, expected %u", fn, clamp->struct_size, (unsigned)sizeof(rr_history_clamp_params));
    if (clamp->radius != 1u && clamp->radius != 2u) return fail(RR_ERR_INVALID_ARGUMENT, "%s: clamp->radius %u, must be 1 or 2", fn, clamp->radius);
    if (!(clamp->sigma_scale >= 0.0f && clamp->sigma_scale <= 65536.0f)) return fail(RR_ERR_INVALID_ARGUMENT, "%s: clamp->sigma_scale must lie in 0 .. 65536", fn);
    const uint64_t n = (uint64_t)cam->width * cam->height;
    const ArgRange t[10] = {{io.records, 32u * n, "records", false, -1}, {io.halves, 64u * n, "halves", false, -1}, {io.history, 32u * n, "history", false, -1},
                            {io.history_halves, 64u * n, "history_halves", false, -1}, {io.history_length, 4u * n, "history_length", false, -1},
                            {io.motion, 12u * n, "motion", false, -1}, {io.out, 32u * n, "out", true, -1}, {io.halves_out, 64u * n, "halves_out", true, 1},
                            {io.length_out, 4u * n, "length_out", true, -1}, {io.rgba8, 4u * n, "rgba8_out", true, -1}};
    return check_arg_ranges(fn, t, 10, false, " (the window reads the records of other pixels, so out may not be records; only halves_out == halves, in place, is allowed)");
}

static int accumulate_clamped_locked(rr_scene* s, const rr_camera* cam, const rr_accumulate_params* prm, const rr_history_clamp_params* clamp, const AccumulateIo& io,
                                     hipStream_t st) {
    const uint32_t W = cam->width, H = cam->height;
    const TpFrame f = accumulate_frame(cam, prm);
    const dim3 grid = accumulate_grid(cam), block(RR_BLOCK);
    const float k = clamp->sigma_scale;
    const float4 *rec = (const float4*)io.records, *hv = (const float4*)io.halves, *hist = (const float4*)io.history, *hist_h = (const float4*)io.history_halves;
    float4 *out = (float4*)io.out, *out_h = (float4*)io.halves_out;
    if (io.halves && clamp->radius == 1u)
        hipLaunchKernelGGL((k_accumulate_clamped_records<true, 1>), grid, block, 0, st, f, k, rec, hv, hist, hist_h, io.history_length, io.motion, out, out_h, io.length_out);
    else if (io.halves)
        hipLaunchKernelGGL((k_accumulate_clamped_records<true, 2>), grid, block, 0, st, f, k, rec, hv, hist, hist_h, io.history_length, io.motion, out, out_h, io.length_out);
    else if (clamp->radius == 1u)
        hipLaunchKernelGGL((k_accumulate_clamped_records<false, 1>), grid, block, 0, st, f, k, rec, (const float4*)nullptr, hist, (const float4*)nullptr, io.history_length,
                           io.motion, out, (float4*)nullptr, io.length_out);
    else
        hipLaunchKernelGGL((k_accumulate_clamped_records<false, 2>), grid, block, 0, st, f, k, rec, (const float4*)nullptr, hist, (const float4*)nullptr, io.history_length,
                           io.motion, out, (float4*)nullptr, io.length_out);
    if (io.rgba8) {
        rr_config cfg{};
        cfg.gamma_correction = prm->gamma_correction ? 1 : 0;
        launch_record_bytes(s, &cfg, io.out, W * H, io.rgba8, st);
    }
    if (hipGetLastError() != hipSuccess) return fail(RR_ERR_DEVICE, "rr_accumulate_clamped_records: a launch failed");
    return RR_OK;
}

int rr_accumulate_clamped_records_device(rr_scene* s, const rr_camera* camera, const rr_accumulate_params* prm, const rr_history_clamp_params* clamp,
                                         const rr_radiance* records, const rr_radiance* halves, const rr_radiance* history, const rr_radiance* history_halves,
                                         const float* history_length, const float* motion, rr_radiance* out, rr_radiance* halves_out, float* length_out,
                                         uint8_t* rgba8_out, void* hip_stream) try {
    const char* fn = "rr_accumulate_clamped_records_device";
    const AccumulateIo io{records, halves, history, history_halves, history_length, motion, out, halves_out, length_out, rgba8_out};
    RR_TRY(check_accumulate_clamped_args(fn, true, s, camera, prm, clamp, io));
    const hipStream_t st = (hipStream_t)hip_stream;
    return record_call(s, fn, false, {{records, "records_dev"}, {halves, "halves_dev"}, {history, "history_dev"}, {history_halves, "history_halves_dev"},
                                      {history_length, "history_length_dev"}, {motion, "motion_dev"}, {out, "out_dev"}, {halves_out, "halves_out_dev"},
                                      {length_out, "length_out_dev"}, {rgba8_out, "rgba8_out_dev"}}, st,
                       [&] { return accumulate_clamped_locked(s, camera, prm, clamp, io, st); });
} RR_GUARD_END("rr_accumulate_clamped_records_device")

int rr_accumulate_clamped_records(rr_scene* s, const rr_camera* camera, const rr_accumulate_params* prm, const rr_history_clamp_params* clamp,
                                  const rr_radiance* records, const rr_radiance* halves, const rr_radiance* history, const rr_radiance* history_halves,
                                  const float* history_length, const float* motion, rr_radiance* out, rr_radiance* halves_out, float* length_out,
                                  uint8_t* rgba8_out) try {
    const char* fn = "rr_accumulate_clamped_records";
    RR_TRY(check_accumulate_clamped_args(fn, false, s, camera, prm, clamp,
                                         AccumulateIo{records, halves, history, history_halves, history_length, motion, out, halves_out, length_out, rgba8_out}));
    const size_t n = (size_t)camera->width * camera->height;
    const StageArg args[10] = {stage_input(records, 32 * n), stage_input(halves, 64 * n), stage_input(history, 32 * n), stage_input(history_halves, 64 * n),
                               stage_input(history_length, 4 * n), stage_input(motion, 12 * n), stage_output(out, 32 * n), stage_output(halves_out, 64 * n),
                               stage_output(length_out, 4 * n), stage_output(rgba8_out, 4 * n)};
    return record_call(s, fn, false, {}, nullptr, [&] {
        return staged_host_call(s->record_stage.buf, args, [&](void* const* d) {
            const AccumulateIo dev{(const rr_radiance*)d[0], (const rr_radiance*)d[1], (const rr_radiance*)d[2], (const rr_radiance*)d[3], (const float*)d[4],
                                   (const float*)d[5], (rr_radiance*)d[6], (rr_radiance*)d[7], (float*)d[8], (uint8_t*)d[9]};
            return accumulate_clamped_locked(s, camera, prm, clamp, dev, nullptr);
        });
    });
} RR_GUARD_END("rr_accumulate_clamped_records")

// ---- rr_accumulate_clamped_split_records: the split call with the colour history held to the box of the current colours and the diffuse
// history to the box of the current diffuse layer
// what it checks: the union of the split call's and the clamped call's rules, with `out` allowed nowhere on `records` and `diffuse_out`
// nowhere on `diffuse` (both windows read other pixels, which another workgroup may already have overwritten)
static int check_accumulate_clamped_split_args(const char* fn, bool device, const rr_scene* s, const rr_camera* cam, const rr_accumulate_params* prm,
                                               const rr_history_clamp_params* clamp, const AccumulateIo& io, const TpSplitIo& d) {
    RR_TRY(check_accumulate_basics(fn, device, s, cam, prm, io));
    if (!clamp) return fail(RR_ERR_INVALID_ARGUMENT, "%s: clamp is NULL", fn);
    if (clamp->struct_size != sizeof(rr_history_clamp_params))
        return fail(RR_ERR_INVALID_ARGUMENT, "%s: clamp->struct_size %u, expected %u", fn, clamp->struct_size, (unsigned)sizeof(rr_history_clamp_params));
    if (clamp->radius != 1u && clamp->radius != 2u) return fail(RR_ERR_INVALID_ARGUMENT, "%s: clamp->radius %u, must be 1 or 2", fn, clamp->radius);
    if (!(clamp->sigma_scale >= 0.0f && clamp->sigma_scale <= 65536.0f)) return fail(RR_ERR_INVALID_ARGUMENT, "%s: clamp->sigma_scale must lie in 0 .. 65536", fn);
    if (!d.diffuse) return fail(RR_ERR_INVALID_ARGUMENT, "%s: diffuse is NULL", fn);
    if (!d.diffuse_out) return fail(RR_ERR_INVALID_ARGUMENT, "%s: diffuse_out is NULL", fn);
    if ((d.dif_halves != nullptr) != (io.halves != nullptr)) return fail(RR_ERR_INVALID_ARGUMENT, "%s: diffuse_halves is required exactly when halves is given", fn);
    if ((d.dif_halves_out != nullptr) != (io.halves != nullptr)) return fail(RR_ERR_INVALID_ARGUMENT, "%s: diffuse_halves_out is required exactly when halves is given", fn);
    if ((d.history_diffuse != nullptr) != (io.history != nullptr)) return fail(RR_ERR_INVALID_ARGUMENT, "%s: history_diffuse is required exactly when history is given", fn);
    if ((d.history_dif_halves != nullptr) != (io.history_halves != nullptr))
        return fail(RR_ERR_INVALID_ARGUMENT, "%s: history_diffuse_halves is required exactly when history_halves is given", fn);
    if (device && (((uintptr_t)d.diffuse | (uintptr_t)d.dif_halves | (uintptr_t)d.history_diffuse | (uintptr_t)d.history_dif_halves | (uintptr_t)d.diffuse_out |
                    (uintptr_t)d.dif_halves_out) & 3u))
        return fail(RR_ERR_INVALID_ARGUMENT, "%s: diffuse_dev, diffuse_halves_dev, history_diffuse_dev, history_diffuse_halves_dev, diffuse_out_dev and diffuse_halves_out_dev must be 4-byte aligned", fn);
    const uint64_t n = (uint64_t)cam->width * cam->height;
    const ArgRange t[16] = {{io.records, 32u * n, "records", false, -1}, {io.halves, 64u * n, "halves", false, -1}, {d.diffuse, 12u * n, "diffuse", false, -1},
                            {d.dif_halves, 24u * n, "diffuse_halves", false, -1}, {io.history, 32u * n, "history", false, -1},
                            {io.history_halves, 64u * n, "history_halves", false, -1}, {d.history_diffuse, 12u * n, "history_diffuse", false, -1},
                            {d.history_dif_halves, 24u * n, "history_diffuse_halves", false, -1}, {io.history_length, 4u * n, "history_length", false, -1},
                            {io.motion, 12u * n, "motion", false, -1}, {io.out, 32u * n, "out", true, -1}, {io.halves_out, 64u * n, "halves_out", true, 1},
                            {d.diffuse_out, 12u * n, "diffuse_out", true, -1}, {d.dif_halves_out, 24u * n, "diffuse_halves_out", true, 3},
                            {io.length_out, 4u * n, "length_out", true, -1}, {io.rgba8, 4u * n, "rgba8_out", true, -1}};
    return check_arg_ranges(fn, t, 16, false,
                            " (the windows read the records and the diffuse of other pixels, so out may not be records and diffuse_out may not be diffuse; only "
                            "halves_out == halves and diffuse_halves_out == diffuse_halves, in place, are allowed)");
}

static int accumulate_clamped_split_locked(rr_scene* s, const rr_camera* cam, const rr_accumulate_params* prm, const rr_history_clamp_params* clamp,
                                           const AccumulateIo& io, const TpSplitIo& split, hipStream_t st) {
    const uint32_t W = cam->width, H = cam->height;
    const TpFrame f = accumulate_frame(cam, prm);
    const dim3 grid = accumulate_grid(cam), block(RR_BLOCK);
    const float k = clamp->sigma_scale;
    const float4 *rec = (const float4*)io.records, *hv = (const float4*)io.halves, *hist = (const float4*)io.history, *hist_h = (const float4*)io.history_halves;
    float4 *out = (float4*)io.out, *out_h = (float4*)io.halves_out;
    if (io.halves && clamp->radius == 1u)
        hipLaunchKernelGGL((k_accumulate_clamped_split_records<true, 1>), grid, block, 0, st, f, k, rec, hv, hist, hist_h, io.history_length, io.motion, out, out_h,
                           io.length_out, split);
    else if (io.halves)
        hipLaunchKernelGGL((k_accumulate_clamped_split_records<true, 2>), grid, block, 0, st, f, k, rec, hv, hist, hist_h, io.history_length, io.motion, out, out_h,
                           io.length_out, split);
    else if (clamp->radius == 1u)
        hipLaunchKernelGGL((k_accumulate_clamped_split_records<false, 1>), grid, block, 0, st, f, k, rec, (const float4*)nullptr, hist, (const float4*)nullptr,
                           io.history_length, io.motion, out, (float4*)nullptr, io.length_out, split);
    else
        hipLaunchKernelGGL((k_accumulate_clamped_split_records<false, 2>), grid, block, 0, st, f, k, rec, (const float4*)nullptr, hist, (const float4*)nullptr,
                           io.history_length, io.motion, out, (float4*)nullptr, io.length_out, split);
    if (io.rgba8) {
        rr_config cfg{};
        cfg.gamma_correction = prm->gamma_correction ? 1 : 0;
        launch_record_bytes(s, &cfg, io.out, W * H, io.rgba8, st);
    }
    if (hipGetLastError() != hipSuccess) return fail(RR_ERR_DEVICE, "rr_accumulate_clamped_split_records: a launch failed");
    return RR_OK;
}

int rr_accumulate_clamped_split_records_device(rr_scene* s, const rr_camera* camera, const rr_accumulate_params* prm, const rr_history_clamp_params* clamp,
                                               const rr_radiance* records, const rr_radiance* halves, const float* diffuse, const float* diffuse_halves,
                                               const rr_radiance* history, const rr_radiance* history_halves, const float* history_diffuse,
                                               const float* history_diffuse_halves, const float* history_length, const float* motion, rr_radiance* out,
                                               rr_radiance* halves_out, float* diffuse_out, float* diffuse_halves_out, float* length_out, uint8_t* rgba8_out,
                                               void* hip_stream) try {
    const char* fn = "rr_accumulate_clamped_split_records_device";
    const AccumulateIo io{records, halves, history, history_halves, history_length, motion, out, halves_out, length_out, rgba8_out};
    const TpSplitIo split{diffuse, diffuse_halves, history_diffuse, history_diffuse_halves, diffuse_out, diffuse_halves_out};
    RR_TRY(check_accumulate_clamped_split_args(fn, true, s, camera, prm, clamp, io, split));
    const hipStream_t st = (hipStream_t)hip_stream;
    return record_call(s, fn, false, {{records, "records_dev"}, {halves, "halves_dev"}, {diffuse, "diffuse_dev"}, {diffuse_halves, "diffuse_halves_dev"},
                                      {history, "history_dev"}, {history_halves, "history_halves_dev"}, {history_diffuse, "history_diffuse_dev"},
                                      {history_diffuse_halves, "history_diffuse_halves_dev"}, {history_length, "history_length_dev"}, {motion, "motion_dev"},
                                      {out, "out_dev"}, {halves_out, "halves_out_dev"}, {diffuse_out, "diffuse_out_dev"}, {diffuse_halves_out, "diffuse_halves_out_dev"},
                                      {length_out, "length_out_dev"}, {rgba8_out, "rgba8_out_dev"}}, st,
                       [&] { return accumulate_clamped_split_locked(s, camera, prm, clamp, io, split, st); });
} RR_GUARD_END("rr_accumulate_clamped_split_records_device")

int rr_accumulate_clamped_split_records(rr_scene* s, const rr_camera* camera, const rr_accumulate_params* prm, const rr_history_clamp_params* clamp,
                                        const rr_radiance* records, const rr_radiance* halves, const float* diffuse, const float* diffuse_halves,
                                        const rr_radiance* history, const rr_radiance* history_halves, const float* history_diffuse, const float* history_diffuse_halves,
                                        const float* history_length, const float* motion, rr_radiance* out, rr_radiance* halves_out, float* diffuse_out,
                                        float* diffuse_halves_out, float* length_out, uint8_t* rgba8_out) try {
    const char* fn = "rr_accumulate_clamped_split_records";
    RR_TRY(check_accumulate_clamped_split_args(fn, false, s, camera, prm, clamp,
                                               AccumulateIo{records, halves, history, history_halves, history_length, motion, out, halves_out, length_out, rgba8_out},
                                               TpSplitIo{diffuse, diffuse_halves, history_diffuse, history_diffuse_halves, diffuse_out, diffuse_halves_out}));
    const size_t n = (size_t)camera->width * camera->height;
    const StageArg args[16] = {stage_input(records, 32 * n), stage_input(halves, 64 * n), stage_input(diffuse, 12 * n), stage_input(diffuse_halves, 24 * n),
                               stage_input(history, 32 * n), stage_input(history_halves, 64 * n), stage_input(history_diffuse, 12 * n),
                               stage_input(history_diffuse_halves, 24 * n), stage_input(history_length, 4 * n), stage_input(motion, 12 * n),
                               stage_output(out, 32 * n), stage_output(halves_out, 64 * n), stage_output(diffuse_out, 12 * n), stage_output(diffuse_halves_out, 24 * n),
                               stage_output(length_out, 4 * n), stage_output(rgba8_out, 4 * n)};
    return record_call(s, fn, false, {}, nullptr, [&] {
        return staged_host_call(s->record_stage.buf, args, [&](void* const* d) {
            const AccumulateIo dev{(const rr_radiance*)d[0], (const rr_radiance*)d[1], (const rr_radiance*)d[4], (const rr_radiance*)d[5], (const float*)d[8],
                                   (const float*)d[9], (rr_radiance*)d[10], (rr_radiance*)d[11], (float*)d[14], (uint8_t*)d[15]};
            const TpSplitIo split{(const float*)d[2], (const float*)d[3], (const float*)d[6], (const float*)d[7], (float*)d[12], (float*)d[13]};
            return accumulate_clamped_split_locked(s, camera, prm, clamp, dev, split, nullptr);
        });
    });
} RR_GUARD_END("rr_accumulate_clamped_split_records")
