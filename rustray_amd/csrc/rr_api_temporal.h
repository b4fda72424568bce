// rr_api_temporal.h — temporal reprojection of a frame of records on the device: the previous call's result is gathered into the
// current frame and the current records are blended into it, the step before rr_denoise_records in a frame-after-frame loop.
// Offers: rr_accumulate_default_params, rr_accumulate_records_device, rr_accumulate_records.
// Needs:  rr_api_query.h (check_query_pointers), rr_api_frame.h (take_stream, IdleOnExit), rr_api_adaptive.h (launch_record_bytes),
//         rr_temporal.h, kernel 7e of rr_kernels.hip.
//
// The call is ONE launch of k_accumulate_records (with or without halves) and, for the bytes, k_record_bytes, on the caller's stream,
// not waited for.  It keeps no working data.  The host form is the device form behind staging copies (TemporalState::stage).

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

// what both forms check before the scene is looked at; `device`: the alignment rule of the device form
static int check_accumulate_args(const char* fn, bool device, const rr_scene* s, const rr_camera* cam, const rr_accumulate_params* prm, const AccumulateIo& io) {
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
    // overlaps: an output with an input or with another output; out == records and halves_out == halves exactly are the in-place call
    const uint64_t n = (uint64_t)width * height;
    struct Range { const void* p; uint64_t bytes; const char* name; };
    const Range in[6] = {{io.records, 32u * n, "records"}, {io.halves, 64u * n, "halves"}, {io.history, 32u * n, "history"},
                         {io.history_halves, 64u * n, "history_halves"}, {io.history_length, 4u * n, "history_length"}, {io.motion, 12u * n, "motion"}};
    const Range outs[4] = {{io.out, 32u * n, "out"}, {io.halves_out, 64u * n, "halves_out"}, {io.length_out, 4u * n, "length_out"}, {io.rgba8, 4u * n, "rgba8_out"}};
    auto overlap = [](const Range& a, const Range& b) {
        return a.p && b.p && (uintptr_t)a.p < (uintptr_t)b.p + b.bytes && (uintptr_t)b.p < (uintptr_t)a.p + a.bytes;
    };
    for (int o = 0; o < 4; o++) {
        for (int i = 0; i < 6; i++) {
            const bool in_place = (o == 0 && i == 0 && io.out == io.records) || (o == 1 && i == 1 && io.halves_out == io.halves);
            if (overlap(outs[o], in[i]) && !in_place)
                return fail(RR_ERR_INVALID_ARGUMENT, "%s: %s overlaps %s (only out == records and halves_out == halves, in place, are allowed)", fn, outs[o].name,
                            in[i].name);
        }
        for (int o2 = o + 1; o2 < 4; o2++)
            if (overlap(outs[o], outs[o2])) return fail(RR_ERR_INVALID_ARGUMENT, "%s: %s overlaps %s", fn, outs[o].name, outs[o2].name);
    }
    return RR_OK;
}

// the launches of one call on stream st, on buffers the device can address; the caller holds the lock and has taken the stream
static int accumulate_locked(rr_scene* s, const rr_camera* cam, const rr_accumulate_params* prm, const AccumulateIo& io, hipStream_t st) {
    const uint32_t W = cam->width, H = cam->height;
    TpFrame f{};
    memcpy(f.proj_inv, cam->projection_inverse, sizeof f.proj_inv);
    memcpy(f.view_inv, cam->view_inverse, sizeof f.view_inv);
    memcpy(f.prev_clip, prm->prev_world_to_clip, sizeof f.prev_clip);
    memcpy(f.prev_eye, prm->prev_eye, sizeof f.prev_eye);
    f.w = (float)W; f.h = (float)H;
    f.max_history = prm->max_history; f.normal_min = prm->normal_min; f.sigma_depth = prm->sigma_depth; f.snap = prm->snap;
    f.width = (int)W; f.height = (int)H;
    const dim3 grid((W + DN_TILE_W - 1) / DN_TILE_W, (H + DN_TILE_H - 1) / DN_TILE_H), block(RR_BLOCK);
    if (io.halves)
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
    const AccumulateIo io{records, halves, history, history_halves, history_length, motion, out, halves_out, length_out, rgba8_out};
    RR_TRY(check_accumulate_args("rr_accumulate_records_device", true, s, camera, prm, io));
    RR_TRY(not_in_pass(s, "rr_accumulate_records_device"));
    std::lock_guard<std::mutex> lk(s->mu);
    HIP_TRY(hipSetDevice(s->device));
    RR_TRY(check_query_pointers(s, "rr_accumulate_records_device", {{records, "records_dev"}, {halves, "halves_dev"}, {history, "history_dev"},
                                                                     {history_halves, "history_halves_dev"}, {history_length, "history_length_dev"},
                                                                     {motion, "motion_dev"}, {out, "out_dev"}, {halves_out, "halves_out_dev"},
                                                                     {length_out, "length_out_dev"}, {rgba8_out, "rgba8_out_dev"}}));
    const hipStream_t st = (hipStream_t)hip_stream;
    RR_TRY(take_stream(s, st));
    IdleOnExit idle(st);
    return idle.done(accumulate_locked(s, camera, prm, io, st));
} RR_GUARD_END("rr_accumulate_records_device")

int rr_accumulate_records(rr_scene* s, const rr_camera* camera, const rr_accumulate_params* prm, const rr_radiance* records, const rr_radiance* halves,
                          const rr_radiance* history, const rr_radiance* history_halves, const float* history_length, const float* motion, rr_radiance* out,
                          rr_radiance* halves_out, float* length_out, uint8_t* rgba8_out) try {
    const AccumulateIo host{records, halves, history, history_halves, history_length, motion, out, halves_out, length_out, rgba8_out};
    RR_TRY(check_accumulate_args("rr_accumulate_records", false, s, camera, prm, host));
    RR_TRY(not_in_pass(s, "rr_accumulate_records"));
    std::lock_guard<std::mutex> lk(s->mu);
    HIP_TRY(hipSetDevice(s->device));
    RR_TRY(take_stream(s, nullptr));
    IdleOnExit idle(nullptr);
    // the staging is the handle's (TemporalState::stage: grown, kept, used by the host form only, which returns with the stream idle):
    // 0 records 32 B, 1 halves 64, 2 history 32, 3 history_halves 64, 4 history_length 4, 5 motion 12, 6 out 32, 7 halves_out 64,
    // 8 length_out 4, 9 rgba8_out 4 per pixel, each only where the call has it
    const size_t n = (size_t)camera->width * camera->height;
    DevBuf* g = s->temporal.stage;
    const void* src[6] = {records, halves, history, history_halves, history_length, motion};
    void* dst[4] = {out, halves_out, length_out, rgba8_out};
    const size_t per_pixel[10] = {32, 64, 32, 64, 4, 12, 32, 64, 4, 4};
    for (int k = 0; k < 10; k++)
        if (k < 6 ? src[k] != nullptr : dst[k - 6] != nullptr) HIP_TRY(g[k].reserve(per_pixel[k] * n));
    for (int k = 0; k < 6; k++)
        if (src[k]) HIP_TRY(hipMemcpyAsync(g[k].p, src[k], per_pixel[k] * n, hipMemcpyHostToDevice, nullptr));
    const AccumulateIo dev{g[0].as<rr_radiance>(), halves ? g[1].as<rr_radiance>() : nullptr, history ? g[2].as<rr_radiance>() : nullptr,
                           history_halves ? g[3].as<rr_radiance>() : nullptr, history_length ? g[4].as<float>() : nullptr, motion ? g[5].as<float>() : nullptr,
                           g[6].as<rr_radiance>(), halves_out ? g[7].as<rr_radiance>() : nullptr, g[8].as<float>(), rgba8_out ? g[9].as<uint8_t>() : nullptr};
    RR_TRY(accumulate_locked(s, camera, prm, dev, nullptr));
    for (int k = 6; k < 10; k++)
        if (dst[k - 6]) HIP_TRY(hipMemcpyAsync(dst[k - 6], g[k].p, per_pixel[k] * n, hipMemcpyDeviceToHost, nullptr));
    HIP_TRY(hipStreamSynchronize(nullptr));
    return idle.done(RR_OK);
} RR_GUARD_END("rr_accumulate_records")
