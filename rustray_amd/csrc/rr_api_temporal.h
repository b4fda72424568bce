// rr_api_temporal.h — temporal reprojection of a frame of records on the device: the previous call's result is gathered into the
// current frame and the current records are blended into it, the step before rr_denoise_records in a frame-after-frame loop.
// Offers: rr_accumulate_default_params, rr_accumulate_records_device, rr_accumulate_records, rr_accumulate_split_records_device,
//         rr_accumulate_split_records, rr_history_clamp_default_params, rr_accumulate_clamped_records_device,
//         rr_accumulate_clamped_records, rr_accumulate_clamped_split_records_device, rr_accumulate_clamped_split_records; tp_frame (for
//         rr_api_motion.h).
// Needs:  rr_api_query.h (check_arg_ranges, record_call, staged_host_call), rr_api_adaptive.h (launch_record_bytes), rr_temporal.h,
//         rr_history_clamp.h, kernels 7e, 7e', 7e'' and 7e''' of rr_kernels.hip.
//
// The four calls are ONE path, accumulate_call: the sixteen buffers of the split calls (the diffuse six NULL in the others) as one
// table of rows, from which the range check, the alignment tests, the device pointers' check and the staging are read off.  A call is
// ONE launch of k_accumulate_records (the split call: of k_accumulate_split_records; the clamped calls: of k_accumulate_clamped_records
// and k_accumulate_clamped_split_records), with or without halves, and, for the bytes, k_record_bytes, on the caller's stream, not waited
// for.  It keeps no working data.  The host form is the device form behind the staging of every record call (staged_host_call, in the
// handle's pool).  The clamped calls differ in that `out` is allowed nowhere on `records` and `diffuse_out` nowhere on `diffuse` (the
// windows read other pixels, which another workgroup may already have overwritten), and in the clamp's own parameters.

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

int rr_history_clamp_default_params(rr_history_clamp_params* out) try {
    if (!out) return fail(RR_ERR_INVALID_ARGUMENT, "rr_history_clamp_default_params: out is NULL");
    memset(out, 0, sizeof *out);
    out->struct_size = (uint32_t)sizeof(rr_history_clamp_params);
    out->radius = 1u;        // chosen by measurement: DESIGN.md section 8, item 24
    out->sigma_scale = 0.5f;
    return RR_OK;
} RR_GUARD_END("rr_history_clamp_default_params")

// the buffers of a call, in the order of the split calls' arguments
struct AccumulateIo {
    const rr_radiance* records; const rr_radiance* halves; const float* diffuse; const float* dif_halves;
    const rr_radiance* history; const rr_radiance* history_halves; const float* history_diffuse; const float* history_dif_halves;
    const float* history_length; const float* motion;
    rr_radiance* out; rr_radiance* halves_out; float* diffuse_out; float* dif_halves_out; float* length_out; uint8_t* rgba8;
};
enum { ACC_ROWS = 16 };
static_assert(sizeof(AccumulateIo) == ACC_ROWS * sizeof(void*), "AccumulateIo is sixteen pointers: the staged call fills it from its sixteen device copies");

// one buffer of a call: row k is member k of AccumulateIo.  in_place_partner: as ArgRange's.  `diffuse`: one of the six of the split calls.
struct AccumulateRow {
    const void* p; uint32_t bytes_per_pixel; const char* name; const char* dev_name; bool is_output; int in_place_partner; uint32_t align; bool diffuse;
};
struct AccumulateRows { AccumulateRow r[ACC_ROWS]; };
#define ACC_ROW(member, bytes, name, is_output, partner, align, diffuse) {io.member, bytes, name, name "_dev", is_output, partner, align, diffuse}
static AccumulateRows accumulate_rows(const AccumulateIo& io, bool clamped) {
    return AccumulateRows{{ACC_ROW(records, 32, "records", false, -1, 16, false), ACC_ROW(halves, 64, "halves", false, -1, 16, false),
                           ACC_ROW(diffuse, 12, "diffuse", false, -1, 4, true), ACC_ROW(dif_halves, 24, "diffuse_halves", false, -1, 4, true),
                           ACC_ROW(history, 32, "history", false, -1, 16, false), ACC_ROW(history_halves, 64, "history_halves", false, -1, 16, false),
                           ACC_ROW(history_diffuse, 12, "history_diffuse", false, -1, 4, true),
                           ACC_ROW(history_dif_halves, 24, "history_diffuse_halves", false, -1, 4, true),
                           ACC_ROW(history_length, 4, "history_length", false, -1, 4, false), ACC_ROW(motion, 12, "motion", false, -1, 4, false),
                           ACC_ROW(out, 32, "out", true, clamped ? -1 : 0, 16, false), ACC_ROW(halves_out, 64, "halves_out", true, 1, 16, false),
                           ACC_ROW(diffuse_out, 12, "diffuse_out", true, clamped ? -1 : 2, 4, true),
                           ACC_ROW(dif_halves_out, 24, "diffuse_halves_out", true, 3, 4, true), ACC_ROW(length_out, 4, "length_out", true, -1, 4, false),
                           ACC_ROW(rgba8, 4, "rgba8_out", true, -1, 4, false)}};
}
#undef ACC_ROW

// the alignment rule of the device form for one group of rows: "<a>_dev, <b>_dev and <c>_dev must be N-byte aligned"
static int check_accumulate_alignment(const char* fn, const AccumulateRows& t, uint32_t align, bool diffuse) {
    uintptr_t bits = 0;
    int left = 0;
    for (const AccumulateRow& r : t.r)
        if (r.align == align && r.diffuse == diffuse) { bits |= (uintptr_t)r.p; left++; }
    if (!(bits & (align - 1u))) return RR_OK;
    std::string names;
    for (const AccumulateRow& r : t.r)
        if (r.align == align && r.diffuse == diffuse) {
            names += r.dev_name;
            if (--left) names += left == 1 ? " and " : ", ";
        }
    return fail(RR_ERR_INVALID_ARGUMENT, "%s: %s must be %u-byte aligned", fn, names.c_str(), align);
}

// what both forms of the four calls check before the scene is looked at, in this order: the basics, the clamp's parameters, what the
// split call needs, the overlaps.  `device`: the alignment rules of the device form
static int check_accumulate_args(const char* fn, bool device, const rr_scene* s, const rr_camera* cam, const rr_accumulate_params* prm, bool clamped,
                                 const rr_history_clamp_params* clamp, bool split, const AccumulateIo& io, const AccumulateRows& t) {
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
    if (device) {
        RR_TRY(check_accumulate_alignment(fn, t, 16u, false));
        RR_TRY(check_accumulate_alignment(fn, t, 4u, false));
    }
    if (clamped) {
        if (!clamp) return fail(RR_ERR_INVALID_ARGUMENT, "%s: clamp is NULL", fn);
        if (clamp->struct_size != sizeof(rr_history_clamp_params))
            return fail(RR_ERR_INVALID_ARGUMENT, "%s: clamp->struct_size %u, expected %u", fn, clamp->struct_size, (unsigned)sizeof(rr_history_clamp_params));
        if (clamp->radius != 1u && clamp->radius != 2u) return fail(RR_ERR_INVALID_ARGUMENT, "%s: clamp->radius %u, must be 1 or 2", fn, clamp->radius);
        if (!(clamp->sigma_scale >= 0.0f && clamp->sigma_scale <= 65536.0f)) return fail(RR_ERR_INVALID_ARGUMENT, "%s: clamp->sigma_scale must lie in 0 .. 65536", fn);
    }
    if (split) {
        if (!io.diffuse) return fail(RR_ERR_INVALID_ARGUMENT, "%s: diffuse is NULL", fn);
        if (!io.diffuse_out) return fail(RR_ERR_INVALID_ARGUMENT, "%s: diffuse_out is NULL", fn);
        if ((io.dif_halves != nullptr) != (io.halves != nullptr)) return fail(RR_ERR_INVALID_ARGUMENT, "%s: diffuse_halves is required exactly when halves is given", fn);
        if ((io.dif_halves_out != nullptr) != (io.halves != nullptr)) return fail(RR_ERR_INVALID_ARGUMENT, "%s: diffuse_halves_out is required exactly when halves is given", fn);
        if ((io.history_diffuse != nullptr) != (io.history != nullptr)) return fail(RR_ERR_INVALID_ARGUMENT, "%s: history_diffuse is required exactly when history is given", fn);
        if ((io.history_dif_halves != nullptr) != (io.history_halves != nullptr))
            return fail(RR_ERR_INVALID_ARGUMENT, "%s: history_diffuse_halves is required exactly when history_halves is given", fn);
        if (device) RR_TRY(check_accumulate_alignment(fn, t, 4u, true));
    }
    // overlaps: an output with an input or with another output; an output and its in-place partner exactly equal are the in-place call
    static const char* const tail[2][2] = {
        {" (only out == records and halves_out == halves, in place, are allowed)",
         " (only out == records, halves_out == halves, diffuse_out == diffuse and diffuse_halves_out == diffuse_halves, in place, are allowed)"},
        {" (the window reads the records of other pixels, so out may not be records; only halves_out == halves, in place, is allowed)",
         " (the windows read the records and the diffuse of other pixels, so out may not be records and diffuse_out may not be diffuse; only "
         "halves_out == halves and diffuse_halves_out == diffuse_halves, in place, are allowed)"}};
    const uint64_t n = (uint64_t)width * height;
    ArgRange ranges[ACC_ROWS];
    for (int k = 0; k < ACC_ROWS; k++) ranges[k] = ArgRange{t.r[k].p, t.r[k].bytes_per_pixel * n, t.r[k].name, t.r[k].is_output, t.r[k].in_place_partner};
    return check_arg_ranges(fn, ranges, ACC_ROWS, false, tail[clamped][split]);
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

// the launches of one call on stream st, on buffers the device can address; the caller holds the lock and has taken the stream.
// clamp: of the clamped calls, else NULL; split: the kernel with the diffuse layers.  One of the twelve builds by (halves, split, radius).
static int accumulate_locked(const char* fn, rr_scene* s, const rr_camera* cam, const rr_accumulate_params* prm, const rr_history_clamp_params* clamp, bool split,
                             const AccumulateIo& io, hipStream_t st) {
    TpFrame f = tp_frame(cam); // and the previous view and the scalars of the call
    memcpy(f.prev_clip, prm->prev_world_to_clip, sizeof f.prev_clip);
    memcpy(f.prev_eye, prm->prev_eye, sizeof f.prev_eye);
    f.max_history = prm->max_history; f.normal_min = prm->normal_min; f.sigma_depth = prm->sigma_depth; f.snap = prm->snap;
    const dim3 grid((cam->width + DN_TILE_W - 1) / DN_TILE_W, (cam->height + DN_TILE_H - 1) / DN_TILE_H), block(RR_BLOCK); // 32x8 tiles
    const TpSplitIo sp{io.diffuse, io.dif_halves, io.history_diffuse, io.history_dif_halves, io.diffuse_out, io.dif_halves_out};
    const bool hv = io.halves != nullptr, r1 = clamp && clamp->radius == 1u;
    // (a call without halves has checked that history_halves and halves_out are NULL too)
#define ACC_BUFFERS                                                                                                                                              \
    (const float4*)io.records, (const float4*)io.halves, (const float4*)io.history, (const float4*)io.history_halves, io.history_length, io.motion, (float4*)io.out, \
        (float4*)io.halves_out, io.length_out
    if (!clamp && !split) {
        const auto k = hv ? k_accumulate_records<true> : k_accumulate_records<false>;
        hipLaunchKernelGGL(k, grid, block, 0, st, f, ACC_BUFFERS);
    } else if (!clamp) {
        const auto k = hv ? k_accumulate_split_records<true> : k_accumulate_split_records<false>;
        hipLaunchKernelGGL(k, grid, block, 0, st, f, ACC_BUFFERS, sp);
    } else if (!split) {
        const auto k = hv ? (r1 ? k_accumulate_clamped_records<true, 1> : k_accumulate_clamped_records<true, 2>)
                          : (r1 ? k_accumulate_clamped_records<false, 1> : k_accumulate_clamped_records<false, 2>);
        hipLaunchKernelGGL(k, grid, block, 0, st, f, clamp->sigma_scale, ACC_BUFFERS);
    } else {
        const auto k = hv ? (r1 ? k_accumulate_clamped_split_records<true, 1> : k_accumulate_clamped_split_records<true, 2>)
                          : (r1 ? k_accumulate_clamped_split_records<false, 1> : k_accumulate_clamped_split_records<false, 2>);
        hipLaunchKernelGGL(k, grid, block, 0, st, f, clamp->sigma_scale, ACC_BUFFERS, sp);
    }
#undef ACC_BUFFERS
    if (io.rgba8) {
        rr_config cfg{};
        cfg.gamma_correction = prm->gamma_correction ? 1 : 0;
        launch_record_bytes(s, &cfg, io.out, cam->width * cam->height, io.rgba8, st);
    }
    if (hipGetLastError() != hipSuccess) return fail(RR_ERR_DEVICE, "%s: a launch failed", fn);
    return RR_OK;
}

// THE call: the checks, then the device form on the caller's buffers, or the host form on their staged copies (device copy k is member k
// of the AccumulateIo the launches get)
static int accumulate_call(const char* fn, bool device, rr_scene* s, const rr_camera* cam, const rr_accumulate_params* prm, bool clamped,
                           const rr_history_clamp_params* clamp, bool split, const AccumulateIo& io, hipStream_t st) {
    const AccumulateRows t = accumulate_rows(io, clamped);
    RR_TRY(check_accumulate_args(fn, device, s, cam, prm, clamped, clamp, split, io, t));
    if (device) {
        QueryPointer pointers[ACC_ROWS];
        for (int k = 0; k < ACC_ROWS; k++) pointers[k] = QueryPointer{t.r[k].p, t.r[k].dev_name};
        return record_call(s, fn, false, pointers, ACC_ROWS, st, [] { return (int)RR_OK; }, [&] { return accumulate_locked(fn, s, cam, prm, clamp, split, io, st); });
    }
    const size_t n = (size_t)cam->width * cam->height;
    StageArg args[ACC_ROWS];
    for (int k = 0; k < ACC_ROWS; k++) args[k] = StageArg{const_cast<void*>(t.r[k].p), t.r[k].bytes_per_pixel * n, t.r[k].is_output};
    return record_call(s, fn, false, {}, nullptr, [&] {
        return staged_host_call(s->record_stage.buf, args, [&](void* const* d) {
            AccumulateIo dev;
            memcpy(&dev, d, sizeof dev);
            return accumulate_locked(fn, s, cam, prm, clamp, split, dev, nullptr);
        });
    });
}

int rr_accumulate_records_device(rr_scene* s, const rr_camera* camera, const rr_accumulate_params* prm, const rr_radiance* records, const rr_radiance* halves,
                                 const rr_radiance* history, const rr_radiance* history_halves, const float* history_length, const float* motion,
                                 rr_radiance* out, rr_radiance* halves_out, float* length_out, uint8_t* rgba8_out, void* hip_stream) try {
    return accumulate_call("rr_accumulate_records_device", true, s, camera, prm, false, nullptr, false,
                           AccumulateIo{records, halves, nullptr, nullptr, history, history_halves, nullptr, nullptr, history_length, motion, out, halves_out, nullptr,
                                        nullptr, length_out, rgba8_out}, (hipStream_t)hip_stream);
} RR_GUARD_END("rr_accumulate_records_device")

int rr_accumulate_records(rr_scene* s, const rr_camera* camera, const rr_accumulate_params* prm, const rr_radiance* records, const rr_radiance* halves,
                          const rr_radiance* history, const rr_radiance* history_halves, const float* history_length, const float* motion, rr_radiance* out,
                          rr_radiance* halves_out, float* length_out, uint8_t* rgba8_out) try {
    return accumulate_call("rr_accumulate_records", false, s, camera, prm, false, nullptr, false,
                           AccumulateIo{records, halves, nullptr, nullptr, history, history_halves, nullptr, nullptr, history_length, motion, out, halves_out, nullptr,
                                        nullptr, length_out, rgba8_out}, nullptr);
} RR_GUARD_END("rr_accumulate_records")

// ---- rr_accumulate_split_records: the same call with the diffuse layers of rr_render_pixel_split riding on the taps of the records
int rr_accumulate_split_records_device(rr_scene* s, const rr_camera* camera, const rr_accumulate_params* prm, const rr_radiance* records, const rr_radiance* halves,
                                       const float* diffuse, const float* diffuse_halves, const rr_radiance* history, const rr_radiance* history_halves,
                                       const float* history_diffuse, const float* history_diffuse_halves, const float* history_length, const float* motion,
                                       rr_radiance* out, rr_radiance* halves_out, float* diffuse_out, float* diffuse_halves_out, float* length_out, uint8_t* rgba8_out,
                                       void* hip_stream) try {
    return accumulate_call("rr_accumulate_split_records_device", true, s, camera, prm, false, nullptr, true,
                           AccumulateIo{records, halves, diffuse, diffuse_halves, history, history_halves, history_diffuse, history_diffuse_halves, history_length, motion,
                                        out, halves_out, diffuse_out, diffuse_halves_out, length_out, rgba8_out}, (hipStream_t)hip_stream);
} RR_GUARD_END("rr_accumulate_split_records_device")

int rr_accumulate_split_records(rr_scene* s, const rr_camera* camera, const rr_accumulate_params* prm, const rr_radiance* records, const rr_radiance* halves,
                                const float* diffuse, const float* diffuse_halves, const rr_radiance* history, const rr_radiance* history_halves,
                                const float* history_diffuse, const float* history_diffuse_halves, const float* history_length, const float* motion, rr_radiance* out,
                                rr_radiance* halves_out, float* diffuse_out, float* diffuse_halves_out, float* length_out, uint8_t* rgba8_out) try {
    return accumulate_call("rr_accumulate_split_records", false, s, camera, prm, false, nullptr, true,
                           AccumulateIo{records, halves, diffuse, diffuse_halves, history, history_halves, history_diffuse, history_diffuse_halves, history_length, motion,
                                        out, halves_out, diffuse_out, diffuse_halves_out, length_out, rgba8_out}, nullptr);
} RR_GUARD_END("rr_accumulate_split_records")

// ---- rr_accumulate_clamped_records: the same call with the history held to the box of the current frame's colours around each pixel
int rr_accumulate_clamped_records_device(rr_scene* s, const rr_camera* camera, const rr_accumulate_params* prm, const rr_history_clamp_params* clamp,
                                         const rr_radiance* records, const rr_radiance* halves, const rr_radiance* history, const rr_radiance* history_halves,
                                         const float* history_length, const float* motion, rr_radiance* out, rr_radiance* halves_out, float* length_out,
                                         uint8_t* rgba8_out, void* hip_stream) try {
    return accumulate_call("rr_accumulate_clamped_records_device", true, s, camera, prm, true, clamp, false,
                           AccumulateIo{records, halves, nullptr, nullptr, history, history_halves, nullptr, nullptr, history_length, motion, out, halves_out, nullptr,
                                        nullptr, length_out, rgba8_out}, (hipStream_t)hip_stream);
} RR_GUARD_END("rr_accumulate_clamped_records_device")

int rr_accumulate_clamped_records(rr_scene* s, const rr_camera* camera, const rr_accumulate_params* prm, const rr_history_clamp_params* clamp,
                                  const rr_radiance* records, const rr_radiance* halves, const rr_radiance* history, const rr_radiance* history_halves,
                                  const float* history_length, const float* motion, rr_radiance* out, rr_radiance* halves_out, float* length_out,
                                  uint8_t* rgba8_out) try {
    return accumulate_call("rr_accumulate_clamped_records", false, s, camera, prm, true, clamp, false,
                           AccumulateIo{records, halves, nullptr, nullptr, history, history_halves, nullptr, nullptr, history_length, motion, out, halves_out, nullptr,
                                        nullptr, length_out, rgba8_out}, nullptr);
} RR_GUARD_END("rr_accumulate_clamped_records")

// ---- rr_accumulate_clamped_split_records: the split call with the colour history held to the box of the current colours and the diffuse
// history to the box of the current diffuse layer
int rr_accumulate_clamped_split_records_device(rr_scene* s, const rr_camera* camera, const rr_accumulate_params* prm, const rr_history_clamp_params* clamp,
                                               const rr_radiance* records, const rr_radiance* halves, const float* diffuse, const float* diffuse_halves,
                                               const rr_radiance* history, const rr_radiance* history_halves, const float* history_diffuse,
                                               const float* history_diffuse_halves, const float* history_length, const float* motion, rr_radiance* out,
                                               rr_radiance* halves_out, float* diffuse_out, float* diffuse_halves_out, float* length_out, uint8_t* rgba8_out,
                                               void* hip_stream) try {
    return accumulate_call("rr_accumulate_clamped_split_records_device", true, s, camera, prm, true, clamp, true,
                           AccumulateIo{records, halves, diffuse, diffuse_halves, history, history_halves, history_diffuse, history_diffuse_halves, history_length, motion,
                                        out, halves_out, diffuse_out, diffuse_halves_out, length_out, rgba8_out}, (hipStream_t)hip_stream);
} RR_GUARD_END("rr_accumulate_clamped_split_records_device")

int rr_accumulate_clamped_split_records(rr_scene* s, const rr_camera* camera, const rr_accumulate_params* prm, const rr_history_clamp_params* clamp,
                                        const rr_radiance* records, const rr_radiance* halves, const float* diffuse, const float* diffuse_halves,
                                        const rr_radiance* history, const rr_radiance* history_halves, const float* history_diffuse, const float* history_diffuse_halves,
                                        const float* history_length, const float* motion, rr_radiance* out, rr_radiance* halves_out, float* diffuse_out,
                                        float* diffuse_halves_out, float* length_out, uint8_t* rgba8_out) try {
    return accumulate_call("rr_accumulate_clamped_split_records", false, s, camera, prm, true, clamp, true,
                           AccumulateIo{records, halves, diffuse, diffuse_halves, history, history_halves, history_diffuse, history_diffuse_halves, history_length, motion,
                                        out, halves_out, diffuse_out, diffuse_halves_out, length_out, rgba8_out}, nullptr);
} RR_GUARD_END("rr_accumulate_clamped_split_records")
