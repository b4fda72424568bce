// rr_api_denoise.h — the variance-guided a-trous filter over a frame of records, on the device: what a host does with the records,
// the halves and the albedo the other calls give it, without a trip through host memory.
// Offers: rr_denoise_default_params, rr_denoise_records_device, rr_denoise_records; rr_test_denoise_forms (the tuning hook of the tests
//         and of tools/denoise_time.py); rr_denoise_split_records_device, rr_denoise_split_records (the filter with the albedo applied to
//         the direct diffuse part of the colour alone: two runs of the launches above between two streaming kernels).
// Needs:  rr_api_query.h (check_arg_ranges, record_call, staged_host_call), rr_api_adaptive.h (launch_record_bytes), rr_denoise.h,
//         kernels 7a .. 7d of rr_kernels.hip.
//
// The call is k_denoise_prepare, one pass launch per iteration (step 1, 2, 4, ...), k_denoise_finish and, for the bytes, k_record_bytes:
// all on the caller's stream, none of them waited for.  The working data are the handle's (DenoiseState): two working colours of 16 B,
// the guide of 16 + 8 B: 56 B per pixel of the largest frame so far.  The host form is the device form behind the staging of every
// record call (staged_host_call, in the handle's pool).

// ---- which form of the pass kernel runs a step.  Measured at 1280x720 (profiles/r10_denoise_time.txt; the forms that lost:
// profiles/r10_dropped.txt): steps 1 and 2 through an LDS tile of the frame, steps 4 and 8 as one dense tile per residue class of the
// step's sub-lattice, step 16 gathered from global memory; step 32 was not measured and is gathered like step 16.  The bits are the
// same in every form (tests/test_gpu_denoise.py).
static int denoise_auto_form(int step) { return step <= 2 ? DN_FORM_TILE : step <= 8 ? DN_FORM_LATTICE : DN_FORM_GATHER; }

// The tuning hook: four bits per pass, pass i in bits 4 i .. 4 i + 3: DN_FORM_AUTO (0), DN_FORM_GATHER, DN_FORM_TILE, DN_FORM_LATTICE.  A
// form that does not exist at a pass's step (rr_denoise.h: denoise_form_available) leaves that pass automatic.  Process-wide, read
// once per call; 0 (always, outside the tests and the timing tool) = automatic.
static std::atomic<uint32_t> g_denoise_forms{0u};
extern "C" void rr_test_denoise_forms(uint32_t forms) { g_denoise_forms.store(forms); }
static int denoise_form(uint32_t forms, uint32_t pass_index, int step) {
    const int forced = (int)((forms >> (4u * pass_index)) & 15u);
    return forced != DN_FORM_AUTO && denoise_form_available(forced, step) ? forced : denoise_auto_form(step);
}

int rr_denoise_default_params(rr_denoise_params* out) try {
    if (!out) return fail(RR_ERR_INVALID_ARGUMENT, "rr_denoise_default_params: out is NULL");
    out->struct_size = (uint32_t)sizeof(rr_denoise_params);
    out->iterations = 5u;
    out->normal_power_log2 = 5u;
    out->sigma_depth = 0.05f;
    out->sigma_luminance = 4.0f;
    out->gamma_correction = 0u;
    return RR_OK;
} RR_GUARD_END("rr_denoise_default_params")

struct DenoiseIo {
    const rr_radiance* records; const rr_radiance* halves; const float* albedo;
    rr_radiance* out; uint8_t* rgba8; float* variance;
};

// what both forms check before the scene is looked at; `device`: the alignment rule of the device form
static int check_denoise_args(const char* fn, bool device, const rr_scene* s, uint32_t width, uint32_t height, const rr_denoise_params* prm, const DenoiseIo& io) {
    if (!s) return fail(RR_ERR_INVALID_ARGUMENT, "%s: scene is NULL", fn);
    if (!prm) return fail(RR_ERR_INVALID_ARGUMENT, "%s: params is NULL", fn);
    if (!io.records) return fail(RR_ERR_INVALID_ARGUMENT, "%s: records is NULL", fn);
    if (!io.out) return fail(RR_ERR_INVALID_ARGUMENT, "%s: out is NULL", fn);
    if (width == 0 || height == 0 || width > 65535u || height > 65535u) return fail(RR_ERR_INVALID_ARGUMENT, "%s: bad frame size %ux%u", fn, width, height);
    if (prm->struct_size != sizeof(rr_denoise_params))
        return fail(RR_ERR_INVALID_ARGUMENT, "%s: params->struct_size %u, expected %u", fn, prm->struct_size, (unsigned)sizeof(rr_denoise_params));
    if (prm->iterations == 0 || prm->iterations > RR_MAX_DENOISE_ITERATIONS)
        return fail(RR_ERR_INVALID_ARGUMENT, "%s: iterations %u (1 .. %u)", fn, prm->iterations, RR_MAX_DENOISE_ITERATIONS);
    if (prm->normal_power_log2 > 7u) return fail(RR_ERR_INVALID_ARGUMENT, "%s: normal_power_log2 %u (0 .. 7)", fn, prm->normal_power_log2);
    if (!(prm->sigma_depth > 0.0f) || !denoise_is_finite(prm->sigma_depth)) return fail(RR_ERR_INVALID_ARGUMENT, "%s: sigma_depth must be finite and above 0", fn);
    if (!(prm->sigma_luminance > 0.0f) || !denoise_is_finite(prm->sigma_luminance))
        return fail(RR_ERR_INVALID_ARGUMENT, "%s: sigma_luminance must be finite and above 0", fn);
    if ((uint64_t)width * height * 2u > (1ull << 30))
        return fail(RR_ERR_UNSUPPORTED, "%s: %ux%u pixels x 2 halves are more than 2^30 records", fn, width, height);
    if (device && (((uintptr_t)io.records | (uintptr_t)io.halves | (uintptr_t)io.out) & 15u))
        return fail(RR_ERR_INVALID_ARGUMENT, "%s: records_dev, halves_dev and out_dev must be 16-byte aligned", fn);
    if (device && (((uintptr_t)io.albedo | (uintptr_t)io.rgba8 | (uintptr_t)io.variance) & 3u))
        return fail(RR_ERR_INVALID_ARGUMENT, "%s: albedo_dev, rgba8_out_dev and variance_out_dev must be 4-byte aligned", fn);
    // overlaps: an output with an input or with another output; out == records exactly is the in-place call
    const uint64_t n = (uint64_t)width * height;
    const ArgRange t[6] = {{io.records, 32u * n, "records", false, -1}, {io.halves, 64u * n, "halves", false, -1}, {io.albedo, 12u * n, "albedo", false, -1},
                           {io.out, 32u * n, "out", true, 0}, {io.rgba8, 4u * n, "rgba8_out", true, -1}, {io.variance, 4u * n, "variance_out", true, -1}};
    return check_arg_ranges(fn, t, 6, false, " (only out == records, in place, is allowed)");
}

// the launches of one call on stream st, on buffers the device can address; the caller holds the lock and has taken the stream
static int denoise_locked(rr_scene* s, uint32_t W, uint32_t H, const rr_denoise_params* prm, const DenoiseIo& io, hipStream_t st) {
    const uint64_t N = (uint64_t)W * H;
    DenoiseState& d = s->denoise;
    HIP_TRY(d.work[0].reserve(16ull * N));
    HIP_TRY(d.work[1].reserve(16ull * N));
    HIP_TRY(d.guide.reserve(16ull * N));
    HIP_TRY(d.meta.reserve(8ull * N));
    float4* work[2] = {d.work[0].as<float4>(), d.work[1].as<float4>()};
    const dim3 grid((W + DN_TILE_W - 1) / DN_TILE_W, (H + DN_TILE_H - 1) / DN_TILE_H), block(RR_BLOCK);
    hipLaunchKernelGGL(k_denoise_prepare, grid, block, 0, st, (const float4*)io.records, (const float4*)io.halves, io.albedo, W, H, work[0], d.guide.as<float4>(),
                       d.meta.as<uint2>());
    const uint32_t forms = g_denoise_forms.load();
    int cur = 0;
    for (uint32_t i = 0; i < prm->iterations; i++, cur ^= 1) {
        DnPass pass{prm->sigma_depth, prm->sigma_luminance, prm->normal_power_log2, io.halves ? 1u : 0u, 1 << i};
        const int form = denoise_form(forms, i, pass.step);
        if (form == DN_FORM_GATHER) {
            hipLaunchKernelGGL(k_denoise_pass_gather, grid, block, 0, st, work[cur], d.guide.as<float4>(), d.meta.as<uint2>(), W, H, pass, work[cur ^ 1]);
        } else {
            const int L = form == DN_FORM_LATTICE ? pass.step : 1, halo = 2 * (pass.step / L);
            // the largest residue class has ceil(W / L) x ceil(H / L) lattice points; workgroups of smaller classes beyond theirs return at once
            const uint32_t wl = (W + L - 1) / L, hl = (H + L - 1) / L;
            const dim3 tgrid((wl + DN_TILE_W - 1) / DN_TILE_W, (hl + DN_TILE_H - 1) / DN_TILE_H, (uint32_t)(L * L));
            hipLaunchKernelGGL(k_denoise_pass_tile, tgrid, block, (size_t)(40ull * denoise_tile_entries(halo)), st, work[cur], d.guide.as<float4>(), d.meta.as<uint2>(), W, H,
                               pass, L, work[cur ^ 1]);
        }
    }
    hipLaunchKernelGGL(k_denoise_finish, grid, block, 0, st, (const float4*)io.records, io.albedo, work[cur], d.meta.as<uint2>(), W, H, (float4*)io.out, io.variance);
    if (io.rgba8) {
        rr_config cfg{};
        cfg.gamma_correction = prm->gamma_correction ? 1 : 0;
        launch_record_bytes(s, &cfg, io.out, (uint32_t)N, io.rgba8, st);
    }
    if (hipGetLastError() != hipSuccess) return fail(RR_ERR_DEVICE, "rr_denoise_records: a launch failed");
    return RR_OK;
}

int rr_denoise_records_device(rr_scene* s, uint32_t width, uint32_t height, const rr_denoise_params* prm, const rr_radiance* records, const rr_radiance* halves,
                              const float* albedo, rr_radiance* out, uint8_t* rgba8_out, float* variance_out, void* hip_stream) try {
    const char* fn = "rr_denoise_records_device";
    const DenoiseIo io{records, halves, albedo, out, rgba8_out, variance_out};
    RR_TRY(check_denoise_args(fn, true, s, width, height, prm, io));
    const hipStream_t st = (hipStream_t)hip_stream;
    return record_call(s, fn, false, {{records, "records_dev"}, {halves, "halves_dev"}, {albedo, "albedo_dev"}, {out, "out_dev"}, {rgba8_out, "rgba8_out_dev"},
                                      {variance_out, "variance_out_dev"}}, st, [&] { return denoise_locked(s, width, height, prm, io, st); });
} RR_GUARD_END("rr_denoise_records_device")

int rr_denoise_records(rr_scene* s, uint32_t width, uint32_t height, const rr_denoise_params* prm, const rr_radiance* records, const rr_radiance* halves,
                       const float* albedo, rr_radiance* out, uint8_t* rgba8_out, float* variance_out) try {
    const char* fn = "rr_denoise_records";
    RR_TRY(check_denoise_args(fn, false, s, width, height, prm, DenoiseIo{records, halves, albedo, out, rgba8_out, variance_out}));
    const size_t n = (size_t)width * height;
    const StageArg args[6] = {stage_input(records, 32 * n), stage_input(halves, 64 * n), stage_input(albedo, 12 * n),
                              stage_output(out, 32 * n), stage_output(rgba8_out, 4 * n), stage_output(variance_out, 4 * n)};
    return record_call(s, fn, false, {}, nullptr, [&] {
        return staged_host_call(s->record_stage.buf, args, [&](void* const* d) {
            const DenoiseIo dev{(const rr_radiance*)d[0], (const rr_radiance*)d[1], (const float*)d[2], (rr_radiance*)d[3], (uint8_t*)d[4], (float*)d[5]};
            return denoise_locked(s, width, height, prm, dev, nullptr);
        });
    });
} RR_GUARD_END("rr_denoise_records")

// ---- rr_denoise_split_records: colour = rest + direct diffuse (rr_render_pixel_split); the filter runs on `rest` without an albedo and on the
// direct part with it, and the two results are added.  k_denoise_split_sets makes the two record sets (and their halves) in the handle's
// scratch (DenoiseState::split, 192 B per pixel with halves), denoise_locked runs on each in place, k_denoise_split_sum adds.
struct DenoiseSplitIo {
    const rr_radiance* records; const rr_radiance* halves; const float* diffuse; const float* diffuse_halves; const float* albedo;
    rr_radiance* out; uint8_t* rgba8;
};

static int check_denoise_split_args(const char* fn, bool device, const rr_scene* s, uint32_t width, uint32_t height, const rr_denoise_params* prm,
                                    const DenoiseSplitIo& io) {
    RR_TRY(check_denoise_args(fn, device, s, width, height, prm, DenoiseIo{io.records, io.halves, io.albedo, io.out, io.rgba8, nullptr}));
    if (!io.diffuse) return fail(RR_ERR_INVALID_ARGUMENT, "%s: diffuse is NULL", fn);
    if ((io.halves != nullptr) != (io.diffuse_halves != nullptr))
        return fail(RR_ERR_INVALID_ARGUMENT, "%s: halves and diffuse_halves are given together or not at all", fn);
    if (device && (((uintptr_t)io.diffuse | (uintptr_t)io.diffuse_halves) & 3u))
        return fail(RR_ERR_INVALID_ARGUMENT, "%s: diffuse_dev and diffuse_halves_dev must be 4-byte aligned", fn);
    const uint64_t n = (uint64_t)width * height;
    const ArgRange t[4] = {{io.diffuse, 12u * n, "diffuse", false, -1}, {io.diffuse_halves, 24u * n, "diffuse_halves", false, -1},
                           {io.out, 32u * n, "out", true, -1}, {io.rgba8, 4u * n, "rgba8_out", true, -1}};
    return check_arg_ranges(fn, t, 4, false, "");
}

static int denoise_split_locked(rr_scene* s, uint32_t W, uint32_t H, const rr_denoise_params* prm, const DenoiseSplitIo& io, hipStream_t st) {
    const uint64_t N = (uint64_t)W * H;
    DenoiseState& d = s->denoise;
    HIP_TRY(d.split[0].reserve(32ull * N));
    HIP_TRY(d.split[1].reserve(32ull * N));
    if (io.halves) {
        HIP_TRY(d.split[2].reserve(64ull * N));
        HIP_TRY(d.split[3].reserve(64ull * N));
    }
    rr_radiance* const rest = d.split[0].as<rr_radiance>();
    rr_radiance* const direct = d.split[1].as<rr_radiance>();
    rr_radiance* const rest_h = io.halves ? d.split[2].as<rr_radiance>() : nullptr;
    rr_radiance* const direct_h = io.halves ? d.split[3].as<rr_radiance>() : nullptr;
    const int grid = (int)std::min<uint64_t>((N + RR_BLOCK - 1) / RR_BLOCK, (uint64_t)s->n_cus * 8u);
    hipLaunchKernelGGL(k_denoise_split_sets, dim3(grid), dim3(RR_BLOCK), 0, st, (const float4*)io.records, (const float4*)io.halves, io.diffuse, io.diffuse_halves, (uint32_t)N,
                       (float4*)rest, (float4*)direct, (float4*)rest_h, (float4*)direct_h);
    // the filter's own launches, twice, each in place on its set; neither writes bytes
    rr_denoise_params plain = *prm;
    plain.gamma_correction = 0u;
    RR_TRY(denoise_locked(s, W, H, &plain, DenoiseIo{rest, rest_h, nullptr, rest, nullptr, nullptr}, st));
    RR_TRY(denoise_locked(s, W, H, &plain, DenoiseIo{direct, direct_h, io.albedo, direct, nullptr, nullptr}, st));
    hipLaunchKernelGGL(k_denoise_split_sum, dim3(grid), dim3(RR_BLOCK), 0, st, (const float4*)io.records, (const float4*)rest, (const float4*)direct, (uint32_t)N, (float4*)io.out);
    if (io.rgba8) {
        rr_config cfg{};
        cfg.gamma_correction = prm->gamma_correction ? 1 : 0;
        launch_record_bytes(s, &cfg, io.out, (uint32_t)N, io.rgba8, st);
    }
    if (hipGetLastError() != hipSuccess) return fail(RR_ERR_DEVICE, "rr_denoise_split_records: a launch failed");
    return RR_OK;
}

// (defined under the C linkage of their declarations in include/rustray_hip.h)
int rr_denoise_split_records_device(rr_scene* s, uint32_t width, uint32_t height, const rr_denoise_params* prm, const rr_radiance* records, const rr_radiance* halves,
                                    const float* diffuse, const float* diffuse_halves, const float* albedo, rr_radiance* out, uint8_t* rgba8_out,
                                    void* hip_stream) try {
    const char* fn = "rr_denoise_split_records_device";
    const DenoiseSplitIo io{records, halves, diffuse, diffuse_halves, albedo, out, rgba8_out};
    RR_TRY(check_denoise_split_args(fn, true, s, width, height, prm, io));
    const hipStream_t st = (hipStream_t)hip_stream;
    return record_call(s, fn, false, {{records, "records_dev"}, {halves, "halves_dev"}, {diffuse, "diffuse_dev"}, {diffuse_halves, "diffuse_halves_dev"},
                                      {albedo, "albedo_dev"}, {out, "out_dev"}, {rgba8_out, "rgba8_out_dev"}}, st,
                       [&] { return denoise_split_locked(s, width, height, prm, io, st); });
} RR_GUARD_END("rr_denoise_split_records_device")

int rr_denoise_split_records(rr_scene* s, uint32_t width, uint32_t height, const rr_denoise_params* prm, const rr_radiance* records, const rr_radiance* halves,
                             const float* diffuse, const float* diffuse_halves, const float* albedo, rr_radiance* out, uint8_t* rgba8_out) try {
    const char* fn = "rr_denoise_split_records";
    RR_TRY(check_denoise_split_args(fn, false, s, width, height, prm, DenoiseSplitIo{records, halves, diffuse, diffuse_halves, albedo, out, rgba8_out}));
    const size_t n = (size_t)width * height;
    const StageArg args[7] = {stage_input(records, 32 * n), stage_input(halves, 64 * n), stage_input(diffuse, 12 * n), stage_input(diffuse_halves, 24 * n),
                              stage_input(albedo, 12 * n), stage_output(out, 32 * n), stage_output(rgba8_out, 4 * n)};
    return record_call(s, fn, false, {}, nullptr, [&] {
        return staged_host_call(s->record_stage.buf, args, [&](void* const* d) {
            const DenoiseSplitIo dev{(const rr_radiance*)d[0], (const rr_radiance*)d[1], (const float*)d[2], (const float*)d[3], (const float*)d[4], (rr_radiance*)d[5],
                                     (uint8_t*)d[6]};
            return denoise_split_locked(s, width, height, prm, dev, nullptr);
        });
    });
} RR_GUARD_END("rr_denoise_split_records")
