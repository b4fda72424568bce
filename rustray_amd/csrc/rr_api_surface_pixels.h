// rr_api_surface_pixels.h — the camera's surface per pixel: the G-buffer of the pixel-centre rays and the albedo rr_denoise_records takes.
// Offers: rr_surface_pixels_device, rr_surface_pixels.
// Needs:  rr_api_query.h (check_arg_ranges, record_call, staged_host_call, reserve_query_records, preset_reach, query_grid, QW_*; writes
//         rr_scene::query), rr_api_frame.h (launch_trace_closest, take_stream), rr_api_scene.h (ensure_tlas_reach),
//         rr_pixel_list.h (pixel_ray_reach, pixel_list_first_bad), kernels 5v and 5w of rr_kernels.hip.
// Borrowed from rr_scene::frame: h_count[HC_REACH + 3] (the list form's one wait) and last_stream (take_stream).
//
// The call is the surface query (rr_surface_rays_device) with its rays made on the device: k_pixel_rays fills the handle's query records
// from the camera, launch_trace_closest walks them as it walks k_pack_rays', k_surface_pixels ends them.  The rays' origins are a function
// of the camera alone, so the reach the top level must be padded for is known on the host BEFORE the first launch (pixel_ray_reach): the
// whole-frame form enqueues three launches behind two small memsets and returns -- it waits for nothing unless the top level has to be
// rebuilt for a camera farther out than any before (ensure_tlas_reach), or a query buffer has to grow.  The list form waits once, for the
// 4 bytes of the first index outside the frame, as rr_render_pixels_device does.

struct SurfacePixelsIo { const uint32_t* pixel_xy; rr_surface_hit* out; float* albedo; };

// what both forms check before the scene is looked at, in the order the header states; `device`: the rules of the device form.
// n_pixels == 0 passes: the caller returns RR_OK before it touches anything.
static int check_surface_pixels_args(const char* fn, bool device, const rr_scene* s, const rr_camera* cam, uint32_t n_pixels, const SurfacePixelsIo& io) {
    if (!s || !cam) return fail(RR_ERR_INVALID_ARGUMENT, "NULL argument");
    if (!io.out && !io.albedo) return fail(RR_ERR_INVALID_ARGUMENT, "%s: out and albedo_out are both NULL", fn);
    if (cam->width == 0 || cam->height == 0 || cam->width > 65535u || cam->height > 65535u) return fail(RR_ERR_INVALID_ARGUMENT, "bad frame size %ux%u", cam->width, cam->height);
    if (!finite16(cam->projection_inverse) || !finite16(cam->view_inverse)) return fail(RR_ERR_INVALID_ARGUMENT, "non-finite camera matrix");
    if (n_pixels > 0x7fffff00u) return fail(RR_ERR_UNSUPPORTED, "%s: %u pixels in one call", fn, n_pixels);
    if (n_pixels == 0) return RR_OK;
    if (!io.pixel_xy && (uint64_t)n_pixels != (uint64_t)cam->width * cam->height)
        return fail(RR_ERR_INVALID_ARGUMENT, "%s: %u pixels without a list, the frame of %ux%u has %llu", fn, n_pixels, cam->width, cam->height,
                    (unsigned long long)cam->width * cam->height);
    if (!device) return RR_OK;
    if ((uintptr_t)io.out & 15u) return fail(RR_ERR_INVALID_ARGUMENT, "%s: out_dev is not 16-byte aligned", fn);
    if ((uintptr_t)io.albedo & 3u) return fail(RR_ERR_INVALID_ARGUMENT, "%s: albedo_out_dev is not 4-byte aligned", fn);
    if ((uintptr_t)io.pixel_xy & 3u) return fail(RR_ERR_INVALID_ARGUMENT, "%s: pixel_xy_dev is not 4-byte aligned", fn);
    const ArgRange t[3] = {{io.pixel_xy, 4ull * n_pixels, "pixel_xy_dev", false, -1}, {io.out, 128ull * n_pixels, "out_dev", true, -1},
                           {io.albedo, 12ull * n_pixels, "albedo_out_dev", true, -1}};
    return check_arg_ranges(fn, t, 3, true, "");
}

// One call on buffers the scene's device can address, in stream order (the caller holds the lock).  `trusted`: the list was checked on
// the host (the host form): nothing is read back.
static int surface_pixels_locked(rr_scene* s, const rr_camera* cam, const SurfacePixelsIo& io, uint32_t n, hipStream_t st, bool trusted) {
    const uint32_t W = cam->width, H = cam->height;
    RR_TRY(take_stream(s, st));
    double need[3];
    pixel_ray_reach(cam->projection_inverse, cam->view_inverse, W, H, need);
    for (int c = 0; c < 3; c++)
        if (!std::isfinite(need[c])) need[c] = 0.0; // (no finite origin lies that far out: binary32 has overflowed long before)
    RR_TRY(ensure_tlas_reach(s, need));
    RR_TRY(reserve_query_records(s, n, false));
    if (!io.pixel_xy) HIP_TRY(s->query.ids.reserve(4ull * n)); // slot -> output index of the whole frame
    char* w = s->query.words.as<char>();
    const DRayQueue q{s->query.rec[0].as<float4>(), s->query.rec[1].as<float4>(), s->query.rec[2].as<uint2>(), s->query.rec[3].as<uint4>()};
    uint32_t* target = io.pixel_xy ? nullptr : s->query.ids.as<uint32_t>();
    RR_TRY(preset_reach(s, st)); // (the count and the head zeroed, the first bad index 0xffffffff)
    PixelCam pc;
    memcpy(pc.proj_inv, cam->projection_inverse, sizeof pc.proj_inv);
    memcpy(pc.view_inv, cam->view_inverse, sizeof pc.view_inv);
    uint32_t* first_bad = (uint32_t*)(w + QW_REACH + 12);
    hipLaunchKernelGGL(k_pixel_rays, dim3(query_grid(s, n)), dim3(RR_BLOCK), 0, st, pc, W, H, io.pixel_xy, n, q.r0, q.r1, q.r2, (uint32_t*)(w + QW_COUNT), target, first_bad);
    HIP_TRY(hipGetLastError());
    if (io.pixel_xy && !trusted) { // THE wait of the list form
        uint32_t* h = s->frame.h_count + HC_REACH + 3;
        HIP_TRY(hipMemcpyAsync(h, first_bad, 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        const uint32_t bad = *h;
        if (bad != RR_PIXEL_LIST_OK) {
            uint32_t xy = 0; // (the stream is idle: the entry for the message comes with one more small copy)
            HIP_TRY(hipMemcpy(&xy, io.pixel_xy + bad, 4, hipMemcpyDefault));
            return fail(RR_ERR_INVALID_ARGUMENT, "pixel_xy[%u] = (%u, %u) lies outside the frame of %ux%u pixels", bad, xy & 0xffffu, xy >> 16, W, H);
        }
    }
    const DPrimary pr{nullptr, PrimaryLaunch{0u, 0u, 0u, 6u}, 0u}; // (as trace_rays_locked: the <false> build reads neither the constants nor the counters)
    RR_TRY(launch_trace_closest(s, false, q, (uint32_t*)(w + QW_COUNT), (uint32_t*)(w + QW_HEAD), n, (const DShadeConst*)(w + QW_CONST), pr,
                                (unsigned long long*)(w + QW_COUNTERS), st, 0u, RR_ALL_PACKETS));
    const dim3 grid(query_grid(s, n)), block(RR_BLOCK);
    if (io.out && io.albedo) hipLaunchKernelGGL((k_surface_pixels<true, true>), grid, block, 0, st, s->data.view, q.r0, q.r1, q.hit, n, target, (uint4*)io.out, (uint32_t*)io.albedo);
    else if (io.out) hipLaunchKernelGGL((k_surface_pixels<true, false>), grid, block, 0, st, s->data.view, q.r0, q.r1, q.hit, n, target, (uint4*)io.out, (uint32_t*)nullptr);
    else hipLaunchKernelGGL((k_surface_pixels<false, true>), grid, block, 0, st, s->data.view, q.r0, q.r1, q.hit, n, target, (uint4*)nullptr, (uint32_t*)io.albedo);
    HIP_TRY(hipGetLastError());
    return RR_OK;
}

// (defined under the C linkage of their declarations in include/rustray_hip.h, as rr_api_motion.h does)
int rr_surface_pixels_device(rr_scene* s, const rr_camera* camera, const uint32_t* pixel_xy, uint32_t n_pixels, rr_surface_hit* out, float* albedo_out, void* hip_stream) try {
    const char* fn = "rr_surface_pixels_device";
    const SurfacePixelsIo io{pixel_xy, out, albedo_out};
    RR_TRY(check_surface_pixels_args(fn, true, s, camera, n_pixels, io));
    if (n_pixels == 0) return RR_OK;
    const hipStream_t st = (hipStream_t)hip_stream;
    return record_call(s, fn, true, {{pixel_xy, "pixel_xy_dev"}, {out, "out_dev"}, {albedo_out, "albedo_out_dev"}}, st,
                       [&] { return surface_pixels_locked(s, camera, io, n_pixels, st, false); });
} RR_GUARD_END("rr_surface_pixels_device")

// The host form: the device form behind the staging of every record call, in buffers of the call's own, freed on return (128 B per pixel
// of answers are not kept resident), on the null stream.  The list is checked here, before anything is uploaded; the caller's outputs
// are written by a finished call only.
int rr_surface_pixels(rr_scene* s, const rr_camera* camera, const uint32_t* pixel_xy, uint32_t n_pixels, rr_surface_hit* out, float* albedo_out) try {
    const char* fn = "rr_surface_pixels";
    RR_TRY(check_surface_pixels_args(fn, false, s, camera, n_pixels, SurfacePixelsIo{pixel_xy, out, albedo_out}));
    if (n_pixels == 0) return RR_OK;
    if (pixel_xy) {
        const uint32_t bad = pixel_list_first_bad(pixel_xy, n_pixels, camera->width, camera->height);
        if (bad != RR_PIXEL_LIST_OK)
            return fail(RR_ERR_INVALID_ARGUMENT, "pixel_xy[%u] = (%u, %u) lies outside the frame of %ux%u pixels", bad, pixel_xy[bad] & 0xffffu, pixel_xy[bad] >> 16,
                        camera->width, camera->height);
    }
    const StageArg args[3] = {stage_input(pixel_xy, 4ull * n_pixels), stage_output(out, 128ull * n_pixels), stage_output(albedo_out, 12ull * n_pixels)};
    return record_call(s, fn, true, {}, nullptr, [&] {
        DevBuf own[3];
        return staged_host_call(own, args, [&](void* const* d) {
            return surface_pixels_locked(s, camera, SurfacePixelsIo{(const uint32_t*)d[0], (rr_surface_hit*)d[1], (float*)d[2]}, n_pixels, nullptr, true);
        });
    });
} RR_GUARD_END("rr_surface_pixels")
