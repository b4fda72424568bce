// rr_api_multi.h — one frame on several devices from one host process, and the epilogue that puts interleaved tiles into frame order.
// Offers: GatherMap, gather_map; rr_deinterleave_device, rr_deinterleave_packed_device; multi_lock_order, rr_multi_lock_order;
//         g_peer_mu, g_peer_state, ensure_peer_access; rr_render_multi.
// Needs:  rr_api_base.h (Workers through rr_scene_build.h), rr_sample_table.h (fill_region, check_region, rr_region_pixel_count),
//         rr_api_handle.h (writes rr_scene::multi, and the multi_* fields of rr_scene::timing.stats), rr_api_frame.h (check_frame_args,
//         render_region_locked, stage_outputs, copy_outputs, OUT_ELEM, out_buffer), the kernels k_gather_frame and k_gather_packed.

// ---------------------------------------------------------------------------
// multi-GPU epilogue: compact per-rank buffers (concatenated in rank order) -> frame order
// ---------------------------------------------------------------------------
// One gather map per (frame size, tiles, ranks, device), each buffer uploaded on first use: per frame pixel its index in the
// concatenation of all ranks' buffers (k_gather_frame), and its rank and its index among that rank's pixels (k_gather_packed).
struct GatherMap { DevBuf index, rank, local; };
using GatherKey = std::tuple<uint32_t, uint32_t, uint32_t, uint32_t, uint32_t, int>; // width, height, tile_w, tile_h, n_ranks, device
static std::mutex g_gather_mu;
static std::map<GatherKey, GatherMap>& g_gather_maps = *new std::map<GatherKey, GatherMap>(); // never destroyed: no hipFree after the HIP runtime's teardown
// the map of `key` with `index` (packed = false) or `rank` and `local` (packed = true) on the device; under g_gather_mu
static int gather_map(const GatherKey& key, bool packed, GatherMap** out) {
    GatherMap& gm = g_gather_maps[key];
    *out = &gm;
    if (packed ? gm.rank.p != nullptr : gm.index.p != nullptr) return RR_OK;
    const auto [width, height, tile_w, tile_h, n_ranks, device] = key;
    const uint32_t np = width * height;
    std::vector<uint32_t> rank(np), local(np), offset(n_ranks), xy;
    uint32_t base = 0;
    for (uint32_t r = 0; r < n_ranks; r++) {
        fill_region(width, height, rr_region{tile_w, tile_h, n_ranks, r}, &xy);
        for (uint32_t p = 0; p < xy.size(); p++) { const size_t o = (size_t)(xy[p] >> 16) * width + (xy[p] & 0xffffu); rank[o] = r; local[o] = p; }
        offset[r] = base; base += (uint32_t)xy.size();
    }
    // a map counts as uploaded once its buffer (of a pair: `rank`) is set: filled aside, moved in when complete
    DevBuf a, b;
    if (packed) HIP_TRY(b.upload(rank, 4));
    else for (uint32_t o = 0; o < np; o++) local[o] += offset[rank[o]];
    HIP_TRY(a.upload(local, 4));
    if (packed) { gm.local = std::move(a); gm.rank = std::move(b); }
    else gm.index = std::move(a);
    return RR_OK;
}

extern "C" int rr_deinterleave_device(uint32_t width, uint32_t height, uint32_t tile_w, uint32_t tile_h, uint32_t n_ranks,
                                      uint32_t elem_bytes, const void* src, void* dst, int device, void* hip_stream) try {
    const rr_region probe{tile_w, tile_h, n_ranks, 0};
    RR_TRY(check_region(width, height, &probe));
    if (!src || !dst || elem_bytes == 0 || (elem_bytes & 3u)) return fail(RR_ERR_INVALID_ARGUMENT, "bad buffers or elem_bytes %u", elem_bytes);
    HIP_TRY(hipSetDevice(device));
    std::lock_guard<std::mutex> lk(g_gather_mu);
    GatherMap* gm = nullptr;
    RR_TRY(gather_map(GatherKey{width, height, tile_w, tile_h, n_ranks, device}, false, &gm));
    const uint32_t np = width * height;
    const uint32_t words = elem_bytes / 4;
    const uint64_t total = (uint64_t)np * words;
    hipLaunchKernelGGL(k_gather_frame, dim3((uint32_t)((total + RR_BLOCK - 1) / RR_BLOCK)), dim3(RR_BLOCK), 0, (hipStream_t)hip_stream,
                       gm->index.as<uint32_t>(), np, words, (const uint32_t*)src, (uint32_t*)dst);
    HIP_TRY(hipGetLastError());
    return RR_OK;
} RR_GUARD_END("rr_deinterleave_device")

// The gathered packs of a multi-rank frame -> the four frame-order buffers, one launch (k_gather_packed).
extern "C" int rr_deinterleave_packed_device(uint32_t width, uint32_t height, uint32_t tile_w, uint32_t tile_h, uint32_t n_ranks,
                                             const void* packs, uint64_t pack_stride, const uint64_t* section_offset, const uint32_t* elem_bytes,
                                             void* const* dst, int device, void* hip_stream) try {
    const rr_region probe{tile_w, tile_h, n_ranks, 0};
    RR_TRY(check_region(width, height, &probe));
    if (!packs || !section_offset || !elem_bytes || !dst) return fail(RR_ERR_INVALID_ARGUMENT, "NULL argument");
    DPackedGather g{};
    for (int k = 0; k < 4; k++) {
        if (elem_bytes[k] & 3u) return fail(RR_ERR_INVALID_ARGUMENT, "elem_bytes[%d] = %u is not a multiple of 4", k, elem_bytes[k]);
        if (elem_bytes[k] && !dst[k]) return fail(RR_ERR_INVALID_ARGUMENT, "dst[%d] is NULL for a present buffer", k);
        if ((section_offset[k] & 3u) || (pack_stride & 3u)) return fail(RR_ERR_INVALID_ARGUMENT, "sections and packs must be 4-byte aligned");
        g.words[k] = elem_bytes[k] / 4u; g.words_total += g.words[k]; g.section[k] = section_offset[k]; g.dst[k] = (uint32_t*)dst[k];
    }
    if (g.words_total == 0) return fail(RR_ERR_INVALID_ARGUMENT, "no buffer to move");
    HIP_TRY(hipSetDevice(device));
    std::lock_guard<std::mutex> lk(g_gather_mu);
    GatherMap* gm = nullptr;
    RR_TRY(gather_map(GatherKey{width, height, tile_w, tile_h, n_ranks, device}, true, &gm));
    const uint32_t np = width * height;
    g.src_rank = gm->rank.as<uint32_t>(); g.src_local = gm->local.as<uint32_t>();
    g.packs = (const char*)packs; g.pack_stride = pack_stride; g.n_pixels = np;
    const uint64_t total = (uint64_t)np * g.words_total;
    hipLaunchKernelGGL(k_gather_packed, dim3((uint32_t)((total + RR_BLOCK - 1) / RR_BLOCK)), dim3(RR_BLOCK), 0, (hipStream_t)hip_stream, g);
    HIP_TRY(hipGetLastError());
    return RR_OK;
} RR_GUARD_END("rr_deinterleave_packed_device")

// Lock order of a set of scene handles: by address (std::less is a total order on pointers).
static std::vector<rr_scene*> multi_lock_order(rr_scene* const* scenes, uint32_t n) {
    std::vector<rr_scene*> v(scenes, scenes + n);
    std::sort(v.begin(), v.end(), std::less<rr_scene*>());
    return v;
}
// test hook (tests/test_abi.py): the order in which rr_render_multi would lock `scenes`, as indices into the caller's array
extern "C" int rr_multi_lock_order(rr_scene* const* scenes, uint32_t n_scenes, uint32_t* order_out) try {
    if (!scenes || !order_out || n_scenes == 0) return fail(RR_ERR_INVALID_ARGUMENT, "NULL argument");
    const std::vector<rr_scene*> v = multi_lock_order(scenes, n_scenes);
    for (uint32_t k = 0; k < n_scenes; k++)
        for (uint32_t i = 0; i < n_scenes; i++) if (scenes[i] == v[k]) { order_out[k] = i; break; }
    return RR_OK;
} RR_GUARD_END("rr_multi_lock_order")

// Peer access between two devices, both ways: checked once per ordered pair, enabled on first use.
// false = no direct path (the caller stages through the host).  The same device counts as direct.
static std::mutex g_peer_mu;
static std::map<std::pair<int, int>, bool> g_peer_state; // (from, to) -> `from` may access memory of `to`
static bool enable_peer_one_way(int from, int to) {
    auto it = g_peer_state.find({from, to});
    if (it != g_peer_state.end()) return it->second;
    bool ok = false;
    int can = 0;
    if (hipDeviceCanAccessPeer(&can, from, to) == hipSuccess && can) {
        int cur = 0;
        (void)hipGetDevice(&cur);
        if (hipSetDevice(from) == hipSuccess) {
            const hipError_t e = hipDeviceEnablePeerAccess(to, 0);
            ok = e == hipSuccess || e == hipErrorPeerAccessAlreadyEnabled;
            (void)hipGetLastError(); // "already enabled" is not an error of this call
        }
        (void)hipSetDevice(cur);
    }
    g_peer_state[{from, to}] = ok;
    return ok;
}
static bool ensure_peer_access(int a, int b) {
    if (a == b) return true;
    std::lock_guard<std::mutex> lk(g_peer_mu);
    const bool ab = enable_peer_one_way(a, b), ba = enable_peer_one_way(b, a);
    return ab && ba;
}

// ---------------------------------------------------------------------------
// one frame on several GPUs from ONE host process (the reference host is one process, src/renderer.rs:105-172):
// one host thread per device renders that device's interleaved tiles, the compact per-device buffers are copied
// peer-to-peer (xGMI) into device 0, de-interleaved there and copied to the host once.  No collective library is
// involved: the exchange is n - 1 point-to-point copies of 1 / n of the frame each.  Every device works on its own
// non-blocking stream.  UNVERIFIED ON N > 1 DEVICES until an N-GPU node has run it (the pool hands out 1-GPU boxes;
// tests/test_gpu_multi.py puts several handles on device 0).
// ---------------------------------------------------------------------------
extern "C" int rr_render_multi(rr_scene* const* scenes, uint32_t n_scenes, const rr_camera* cam, const rr_config* cfg,
                               const uint16_t* sample_xy, const rr_frame* out, const volatile int* cancel) try {
    if (!scenes || n_scenes == 0) return fail(RR_ERR_INVALID_ARGUMENT, "no scenes");
    if (n_scenes > 64) return fail(RR_ERR_UNSUPPORTED, "%u scene handles", n_scenes);
    for (uint32_t i = 0; i < n_scenes; i++) {
        if (!scenes[i]) return fail(RR_ERR_INVALID_ARGUMENT, "scene %u is NULL", i);
        for (uint32_t j = 0; j < i; j++) if (scenes[j] == scenes[i]) return fail(RR_ERR_INVALID_ARGUMENT, "scene handle %u is passed twice", i);
        RR_TRY(check_frame_args(scenes[i], cam, cfg, sample_xy));
        RR_TRY(not_in_pass(scenes[i], "rr_render_multi"));
    }
    if (!out || !out->rgba8) return fail(RR_ERR_INVALID_ARGUMENT, "out->rgba8 is required");
    const uint32_t W = cam->width, H = cam->height, TW = 32, TH = 8; // interleaved 32x8 tiles: tile_index % n == device slot
    const size_t np = (size_t)W * H;
    void* host[4] = {out->rgba8, out->normal, out->depth, out->object_id};
    std::vector<uint64_t> count(n_scenes), offset(n_scenes);
    uint64_t total = 0;
    for (uint32_t i = 0; i < n_scenes; i++) {
        rr_region rg{TW, TH, n_scenes, i};
        count[i] = rr_region_pixel_count(W, H, &rg);
        offset[i] = total; total += count[i];
    }
    rr_scene* s0 = scenes[0];
    // Handles are locked in ADDRESS order, whatever order the caller passed them in: two calls that share handles in
    // opposite orders (or a call racing rr_render on one of them) then serialise instead of deadlocking.
    std::vector<std::unique_lock<std::mutex>> locks;
    for (rr_scene* s : multi_lock_order(scenes, n_scenes)) locks.emplace_back(s->mu);
    // Peer access between device 0 and every other device taking part: checked, and enabled both ways on first use.
    // A pair without it does not fall back silently to whatever hipMemcpyPeerAsync does: its buffers are staged
    // through pinned host memory here, and the frame's stats say so.
    std::vector<char> direct(n_scenes, 1);
    uint32_t n_peer = 0, n_staged = 0;
    for (uint32_t i = 1; i < n_scenes; i++) {
        direct[i] = (s0->tuning.multi_force_staged == 0u && ensure_peer_access(scenes[i]->device, s0->device)) ? 1 : 0;
        if (direct[i]) n_peer++; else n_staged++;
    }
    auto own_stream = [](rr_scene* s) -> int { // on the scene's device
        if (!s->multi.stream) HIP_TRY(hipStreamCreateWithFlags(&s->multi.stream, hipStreamNonBlocking));
        return RR_OK;
    };
    // device 0: the concatenation of the compact buffers (rank order) and the frame-order buffers
    HIP_TRY(hipSetDevice(s0->device));
    RR_TRY(own_stream(s0));
    for (int k = 0; k < 4; k++)
        if (host[k]) HIP_TRY(s0->multi.cat[k].reserve(np * OUT_ELEM[k]));
    rr_frame frame_dev{};
    RR_TRY(stage_outputs(s0, *out, np, false, &frame_dev));
    // every device renders its tiles into its own compact buffers on its own stream, then pushes them towards device 0
    std::vector<int> rcs(n_scenes, RR_OK);
    std::vector<std::string> errs(n_scenes);
    auto work = [&](uint32_t i) {
        rr_scene* s = scenes[i];
        auto body = [&]() -> int {
            HIP_TRY(hipSetDevice(s->device));
            RR_TRY(own_stream(s));
            rr_frame dev{};
            void** devp[4] = {(void**)&dev.rgba8, (void**)&dev.normal, (void**)&dev.depth, (void**)&dev.object_id};
            for (int k = 0; k < 4; k++) {
                if (!host[k]) continue;
                if (i == 0) *devp[k] = (char*)s0->multi.cat[k].p + offset[0] * OUT_ELEM[k]; // device 0 renders straight into its slot
                else { HIP_TRY(s->multi.part[k].reserve(std::max<uint64_t>(count[i], 1) * OUT_ELEM[k])); *devp[k] = s->multi.part[k].p; }
            }
            rr_region rg{TW, TH, n_scenes, i};
            RR_TRY(render_region_locked(s, cam, cfg, sample_xy, frame_io(&rg, &dev, false), s->multi.stream, cancel));
            if (i != 0)
                for (int k = 0; k < 4; k++) {
                    if (!host[k] || !count[i]) continue;
                    const size_t bytes = count[i] * OUT_ELEM[k];
                    void* dst = (char*)s0->multi.cat[k].p + offset[i] * OUT_ELEM[k];
                    if (direct[i] && s->device == s0->device) HIP_TRY(hipMemcpyAsync(dst, s->multi.part[k].p, bytes, hipMemcpyDeviceToDevice, s->multi.stream));
                    else if (direct[i]) HIP_TRY(hipMemcpyPeerAsync(dst, s0->device, s->multi.part[k].p, s->device, bytes, s->multi.stream));
                    else { // no peer access: device -> pinned host here, host -> device 0 after the join
                        if (s->multi.stage_bytes[k] < bytes) {
                            if (s->multi.stage[k]) { (void)hipHostFree(s->multi.stage[k]); s->multi.stage[k] = nullptr; s->multi.stage_bytes[k] = 0; }
                            HIP_TRY(hipHostMalloc(&s->multi.stage[k], bytes, hipHostMallocPortable));
                            s->multi.stage_bytes[k] = bytes;
                        }
                        HIP_TRY(hipMemcpyAsync(s->multi.stage[k], s->multi.part[k].p, bytes, hipMemcpyDeviceToHost, s->multi.stream));
                    }
                }
            HIP_TRY(hipStreamSynchronize(s->multi.stream));
            return RR_OK;
        };
        try { RR_FAULT_POINT("render_multi.worker"); rcs[i] = body(); }
        catch (...) { rcs[i] = guard_fail("rr_render_multi (device worker)"); }
        if (rcs[i] != RR_OK) { try { errs[i] = tl_error; } catch (...) { } } // the message lives in the worker's thread-local slot
    };
    {
        Workers threads; // joined on every path out of this block
        std::vector<char> inline_run(n_scenes, 0);
        for (uint32_t i = 1; i < n_scenes; i++)
            if (!threads.spawn([&work, i]() { work(i); })) inline_run[i] = 1;
        work(0);
        for (uint32_t i = 1; i < n_scenes; i++) if (inline_run[i]) work(i); // a thread that could not be started: its device waits for ours
        threads.join_and_rethrow();
    }
    const auto t_joined = std::chrono::steady_clock::now();
    for (uint32_t i = 0; i < n_scenes; i++)
        if (rcs[i] != RR_OK) return fail(rcs[i], "device slot %u: %s", i, errs[i].c_str());
    HIP_TRY(hipSetDevice(s0->device));
    for (uint32_t i = 1; i < n_scenes; i++) {
        if (direct[i]) continue;
        for (int k = 0; k < 4; k++)
            if (host[k] && count[i])
                HIP_TRY(hipMemcpyAsync((char*)s0->multi.cat[k].p + offset[i] * OUT_ELEM[k], scenes[i]->multi.stage[k], count[i] * OUT_ELEM[k], hipMemcpyHostToDevice, s0->multi.stream));
    }
    for (int k = 0; k < 4; k++)
        if (host[k]) RR_TRY(rr_deinterleave_device(W, H, TW, TH, n_scenes, (uint32_t)OUT_ELEM[k], s0->multi.cat[k].p, out_buffer(frame_dev, k), s0->device, s0->multi.stream));
    RR_TRY(copy_outputs(s0->sched, *out, frame_dev, np, s0->multi.stream));
    s0->timing.stats.multi_devices = n_scenes; s0->timing.stats.multi_peer_links = n_peer; s0->timing.stats.multi_staged_links = n_staged;
    s0->timing.stats.ms_multi_exchange = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_joined).count();
    return RR_OK;
} RR_GUARD_END("rr_render_multi")

