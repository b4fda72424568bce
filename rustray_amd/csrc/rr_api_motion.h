// rr_api_motion.h — the per-pixel motion of moved items on the device: what rr_accumulate_records takes as motion_dev when items moved
// between two frames, from the records the device already holds.
// Offers: rr_motion_records_device, rr_motion_records.
// Needs:  rr_api_query.h (check_arg_ranges, record_call, staged_host_call), rr_api_temporal.h (tp_frame), rr_api_handle.h (MotionState),
//         rr_motion.h (motion_build_table), kernel 7f of rr_kernels.hip.
//
// The call is ONE copy of the table (from one of the handle's pinned copies) and ONE launch of k_motion_records on the caller's stream, not waited
// for; with nothing moved and no world_out it is one hipMemsetAsync.  The caller's host arrays are read before the call returns: the
// table is built on the host from them and from the handle's item records (SceneData::h_items: the trans_inv and id the current frame
// was traced with).  The host form is the device form behind the staging of every record call (staged_host_call, in the handle's pool).

struct MotionIo {
    const rr_radiance* records; float* motion; float* world;
};

// what both forms check before the scene is looked at; `device`: the alignment rule of the device form
static int check_motion_args(const char* fn, bool device, const rr_scene* s, const rr_camera* cam, const uint32_t* item_index, const float* prev_trans, uint32_t n_moved,
                             const MotionIo& io) {
    if (!s) return fail(RR_ERR_INVALID_ARGUMENT, "%s: scene is NULL", fn);
    if (!cam) return fail(RR_ERR_INVALID_ARGUMENT, "%s: camera is NULL", fn);
    if (!io.records) return fail(RR_ERR_INVALID_ARGUMENT, "%s: records is NULL", fn);
    if (!io.motion) return fail(RR_ERR_INVALID_ARGUMENT, "%s: motion_out is NULL", fn);
    const uint32_t width = cam->width, height = cam->height;
    if (width == 0 || height == 0 || width > 65535u || height > 65535u) return fail(RR_ERR_INVALID_ARGUMENT, "%s: bad frame size %ux%u", fn, width, height);
    if (n_moved > 0 && !item_index) return fail(RR_ERR_INVALID_ARGUMENT, "%s: item_index is NULL with n_moved = %u", fn, n_moved);
    if (n_moved > 0 && !prev_trans) return fail(RR_ERR_INVALID_ARGUMENT, "%s: prev_trans is NULL with n_moved = %u", fn, n_moved);
    if ((uint64_t)width * height * 2u > (1ull << 30))
        return fail(RR_ERR_UNSUPPORTED, "%s: %ux%u pixels x 2 are more than 2^30 records", fn, width, height);
    if (device && ((uintptr_t)io.records & 15u)) return fail(RR_ERR_INVALID_ARGUMENT, "%s: records_dev must be 16-byte aligned", fn);
    if (device && (((uintptr_t)io.motion | (uintptr_t)io.world) & 3u)) return fail(RR_ERR_INVALID_ARGUMENT, "%s: motion_out_dev and world_out_dev must be 4-byte aligned", fn);
    const uint64_t n = (uint64_t)width * height;
    const ArgRange t[3] = {{io.records, 32u * n, "records", false, -1}, {io.motion, 12u * n, "motion_out", true, -1}, {io.world, 12u * n, "world_out", true, -1}};
    return check_arg_ranges(fn, t, 3, true, "");
}

// The table of this call, built on the host from the caller's arrays and the handle's item records: every refusal that concerns the list
// comes from here, before anything is enqueued.  The caller holds the lock.
static int build_motion_table(rr_scene* s, const char* fn, const uint32_t* item_index, const float* prev_trans, uint32_t n_moved, std::vector<MoEntry>* table) {
    const std::vector<DItem>& items = s->data.h_items;
    if (n_moved > items.size()) return fail(RR_ERR_INVALID_ARGUMENT, "%s: n_moved %u, the scene has %zu items", fn, n_moved, items.size());
    char msg[256];
    const bool ok = motion_build_table([&](unsigned int i, float* inv, unsigned int* id) {
        const float4 rows[3] = {items[i].inv0, items[i].inv1, items[i].inv2};
        memcpy(inv, rows, sizeof rows);
        *id = items[i].id;
    }, (unsigned int)items.size(), item_index, prev_trans, n_moved, table, msg, sizeof msg);
    if (!ok) return fail(RR_ERR_INVALID_ARGUMENT, "%s: %s", fn, msg);
    return RR_OK;
}

// The table in the handle's device buffer, copied on stream st from one of the handle's four pinned copies, used in turn.
// The one wait: for the copy of the fourth call before, which reads the pinned copy this call writes (it sits behind that call's
// producer, never behind this one's).
static int upload_motion_table(rr_scene* s, const std::vector<MoEntry>& table, hipStream_t st) {
    const size_t bytes = table.size() * sizeof(MoEntry);
    MotionSlot& m = s->motion.slot[s->motion.next];
    if (m.pending) { HIP_TRY(hipEventSynchronize(m.copied)); m.pending = false; }
    if (!m.copied) HIP_TRY(hipEventCreateWithFlags(&m.copied, hipEventDisableTiming));
    if (m.entries < table.size()) {
        if (m.h_table) { (void)hipHostFree(m.h_table); m.h_table = nullptr; m.entries = 0; }
        HIP_TRY(hipHostMalloc((void**)&m.h_table, bytes, hipHostMallocDefault));
        m.entries = table.size();
    }
    HIP_TRY(s->motion.table.reserve(bytes));
    memcpy(m.h_table, table.data(), bytes);
    HIP_TRY(hipMemcpyAsync(s->motion.table.p, m.h_table, bytes, hipMemcpyHostToDevice, st));
    HIP_TRY(hipEventRecord(m.copied, st));
    m.pending = true;
    s->motion.next = (s->motion.next + 1) % 4;
    return RR_OK;
}

// the work of one call on stream st, on buffers the device can address, with its table built; the caller holds the lock and has taken the stream
static int motion_locked(rr_scene* s, const char* fn, const rr_camera* cam, const std::vector<MoEntry>& table, const MotionIo& io, hipStream_t st) {
    const uint32_t W = cam->width, H = cam->height, n_moved = (uint32_t)table.size();
    if (n_moved == 0 && !io.world) {
        HIP_TRY(hipMemsetAsync(io.motion, 0, 12ull * W * H, st));
        return RR_OK;
    }
    if (n_moved) RR_TRY(upload_motion_table(s, table, st));
    const dim3 grid((W + DN_TILE_W - 1) / DN_TILE_W, (H + DN_TILE_H - 1) / DN_TILE_H), block(RR_BLOCK);
    hipLaunchKernelGGL(k_motion_records, grid, block, 0, st, tp_frame(cam), (const float4*)io.records, n_moved ? s->motion.table.as<MoEntry>() : (const MoEntry*)nullptr, n_moved,
                       io.motion, io.world);
    if (hipGetLastError() != hipSuccess) return fail(RR_ERR_DEVICE, "%s: a launch failed", fn);
    return RR_OK;
}

int rr_motion_records_device(rr_scene* s, const rr_camera* camera, const uint32_t* item_index, const float* prev_trans, uint32_t n_moved, const rr_radiance* records,
                             float* motion_out, float* world_out, void* hip_stream) try {
    const char* fn = "rr_motion_records_device";
    const MotionIo io{records, motion_out, world_out};
    RR_TRY(check_motion_args(fn, true, s, camera, item_index, prev_trans, n_moved, io));
    const hipStream_t st = (hipStream_t)hip_stream;
    std::vector<MoEntry> table;
    return record_call(s, fn, true, {{records, "records_dev"}, {motion_out, "motion_out_dev"}, {world_out, "world_out_dev"}}, st,
                       [&] { return build_motion_table(s, fn, item_index, prev_trans, n_moved, &table); },
                       [&] { return motion_locked(s, fn, camera, table, io, st); });
} RR_GUARD_END("rr_motion_records_device")

int rr_motion_records(rr_scene* s, const rr_camera* camera, const uint32_t* item_index, const float* prev_trans, uint32_t n_moved, const rr_radiance* records,
                      float* motion_out, float* world_out) try {
    const char* fn = "rr_motion_records";
    RR_TRY(check_motion_args(fn, false, s, camera, item_index, prev_trans, n_moved, MotionIo{records, motion_out, world_out}));
    const size_t n = (size_t)camera->width * camera->height;
    const StageArg args[3] = {stage_input(records, 32 * n), stage_output(motion_out, 12 * n), stage_output(world_out, 12 * n)};
    std::vector<MoEntry> table;
    return record_call(s, fn, true, {}, nullptr, [&] { return build_motion_table(s, fn, item_index, prev_trans, n_moved, &table); }, [&] {
        return staged_host_call(s->record_stage.buf, args, [&](void* const* d) {
            return motion_locked(s, fn, camera, table, MotionIo{(const rr_radiance*)d[0], (float*)d[1], (float*)d[2]}, nullptr);
        });
    });
} RR_GUARD_END("rr_motion_records")
