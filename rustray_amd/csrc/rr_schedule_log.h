// rr_schedule_log.h — the schedule recorder of a frame: what render_region_locked enqueues, in host order, for tests/launch_order.py.
// Offers: SchedAccess and its makers sa_r, sa_w, sa_a, sa_host_w, sa_host_r; SchedOp, ScheduleLog (rr_scene::sched); the wrappers every event and
//         stream call of the frame path goes through (sched_record, sched_wait, sched_sync_stream, sched_sync_event, sched_memset,
//         sched_copy, sched_copy_blocking), sched_launch (the declaration next to a kernel launch), sched_host_read; ScheduleScope.
// Needs:  rr_api_base.h.  The two entry points that switch it on and read it back: rr_api_schedule_probe.h.
//
// Off by default: every wrapper is `if (log.on) log.add(...)` in front of the HIP call it returns, so recording cannot add, drop or
// reorder an operation, and logging and enqueueing cannot drift apart.  A launch's accesses are declared where the launch is, from the
// variables its arguments are made of; the initializer list is built behind the same branch.
// An access is a device address range [lo, hi) and a mode: R, W, or A = an integer atomic add / or (also min / max: the binning bounds),
// which commutes with every other A.  A range in HOST memory (the target of a D2H copy, a word the host reads behind a wait) is marked.
// LEFT OUT: the scene's records (items, trees, triangles, materials, textures, lights, flat normals).  No frame writes them -- an edit
// holds the scene's lock and waits for the device -- with one exception that is left out as well: the top level's re-upload for a
// camera far outside the scene (ensure_tlas_reach), which stands behind a hipDeviceSynchronize and consists of blocking copies.
// Allocation (DevBuf::reserve: hipFree, hipMalloc) is not an operation either: the checker credits it with no ordering.

struct SchedAccess { unsigned long long lo, hi; char mode; bool host; const char* what; };
static SchedAccess sa_r(const void* p, size_t bytes, const char* what) { return SchedAccess{(unsigned long long)(uintptr_t)p, (unsigned long long)(uintptr_t)p + bytes, 'R', false, what}; }
static SchedAccess sa_w(const void* p, size_t bytes, const char* what) { return SchedAccess{(unsigned long long)(uintptr_t)p, (unsigned long long)(uintptr_t)p + bytes, 'W', false, what}; }
static SchedAccess sa_a(const void* p, size_t bytes, const char* what) { return SchedAccess{(unsigned long long)(uintptr_t)p, (unsigned long long)(uintptr_t)p + bytes, 'A', false, what}; }
static SchedAccess sa_host_w(const void* p, size_t bytes, const char* what) { return SchedAccess{(unsigned long long)(uintptr_t)p, (unsigned long long)(uintptr_t)p + bytes, 'W', true, what}; }
static SchedAccess sa_host_r(const void* p, size_t bytes, const char* what) { return SchedAccess{(unsigned long long)(uintptr_t)p, (unsigned long long)(uintptr_t)p + bytes, 'R', true, what}; }

// kind: L launch, M memset, U copy to the device, D copy to the host, E event record, W stream-wait-event, S stream synchronize,
// Y event synchronize, H a host read (of what a D2H copy brought), B / X the entry and the return of render_region_locked (X: name = its code)
struct SchedOp { char kind; const void* stream; const void* event; std::string name; std::vector<SchedAccess> acc; };
struct ScheduleLog {
    bool on = false;
    std::vector<SchedOp> ops;
    void add(char kind, const void* stream, const void* event, std::string name, std::initializer_list<SchedAccess> acc = {}) {
        SchedOp op{kind, stream, event, std::move(name), {}};
        for (const SchedAccess& a : acc)
            if (a.lo && a.hi > a.lo) op.acc.push_back(a); // (a NULL plane or an empty range: the kernel does not touch it)
        ops.push_back(std::move(op));
    }
};
// an event's tag at the call site: "stage_traced" and 1 -> "stage_traced[1]"
static std::string sched_tag(const char* tag, int index) { return index < 0 ? std::string(tag) : std::string(tag) + "[" + std::to_string(index) + "]"; }

static hipError_t sched_record(ScheduleLog& log, hipEvent_t ev, hipStream_t st, const char* tag, int index = -1) {
    if (log.on) log.add('E', st, ev, sched_tag(tag, index));
    return hipEventRecord(ev, st);
}
static hipError_t sched_wait(ScheduleLog& log, hipStream_t st, hipEvent_t ev, const char* tag, int index = -1) {
    if (log.on) log.add('W', st, ev, sched_tag(tag, index));
    return hipStreamWaitEvent(st, ev, 0);
}
static hipError_t sched_sync_stream(ScheduleLog& log, hipStream_t st, const char* why) {
    if (log.on) log.add('S', st, nullptr, why);
    return hipStreamSynchronize(st);
}
static hipError_t sched_sync_event(ScheduleLog& log, hipEvent_t ev, const char* tag) {
    if (log.on) log.add('Y', nullptr, ev, tag);
    return hipEventSynchronize(ev);
}
static hipError_t sched_memset(ScheduleLog& log, void* p, int value, size_t bytes, hipStream_t st, const char* what) {
    if (log.on) log.add('M', st, nullptr, what, {sa_w(p, bytes, what)});
    return hipMemsetAsync(p, value, bytes, st);
}
// an asynchronous copy between the host and the device (no other kind is part of a frame)
static hipError_t sched_copy(ScheduleLog& log, void* dst, const void* src, size_t bytes, hipMemcpyKind kind, hipStream_t st, const char* what) {
    if (log.on) {
        if (kind == hipMemcpyHostToDevice) log.add('U', st, nullptr, what, {sa_w(dst, bytes, what)});
        else log.add('D', st, nullptr, what, {sa_r(src, bytes, what), sa_host_w(dst, bytes, what)});
    }
    return hipMemcpyAsync(dst, src, bytes, kind, st);
}
// hipMemcpy: a copy on the legacy null stream that the host waits for
static hipError_t sched_copy_blocking(ScheduleLog& log, void* dst, const void* src, size_t bytes, hipMemcpyKind kind, const char* what) {
    if (log.on) {
        if (kind == hipMemcpyHostToDevice) log.add('U', nullptr, nullptr, what, {sa_w(dst, bytes, what)});
        else log.add('D', nullptr, nullptr, what, {sa_r(src, bytes, what), sa_host_w(dst, bytes, what)});
        log.add('S', nullptr, nullptr, "hipMemcpy");
    }
    return hipMemcpy(dst, src, bytes, kind);
}
// next to a kernel launch: `if (log.on) sched_launch(log, st, "k_name", {...})`
static void sched_launch(ScheduleLog& log, hipStream_t st, const char* name, std::initializer_list<SchedAccess> acc) { log.add('L', st, nullptr, name, acc); }
// the host reads what a D2H copy wrote, behind the wait that says it has arrived
static void sched_host_read(ScheduleLog& log, const void* p, size_t bytes, const char* what) {
    if (log.on) log.add('H', nullptr, nullptr, what, {sa_host_r(p, bytes, what)});
}
// the entry and every return of render_region_locked, the unwinding of an exception included (its code is then "unwound")
struct ScheduleScope {
    ScheduleLog& log; hipStream_t st; bool closed = false;
    ScheduleScope(ScheduleLog& log_, hipStream_t st_) : log(log_), st(st_) { if (log.on) log.add('B', st, nullptr, "render_region_locked"); }
    int done(int rc) { if (log.on) log.add('X', st, nullptr, std::to_string(rc)); closed = true; return rc; }
    ~ScheduleScope() {
        if (closed || !log.on) return;
        try { log.add('X', st, nullptr, "unwound"); } catch (...) { /* no memory for the marker: the log ends without it */ }
    }
    ScheduleScope(const ScheduleScope&) = delete;
    ScheduleScope& operator=(const ScheduleScope&) = delete;
};
