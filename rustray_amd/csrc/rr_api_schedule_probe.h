// rr_api_schedule_probe.h — test entry points of the schedule recorder (rr_schedule_log.h); like rr_math_probe and rr_test_fault they
// are not part of include/rustray_hip.h.
// Offers: rr_test_schedule_record, rr_test_schedule_read (tests/test_gpu_launch_order.py through rustray_amd/capi.py).
// Needs:  rr_api_base.h, rr_api_handle.h (rr_scene::sched).

// on != 0: empty the log and record every frame call on this handle from now on; 0: stop and drop the log
extern "C" int rr_test_schedule_record(rr_scene* s, int on) try {
    if (!s) return fail(RR_ERR_INVALID_ARGUMENT, "NULL argument");
    RR_TRY(not_in_pass(s, "rr_test_schedule_record"));
    std::lock_guard<std::mutex> lk(s->mu);
    s->sched.ops.clear();
    s->sched.on = on != 0;
    return RR_OK;
} RR_GUARD_END("rr_test_schedule_record")

// The log as text, one operation per line in host order, fields separated by tabs:
//   kind  stream  event  name-or-tag  accesses
// kind: the letter of SchedOp; stream and event: the handles in hex (0 = the legacy null stream / none); accesses: `mode,space,lo,hi,what`
// joined by ';' -- mode R, W or A, space d (device) or h (host), [lo, hi) in hex.
// *needed = the bytes of the text with its final NUL; the text is written when it fits `capacity` (out may be NULL to ask for the size).
// The log itself stays as it is.
extern "C" int rr_test_schedule_read(rr_scene* s, char* out, uint64_t capacity, uint64_t* needed) try {
    if (!s || !needed) return fail(RR_ERR_INVALID_ARGUMENT, "NULL argument");
    RR_TRY(not_in_pass(s, "rr_test_schedule_read"));
    std::lock_guard<std::mutex> lk(s->mu);
    std::string text;
    char buf[96];
    for (const SchedOp& op : s->sched.ops) {
        snprintf(buf, sizeof buf, "%c\t%llx\t%llx\t", op.kind, (unsigned long long)(uintptr_t)op.stream, (unsigned long long)(uintptr_t)op.event);
        text += buf; text += op.name; text += '\t';
        for (size_t k = 0; k < op.acc.size(); k++) {
            const SchedAccess& a = op.acc[k];
            snprintf(buf, sizeof buf, "%s%c,%c,%llx,%llx,", k ? ";" : "", a.mode, a.host ? 'h' : 'd', a.lo, a.hi);
            text += buf; text += a.what;
        }
        text += '\n';
    }
    *needed = text.size() + 1;
    if (out && capacity >= *needed) memcpy(out, text.c_str(), text.size() + 1);
    return RR_OK;
} RR_GUARD_END("rr_test_schedule_read")
