// rr_api_base.h — what every host layer of rr_api.hip stands on.
// Offers: tl_error, fail; guard_fail, RR_GUARD_END; the test fault hook (RR_FAULT_POINT, rr_test_fault); HIP_TRY, RR_TRY; InPass,
//         not_in_pass; DevBuf; rr_abi_version, rr_device_count, rr_last_error.  Includes rr_scene_build.h behind `fail` and the hook.
// Needs:  the system headers and include/rustray_hip.h (rr_api.hip includes them first).

// ---------------------------------------------------------------------------
// errors
// ---------------------------------------------------------------------------
static thread_local std::string tl_error;

static int fail(int code, const char* fmt, ...) noexcept {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    try { tl_error = buf; } catch (...) { /* no memory for the message: the code still says what happened */ }
    return code;
}

// ---------------------------------------------------------------------------
// Nothing unwinds across the C ABI (include/rustray_hip.h: "no function aborts or throws").  The host is Rust built with
// panic = "abort" (reference Cargo.toml:9-11); a C++ exception that reached one of its frames would be undefined behaviour.
// Every extern "C" entry point below is a function-try-block that ends in RR_GUARD_END: std::bad_alloc (the std::vectors
// sized by the caller's scene) becomes RR_ERR_OUT_OF_MEMORY, anything else RR_ERR_DEVICE with what() in rr_last_error().
// Host worker threads (mesh tree builds, one thread per device in rr_render_multi) run under `Workers` (rr_scene_build.h): an exception inside
// a worker is carried to the calling thread and rethrown there, a thread that cannot be started is not fatal (the caller
// does that work itself), and the destructor joins -- no path ends in std::terminate.
// ---------------------------------------------------------------------------
static int guard_fail(const char* fn) noexcept {
    try { throw; }
    catch (const std::bad_alloc&) { return fail(RR_ERR_OUT_OF_MEMORY, "%s: out of host memory", fn); }
    catch (const std::exception& e) { return fail(RR_ERR_DEVICE, "%s: %s", fn, e.what()); }
    catch (...) { return fail(RR_ERR_DEVICE, "%s: unknown exception", fn); }
}
#define RR_GUARD_END(fn) catch (...) { return guard_fail(fn); }

// Test-only fault injection (tests/test_abi.py, tests/test_gpu_guard.py, tests/test_gpu_scene_edits.py): rr_test_fault("point", kind, skip)
// arms ONE fault; the (skip + 1)-th crossing of RR_FAULT_POINT("point") on any thread throws std::bad_alloc (kind 1), std::runtime_error (2)
// or an int (3) and disarms.  Kinds 4, 5, 6 throw as 1, 2, 3 and stay armed: every later crossing throws too, until the next call of
// rr_test_fault (a failed update whose rollback crosses the same point fails as well).  Points: scene_create.host, scene_create.mesh_worker, render_multi.worker, trace_rays.host, trace_shadow_rays.host, shade_rays.host,
// update_transforms.host (before the update writes anything), update_transforms.derive (after the items' upload),
// update_transforms.upload_tlas (after the top level's rebuild, before its upload), update_materials.device (between the materials'
// and the items' copy), tlas_reach.upload (a frame's top-level rebuild, before its upload), update_lights.device (after the light
// records' copy), update_item_flags.device (after the items' copy), add_textures.device (after the grown pool's upload, before it
// replaces the old one), add_meshes.device and set_items.device (after the new state's upload, before the commit), level1_stages.stage (once per stage of the staged
// level 1, in front of the stage's launches: enqueue_level1_stages).  Not armed (always, outside the tests): one
// acquire load per crossing (it pairs with the release store of rr_test_fault: a thread that sees the kind sees the point's name), and
// the points sit outside every per-ray and per-triangle loop.
static std::atomic<int> g_fault_kind{0};
static std::atomic<int> g_fault_skip{0};
static char g_fault_point[64] = "";
static void fault_point(const char* name) {
    if (g_fault_kind.load(std::memory_order_acquire) == 0 || strcmp(name, g_fault_point) != 0) return;
    if (g_fault_skip.fetch_sub(1) > 0) return;
    int kind = g_fault_kind.load(std::memory_order_acquire);
    kind = kind > 3 ? kind - 3 : g_fault_kind.exchange(0);
    if (kind == 1) throw std::bad_alloc();
    if (kind == 2) throw std::runtime_error(std::string("injected fault at ") + name);
    if (kind == 3) throw 42;
}
#define RR_FAULT_POINT(name) fault_point(name)
#include "rr_scene_build.h" // after `fail` and RR_FAULT_POINT: the scene builder reports and is probed through both
extern "C" int rr_test_fault(const char* point, int kind, int skip) {
    g_fault_kind.store(0);
    if (!point || kind < 0 || kind > 6 || strlen(point) >= sizeof g_fault_point) return fail(RR_ERR_INVALID_ARGUMENT, "rr_test_fault: bad arguments");
    strcpy(g_fault_point, point);
    g_fault_skip.store(skip < 0 ? 0 : skip);
    g_fault_kind.store(kind, std::memory_order_release);
    return RR_OK;
}
#define HIP_TRY(expr)                                                                                   \
    do {                                                                                                \
        hipError_t e_ = (expr);                                                                         \
        if (e_ != hipSuccess)                                                                           \
            return fail(e_ == hipErrorOutOfMemory ? RR_ERR_OUT_OF_MEMORY : RR_ERR_DEVICE, "%s: %s", #expr, hipGetErrorString(e_)); \
    } while (0)
#define RR_TRY(expr)                                                                                    \
    do {                                                                                                \
        const int rc_ = (expr);                                                                         \
        if (rc_ != RR_OK) return rc_;                                                                   \
    } while (0)

// The scene whose on_pass callback (rr_render_progressive, rr_render_progressive_tiles) runs on this thread, if any.  The frame
// holds that scene's mutex across the callback: rr_scene_last_stats serves the scene without it, and every other entry point that
// would take it refuses instead of deadlocking on a non-recursive std::mutex.
static thread_local const rr_scene* tl_in_pass = nullptr;
struct InPass {
    const rr_scene* prev;
    explicit InPass(const rr_scene* s) : prev(tl_in_pass) { tl_in_pass = s; }
    ~InPass() { tl_in_pass = prev; }
    InPass(const InPass&) = delete;
    InPass& operator=(const InPass&) = delete;
};
static int not_in_pass(const rr_scene* s, const char* fn) {
    if (s && tl_in_pass == s) return fail(RR_ERR_INVALID_ARGUMENT, "%s: re-entry from on_pass of the same scene (only rr_scene_last_stats may be called there)", fn);
    return RR_OK;
}

// ---------------------------------------------------------------------------
// device buffer helper
// ---------------------------------------------------------------------------
// Owns one device allocation (freed on destruction: every exit path of rr_scene_create and the scratch buffers of
// rr_pick / rr_post_process release what they hold).  Move-only.
struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept : p(o.p), bytes(o.bytes) { o.p = nullptr; o.bytes = 0; }
    DevBuf& operator=(DevBuf&& o) noexcept { if (this != &o) { release(); p = o.p; bytes = o.bytes; o.p = nullptr; o.bytes = 0; } return *this; }
    ~DevBuf() { release(); }
    hipError_t reserve(size_t n) {
        if (n <= bytes) return hipSuccess;
        if (p) { (void)hipFree(p); p = nullptr; bytes = 0; }
        hipError_t e = hipMalloc(&p, n);
        if (e == hipSuccess) bytes = n;
        return e;
    }
    // room for the host's array, never less than min_bytes (an empty array still gives the kernels a pointer), then its bytes; blocking
    template <class T> hipError_t upload(const std::vector<T>& v, size_t min_bytes) {
        const hipError_t e = reserve(std::max(v.size() * sizeof(T), min_bytes));
        if (e != hipSuccess || v.empty()) return e;
        return hipMemcpy(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice);
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; bytes = 0; }
    template <class T> T* as() const { return (T*)p; }
};

// ---------------------------------------------------------------------------
// misc entry points
// ---------------------------------------------------------------------------
extern "C" uint32_t rr_abi_version(void) { return RR_ABI_VERSION; }
extern "C" int rr_device_count(void) try {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
} RR_GUARD_END("rr_device_count")
extern "C" const char* rr_last_error(void) { return tl_error.c_str(); }

