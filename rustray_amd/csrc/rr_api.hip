// rr_api.hip — host side of librustray_hip.so: the C ABI of include/rustray_hip.h.
//
// Replaces the frame loop of `RendererManager::start` (reference
// src/renderer.rs:105-172): instead of a shuffled queue of 2x2-pixel cells and
// num_cpus-2 worker threads calling Raytracing::render per pixel, one call
// uploads the frame constants and drives the wavefront kernels of
// rr_kernels.hip over batches of primary samples.
#include "../../include/rustray_hip.h"
#include "rr_bvh.h"
#include "rr_device.h"
#include "rr_frame_plan.h"
#include "rr_primary_setup.h"
#include "rr_query_pointers.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <initializer_list>
#include <new>
#include <stdexcept>
#include <limits>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <tuple>
#include <vector>

#include "rr_kernels.hip"

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
// replaces the old one), add_meshes.device and set_items.device (after the new state's upload, before the commit).  Not armed (always, outside the tests): one
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

enum TimerKernel { TK_CLOSEST, TK_SHADOW, TK_SHADE, TK_BINNING }; // what a timed launch ran (resolve_timers)
struct TimedLaunch { hipEvent_t a, b; TimerKernel kernel; bool level1; }; // level1: the kernel's level-1 build

struct rr_scene {
    int device = 0;
    int n_cus = 256;
    std::mutex mu;
    // scene data
    DevBuf items, nodes4, tnodes4, tris, trix, attrs, face_slot, materials, textures, texels, lights, flat_normals;
    DSceneView view{};
    std::vector<DItem> h_items;
    std::vector<ItemHost> item_host; // what rr_scene_update_materials needs to rebuild the item flag words
    // the meshes: where each one's records sit in the arenas (what an item takes from the mesh it names, rr_scene_set_items), how many
    // records the arenas hold (rr_scene_add_meshes appends behind them), the scene's own copy of the caller's arrays (the trees are
    // rebuilt from it when an edit of the item list changes their share of the traversal stack) and that share
    std::vector<MeshDev> mesh_table;
    std::vector<HostMesh> h_meshes;
    size_t n_nodes4 = 0, n_mesh_tris = 0;
    int blas_depth_limit = RR_BLAS_MAX_DEPTH;
    // per item: the extent of its surface along the rows of its transform (k_item_spans: minima, maxima, largest |local coordinate|; 9 doubles),
    // read back after every upload of the items' transforms; the top level's surface boxes are derived from it (exact_world_box)
    std::vector<double> h_spans;
    DevBuf spans, item_chunks;              // item_chunks: (item, first triangle) per workgroup of k_world_normals / k_item_spans (RR_ITEM_CHUNK triangles each)
    std::vector<uint32_t> h_chunk_item;     // the item of every chunk (chunks of one item are consecutive)
    std::vector<uint32_t> tex_width;
    std::vector<DTexture> h_textures; // descriptors of the uploaded images (copied into the material records, make_dmaterial)
    uint32_t n_materials = 0;
    uint32_t n_enabled_lights = 0;
    uint32_t tlas_node_capacity = 0;
    std::vector<float4> h_item_boxes; // padded world boxes per item (lo, hi), built by build_tlas, kept by upload_tlas
    DevBuf item_boxes;
    DevBuf sq_valid; // one 64-bit word per (enabled light, 64 shadow slots): which lanes hold a ray
    double tlas_reach[3] = {0.0, 0.0, 0.0}; // the top level's boxes are padded for ray origins within +-tlas_reach (build_tlas)
    double tlas_floor[3] = {0.0, 0.0, 0.0}; // ... and never for less than this: the items' own extent
    bool tlas_stale = false; // a top-level upload failed part-way: the device trees match no tlas_reach, the next frame rebuilds them
    // An update that failed and could not be rolled back either (update_all_or_nothing): the device holds a mix of two scenes, and every
    // frame call refuses until an update of that kind succeeds.  geometry: items, flat normals, top level; materials: materials, item flags.
    // lights: the light records; item_flags: the items' records after a failed rr_scene_update_item_flags.
    bool broken_geometry = false, broken_materials = false, broken_lights = false, broken_item_flags = false;
    std::vector<DMaterial> h_dmat; // the material records on the device (rr_scene_update_materials puts them back after a failed update)
    std::vector<DLight> h_lights;  // the light records on the device (rr_scene_update_lights puts them back after a failed update)
    int tlas_depth_limit = RR_TLAS_MAX_DEPTH; // the top level's share of the traversal stack (build_scene_records), for its rebuilds
    // frame state (grown on demand, reused across frames)
    DevBuf hit1;      // hit records of depth level 1 (the primary rays are derived from their index, not stored)
    DevBuf arena[4];  // ray records of the deeper live depth levels, SoA: r0 r1 r2 hit
    size_t arena_cap = 0; // rays
    uint32_t arena_factor = 2; // arena rays per primary ray of a batch; doubled after a frame that had to slice levels
    DevBuf sq[3];
    size_t sq_cap = 0;
    DevBuf acc_rgb, acc_normal, acc_depth, acc_id, acc_flags, shade_const;
    DevBuf region_xy, trace_order, pool, counters; // region_xy: pixel of each accumulator slot; trace_order: its output index
    // what primary_ray reads (rr_primary_setup.h): slot_c, the screen point of each slot's pixel centre, lives and dies with region_xy;
    // sample_tr, the screen offset of each sample, is uploaded when the sub-sample table or one of the frame constants in tr_key changes
    DevBuf slot_c, sample_tr;
    std::vector<uint16_t> tr_table; PrimarySampleKey tr_key{}; bool tr_valid = false;
    std::vector<DevBuf> pool_more; // further segments of per-batch counters, for batches with very many launches (kept for the next frame)
    DevBuf tmp_out[4];
    // ray queries (the host forms are the device forms behind a staging copy): what the launches of a device form read and write after the
    // call has returned belongs to the handle, grows on demand and is never shrunk.  query_rec: the packed records r0, r1, r2 and the walks'
    // raw hits (16 + 16 + 8 + 16 = 56 B per ray of the largest closest-hit or shadow query, host or device form; a shadow query uses 48 of
    // them); query_words: QW_* below; query_ids: the stream ids 0 .. n - 1 of rr_shade_rays_device without the caller's (4 B per result)
    DevBuf query_rec[4], query_words, query_ids;
    DevBuf multi_part[4], multi_cat[4]; // rr_render_multi: this device's compact buffers; on device slot 0 the concatenation of all
    hipStream_t multi_stream = nullptr; // rr_render_multi: this handle's own non-blocking stream (created on first use)
    void* multi_stage[4] = {nullptr, nullptr, nullptr, nullptr}; size_t multi_stage_bytes[4] = {0, 0, 0, 0}; // pinned staging, devices without peer access
    std::vector<uint32_t> h_region_xy;
    rr_region region_cached{0, 0, 0, 0};
    uint32_t region_w = 0, region_h = 0;
    // stats
    rr_frame_stats stats{};
    bool stats_final = false; // s->stats already holds the sums over the passes of rr_render_progressive_tiles (nothing to collect from the device)
    bool profiling = false;
    std::vector<TimedLaunch> timed;
    std::vector<hipEvent_t> event_pool;
    hipEvent_t frame_a = nullptr, frame_b = nullptr, count_ready = nullptr;
    hipStream_t last_stream = nullptr; // frame state (queues, accumulators) is shared: frames on different streams are serialised
    // level 1 in stages (run_level1_stages): this handle's second non-blocking stream, created on first use on the handle's device, and per
    // shadow-queue buffer the event behind its shade launch (first stream) and behind its shadow launch (second stream)
    hipStream_t overlap_stream = nullptr;
    hipEvent_t stage_shaded[3] = {nullptr, nullptr, nullptr}, stage_traced[3] = {nullptr, nullptr, nullptr};
    uint32_t overlap_stages = 0; // level-1 stages of the last frame that ran on the two streams (rr_scene_overlap_stages)
    uint32_t* h_count = nullptr; // pinned: level sizes read back between depth levels
    rr_tuning tuning{};          // rr_scene_set_tuning; all zero = automatic
    std::vector<uint16_t> table_cache; uint16_t table_samples = 0; // built-in sub-sample table of the last sample count
    // every device buffer is a DevBuf member (freed by its destructor, on the scene's device)
    ~rr_scene() {
        (void)hipSetDevice(device);
        for (hipEvent_t e : event_pool) (void)hipEventDestroy(e);
        for (auto& t : timed) { (void)hipEventDestroy(t.a); (void)hipEventDestroy(t.b); }
        if (frame_a) (void)hipEventDestroy(frame_a);
        if (frame_b) (void)hipEventDestroy(frame_b);
        if (count_ready) (void)hipEventDestroy(count_ready);
        if (h_count) (void)hipHostFree(h_count);
        if (multi_stream) (void)hipStreamDestroy(multi_stream);
        for (hipEvent_t e : stage_shaded) if (e) (void)hipEventDestroy(e);
        for (hipEvent_t e : stage_traced) if (e) (void)hipEventDestroy(e);
        if (overlap_stream) (void)hipStreamDestroy(overlap_stream);
        for (void* p : multi_stage) if (p) (void)hipHostFree(p);
    }
};

static const uint32_t POOL_WORDS = 1u << 22; // per-batch counters (level sizes, fetch heads, shadow shard counts): 16 MB, zeroed per batch

// ---------------------------------------------------------------------------
// the reference's sub-sample table: StdRng::seed_from_u64(0) + shuffle + truncate
// (reference src/raytracing.rs:290-313; rand 0.8: ChaCha12 core, PCG32 seed
// expansion, Fisher-Yates from the back with widening-multiply rejection)
// ---------------------------------------------------------------------------
namespace {

inline uint32_t rotl(uint32_t v, int n) { return (v << n) | (v >> (32 - n)); }

struct ChaCha12 {
    uint32_t key[8];
    uint64_t counter = 0;
    uint32_t block[16];
    int pos = 16;
    explicit ChaCha12(uint64_t seed) {
        uint64_t state = seed;
        for (int i = 0; i < 8; i++) { // SeedableRng::seed_from_u64
            state = state * 6364136223846793005ull + 11634580027462260723ull;
            uint32_t xs = (uint32_t)(((state >> 18) ^ state) >> 27);
            uint32_t rot = (uint32_t)(state >> 59);
            key[i] = (xs >> rot) | (xs << ((32u - rot) & 31u));
        }
    }
    void refill() {
        uint32_t in[16] = {0x61707865u, 0x3320646eu, 0x79622d32u, 0x6b206574u, key[0], key[1], key[2], key[3],
                           key[4], key[5], key[6], key[7], (uint32_t)counter, (uint32_t)(counter >> 32), 0u, 0u};
        uint32_t x[16];
        memcpy(x, in, sizeof x);
        auto qr = [&](int a, int b, int c, int d) {
            x[a] += x[b]; x[d] = rotl(x[d] ^ x[a], 16);
            x[c] += x[d]; x[b] = rotl(x[b] ^ x[c], 12);
            x[a] += x[b]; x[d] = rotl(x[d] ^ x[a], 8);
            x[c] += x[d]; x[b] = rotl(x[b] ^ x[c], 7);
        };
        for (int r = 0; r < 6; r++) { // 12 rounds = 6 double rounds
            qr(0, 4, 8, 12); qr(1, 5, 9, 13); qr(2, 6, 10, 14); qr(3, 7, 11, 15);
            qr(0, 5, 10, 15); qr(1, 6, 11, 12); qr(2, 7, 8, 13); qr(3, 4, 9, 14);
        }
        for (int i = 0; i < 16; i++) block[i] = x[i] + in[i];
        counter++;
        pos = 0;
    }
    uint32_t next_u32() { if (pos >= 16) refill(); return block[pos++]; }
    uint32_t below(uint32_t range) { // UniformInt<u32>::sample_single(0, range)
        uint32_t zone = (range << __builtin_clz(range)) - 1u;
        for (;;) {
            uint64_t m = (uint64_t)next_u32() * range;
            if ((uint32_t)m <= zone) return (uint32_t)(m >> 32);
        }
    }
};

uint32_t cell_size_of(uint16_t samples) {
    if (samples <= 1) return 1;
    uint16_t v = (uint16_t)(samples + 2);
    uint32_t p = 1;
    while (p < v) p <<= 1;
    return p / 2;
}

} // namespace

extern "C" int rr_sample_table(uint16_t samples, uint16_t* xy_out, uint32_t* cell_size_out) try {
    if (!xy_out && samples) return fail(RR_ERR_INVALID_ARGUMENT, "rr_sample_table: xy_out is NULL");
    if (samples > RR_MAX_SAMPLES) return fail(RR_ERR_UNSUPPORTED, "samples %u > %u", (unsigned)samples, RR_MAX_SAMPLES);
    uint32_t cs = cell_size_of(samples);
    std::vector<uint32_t> cells;
    try { cells.resize((size_t)cs * cs); } // 268 MB at the largest cell size: a failure must not cross the C ABI as an exception
    catch (const std::exception&) { return fail(RR_ERR_OUT_OF_MEMORY, "rr_sample_table: no host memory for %u x %u cells", cs, cs); }
    size_t k = 0;
    for (uint32_t xi = 0; xi < cs; xi++)
        for (uint32_t yi = 0; yi < cs; yi++) cells[k++] = xi | (yi << 16);
    ChaCha12 rng(0);
    for (size_t i = cells.size(); i-- > 1;) std::swap(cells[i], cells[rng.below((uint32_t)(i + 1))]);
    for (uint32_t s = 0; s < samples && s < cells.size(); s++) {
        xy_out[2 * s] = (uint16_t)(cells[s] & 0xffffu);
        xy_out[2 * s + 1] = (uint16_t)(cells[s] >> 16);
    }
    if (cell_size_out) *cell_size_out = cs;
    return RR_OK;
} RR_GUARD_END("rr_sample_table")

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

// xy: the region's pixels in OUTPUT order (tile order, row-major inside the tile; the ABI contract).
// trace_order (optional): a permutation of region indices = the order of the ACCUMULATOR SLOTS, in which
// primary rays are generated: 8x8-pixel blocks inside each tile, so that the 64 lanes of a wave start as one
// compact bundle of rays whatever the tile shape is (32x8 tiles traced in row-major order cost 4 % more than
// 8x8 blocks on sponza_syn) and add to 64 consecutive accumulator words.
static void fill_region(uint32_t w, uint32_t h, const rr_region& rg, std::vector<uint32_t>* xy, std::vector<uint32_t>* trace_order = nullptr) {
    xy->clear();
    if (trace_order) trace_order->clear();
    uint32_t tx = (w + rg.tile_w - 1) / rg.tile_w, ty = (h + rg.tile_h - 1) / rg.tile_h;
    for (uint32_t t = rg.rank; t < tx * ty; t += rg.n_ranks) {
        uint32_t x0 = (t % tx) * rg.tile_w, y0 = (t / tx) * rg.tile_h;
        uint32_t x1 = std::min(x0 + rg.tile_w, w), y1 = std::min(y0 + rg.tile_h, h);
        const uint32_t base = (uint32_t)xy->size(), tw = x1 - x0;
        for (uint32_t y = y0; y < y1; y++)
            for (uint32_t x = x0; x < x1; x++) xy->push_back(x | (y << 16));
        if (trace_order)
            for (uint32_t by = y0; by < y1; by += 8)
                for (uint32_t bx = x0; bx < x1; bx += 8)
                    for (uint32_t y = by; y < std::min(by + 8, y1); y++)
                        for (uint32_t x = bx; x < std::min(bx + 8, x1); x++) trace_order->push_back(base + (y - y0) * tw + (x - x0));
    }
}
static int check_region(uint32_t w, uint32_t h, const rr_region* rg) {
    if (!rg) return fail(RR_ERR_INVALID_ARGUMENT, "region is NULL");
    if (rg->tile_w == 0 || rg->tile_h == 0 || rg->n_ranks == 0 || rg->rank >= rg->n_ranks)
        return fail(RR_ERR_INVALID_ARGUMENT, "bad region: tile %ux%u rank %u of %u", rg->tile_w, rg->tile_h, rg->rank, rg->n_ranks);
    if (w == 0 || h == 0 || w > 65535u || h > 65535u) return fail(RR_ERR_INVALID_ARGUMENT, "bad frame size %ux%u", w, h);
    return RR_OK;
}
extern "C" uint64_t rr_region_pixel_count(uint32_t width, uint32_t height, const rr_region* rg) {
    if (check_region(width, height, rg) != RR_OK) return 0;
    uint32_t tx = (width + rg->tile_w - 1) / rg->tile_w, ty = (height + rg->tile_h - 1) / rg->tile_h;
    uint64_t n = 0;
    for (uint32_t t = rg->rank; t < tx * ty; t += rg->n_ranks) {
        uint32_t x0 = (t % tx) * rg->tile_w, y0 = (t / tx) * rg->tile_h;
        n += (uint64_t)(std::min(x0 + rg->tile_w, width) - x0) * (std::min(y0 + rg->tile_h, height) - y0);
    }
    return n;
}

// ---------------------------------------------------------------------------
// top level: upload, and the reach it is padded for (the scene's records and trees are built by rr_scene_build.h)
// ---------------------------------------------------------------------------
// The two trees into the scene's node buffer (the corner tree in its first half, the surface tree in the second: tlas_node_capacity
// nodes each) and the item boxes; then, and only then, the scene keeps what they were built for: the reach, the NaN-ball hint, the host
// copy of the boxes and the roots in the view.  A failed copy leaves all of that as it was and marks the device trees stale.
// Blocking copies.
// copy_tlas / keep_tlas: the two halves, which rr_scene_set_items runs on buffers built beside the scene's and at its commit.
static int copy_tlas(const TlasTrees& t, DNode4* tnodes4, uint32_t capacity, float4* item_boxes) {
    if (t.corner.size() > capacity || t.surface.size() > capacity)
        return fail(RR_ERR_DEVICE, "top-level rebuild needs %zu / %zu nodes, capacity %u", t.corner.size(), t.surface.size(), capacity);
    if (!t.corner.empty()) HIP_TRY(hipMemcpy(tnodes4, t.corner.data(), t.corner.size() * sizeof(DNode4), hipMemcpyHostToDevice));
    if (!t.surface.empty()) HIP_TRY(hipMemcpy(tnodes4 + capacity, t.surface.data(), t.surface.size() * sizeof(DNode4), hipMemcpyHostToDevice));
    if (!t.item_boxes.empty()) HIP_TRY(hipMemcpy(item_boxes, t.item_boxes.data(), t.item_boxes.size() * sizeof(float4), hipMemcpyHostToDevice));
    return RR_OK;
}
static void keep_tlas(rr_scene* s, TlasTrees& t) noexcept {
    for (int c = 0; c < 3; c++) s->tlas_reach[c] = t.reach[c];
    s->view.compat = t.nan_balls ? (s->view.compat | RR_VIEW_NAN_BALLS) : (s->view.compat & ~RR_VIEW_NAN_BALLS);
    s->h_item_boxes.swap(t.item_boxes);
    s->view.tlas_root4 = t.root;
    s->view.tnodes4c = t.has_surface ? s->tnodes4.as<DNode4>() + s->tlas_node_capacity : s->tnodes4.as<DNode4>();
    s->view.tlas_root4c = t.has_surface ? t.root_surface : t.root;
}
static int upload_tlas(rr_scene* s, TlasTrees& t) {
    if (t.corner.size() > s->tlas_node_capacity || t.surface.size() > s->tlas_node_capacity)
        return fail(RR_ERR_DEVICE, "top-level rebuild needs %zu / %zu nodes, capacity %u", t.corner.size(), t.surface.size(), s->tlas_node_capacity);
    s->tlas_stale = true;
    RR_TRY(copy_tlas(t, s->tnodes4.as<DNode4>(), s->tlas_node_capacity, s->item_boxes.as<float4>()));
    s->tlas_stale = false;
    keep_tlas(s, t);
    return RR_OK;
}

// Ray origins of the coming launch reach out to +-need: rebuilds the top level when its boxes were padded for less
// (a camera far outside the scene), or for more than 16x as much (the camera came back), or when an upload failed part-way.
// s->tlas_reach changes with the upload only (upload_tlas): after a failure the next frame from this camera rebuilds again.
static int ensure_tlas_reach(rr_scene* s, const double need[3]) {
    bool grow = false, shrink = s->tlas_stale;
    for (int c = 0; c < 3; c++) {
        if (need[c] > s->tlas_reach[c]) grow = true;
        if (s->tlas_reach[c] > 16.0 * std::max(need[c], s->tlas_floor[c])) shrink = true;
    }
    if (!grow && !shrink) return RR_OK;
    double want[3];
    for (int c = 0; c < 3; c++) want[c] = 2.0 * need[c]; // build_tlas raises it to the items' own extent
    TlasTrees trees;
    RR_TRY(build_tlas(s->h_items, s->h_spans, s->tlas_depth_limit, want, &trees));
    RR_FAULT_POINT("tlas_reach.upload");
    HIP_TRY(hipDeviceSynchronize());
    return upload_tlas(s, trees);
}
// the top level padded for the primary-ray origins of a camera: a bound on them (primary_ray: view_inv * (proj_inv * (sx, sy, -1, 1)).xyz1, |sx|, |sy| <= smax)
static int ensure_camera_reach(rr_scene* s, const rr_camera* cam, const rr_config* cfg) {
    double need[3];
    const double aperture = cfg ? std::max(1.0, (double)cfg->aperture_size) : 1.0;
    const double smax = 1.0 + 2.0 * (1.0 + aperture * cam->width / 800.0) * (2.0 / std::max(1u, std::min(cam->width, cam->height)));
    const double v[4] = {smax, smax, 1.0, 1.0};
    double pp[3];
    for (int k = 0; k < 3; k++) {
        pp[k] = 0.0;
        for (int j = 0; j < 4; j++) pp[k] += std::fabs((double)cam->projection_inverse[4 * j + k]) * v[j];
    }
    for (int c = 0; c < 3; c++) {
        double m = std::fabs((double)cam->view_inverse[12 + c]);
        for (int k = 0; k < 3; k++) m += std::fabs((double)cam->view_inverse[4 * k + c]) * pp[k];
        need[c] = m * 1.001;
    }
    return ensure_tlas_reach(s, need);
}

// DSceneView::flat_normals from the items and triangles on the device (k_world_normals); after every upload of the items' transforms
// ... and the extent of every item's surface along its transform's rows (k_item_spans -> s->h_spans, for the top level's surface boxes).
// Everything that depends on the transforms and on the meshes is derived HERE, on the device, where the meshes are resident: the one
// blocking copy of 72 B per item at the end is the call's only wait.
static_assert(RR_HOST_ITEM_CHUNK == RR_ITEM_CHUNK, "the host's chunk map is the kernels'");
// the spans of n items before any chunk is merged into them: what k_item_spans gives a ball or an empty mesh
static void empty_spans(uint32_t n, std::vector<double>* spans) {
    spans->resize(9 * (size_t)n);
    for (uint32_t i = 0; i < n; i++)
        for (int k = 0; k < 9; k++) (*spans)[9 * (size_t)i + k] = k < 3 ? std::numeric_limits<double>::infinity() : (k < 6 ? -std::numeric_limits<double>::infinity() : 0.0);
}
// one chunk's 9 doubles (k_item_spans) into its item's
static void merge_chunk_span(const double* q, double* d) {
    for (int k = 0; k < 9; k++) {
        if (q[k] != q[k]) d[k] = q[k];                       // a NaN chunk poisons the item (the corner box is kept for it)
        else if (d[k] == d[k]) d[k] = k < 3 ? std::min(d[k], q[k]) : std::max(d[k], q[k]);
    }
}
static int derive_from_transforms(rr_scene* s) {
    const uint32_t n = (uint32_t)s->h_items.size();
    s->h_spans.clear();
    if (n == 0) return RR_OK;
    if (s->h_chunk_item.empty()) { // the chunk map depends on the items' triangle counts only: laid out once
        std::vector<uint2> chunks;
        item_chunk_map(s->h_items, &chunks, &s->h_chunk_item);
        HIP_TRY(s->item_chunks.reserve(chunks.size() * sizeof(uint2)));
        HIP_TRY(hipMemcpy(s->item_chunks.p, chunks.data(), chunks.size() * sizeof(uint2), hipMemcpyHostToDevice));
        HIP_TRY(s->spans.reserve(9 * sizeof(double) * chunks.size()));
    }
    const size_t nc = s->h_chunk_item.size();
    if (nc > 0x7fffffffull) return fail(RR_ERR_UNSUPPORTED, "%zu chunks of instanced triangles", nc);
    hipLaunchKernelGGL(k_world_normals, dim3((uint32_t)nc), dim3(RR_BLOCK), 0, nullptr, s->items.as<DItem>(), s->item_chunks.as<uint2>(), s->tris.as<DTri>(), s->flat_normals.as<float4>());
    hipLaunchKernelGGL(k_item_spans, dim3((uint32_t)nc), dim3(RR_BLOCK), 0, nullptr, s->items.as<DItem>(), s->item_chunks.as<uint2>(), s->tris.as<DTri>(), s->spans.as<double>());
    HIP_TRY(hipGetLastError());
    std::vector<double> part(9 * nc);
    HIP_TRY(hipMemcpy(part.data(), s->spans.p, 9 * sizeof(double) * nc, hipMemcpyDeviceToHost)); // (waits for both kernels)
    empty_spans(n, &s->h_spans);
    for (size_t c = 0; c < nc; c++) merge_chunk_span(&part[9 * c], &s->h_spans[9 * (size_t)s->h_chunk_item[c]]);
    return RR_OK;
}

// Test-only (tests/test_abi.py; not in the header): the host half of rr_scene_create -- validation and the threaded mesh tree
// builds -- without a device, so that the no-throw guard and the worker net can be exercised on a CPU-only box.
extern "C" int rr_test_host_build(const rr_flat_scene* fs, uint64_t* n_nodes_out) try {
    int rc = validate_scene(fs);
    if (rc != RR_OK) return rc;
    RR_FAULT_POINT("scene_create.host");
    std::vector<rr::BvhResult> built(fs->n_meshes);
    std::vector<char> built_ok(fs->n_meshes, 0);
    build_mesh_trees(fs, RR_BLAS_MAX_DEPTH, &built, &built_ok);
    uint64_t n = 0;
    for (uint32_t mi = 0; mi < fs->n_meshes; mi++) {
        if (!built_ok[mi]) return fail(RR_ERR_UNSUPPORTED, "mesh %u: BVH depth limit exceeded", mi);
        n += built[mi].nodes.size();
    }
    if (n_nodes_out) *n_nodes_out = n;
    return RR_OK;
} RR_GUARD_END("rr_test_host_build")

// the images' texels into the RGBA8 pool, at the offsets their descriptors name (append_texture_layout)
static int upload_images(uint32_t* pool, const rr_texture* textures, uint32_t n, const DTexture* dtex) {
    for (uint32_t i = 0; i < n; i++) {
        const uint64_t texels = (uint64_t)dtex[i].width * dtex[i].height;
        if (texels) HIP_TRY(hipMemcpy(pool + dtex[i].offset, textures[i].rgba8, texels * 4, hipMemcpyHostToDevice));
    }
    return RR_OK;
}

extern "C" int rr_scene_create(const rr_flat_scene* fs, int device, rr_scene** out) try {
    if (!out) return fail(RR_ERR_INVALID_ARGUMENT, "out is NULL");
    *out = nullptr;
    RR_TRY(validate_scene(fs));
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(RR_ERR_NO_DEVICE, "no HIP device available");
    if (device < 0 || device >= ndev) return fail(RR_ERR_INVALID_ARGUMENT, "device %d of %d", device, ndev);
    HIP_TRY(hipSetDevice(device));
    std::unique_ptr<rr_scene> s(new rr_scene);
    RR_FAULT_POINT("scene_create.host");
    s->device = device;
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    s->n_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;

    // u8 -> f32 table, exactly (float)i / 255.0f
    float lut[256];
    for (int i = 0; i < 256; i++) lut[i] = (float)i / 255.0f;
    HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(c_u8_to_f32), lut, sizeof lut));

    // ---- the records, built on the host (rr_scene_build.h), then uploaded; an empty array still gets a buffer
    SceneRecords r;
    RR_TRY(build_scene_records(fs, &r));
    HIP_TRY(s->texels.reserve(std::max<uint64_t>(pool_texels(r.dtex), 1) * 4));
    RR_TRY(upload_images(s->texels.as<uint32_t>(), fs->textures, fs->n_textures, r.dtex.data()));
    HIP_TRY(s->textures.upload(r.dtex, sizeof(DTexture)));
    HIP_TRY(s->materials.upload(r.dmat, sizeof(DMaterial)));
    HIP_TRY(s->lights.upload(r.dlights, sizeof(DLight)));
    HIP_TRY(s->nodes4.upload(r.nodes4, 16));
    HIP_TRY(s->tris.upload(r.tris, 16));
    HIP_TRY(s->trix.upload(r.trix, 16));
    HIP_TRY(s->attrs.upload(r.attrs, 16));
    HIP_TRY(s->face_slot.upload(r.face_slot, 16));
    HIP_TRY(s->items.upload(r.items, 16));
    HIP_TRY(s->flat_normals.reserve(std::max<size_t>((size_t)r.n_flat_normals * sizeof(float4), 16)));
    // the host copies that the scene's edits and queries work from
    s->tex_width.swap(r.tex_width); s->h_textures.swap(r.dtex); s->h_dmat.swap(r.dmat); s->h_lights.swap(r.dlights);
    s->h_items.swap(r.items); s->item_host.swap(r.item_host);
    s->mesh_table.swap(r.meshes); s->n_nodes4 = r.nodes4.size(); s->n_mesh_tris = r.tris.size(); s->blas_depth_limit = r.blas_depth_limit;
    s->h_meshes.reserve(fs->n_meshes);
    for (uint32_t i = 0; i < fs->n_meshes; i++) s->h_meshes.emplace_back(fs->meshes[i]);
    s->n_materials = fs->n_materials;
    s->n_enabled_lights = r.n_enabled_lights;
    s->tlas_depth_limit = r.tlas_depth_limit;
    RR_TRY(derive_from_transforms(s.get())); // flat world normals; the extent of every item's surface, for the top level below

    // ---- top level: always present (even for one item), so the kernels have a single traversal path.
    // The reference's choice between "all items" and its scene BVH (src/raytracing.rs:434) only changes the
    // candidate set, never the result.
    {
        TlasTrees trees;
        const double none[3] = {0.0, 0.0, 0.0};
        RR_TRY(build_tlas(s->h_items, s->h_spans, s->tlas_depth_limit, none, &trees));
        for (int c = 0; c < 3; c++) s->tlas_floor[c] = trees.reach[c];
        s->tlas_node_capacity = std::max<uint32_t>((uint32_t)std::max(trees.corner.size(), trees.surface.size()), fs->n_items ? fs->n_items : 1u); // room for rebuilds after transform updates
        HIP_TRY(s->tnodes4.reserve(2 * (size_t)s->tlas_node_capacity * sizeof(DNode4)));
        HIP_TRY(hipMemset(s->tnodes4.p, 0, 2 * (size_t)s->tlas_node_capacity * sizeof(DNode4)));
        HIP_TRY(s->item_boxes.reserve(std::max<size_t>(trees.item_boxes.size() * sizeof(float4), 16)));
        s->view.tnodes4 = s->tnodes4.as<DNode4>();
        RR_TRY(upload_tlas(s.get(), trees));
    }

    DSceneView& v = s->view;
    v.flat_normals = s->flat_normals.as<float4>();
    v.items = s->items.as<DItem>(); v.nodes4 = s->nodes4.as<DNode4>(); v.tris = s->tris.as<DTri>(); v.trix = s->trix.as<DTriX>(); v.attrs = s->attrs.as<DTriAttr>();
    v.face_slot = s->face_slot.as<uint32_t>();
    v.materials = s->materials.as<DMaterial>(); v.textures = s->textures.as<DTexture>(); v.texels = s->texels.as<uint32_t>();
    v.lights = s->lights.as<DLight>();
    v.n_items = fs->n_items; v.n_lights = fs->n_lights; v.n_enabled_lights = s->n_enabled_lights;
    v.item_boxes = s->item_boxes.as<float4>();
    v.general_w = r.general_w ? 1u : 0u;
    v.any_alpha_occluder = r.any_alpha_occluder ? 1u : 0u;

    HIP_TRY(s->pool.reserve(POOL_WORDS * 4));
    HIP_TRY(s->counters.reserve(RR_CNT_WORDS * 8));
    HIP_TRY(hipEventCreate(&s->frame_a));
    HIP_TRY(hipEventCreate(&s->frame_b));
    HIP_TRY(hipEventCreateWithFlags(&s->count_ready, hipEventDisableTiming));
    HIP_TRY(hipHostMalloc((void**)&s->h_count, 64, hipHostMallocDefault));
    *out = s.release();
    return RR_OK;
} RR_GUARD_END("rr_scene_create")

extern "C" void rr_scene_destroy(rr_scene* s) {
    if (!s) return;
    try {
        (void)hipSetDevice(s->device);
        (void)hipDeviceSynchronize();
        delete s; // ~rr_scene: events, pinned memory; ~DevBuf: every device buffer
    } catch (...) { (void)guard_fail("rr_scene_destroy"); }
}

// ---------------------------------------------------------------------------
// scene edits: all or nothing
// ---------------------------------------------------------------------------
// Runs apply(); when it fails -- a status code or an exception -- runs restore(), which puts back everything apply may have written,
// and returns apply's status and message.  When restore fails as well the scene holds a mix of before and after: *broken is set, and
// frame calls refuse (check_intact) until an update of the same kind succeeds.
template <class Apply, class Restore>
static int all_or_nothing(const char* fn, bool* broken, Apply apply, Restore restore) {
    int rc;
    try { rc = apply(); } catch (...) { rc = guard_fail(fn); }
    if (rc == RR_OK) { *broken = false; return RR_OK; }
    std::string msg;
    try { msg = tl_error; } catch (...) { /* the code still says what happened */ }
    int rrc;
    try { rrc = restore(); } catch (...) { rrc = guard_fail(fn); }
    if (rrc != RR_OK) {
        *broken = true;
        return fail(rc, "%s; rolling back failed too (%s): the scene is broken until an update succeeds", msg.c_str(), tl_error.c_str());
    }
    try { tl_error = msg; } catch (...) {}
    return rc;
}
// every frame call on a scene: a scene that a failed update left mixed is not rendered
static int check_intact(const rr_scene* s) {
    if (s->broken_geometry || s->broken_materials || s->broken_lights || s->broken_item_flags)
        return fail(RR_ERR_DEVICE, "the scene is broken: a failed %s update could not be rolled back (update again, or create the scene anew)",
                    s->broken_geometry ? "transform" : s->broken_materials ? "material" : s->broken_lights ? "light" : "item flag");
    return RR_OK;
}

// The items' records to the device, then what derives from their transforms there: the update's way there and its way back.
static int upload_items_and_derive(rr_scene* s) {
    HIP_TRY(hipDeviceSynchronize()); // no frame may be in flight on the records that change (a caller that renders asynchronously through rr_render_region_device)
    HIP_TRY(hipMemcpyAsync(s->items.p, s->h_items.data(), s->h_items.size() * sizeof(DItem), hipMemcpyHostToDevice, nullptr));
    RR_FAULT_POINT("update_transforms.derive");
    return derive_from_transforms(s);
}

// All or nothing: every matrix is checked before anything is written, and a failure after the first write puts the items, their
// flat normals and spans, the top level and the view back as they were (derive_from_transforms and build_tlas are deterministic).
extern "C" int rr_scene_update_transforms(rr_scene* s, const float* trans, const float* trans_inv) try {
    if (!s || !trans || !trans_inv) return fail(RR_ERR_INVALID_ARGUMENT, "NULL argument");
    RR_TRY(not_in_pass(s, "rr_scene_update_transforms"));
    std::lock_guard<std::mutex> lk(s->mu);
    HIP_TRY(hipSetDevice(s->device));
    RR_FAULT_POINT("update_transforms.host");
    const uint32_t n = (uint32_t)s->h_items.size();
    bool general_w = false;
    for (uint32_t i = 0; i < n; i++) {
        const float *t = trans + 16 * (size_t)i, *ti = trans_inv + 16 * (size_t)i;
        RR_TRY(check_item_transform(i, t, ti));
        if (!affine_inverse(make_float4(ti[3], ti[7], ti[11], ti[15]))) general_w = true;
    }
    // what the update writes, for the way back
    const std::vector<DItem> items0 = s->h_items;
    const std::vector<double> spans0 = s->h_spans;
    const std::vector<float4> boxes0 = s->h_item_boxes;
    double reach0[3], floor0[3];
    memcpy(reach0, s->tlas_reach, sizeof reach0); memcpy(floor0, s->tlas_floor, sizeof floor0);
    const DSceneView view0 = s->view;
    auto apply = [&]() -> int {
        for (uint32_t i = 0; i < n; i++) fill_item_matrices(s->h_items[i], trans + 16 * (size_t)i, trans_inv + 16 * (size_t)i);
        RR_TRY(upload_items_and_derive(s));
        s->view.general_w = general_w ? 1u : 0u;
        TlasTrees trees;
        const double none[3] = {0.0, 0.0, 0.0};
        RR_TRY(build_tlas(s->h_items, s->h_spans, s->tlas_depth_limit, none, &trees)); // the next frame's camera grows the reach again if it has to
        RR_FAULT_POINT("update_transforms.upload_tlas");
        RR_TRY(upload_tlas(s, trees));
        for (int c = 0; c < 3; c++) s->tlas_floor[c] = s->tlas_reach[c];
        return RR_OK;
    };
    auto restore = [&]() -> int {
        s->h_items = items0; s->h_spans = spans0; s->h_item_boxes = boxes0;
        memcpy(s->tlas_reach, reach0, sizeof reach0); memcpy(s->tlas_floor, floor0, sizeof floor0);
        s->view = view0;
        RR_TRY(upload_items_and_derive(s)); // the flat normals and spans of before, bit for bit
        TlasTrees trees;
        RR_TRY(build_tlas(s->h_items, s->h_spans, s->tlas_depth_limit, reach0, &trees)); // reach0 already covers the items: the same reach, boxes and trees as before
        RR_TRY(upload_tlas(s, trees));
        s->view = view0;
        return RR_OK;
    };
    return all_or_nothing("rr_scene_update_transforms", &s->broken_geometry, apply, restore);
} RR_GUARD_END("rr_scene_update_transforms")

// Records of an update to buffers that hold them already: the update's way there and its way back.  `point` (a test's fault point) is
// crossed after the first copy: between the two of a material update, behind the only one of the others.
struct RecordCopy { void* dst; const void* src; size_t bytes; };
static int copy_records(const char* point, std::initializer_list<RecordCopy> copies) {
    HIP_TRY(hipDeviceSynchronize()); // no frame enqueued through rr_render_region_device may still read the records
    for (const RecordCopy& c : copies) {
        if (c.bytes) HIP_TRY(hipMemcpy(c.dst, c.src, c.bytes, hipMemcpyHostToDevice));
        if (&c == copies.begin()) RR_FAULT_POINT(point);
    }
    return RR_OK;
}
template <class T> static RecordCopy records_to(const DevBuf& b, const std::vector<T>& v) { return RecordCopy{b.p, v.data(), v.size() * sizeof(T)}; }

// Material edits between frames (GUI sliders: reference src/run.rs:1132-1133 writes through Material::apply_diff,
// src/shape/mod.rs:182-242): every material record is replaced and the item flag words derived from the material
// caches are rebuilt; geometry, acceleration structures and texture images stay as uploaded.  All or nothing: after a failed copy the
// records of before are copied back.
extern "C" int rr_scene_update_materials(rr_scene* s, const rr_material* materials, uint32_t n_materials) try {
    if (!s || !materials) return fail(RR_ERR_INVALID_ARGUMENT, "NULL argument");
    RR_TRY(not_in_pass(s, "rr_scene_update_materials"));
    std::lock_guard<std::mutex> lk(s->mu);
    if (n_materials != s->n_materials) return fail(RR_ERR_INVALID_ARGUMENT, "%u materials, the scene was created with %u", n_materials, s->n_materials);
    RR_TRY(check_material_textures(materials, n_materials, s->tex_width.size()));
    for (const ItemHost& ih : s->item_host)
        if (carries_textures(materials[ih.material_cache]))
            return fail(RR_ERR_INVALID_ARGUMENT, "material %d is a material cache and must not carry textures (reference src/shape/mod.rs:769-772)", ih.material_cache);
    HIP_TRY(hipSetDevice(s->device));
    std::vector<DMaterial> dmat(n_materials);
    for (uint32_t i = 0; i < n_materials; i++) dmat[i] = make_dmaterial(materials[i], s->tex_width, s->h_textures);
    // the item flag words and the alpha-occluder hint of the new materials: the scene keeps them once both copies have succeeded
    std::vector<DItem> items = s->h_items;
    uint32_t any_alpha_occluder = 0u;
    for (size_t i = 0; i < s->item_host.size(); i++) {
        items[i].flags = item_flags(s->item_host[i], materials[s->item_host[i].material_cache], materials[s->item_host[i].material], s->tex_width);
        if (items[i].flags & RR_IF_OCCLUDER_ALPHA_TEX) any_alpha_occluder = 1u;
    }
    auto apply = [&]() -> int { return copy_records("update_materials.device", {records_to(s->materials, dmat), records_to(s->items, items)}); };
    auto restore = [&]() -> int { // the host copies still hold the records of before
        return copy_records("update_materials.device", {records_to(s->materials, s->h_dmat), records_to(s->items, s->h_items)});
    };
    RR_TRY(all_or_nothing("rr_scene_update_materials", &s->broken_materials, apply, restore));
    s->h_items.swap(items);
    s->h_dmat.swap(dmat);
    s->view.any_alpha_occluder = any_alpha_occluder;
    return RR_OK;
} RR_GUARD_END("rr_scene_update_materials")

// Light edits between frames (the GUI's light panel: reference src/run.rs:1294-1409 adds, edits and deletes `Scene::lights`): the
// whole list is replaced; its length may change.  A light's index is the RNG stream of its shadow jitter, so the list is taken in
// the caller's order, as rr_scene_create takes it.  A list longer than the buffer holds goes to a new buffer that replaces the old
// one only after the copy.  All or nothing: after a failed copy the records of before are copied back.
extern "C" int rr_scene_update_lights(rr_scene* s, const rr_light* lights, uint32_t n_lights) try {
    if (!s || (n_lights && !lights)) return fail(RR_ERR_INVALID_ARGUMENT, "NULL argument");
    RR_TRY(not_in_pass(s, "rr_scene_update_lights"));
    std::lock_guard<std::mutex> lk(s->mu);
    RR_TRY(check_lights(lights, n_lights));
    HIP_TRY(hipSetDevice(s->device));
    uint32_t n_enabled = 0;
    std::vector<DLight> dl = make_dlights(lights, n_lights, &n_enabled);
    DevBuf grown; // a list longer than the scene's buffer holds goes to a new one
    const bool grow = (size_t)n_lights * sizeof(DLight) > s->lights.bytes;
    if (grow) HIP_TRY(grown.reserve((size_t)n_lights * sizeof(DLight)));
    auto apply = [&]() -> int { return copy_records("update_lights.device", {records_to(grow ? grown : s->lights, dl)}); };
    auto restore = [&]() -> int { return copy_records("update_lights.device", {records_to(s->lights, s->h_lights)}); };
    RR_TRY(all_or_nothing("rr_scene_update_lights", &s->broken_lights, apply, restore));
    // the device holds the new records: the frame path reads the count, the enabled count (shadow-queue plan, fixed shadow slots) and the pointer together
    if (grow) s->lights = std::move(grown); // frees the old buffer: nothing reads it since the synchronisation in copy_records
    s->h_lights.swap(dl);
    s->n_enabled_lights = n_enabled;
    s->view.lights = s->lights.as<DLight>();
    s->view.n_lights = n_lights;
    s->view.n_enabled_lights = n_enabled;
    return RR_OK;
} RR_GUARD_END("rr_scene_update_lights")

// The GUI's "Visible" and "flip normals" checkboxes (reference src/run.rs:1464-1489, ShapeBasics::visible / flip_normals): only
// RR_IF_VISIBLE and RR_IF_FLIP_NORMALS of each item's flag word change.  The kernels read both per candidate and per hit
// (rr_kernels.hip), the flat world normals hold both signs, and hidden items keep their place in the top level: nothing is re-derived.
// item_host keeps the new values, from which rr_scene_update_materials rebuilds the flag words.  All or nothing, as the others.
extern "C" int rr_scene_update_item_flags(rr_scene* s, const uint8_t* visible, const uint8_t* flip_normals, uint32_t n_items) try {
    if (!s || !visible || !flip_normals) return fail(RR_ERR_INVALID_ARGUMENT, "NULL argument");
    RR_TRY(not_in_pass(s, "rr_scene_update_item_flags"));
    std::lock_guard<std::mutex> lk(s->mu);
    if (n_items != s->h_items.size()) return fail(RR_ERR_INVALID_ARGUMENT, "%u items, the scene was created with %zu", n_items, s->h_items.size());
    HIP_TRY(hipSetDevice(s->device));
    std::vector<DItem> items = s->h_items;
    for (uint32_t i = 0; i < n_items; i++)
        items[i].flags = (items[i].flags & ~(uint32_t)(RR_IF_VISIBLE | RR_IF_FLIP_NORMALS)) | (visible[i] ? (uint32_t)RR_IF_VISIBLE : 0u) |
                         (flip_normals[i] ? (uint32_t)RR_IF_FLIP_NORMALS : 0u);
    auto apply = [&]() -> int { return copy_records("update_item_flags.device", {records_to(s->items, items)}); };
    auto restore = [&]() -> int { return copy_records("update_item_flags.device", {records_to(s->items, s->h_items)}); };
    RR_TRY(all_or_nothing("rr_scene_update_item_flags", &s->broken_item_flags, apply, restore));
    s->h_items.swap(items);
    for (uint32_t i = 0; i < n_items; i++) { s->item_host[i].visible = visible[i] != 0; s->item_host[i].flip_normals = flip_normals[i] != 0; }
    return RR_OK;
} RR_GUARD_END("rr_scene_update_item_flags")

// A material's texture "+" (reference src/run.rs:936-947 loads a new image): the images are appended to the scene's texture list,
// in order, and *first_index is the index of the first.  rr_scene_create lays the RGBA8 pool out in list order, so the existing
// images keep their offsets and the new ones get those a scene created with the longer list gives them.  The grown pool and
// descriptor array are built aside (device-to-device copy of the old pool, upload of the new images) and replace the old ones only
// once complete: a failure leaves the scene as it was, with nothing to roll back.  Texture memory never shrinks.
extern "C" int rr_scene_add_textures(rr_scene* s, const rr_texture* textures, uint32_t n_textures, uint32_t* first_index) try {
    if (!s || !first_index || (n_textures && !textures)) return fail(RR_ERR_INVALID_ARGUMENT, "NULL argument");
    RR_TRY(not_in_pass(s, "rr_scene_add_textures"));
    std::lock_guard<std::mutex> lk(s->mu);
    RR_TRY(check_textures(textures, n_textures));
    const uint32_t first = (uint32_t)s->tex_width.size();
    if (n_textures == 0) { *first_index = first; return RR_OK; }
    HIP_TRY(hipSetDevice(s->device));
    std::vector<DTexture> dtex = s->h_textures;
    std::vector<uint32_t> widths = s->tex_width;
    const uint64_t old_texels = pool_texels(dtex);
    append_texture_layout(textures, n_textures, &dtex, &widths);
    DevBuf texels, descs;
    HIP_TRY(texels.reserve(std::max<uint64_t>(pool_texels(dtex), 1) * 4));
    if (old_texels) HIP_TRY(hipMemcpy(texels.p, s->texels.p, old_texels * 4, hipMemcpyDeviceToDevice)); // frames in flight only read the old pool
    RR_TRY(upload_images(texels.as<uint32_t>(), textures, n_textures, &dtex[first]));
    HIP_TRY(descs.upload(dtex, sizeof(DTexture)));
    RR_FAULT_POINT("add_textures.device");
    HIP_TRY(hipDeviceSynchronize()); // no frame enqueued through rr_render_region_device may still read the pool that is freed below
    // the pool and the descriptors of the longer list replace the old ones (frees them); material records keep their descriptors
    // (the old images did not move) and name the new images after a rr_scene_update_materials
    s->texels = std::move(texels);
    s->textures = std::move(descs);
    s->h_textures.swap(dtex);
    s->tex_width.swap(widths);
    s->view.texels = s->texels.as<uint32_t>();
    s->view.textures = s->textures.as<DTexture>();
    *first_index = first;
    return RR_OK;
} RR_GUARD_END("rr_scene_add_textures")

// ---------------------------------------------------------------------------
// structural edits: meshes appended, the item list replaced
// ---------------------------------------------------------------------------
// Both build what changes BESIDE what the scene holds -- new device buffers, new host vectors -- and commit by moving buffers, host
// copies and the view last, after the device has finished every frame in flight.  Nothing the scene renders from is written before
// the commit and nothing in the commit can fail, so a failure leaves the scene exactly as it was: there is no way back to take and
// no "broken" state (check_intact has no flag for these).

// The device copies of the mesh arenas: `before` records of the scene's own buffers (device to device), then the host's records.
struct MeshBuffers { DevBuf nodes4, tris, trix, attrs, face_slot; };
template <class T> static int grown_copy(DevBuf* dst, const DevBuf& resident, size_t before, const std::vector<T>& more) {
    HIP_TRY(dst->reserve(std::max<size_t>((before + more.size()) * sizeof(T), 16)));
    if (before) HIP_TRY(hipMemcpy(dst->p, resident.p, before * sizeof(T), hipMemcpyDeviceToDevice)); // frames in flight only read the resident records
    if (!more.empty()) HIP_TRY(hipMemcpy(dst->as<T>() + before, more.data(), more.size() * sizeof(T), hipMemcpyHostToDevice));
    return RR_OK;
}
static int upload_mesh_arenas(const rr_scene* s, const MeshArenas& a, MeshBuffers* b) {
    RR_TRY(grown_copy(&b->nodes4, s->nodes4, a.nodes4_before, a.nodes4));
    RR_TRY(grown_copy(&b->tris, s->tris, a.tris_before, a.tris));
    RR_TRY(grown_copy(&b->trix, s->trix, a.tris_before, a.trix));
    RR_TRY(grown_copy(&b->attrs, s->attrs, a.tris_before, a.attrs));
    return grown_copy(&b->face_slot, s->face_slot, a.tris_before, a.face_slot);
}
// the commit's half for the meshes
static void keep_mesh_buffers(rr_scene* s, MeshBuffers& b) noexcept {
    s->nodes4 = std::move(b.nodes4); s->tris = std::move(b.tris); s->trix = std::move(b.trix); s->attrs = std::move(b.attrs); s->face_slot = std::move(b.face_slot);
    DSceneView& v = s->view;
    v.nodes4 = s->nodes4.as<DNode4>(); v.tris = s->tris.as<DTri>(); v.trix = s->trix.as<DTriX>(); v.attrs = s->attrs.as<DTriAttr>(); v.face_slot = s->face_slot.as<uint32_t>();
}

// The GUI's "add ground plane" (reference src/scene.rs:1564-1578 loads a scene file with a mesh the scene does not hold yet): the
// meshes are appended to the scene's mesh list, in order, and *first_index is the index of the first.  A mesh's records name
// nothing outside the mesh (rr_scene_build.h: MeshArenas), so the resident meshes keep their records and the new ones get those a
// scene created with the longer list gives them; their trees are built for the scene's current share of the traversal stack.
// Nothing is rendered from them until rr_scene_set_items names them.  Mesh memory never shrinks.
extern "C" int rr_scene_add_meshes(rr_scene* s, const rr_mesh* meshes, uint32_t n_meshes, uint32_t* first_index) try {
    if (!s || !first_index || (n_meshes && !meshes)) return fail(RR_ERR_INVALID_ARGUMENT, "NULL argument");
    RR_TRY(not_in_pass(s, "rr_scene_add_meshes"));
    std::lock_guard<std::mutex> lk(s->mu);
    const uint32_t first = (uint32_t)s->mesh_table.size();
    RR_TRY(check_meshes(meshes, n_meshes, first));
    if (n_meshes == 0) { *first_index = first; return RR_OK; }
    if ((uint64_t)first + n_meshes > 0x7fffffffull) return fail(RR_ERR_UNSUPPORTED, "%u + %u meshes (rr_item::mesh is an int32_t)", first, n_meshes);
    HIP_TRY(hipSetDevice(s->device));
    MeshArenas a;
    a.meshes = s->mesh_table;
    a.tris_before = s->n_mesh_tris; a.nodes4_before = s->n_nodes4;
    RR_TRY(append_mesh_records(meshes, n_meshes, s->blas_depth_limit, (uint32_t)s->h_items.size(), &a));
    std::vector<HostMesh> h_meshes;
    h_meshes.reserve(s->h_meshes.size() + n_meshes);
    for (uint32_t i = 0; i < n_meshes; i++) h_meshes.emplace_back(meshes[i]);
    s->h_meshes.reserve(s->h_meshes.size() + n_meshes); // (capacity only: the commit's moves then cannot fail)
    MeshBuffers b;
    RR_TRY(upload_mesh_arenas(s, a, &b));
    RR_FAULT_POINT("add_meshes.device");
    HIP_TRY(hipDeviceSynchronize()); // no frame enqueued through rr_render_region_device may still read the arenas that are freed below
    // ---- commit
    keep_mesh_buffers(s, b);
    s->n_nodes4 = a.nodes4_before + a.nodes4.size(); s->n_mesh_tris = a.tris_before + a.tris.size();
    s->mesh_table.swap(a.meshes);
    for (HostMesh& m : h_meshes) s->h_meshes.push_back(std::move(m));
    *first_index = first;
    return RR_OK;
} RR_GUARD_END("rr_scene_add_meshes")

// The GUI's "delete" of an object, "add ground plane" and "add environment sphere" (reference src/scene.rs:1602-1620, :1564-1578):
// the whole item list and the whole material list are replaced, together -- items name materials by index, and a host that keeps
// the material caches behind the full materials moves every cache index when one item comes or goes.  Any item count, any order; an
// item may name any resident mesh, a material any resident texture; the checks and limits are rr_scene_create's.  Afterwards the
// handle renders, bit for bit, what a handle created from the flat scene (resident meshes and textures, current lights, these items
// and materials) renders.
//   Device work follows what changed: an item whose matrices, mesh and flag word are those of an item of the list before keeps that
// item's surface spans (host copy) and flat world normals (k_world_normals_edit copies its run into the new arena); only the other
// mesh items are derived.  The top level is rebuilt (host, items only).
//   The stack share: the top level's share of the traversal stack depends on the item count (stack_shares), and the per-mesh trees
// are built and collapsed for the rest.  An edit that changes the share rebuilds every mesh's records from the scene's host copies,
// as a fresh scene builds them (and derives every item: the leaf order changed); a mesh that no longer fits is RR_ERR_UNSUPPORTED.
extern "C" int rr_scene_set_items(rr_scene* s, const rr_item* items, uint32_t n_items, const rr_material* materials, uint32_t n_materials) try {
    if (!s || (n_items && !items) || (n_materials && !materials)) return fail(RR_ERR_INVALID_ARGUMENT, "NULL argument");
    RR_TRY(not_in_pass(s, "rr_scene_set_items"));
    std::lock_guard<std::mutex> lk(s->mu);
    RR_TRY(check_intact(s)); // (a scene that an earlier edit left mixed has no derived data worth keeping)
    RR_TRY(check_material_textures(materials, n_materials, s->tex_width.size()));
    int tlas_depth_limit = 0, blas_depth_limit = 0;
    if (n_items < (1u << 27)) RR_TRY(stack_shares(n_items, &tlas_depth_limit, &blas_depth_limit)); // the count's limits before an item is read
    RR_TRY(check_items(items, n_items, materials, n_materials, s->mesh_table.size()));
    HIP_TRY(hipSetDevice(s->device));

    // ---- the meshes, when their share of the stack changes: every record anew
    const bool rebuild_meshes = blas_depth_limit != s->blas_depth_limit && !s->h_meshes.empty();
    MeshArenas arenas;
    MeshBuffers mesh_buffers;
    if (rebuild_meshes) {
        std::vector<rr_mesh> views;
        views.reserve(s->h_meshes.size());
        for (const HostMesh& m : s->h_meshes) views.push_back(m.view());
        RR_TRY(append_mesh_records(views.data(), (uint32_t)views.size(), blas_depth_limit, n_items, &arenas));
        RR_TRY(upload_mesh_arenas(s, arenas, &mesh_buffers));
    }
    const std::vector<MeshDev>& mesh_table = rebuild_meshes ? arenas.meshes : s->mesh_table;
    const DTri* tris = rebuild_meshes ? mesh_buffers.tris.as<DTri>() : s->tris.as<DTri>();

    // ---- item and material records
    ItemRecords rec;
    RR_TRY(build_item_records(items, n_items, materials, mesh_table, s->tex_width, &rec));
    std::vector<DMaterial> dmat(n_materials);
    for (uint32_t i = 0; i < n_materials; i++) dmat[i] = make_dmaterial(materials[i], s->tex_width, s->h_textures);

    // ---- keep or derive, per chunk of the new chunk map
    std::vector<uint2> chunks;
    std::vector<uint32_t> chunk_item;
    item_chunk_map(rec.items, &chunks, &chunk_item);
    const size_t nc = chunks.size();
    if (nc > 0x7fffffffull) return fail(RR_ERR_UNSUPPORTED, "%zu chunks of instanced triangles", nc);
    std::vector<int32_t> keep_from;
    const bool old_spans = s->h_spans.size() == 9 * s->h_items.size();
    const std::vector<DItem> no_items;
    plan_item_reuse(rebuild_meshes || !old_spans ? no_items : s->h_items, rec.items, &keep_from);
    std::vector<uint32_t> chunk_src(nc, RR_CHUNK_DERIVE);
    std::vector<uint2> derive_chunks;
    std::vector<uint32_t> derive_item;
    for (size_t c = 0; c < nc; c++) {
        const uint32_t i = chunk_item[c];
        if (rec.items[i].flags & RR_IF_SPHERE) continue; // nothing is derived for a ball
        if (keep_from[i] >= 0) chunk_src[c] = s->h_items[keep_from[i]].wn_base;
        else { derive_chunks.push_back(chunks[c]); derive_item.push_back(i); }
    }
    const size_t nd = derive_chunks.size();

    // ---- the new device state, beside the old
    DevBuf d_items, d_materials, d_flat_normals, d_item_chunks, d_spans, d_chunk_src, d_derive_chunks, d_tnodes4, d_item_boxes;
    HIP_TRY(d_items.upload(rec.items, 16));
    HIP_TRY(d_materials.upload(dmat, sizeof(DMaterial)));
    HIP_TRY(d_flat_normals.reserve(std::max<size_t>((size_t)rec.n_flat_normals * sizeof(float4), 16)));
    HIP_TRY(d_item_chunks.upload(chunks, 16));
    HIP_TRY(d_spans.reserve(std::max<size_t>(9 * sizeof(double) * nc, 16))); // room for every chunk: a transform update derives them all
    HIP_TRY(d_chunk_src.upload(chunk_src, 16));
    HIP_TRY(d_derive_chunks.upload(derive_chunks, 16));
    std::vector<double> spans;
    empty_spans(n_items, &spans);
    for (uint32_t i = 0; i < n_items; i++)
        if (keep_from[i] >= 0) memcpy(&spans[9 * (size_t)i], &s->h_spans[9 * (size_t)keep_from[i]], 9 * sizeof(double));
    if (nc) hipLaunchKernelGGL(k_world_normals_edit, dim3((uint32_t)nc), dim3(RR_BLOCK), 0, nullptr, d_items.as<DItem>(), d_item_chunks.as<uint2>(), d_chunk_src.as<uint32_t>(),
                               tris, s->flat_normals.as<float4>(), d_flat_normals.as<float4>());
    if (nd) hipLaunchKernelGGL(k_item_spans, dim3((uint32_t)nd), dim3(RR_BLOCK), 0, nullptr, d_items.as<DItem>(), d_derive_chunks.as<uint2>(), tris, d_spans.as<double>());
    HIP_TRY(hipGetLastError());
    if (nd) {
        std::vector<double> part(9 * nd);
        HIP_TRY(hipMemcpy(part.data(), d_spans.p, 9 * sizeof(double) * nd, hipMemcpyDeviceToHost)); // (waits for both kernels)
        for (size_t c = 0; c < nd; c++) merge_chunk_span(&part[9 * c], &spans[9 * (size_t)derive_item[c]]);
    }

    // ---- the top level over the new items, as rr_scene_create builds it
    TlasTrees trees;
    const double none[3] = {0.0, 0.0, 0.0};
    RR_TRY(build_tlas(rec.items, spans, tlas_depth_limit, none, &trees));
    const uint32_t capacity = std::max<uint32_t>((uint32_t)std::max(trees.corner.size(), trees.surface.size()), n_items ? n_items : 1u);
    HIP_TRY(d_tnodes4.reserve(2 * (size_t)capacity * sizeof(DNode4)));
    HIP_TRY(hipMemset(d_tnodes4.p, 0, 2 * (size_t)capacity * sizeof(DNode4)));
    HIP_TRY(d_item_boxes.reserve(std::max<size_t>(trees.item_boxes.size() * sizeof(float4), 16)));
    RR_TRY(copy_tlas(trees, d_tnodes4.as<DNode4>(), capacity, d_item_boxes.as<float4>()));
    RR_FAULT_POINT("set_items.device");
    HIP_TRY(hipDeviceSynchronize()); // the kernels above; and no frame enqueued through rr_render_region_device may still read what is freed below

    // ---- commit: buffers, host copies, the view
    if (rebuild_meshes) {
        keep_mesh_buffers(s, mesh_buffers);
        s->mesh_table.swap(arenas.meshes);
        s->n_nodes4 = arenas.nodes4.size(); s->n_mesh_tris = arenas.tris.size();
    }
    s->blas_depth_limit = blas_depth_limit; s->tlas_depth_limit = tlas_depth_limit;
    s->items = std::move(d_items); s->materials = std::move(d_materials); s->flat_normals = std::move(d_flat_normals);
    s->item_chunks = std::move(d_item_chunks); s->spans = std::move(d_spans); s->tnodes4 = std::move(d_tnodes4); s->item_boxes = std::move(d_item_boxes);
    s->h_items.swap(rec.items); s->item_host.swap(rec.item_host); s->h_dmat.swap(dmat); s->h_spans.swap(spans); s->h_chunk_item.swap(chunk_item);
    s->n_materials = n_materials;
    s->tlas_node_capacity = capacity;
    DSceneView& v = s->view;
    v.items = s->items.as<DItem>(); v.materials = s->materials.as<DMaterial>(); v.flat_normals = s->flat_normals.as<float4>();
    v.tnodes4 = s->tnodes4.as<DNode4>(); v.item_boxes = s->item_boxes.as<float4>();
    v.n_items = n_items;
    v.general_w = rec.general_w ? 1u : 0u;
    v.any_alpha_occluder = rec.any_alpha_occluder ? 1u : 0u;
    for (int c = 0; c < 3; c++) s->tlas_floor[c] = trees.reach[c];
    keep_tlas(s, trees);
    s->tlas_stale = false;
    return RR_OK;
} RR_GUARD_END("rr_scene_set_items")

// ---------------------------------------------------------------------------
// frame
// ---------------------------------------------------------------------------
static int check_frame_args(const rr_scene* s, const rr_camera* cam, const rr_config* cfg, const uint16_t* sample_xy) {
    if (!s || !cam || !cfg) return fail(RR_ERR_INVALID_ARGUMENT, "NULL argument");
    if (cfg->samples == 0) return fail(RR_ERR_INVALID_ARGUMENT, "samples must be >= 1");
    // with the caller's table the reference's own u16 limit applies; the built-in table stops where its shuffle stays affordable
    if (cfg->samples > (sample_xy ? RR_MAX_SAMPLES_WITH_TABLE : RR_MAX_SAMPLES))
        return fail(RR_ERR_UNSUPPORTED, "samples %u > %u%s", (unsigned)cfg->samples, sample_xy ? RR_MAX_SAMPLES_WITH_TABLE : RR_MAX_SAMPLES,
                    sample_xy ? "" : " (the built-in sub-sample table; pass sample_xy for up to 32766)");
    if (cfg->max_recursion > RR_MAX_RECURSION) return fail(RR_ERR_UNSUPPORTED, "max_recursion %u > %u", cfg->max_recursion, RR_MAX_RECURSION);
    if (cam->width == 0 || cam->height == 0 || cam->width > 65535u || cam->height > 65535u) return fail(RR_ERR_INVALID_ARGUMENT, "bad frame size %ux%u", cam->width, cam->height);
    if (!finite16(cam->projection_inverse) || !finite16(cam->view_inverse)) return fail(RR_ERR_INVALID_ARGUMENT, "non-finite camera matrix");
    return RR_OK;
}

static hipEvent_t take_event(rr_scene* s) {
    if (!s->event_pool.empty()) { hipEvent_t e = s->event_pool.back(); s->event_pool.pop_back(); return e; }
    hipEvent_t e = nullptr;
    (void)hipEventCreate(&e);
    return e;
}
struct ScopedTimer {
    rr_scene* s; hipStream_t st; TimerKernel kernel; bool level1; hipEvent_t a = nullptr, b = nullptr;
    ScopedTimer(rr_scene* s_, hipStream_t st_, TimerKernel kernel_, bool level1_) : s(s_), st(st_), kernel(kernel_), level1(level1_) {
        if (s->profiling) { a = take_event(s); b = take_event(s); (void)hipEventRecord(a, st); }
    }
    ~ScopedTimer() { if (s->profiling) { (void)hipEventRecord(b, st); s->timed.push_back(TimedLaunch{a, b, kernel, level1}); } }
};

// the rr_frame_stats fields of each TimerKernel: every launch, and the launches of its level-1 build (binning: time only)
static const struct {
    double rr_frame_stats::*ms; uint64_t rr_frame_stats::*launches;
    double rr_frame_stats::*ms_level1; uint64_t rr_frame_stats::*launches_level1;
} k_timer_fields[] = {
    {&rr_frame_stats::ms_trace_closest, &rr_frame_stats::launches_trace_closest, &rr_frame_stats::ms_trace_closest_level1, &rr_frame_stats::launches_trace_closest_level1},
    {&rr_frame_stats::ms_trace_shadow, &rr_frame_stats::launches_trace_shadow, &rr_frame_stats::ms_trace_shadow_level1, &rr_frame_stats::launches_trace_shadow_level1},
    {&rr_frame_stats::ms_shade, &rr_frame_stats::launches_shade, &rr_frame_stats::ms_shade_level1, &rr_frame_stats::launches_shade_level1},
    {&rr_frame_stats::ms_binning, nullptr, nullptr, nullptr},
};

static void resolve_timers(rr_scene* s) {
    for (auto& t : s->timed) {
        float ms = 0.0f;
        if (hipEventSynchronize(t.b) == hipSuccess && hipEventElapsedTime(&ms, t.a, t.b) == hipSuccess) {
            const auto& f = k_timer_fields[t.kernel];
            s->stats.*f.ms += ms;
            if (f.launches) s->stats.*f.launches += 1;
            if (t.level1) { s->stats.*f.ms_level1 += ms; s->stats.*f.launches_level1 += 1; }
        }
        s->event_pool.push_back(t.a); s->event_pool.push_back(t.b);
    }
    s->timed.clear();
}

// ---- the output buffers of a frame, in rr_frame order, and their bytes per pixel: rgba8, normal (3 x f32), depth, object_id
static const size_t OUT_ELEM[4] = {4, 12, 4, 4};
static void* out_buffer(const rr_frame& f, int k) {
    void* const b[4] = {f.rgba8, f.normal, f.depth, f.object_id};
    return b[k];
}
// The device frame behind a frame for the host: s->tmp_out[k] of np pixels for every buffer `host` asks for, zeroed on request.
static int stage_outputs(rr_scene* s, const rr_frame& host, size_t np, bool zero, rr_frame* dev) {
    void* p[4] = {nullptr, nullptr, nullptr, nullptr};
    for (int k = 0; k < 4; k++) {
        if (!out_buffer(host, k)) continue;
        HIP_TRY(s->tmp_out[k].reserve(np * OUT_ELEM[k]));
        p[k] = s->tmp_out[k].p;
        if (zero) HIP_TRY(hipMemsetAsync(p[k], 0, np * OUT_ELEM[k], nullptr));
    }
    *dev = rr_frame{(uint8_t*)p[0], (float*)p[1], (float*)p[2], (uint32_t*)p[3]};
    return RR_OK;
}
// dev -> host for every buffer both have (np pixels each), on stream st; returns when they are on the host
static int copy_outputs(const rr_frame& host, const rr_frame& dev, size_t np, hipStream_t st) {
    for (int k = 0; k < 4; k++)
        if (out_buffer(host, k) && out_buffer(dev, k))
            HIP_TRY(hipMemcpyAsync(out_buffer(host, k), out_buffer(dev, k), np * OUT_ELEM[k], hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return RR_OK;
}

// Progressive preview (rr_render_progressive): after every device batch that ends on a whole slice of samples the
// accumulators are resolved over the samples finished so far and handed to the caller (the device frame -> `host`).
struct PassHook { rr_pass_fn fn; void* user; uint32_t min_passes; const rr_frame* host; };

// The ONE place that launches the closest-hit kernel: the frame path (run_level), rr_pick and rr_trace_rays all come through here, so a
// change to the kernel's arguments cannot leave one caller behind.  Every pointer the kernel may touch is checked here, on the host,
// before the launch: a NULL one would be a write to address 16 * i on the device.  Level 1 reads no ray records (the rays are
// derived from their index), so its queue carries the hit records only and its ray pointers are passed as NULL.
static int launch_trace_closest(rr_scene* s, bool primary, DRayQueue q, uint32_t* count, uint32_t* head, uint64_t n, const DShadeConst* kc,
                                const DPrimary& pr, unsigned long long* counters, hipStream_t st) {
    if (!count || !head || !q.hit || !kc || !counters) return fail(RR_ERR_DEVICE, "internal: closest-hit launch with a NULL argument");
    if (primary && (!pr.sample_tr || pr.n != n)) return fail(RR_ERR_DEVICE, "internal: level-1 closest-hit launch without its ray table");
    if (!primary && (!q.r0 || !q.r1 || !q.r2)) return fail(RR_ERR_DEVICE, "internal: closest-hit launch without ray records");
    if (n == 0 || n > 0x7fffff00ull) return fail(RR_ERR_DEVICE, "internal: closest-hit launch of %llu rays", (unsigned long long)n);
    const int grid = (int)std::min<uint64_t>((n + RR_BLOCK - 1) / RR_BLOCK, (uint64_t)s->n_cus * RR_CLOSEST_WAVES);
    if (primary) {
        q.r0 = nullptr; q.r1 = nullptr; q.r2 = nullptr;
        hipLaunchKernelGGL(k_trace_closest<true>, dim3(grid), dim3(RR_BLOCK), 0, st, s->view, q, count, head, kc, pr, counters);
    } else {
        hipLaunchKernelGGL(k_trace_closest<false>, dim3(grid), dim3(RR_BLOCK), 0, st, s->view, q, count, head, kc, pr, counters);
    }
    HIP_TRY(hipGetLastError());
    return RR_OK;
}

// The ONE place that launches the shadow-query kernel (rr_trace_shadow_rays), as launch_trace_closest: every pointer the kernel
// touches is checked here, on the host.  r0 / r1: n ray records each; out: n result records; head: the zeroed fetch word.
static int launch_query_shadow(rr_scene* s, const float4* r0, const float4* r1, uint64_t n, uint32_t* head, uint4* out, hipStream_t st) {
    if (!r0 || !r1 || !head || !out) return fail(RR_ERR_DEVICE, "internal: shadow-query launch with a NULL argument");
    if (!s->view.items || !s->view.tnodes4 || !s->view.item_boxes) return fail(RR_ERR_DEVICE, "internal: shadow-query launch on a scene without a top level");
    if (n == 0 || n > 0x7fffff00ull) return fail(RR_ERR_DEVICE, "internal: shadow-query launch of %llu rays", (unsigned long long)n);
    const int grid = (int)std::min<uint64_t>((n + RR_BLOCK - 1) / RR_BLOCK, (uint64_t)s->n_cus * RR_SHADOW_GRID_WG);
    hipLaunchKernelGGL(k_query_shadow, dim3(grid), dim3(RR_BLOCK), 0, st, s->view, r0, r1, (uint32_t)n, head, out);
    HIP_TRY(hipGetLastError());
    return RR_OK;
}

// ---- the steps of a frame (render_region_locked)

// the region's accumulator slots on the device (slot -> pixel, slot -> output index), uploaded when the region changes
static int update_region_map(rr_scene* s, uint32_t W, uint32_t H, const rr_region& rg, hipStream_t st) {
    if (memcmp(&s->region_cached, &rg, sizeof rg) == 0 && s->region_w == W && s->region_h == H) return RR_OK;
    std::vector<uint32_t> order;
    fill_region(W, H, rg, &s->h_region_xy, &order);
    HIP_TRY(hipStreamSynchronize(st));
    HIP_TRY(s->region_xy.reserve(std::max<size_t>(s->h_region_xy.size(), 1) * 4));
    HIP_TRY(s->slot_c.reserve(std::max<size_t>(s->h_region_xy.size(), 1) * 8));
    HIP_TRY(s->trace_order.reserve(std::max<size_t>(order.size(), 1) * 4));
    if (!s->h_region_xy.empty()) {
        // slot_xy[j] = pixel of accumulator slot j; slot_out[j] = its index in the compact output order
        std::vector<uint32_t> slot_xy(order.size());
        for (size_t j = 0; j < order.size(); j++) slot_xy[j] = s->h_region_xy[order[j]];
        HIP_TRY(hipMemcpy(s->region_xy.p, slot_xy.data(), slot_xy.size() * 4, hipMemcpyHostToDevice));
        std::vector<float> slot_c(slot_xy.size() * 2); // the pixel centres on the screen, as primary_ray adds the sample's offset to them
        primary_slot_centres(slot_xy.data(), slot_xy.size(), W, H, slot_c.data());
        HIP_TRY(hipMemcpy(s->slot_c.p, slot_c.data(), slot_c.size() * 4, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(s->trace_order.p, order.data(), order.size() * 4, hipMemcpyHostToDevice));
    }
    s->region_cached = rg; s->region_w = W; s->region_h = H;
    return RR_OK;
}

// the frame constants of a camera and config (n_region_pixels is the caller's)
static DFrame make_frame(const rr_camera* cam, const rr_config* cfg) {
    DFrame fr;
    memset(&fr, 0, sizeof fr);
    memcpy(fr.proj_inv, cam->projection_inverse, 64);
    memcpy(fr.view_inv, cam->view_inverse, 64);
    fr.width = cam->width; fr.height = cam->height; fr.samples = cfg->samples; fr.cell_size = cell_size_of(cfg->samples);
    fr.max_recursion = cfg->max_recursion; fr.monte_carlo = cfg->monte_carlo ? 1u : 0u; fr.gamma = cfg->gamma_correction ? 1u : 0u;
    fr.dof = (cfg->aperture_size > 1.0f && cfg->focal_length > 1.0f) ? 1u : 0u;
    fr.focal_length = cfg->focal_length; fr.aperture_size = cfg->aperture_size; fr.fog_density = cfg->fog_density;
    for (int k = 0; k < 3; k++) fr.fog_color[k] = cfg->fog_color[k];
    fr.seed_lo = (uint32_t)cfg->seed; fr.seed_hi = (uint32_t)(cfg->seed >> 32);
    return fr;
}

// the shade kernel's constants (scene view + frame), read from device memory
static int upload_shade_const(rr_scene* s, const DFrame& fr, const PrimaryFrame& ps, hipStream_t st) {
    DShadeConst hc;
    hc.sc = s->view; hc.fr = fr; hc.ps = ps;
    HIP_TRY(s->shade_const.reserve(sizeof hc));
    HIP_TRY(hipMemcpyAsync(s->shade_const.p, &hc, sizeof hc, hipMemcpyHostToDevice, st));
    HIP_TRY(hipStreamSynchronize(st)); // `hc` is a stack local
    return RR_OK;
}

// sample_tr on the device: the screen offset of every sample of this frame (primary_sample_offsets), uploaded only when the
// sub-sample table or a frame constant it depends on differs from what the buffer holds
static int upload_sample_table(rr_scene* s, const DFrame& fr, const uint16_t* sample_xy, hipStream_t st) {
    const uint32_t samples = fr.samples;
    if (!sample_xy) { // the built-in table depends on the sample count only: built once per count, not once per frame
        if (s->table_samples != samples) {
            s->table_samples = 0; // the cache names a sample count only once its table is complete
            try { s->table_cache.resize((size_t)samples * 2); }
            catch (const std::exception&) { return fail(RR_ERR_OUT_OF_MEMORY, "no host memory for the sub-sample table"); }
            RR_TRY(rr_sample_table((uint16_t)samples, s->table_cache.data(), nullptr));
            s->table_samples = (uint16_t)samples;
        }
        sample_xy = s->table_cache.data();
    }
    const PrimarySampleKey key{fr.width, fr.height, fr.cell_size, fr.dof, samples, fr.aperture_size};
    if (s->tr_valid && same_key(s->tr_key, key) && s->tr_table.size() == (size_t)samples * 2 &&
        memcmp(s->tr_table.data(), sample_xy, (size_t)samples * 4) == 0) return RR_OK;
    s->tr_valid = false;
    std::vector<float> tr;
    try { s->tr_table.assign(sample_xy, sample_xy + (size_t)samples * 2); tr.resize((size_t)samples * 2); }
    catch (const std::exception&) { return fail(RR_ERR_OUT_OF_MEMORY, "no host memory for the sample offsets"); }
    primary_sample_offsets(sample_xy, key, tr.data());
    HIP_TRY(hipStreamSynchronize(st)); // an earlier frame on this stream may still read the buffer
    HIP_TRY(s->sample_tr.reserve((size_t)samples * 8));
    HIP_TRY(hipMemcpyAsync(s->sample_tr.p, tr.data(), (size_t)samples * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(hipStreamSynchronize(st)); // `tr` is a local
    s->tr_key = key; s->tr_valid = true;
    return RR_OK;
}

// zeroed accumulators (and work counters) for npix slots; aux outputs the caller did not ask for are not accumulated at all
static int reset_accumulators(rr_scene* s, uint32_t npix, bool want_normal, bool want_depth, bool want_id, hipStream_t st, DAccum* acc) {
    HIP_TRY(s->acc_rgb.reserve((size_t)npix * 24));
    HIP_TRY(s->acc_normal.reserve((size_t)npix * 24));
    HIP_TRY(s->acc_depth.reserve((size_t)npix * 8));
    HIP_TRY(s->acc_id.reserve((size_t)npix * 4));
    HIP_TRY(s->acc_flags.reserve((size_t)npix * 4));
    HIP_TRY(hipMemsetAsync(s->acc_flags.p, 0, (size_t)npix * 4, st));
    HIP_TRY(hipMemsetAsync(s->acc_rgb.p, 0, (size_t)npix * 24, st));
    HIP_TRY(hipMemsetAsync(s->acc_normal.p, 0, (size_t)npix * 24, st));
    HIP_TRY(hipMemsetAsync(s->acc_depth.p, 0, (size_t)npix * 8, st));
    HIP_TRY(hipMemsetAsync(s->acc_id.p, 0, (size_t)npix * 4, st));
    HIP_TRY(hipMemsetAsync(s->counters.p, 0, RR_CNT_WORDS * 8, st));
    *acc = DAccum{s->acc_rgb.as<long long>(), want_normal ? s->acc_normal.as<long long>() : nullptr, want_depth ? s->acc_depth.as<long long>() : nullptr,
                  want_id ? s->acc_id.as<uint32_t>() : nullptr, (unsigned long long)npix, s->acc_flags.as<uint32_t>()};
    return RR_OK;
}

// Ray memory (rr_frame_plan.h): a quarter of what is free on the device, at most 64 GB (MI355X has 288 GB of HBM3E),
// unless rr_tuning::queue_budget_bytes says otherwise.  Memory already held by this scene's arena counts as free.
static int queue_budget(rr_scene* s, uint64_t* budget) {
    if (s->tuning.queue_budget_bytes) { *budget = s->tuning.queue_budget_bytes; return RR_OK; }
    size_t free_b = 0, total_b = 0;
    HIP_TRY(hipMemGetInfo(&free_b, &total_b));
    *budget = std::min<uint64_t>((free_b + 56ull * s->arena_cap + s->hit1.bytes) / 4, 64ull << 30);
    return RR_OK;
}

// how n hits of level 1 are cut into stages for the two-stream path (rr_frame_plan.h; the knobs: rr_kernels.hip)
static bool level1_stages_wanted(const rr_scene* s) { return RR_L1_OVERLAP >= 2 || (RR_L1_OVERLAP == 1 && s->tuning.shade_chunk_rays != 0); }
static Level1Stages level1_stages(const rr_scene* s, uint64_t n) {
    return plan_level1_stages(Level1StageInputs{n, s->n_enabled_lights, s->tuning.shade_chunk_rays, RR_L1_STAGE_RAYS, RR_L1_BUFFERS});
}

// the ray arena for M rays and the shadow queue for sq_need rays, with at least valid_need words of lane masks (grown, never shrunk)
static int grow_ray_queues(rr_scene* s, uint64_t M, uint64_t sq_need, uint64_t valid_need) {
    const size_t elem[4] = {16, 16, 8, 16};
    if (M > s->arena_cap) {
        for (int k = 0; k < 4; k++) HIP_TRY(s->arena[k].reserve(M * elem[k]));
        s->arena_cap = M;
    }
    if (sq_need > s->sq_cap) { // (one word of sq_valid per 64 rays of the queue)
        for (int k = 0; k < 3; k++) HIP_TRY(s->sq[k].reserve(sq_need * 16));
        HIP_TRY(s->sq_valid.reserve(std::max<uint64_t>(sq_need / RR_WAVE + 1, valid_need) * 8));
        s->sq_cap = sq_need;
    }
    return RR_OK;
}

// the frame's plan (rr_frame_plan.h), and its ray arena, level-1 hit records and shadow queue
static int plan_queues(rr_scene* s, uint32_t npix, const rr_config* cfg, uint32_t min_passes, FramePlan* plan) {
    uint64_t budget = 0;
    RR_TRY(queue_budget(s, &budget));
    const FramePlan& p = *plan = plan_frame(FramePlanInputs{npix, cfg->samples, cfg->max_recursion, budget, s->tuning.sample_group, min_passes,
                                                            s->arena_factor, s->n_enabled_lights, s->tuning.shade_chunk_rays});
    HIP_TRY(s->hit1.reserve(p.B * 16));
    // the shadow queue serves the serial loop and, where level 1 runs in stages, the stage buffers (their layout is the same for every batch)
    const Level1Stages sp = level1_stages(s, p.B);
    return grow_ray_queues(s, p.M, std::max<uint64_t>(p.sq_need, level1_stages_wanted(s) ? sp.sq_need : 0ull), sp.valid_need);
}

// Per-batch counters (level sizes, fetch heads, shadow shard counts) come out of zeroed segments of POOL_WORDS words.  A segment
// is never recycled inside a batch (launches still in flight and the levels above in the recursion hold pointers into it); a
// batch with more launches than one segment serves (a deeply branching scene in a very small ray arena) gets another one.
struct CounterPool {
    rr_scene* s; hipStream_t st;
    uint32_t* pool = nullptr;
    uint32_t next_word = 0;
    size_t pool_segment = 0; // 0 = s->pool, k = s->pool_more[k - 1]
    int start_batch() {
        pool = s->pool.as<uint32_t>(); pool_segment = 0;
        HIP_TRY(hipMemsetAsync(pool, 0, POOL_WORDS * 4, st));
        next_word = 0;
        return RR_OK;
    }
    // n zeroed words; nullptr = no memory for another segment
    uint32_t* take(uint32_t n) {
        if (next_word + n > POOL_WORDS) {
            if (pool_segment == s->pool_more.size()) {
                if (s->pool_more.size() >= 255) return nullptr; // 4 GB of counters: something else is wrong
                s->pool_more.emplace_back();
                if (s->pool_more.back().reserve(POOL_WORDS * 4) != hipSuccess) { s->pool_more.pop_back(); return nullptr; }
            }
            pool = s->pool_more[pool_segment++].as<uint32_t>();
            if (hipMemsetAsync(pool, 0, POOL_WORDS * 4, st) != hipSuccess) return nullptr;
            next_word = 0;
        }
        uint32_t* p = pool + next_word; next_word += n; return p;
    }
    void align_line() { next_word = (next_word + 31u) & ~31u; } // the next words start on a 128-B line
};
static int counters_exhausted() { return fail(RR_ERR_UNSUPPORTED, "out of memory for the per-launch counters of a batch"); }

// what the depth levels of a frame share
struct FrameRun {
    rr_scene* s; hipStream_t st;
    FramePlan plan; uint32_t R;
    DShadowQueue SQ; DAccum acc;
    CounterPool pool;
    DPrimary pr; // the batch being traced: depth level 1
    const volatile int* cancel;
    int shadow_grid, shade_grid_max;
    const uint32_t* slot_xy = nullptr; // accumulator slot -> RNG pixel as (x | y << 16): the region's map, or the stream ids of rr_shade_rays
    bool seeded = false;               // rr_shade_rays: depth level 1 is ray RECORDS at the front of the arena (k_seed_rays), not derived from its index
    DRayQueue queue_at(uint64_t base) const {
        return DRayQueue{s->arena[0].as<float4>() + base, s->arena[1].as<float4>() + base, s->arena[2].as<uint2>() + base, s->arena[3].as<uint4>() + base};
    }
};

// On request (rr_tuning::bin_min_rays) a deeper level of m rays at child_base is traced in bins of (origin cell, direction octant)
// when the sorted copy fits behind the unsorted one (rr_kernels.hip: ray binning; off by default, it does not pay).
// *level_base = child_base + m (the sorted copy) when the level was binned.
static int bin_level(FrameRun& f, uint64_t child_base, uint64_t m, uint64_t* level_base) {
    rr_scene* s = f.s;
    const uint64_t bin_min = s->tuning.bin_min_rays;
    if (bin_min == 0 || m < bin_min || f.plan.M - child_base < 3 * m + 2ull * RR_BLOCK * (f.R + 1)) return RR_OK;
    f.pool.align_line();
    int* bounds = (int*)f.pool.take(8);
    uint32_t* hist = f.pool.take(RR_BIN_COUNT);
    if (!bounds || !hist) return RR_OK;
    const int init[8] = {0x7f7fffff, 0x7f7fffff, 0x7f7fffff, (int)0x80800000, (int)0x80800000, (int)0x80800000, 0, 0}; // ordered(+FLT_MAX) x3, ordered(-FLT_MAX) x3
    HIP_TRY(hipMemcpyAsync(bounds, init, sizeof init, hipMemcpyHostToDevice, f.st));
    const DRayQueue qsrc = f.queue_at(child_base), qdst = f.queue_at(child_base + m);
    const int g = (int)std::min<uint64_t>((m + RR_BLOCK - 1) / RR_BLOCK, (uint64_t)s->n_cus * 8);
    ScopedTimer t(s, f.st, TK_BINNING, false);
    hipLaunchKernelGGL(k_bin_bounds, dim3(g), dim3(RR_BLOCK), 0, f.st, qsrc, (uint32_t)m, bounds);
    hipLaunchKernelGGL(k_bin_count, dim3(g), dim3(RR_BLOCK), 0, f.st, qsrc, (uint32_t)m, bounds, hist);
    hipLaunchKernelGGL(k_bin_prefix, dim3(1), dim3(1024), 0, f.st, hist);
    hipLaunchKernelGGL(k_bin_scatter, dim3(g), dim3(RR_BLOCK), 0, f.st, qsrc, qdst, (uint32_t)m, hist);
    *level_base = child_base + m;
    s->stats.binned_rays += m;
    return RR_OK;
}

// ---- level 1 in stages on two streams ---------------------------------------------------------------------------------------------
// k_shade<true> is bound by instruction issue and k_trace_shadow<true> by memory latency; one after the other, each has the whole
// GPU in turn.  Here the hits [s0, s1) are cut into stages (rr_frame_plan.h, plan_level1_stages): stage k is shaded on the frame's
// stream `st` into shadow buffer k % n_buf, and its shadow rays are traced on the handle's second stream behind an event that
// follows the shade launch, while `st` already shades stage k + 1.  Shade k + n_buf waits for the event behind shadow k, so a
// buffer is never rewritten while it is read.  `st` may be the legacy null stream and the second stream is non-blocking: all
// ordering is by these events.  The frame cannot change: the kernels are the serial loop's, every write they share is an integer
// atomic, and all else goes to the stage's own buffer.  Which frames take this path, and the sizes of the two grids: RR_L1_OVERLAP
// and the knobs after it (rr_kernels.hip), with what was measured.
static int ensure_overlap_stream(rr_scene* s) {
    if (!s->overlap_stream) HIP_TRY(hipStreamCreateWithFlags(&s->overlap_stream, hipStreamNonBlocking));
    for (int b = 0; b < 3; b++) {
        if (!s->stage_shaded[b]) HIP_TRY(hipEventCreateWithFlags(&s->stage_shaded[b], hipEventDisableTiming));
        if (!s->stage_traced[b]) HIP_TRY(hipEventCreateWithFlags(&s->stage_traced[b], hipEventDisableTiming));
    }
    return RR_OK;
}

// enqueues every stage; on any error the caller (run_level1_stages) drains both streams
static int enqueue_level1_stages(FrameRun& f, const Level1Stages& sp, const DRayQueue& qin, const uint32_t* count, uint64_t s0, uint64_t s1,
                                 const DRayQueue& qout, uint32_t* child_count, bool spawns) {
    rr_scene* s = f.s;
    const hipStream_t st = f.st, st2 = s->overlap_stream;
    const uint32_t L = s->n_enabled_lights;
    unsigned long long* counters = s->counters.as<unsigned long long>();
    if (sp.sq_need > s->sq_cap || sp.valid_need * 8 > s->sq_valid.bytes) return fail(RR_ERR_DEVICE, "internal: shadow queue smaller than its stage buffers");
    for (uint32_t k = 0; k < sp.n_stages; k++) {
        if (f.cancel && *f.cancel) return fail(RR_ERR_CANCELLED, "cancelled");
        const uint64_t c0 = s0 + sp.begin_of(k), c1 = std::min<uint64_t>(c0 + sp.stage, s1);
        const uint32_t b = sp.buffer_of(k);
        const bool first = k == 0, last = k + 1 == sp.n_stages;
        const uint64_t groups = (c1 - c0 + RR_BLOCK - 1) / RR_BLOCK;
        const uint32_t sq_chunk_cap = (uint32_t)(groups * RR_BLOCK); // <= sp.stage: L x this many slots fit the buffer
        const uint32_t segcap = (uint32_t)(((groups + RR_SQ_SHARDS - 1) / RR_SQ_SHARDS) * RR_BLOCK * L);
        const DShadowQueue SQ{f.SQ.s0 + sp.ray_offset[b], f.SQ.s1 + sp.ray_offset[b], f.SQ.s2 + sp.ray_offset[b]};
        unsigned long long* sq_valid = s->sq_valid.as<unsigned long long>() + sp.valid_offset[b];
        f.pool.align_line();
        uint32_t* sq_counts = f.pool.take(RR_SQ_SHARDS * RR_SQ_STRIDE);
        uint32_t* shead = f.pool.take(1); // (zeroed on `st` before the event the second stream waits for)
        if (!sq_counts || !shead) return counters_exhausted();
        // the first stage's shade and the last stage's shadow run alone: the serial loop's grids.  In between the two launches share the CUs.
        const uint64_t shade_wg = first ? (uint64_t)f.shade_grid_max : (RR_L1_SHADE_WG ? (uint64_t)s->n_cus * RR_L1_SHADE_WG : groups);
        const uint64_t shadow_wg = last ? (uint64_t)f.shadow_grid : (uint64_t)s->n_cus * RR_L1_SHADOW_WG;
        if (k >= sp.n_buf) HIP_TRY(hipStreamWaitEvent(st, s->stage_traced[b], 0));
        {
            ScopedTimer t(s, st, TK_SHADE, true);
            hipLaunchKernelGGL(k_shade<true>, dim3((uint32_t)std::min<uint64_t>(groups, shade_wg)), dim3(RR_BLOCK), 0, st, s->shade_const.as<DShadeConst>(), s->region_xy.as<uint32_t>(),
                               f.pr, qin, count, (uint32_t)c0, (uint32_t)c1, qout, child_count, SQ, sq_counts, segcap, sq_valid, sq_chunk_cap, f.acc, counters);
        }
        HIP_TRY(hipGetLastError());
        if (spawns && last) { // the next level's size, behind the last shade stage (run_level waits for it)
            HIP_TRY(hipMemcpyAsync(s->h_count, child_count, 4, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipEventRecord(s->count_ready, st));
        }
        HIP_TRY(hipEventRecord(s->stage_shaded[b], st));
        HIP_TRY(hipStreamWaitEvent(st2, s->stage_shaded[b], 0));
        {
            ScopedTimer t(s, st2, TK_SHADOW, true);
            const uint32_t sq_packets = (sq_chunk_cap / RR_WAVE) * L;
            const int sgrid = (int)std::min<uint64_t>(((uint64_t)sq_packets * RR_WAVE + RR_BLOCK - 1) / RR_BLOCK, shadow_wg);
            hipLaunchKernelGGL(k_trace_shadow<true>, dim3(sgrid), dim3(RR_BLOCK), 0, st2, s->view, SQ, sq_counts, segcap, sq_valid, sq_packets, shead, f.acc);
        }
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventRecord(s->stage_traced[b], st2));
    }
    // the second stream joins `st` here: before the deeper levels reuse the shadow queue, before k_resolve and before the frame's end event
    HIP_TRY(hipStreamWaitEvent(st, s->stage_traced[sp.buffer_of(sp.n_stages - 1)], 0));
    return RR_OK;
}

// THE one way in and out of the staged path: whatever ends it early (cancel flag, HIP error, counter pool exhausted) leaves both streams idle,
// so the handle stays usable and the next frame cannot race a straggler.
static int run_level1_stages(FrameRun& f, const Level1Stages& sp, const DRayQueue& qin, const uint32_t* count, uint64_t s0, uint64_t s1,
                             const DRayQueue& qout, uint32_t* child_count, bool spawns) {
    rr_scene* s = f.s;
    RR_TRY(ensure_overlap_stream(s));
    const int rc = enqueue_level1_stages(f, sp, qin, count, s0, s1, qout, child_count, spawns);
    if (rc != RR_OK) {
        (void)hipStreamSynchronize(s->overlap_stream);
        (void)hipStreamSynchronize(f.st);
        return rc;
    }
    s->overlap_stages += sp.n_stages;
    return RR_OK;
}

// One depth level: rays [base, base + n) of the arena, their count also in the device word `count`.
// The size of the next level is read back once per slice (4 bytes + stream sync), so launches are sized by the
// rays that exist and empty levels are never launched.
// depth level 1 = the batch's primary rays [pr.first, pr.first + pr.n): only hit records (hit1); its children start the arena
// SEEDED (rr_shade_rays): depth level 1 is n ray records at the front of the arena like any deeper level -- arena hit records, the
// <false> builds of the three kernels (a path is a root where its record says depth 1 and carries the id bit), children behind
// the level, the dense shadow queue, no stages.
static int run_level(FrameRun& f, uint32_t d, uint64_t base, uint64_t n, uint32_t* count) {
    rr_scene* s = f.s;
    const hipStream_t st = f.st;
    const uint32_t L = s->n_enabled_lights;
    unsigned long long* counters = s->counters.as<unsigned long long>();
    const bool l1 = d == 1 && !f.seeded; // the level-1 builds: rays derived from their index
    DRayQueue qin = f.queue_at(base);
    if (l1) { qin.r0 = nullptr; qin.r1 = nullptr; qin.r2 = nullptr; qin.hit = s->hit1.as<uint4>(); }
    {
        uint32_t* head = f.pool.take(1);
        if (!head) return counters_exhausted();
        ScopedTimer t(s, st, TK_CLOSEST, l1);
        RR_TRY(launch_trace_closest(s, l1, qin, count, head, n, s->shade_const.as<DShadeConst>(), f.pr, counters, st));
    }
    const bool spawns = d <= f.R; // the deepest level spawns nothing (k_shade: depth <= max_recursion)
    const uint64_t M = f.plan.M, child_base = l1 ? 0 : base + n;
    const uint64_t slice = level_slice(M, child_base, n, d, f.R);
    if (slice == 0) return fail(RR_ERR_OUT_OF_MEMORY, "ray arena of %llu rays is too small for depth level %u", (unsigned long long)M, d);
    if (slice < n) s->stats.sliced_levels++;
    for (uint64_t s0 = 0; s0 < n; s0 += slice) {
        const uint64_t s1 = std::min<uint64_t>(s0 + slice, n);
        uint32_t* child_count = f.pool.take(1);
        if (!child_count) return counters_exhausted();
        const DRayQueue qout = f.queue_at(child_base);
        // level 1 with fixed shadow slots and at least two stages: shade and shadow launches side by side on two streams
        const bool staged = level1_stages_wanted(s) && l1 && L >= 1 && L <= RR_FIXED_SLOT_LIGHTS && s->view.n_items >= RR_BEAM_MIN_ITEMS &&
                            s->view.n_items <= RR_BEAM_MAX_ITEMS && level1_stages(s, s1 - s0).overlapped();
        if (staged) RR_TRY(run_level1_stages(f, level1_stages(s, s1 - s0), qin, count, s0, s1, qout, child_count, spawns));
        for (uint64_t c0 = s0; c0 < s1 && !staged; c0 += f.plan.chunk) {
            if (f.cancel && *f.cancel) { (void)hipStreamSynchronize(st); return fail(RR_ERR_CANCELLED, "cancelled"); }
            const uint64_t c1 = std::min<uint64_t>(c0 + f.plan.chunk, s1);
            const int grid = (int)std::min<uint64_t>((c1 - c0 + RR_BLOCK - 1) / RR_BLOCK, (uint64_t)f.shade_grid_max);
            // level 1: shadow slots of this chunk = L x (the chunk padded to whole workgroup iterations), one validity word per 64
            // (only where the shadow kernel's packet form applies: rr_kernels.hip, RR_BEAM_MIN_ITEMS .. RR_BEAM_MAX_ITEMS)
            // and up to RR_FIXED_SLOT_LIGHTS enabled lights: k_shade keeps one bit per light and lane for the validity words; more lights
            // take the dense queue of the deeper levels, which has no such limit
            const bool sq_fixed = l1 && s->view.n_items >= RR_BEAM_MIN_ITEMS && s->view.n_items <= RR_BEAM_MAX_ITEMS && L <= RR_FIXED_SLOT_LIGHTS;
            const uint32_t sq_chunk_cap = sq_fixed ? (uint32_t)(((c1 - c0 + RR_BLOCK - 1) / RR_BLOCK) * RR_BLOCK) : 0u;
            unsigned long long* sq_valid = s->sq_valid.as<unsigned long long>();
            // deeper levels: shadow sub-queues, a shard gets the packets with (packet % RR_SQ_SHARDS == shard), L rays per hit at most
            const uint64_t groups = (c1 - c0 + RR_BLOCK - 1) / RR_BLOCK; // 256-ray groups, dealt round-robin to the shards
            const uint32_t segcap = (uint32_t)(((groups + RR_SQ_SHARDS - 1) / RR_SQ_SHARDS) * RR_BLOCK * std::max(L, 1u));
            f.pool.align_line(); // the append counters start on a 128-B line
            uint32_t* sq_counts = f.pool.take(RR_SQ_SHARDS * RR_SQ_STRIDE);
            uint32_t* shead = f.pool.take(1);
            if (!sq_counts || !shead) return counters_exhausted();
            {
                ScopedTimer t(s, st, TK_SHADE, l1);
                if (l1) hipLaunchKernelGGL(k_shade<true>, dim3(grid), dim3(RR_BLOCK), 0, st, s->shade_const.as<DShadeConst>(), f.slot_xy, f.pr, qin, count,
                                               (uint32_t)c0, (uint32_t)c1, qout, child_count, f.SQ, sq_counts, segcap, sq_valid, sq_chunk_cap, f.acc, counters);
                else hipLaunchKernelGGL(k_shade<false>, dim3(grid), dim3(RR_BLOCK), 0, st, s->shade_const.as<DShadeConst>(), f.slot_xy, f.pr, qin, count,
                                        (uint32_t)c0, (uint32_t)c1, qout, child_count, f.SQ, sq_counts, segcap, sq_valid, sq_chunk_cap, f.acc, counters);
            }
            // The size of the next level is final once the slice's last shade chunk has run: its read-back is enqueued
            // BEFORE that chunk's shadow kernel, so the host learns it (and enqueues the next level) while the shadow
            // rays are still being traced, instead of leaving the device idle for a host round trip per level.
            if (spawns && c1 == s1) {
                HIP_TRY(hipMemcpyAsync(s->h_count, child_count, 4, hipMemcpyDeviceToHost, st));
                HIP_TRY(hipEventRecord(s->count_ready, st));
            }
            if (L) {
                ScopedTimer t(s, st, TK_SHADOW, sq_fixed); // (by kernel BUILD: level 1 of a scene without fixed shadow slots runs k_trace_shadow<false>)
                if (sq_fixed) {
                    const uint32_t sq_packets = (sq_chunk_cap / RR_WAVE) * L;
                    const int sgrid = (int)std::min<uint64_t>(((uint64_t)sq_packets * RR_WAVE + RR_BLOCK - 1) / RR_BLOCK, (uint64_t)f.shadow_grid);
                    hipLaunchKernelGGL(k_trace_shadow<true>, dim3(sgrid), dim3(RR_BLOCK), 0, st, s->view, f.SQ, sq_counts, segcap, sq_valid, sq_packets, shead, f.acc);
                } else {
                    const uint64_t sq_ub = (c1 - c0) * L;
                    const int sgrid = (int)std::min<uint64_t>((sq_ub + RR_BLOCK - 1) / RR_BLOCK, (uint64_t)f.shadow_grid);
                    hipLaunchKernelGGL(k_trace_shadow<false>, dim3(sgrid), dim3(RR_BLOCK), 0, st, s->view, f.SQ, sq_counts, segcap, sq_valid, 0u, shead, f.acc);
                }
            }
        }
        if (!spawns) continue;
        HIP_TRY(hipEventSynchronize(s->count_ready));
        const uint64_t m = *s->h_count;
        if (m > M - child_base) return fail(RR_ERR_DEVICE, "internal: level %u holds %llu rays, room for %llu", d + 1, (unsigned long long)m, (unsigned long long)(M - child_base));
        if (m == 0) continue;
        uint64_t level_base = child_base;
        RR_TRY(bin_level(f, child_base, m, &level_base));
        RR_TRY(run_level(f, d + 1, level_base, m, child_count));
    }
    return RR_OK;
}

static void launch_resolve(const FrameRun& f, const DFrame& fr, const rr_frame* out, bool frame_layout) {
    const uint32_t npix = fr.n_region_pixels;
    hipLaunchKernelGGL(k_resolve, dim3((npix + RR_BLOCK - 1) / RR_BLOCK), dim3(RR_BLOCK), 0, f.st, fr, f.s->region_xy.as<uint32_t>(), f.s->trace_order.as<uint32_t>(),
                       f.acc, out->rgba8, out->normal, out->depth, out->object_id, frame_layout ? 1u : 0u);
}

// The frame's batches of primary rays, in order.  After a batch that ends on a whole slice of samples the pass hook
// (if any) gets the frame resolved over the samples finished so far.
static int run_batches(FrameRun& f, const DFrame& fr, const rr_frame* out, bool frame_layout, const PassHook* hook) {
    rr_scene* s = f.s;
    const uint32_t npix = fr.n_region_pixels;
    const uint64_t B = f.plan.B, total_primary = f.plan.total_primary;
    for (uint64_t first = 0; first < total_primary; first += B) {
        if (f.cancel && *f.cancel) { (void)hipStreamSynchronize(f.st); return fail(RR_ERR_CANCELLED, "cancelled"); }
        const uint32_t n_batch = (uint32_t)std::min<uint64_t>(B, total_primary - first);
        RR_TRY(f.pool.start_batch());
        uint32_t* level1_count = f.pool.take(1);
        // The batch covers primary indices [first, first + n_batch): index i -> sample i / npix, pixel i % npix.
        f.pr.at = primary_launch(first, npix, batch_group(f.plan, npix, first, n_batch)); f.pr.n = n_batch;
        s->stats.batches++;
        RR_TRY(run_level(f, 1, 0, n_batch, level1_count));
        HIP_TRY(hipGetLastError());
        // batches are stream-ordered; only a caller that can cancel needs the host to keep pace with the device
        if (f.cancel && first + B < total_primary) HIP_TRY(hipStreamSynchronize(f.st));
        const uint64_t done = first + n_batch;
        if (hook && hook->fn && done < total_primary && done % npix == 0) {
            DFrame pf = fr;
            pf.samples = (uint32_t)(done / npix); // the mean over the sample slices finished so far
            launch_resolve(f, pf, out, frame_layout);
            RR_TRY(copy_outputs(*hook->host, *out, (size_t)fr.width * fr.height, f.st));
            InPass in_pass(s);
            if (hook->fn(hook->user, done, total_primary) != 0) return fail(RR_ERR_CANCELLED, "stopped by the pass callback");
        }
    }
    return RR_OK;
}

static int render_region_locked(rr_scene* s, const rr_camera* cam, const rr_config* cfg, const uint16_t* sample_xy,
                                const rr_region* rg, const rr_frame* out, bool frame_layout, hipStream_t st, const volatile int* cancel,
                                const PassHook* hook = nullptr) {
    RR_TRY(check_intact(s));
    HIP_TRY(hipSetDevice(s->device));
    if (st != s->last_stream) { HIP_TRY(hipStreamSynchronize(s->last_stream)); s->last_stream = st; }
    const uint32_t W = cam->width, H = cam->height;
    if ((uint64_t)W * H > (1ull << 30)) return fail(RR_ERR_UNSUPPORTED, "frame of %ux%u pixels", W, H);
    RR_TRY(update_region_map(s, W, H, *rg, st));
    const uint32_t npix = (uint32_t)s->h_region_xy.size();
    resolve_timers(s); // launches of an earlier frame nobody asked about must not leak into this frame's stats
    memset(&s->stats, 0, sizeof s->stats);
    s->stats_final = false;
    s->overlap_stages = 0;
    if (npix == 0) return RR_OK;
    RR_TRY(ensure_camera_reach(s, cam, cfg)); // the top level's boxes must be padded for this camera's distance from the origin
    DFrame fr = make_frame(cam, cfg);
    fr.n_region_pixels = npix;
    RR_TRY(upload_sample_table(s, fr, sample_xy, st));
    DAccum acc;
    RR_TRY(reset_accumulators(s, npix, out->normal != nullptr, out->depth != nullptr, out->object_id != nullptr, st, &acc));
    FramePlan plan;
    RR_TRY(plan_queues(s, npix, cfg, hook ? hook->min_passes : 0u, &plan));
    RR_TRY(upload_shade_const(s, fr, primary_frame(s->slot_c.as<float>(), npix, plan.G), st)); // (after the plan: the index constants follow its sample group)
    FrameRun f{s, st, plan, cfg->max_recursion, DShadowQueue{s->sq[0].as<float4>(), s->sq[1].as<float4>(), s->sq[2].as<float4>()}, acc,
               CounterPool{s, st}, DPrimary{s->sample_tr.as<float>(), primary_launch(0, npix, 1u), 0u}, cancel,
               s->n_cus * RR_SHADOW_GRID_WG, // RR_STACK_DEPTH KB of LDS stack per 256-thread workgroup
               s->n_cus * RR_SHADE_GRID_WG};
    f.slot_xy = s->region_xy.as<uint32_t>();
    HIP_TRY(hipEventRecord(s->frame_a, st));
    RR_TRY(run_batches(f, fr, out, frame_layout, hook));
    launch_resolve(f, fr, out, frame_layout);
    HIP_TRY(hipEventRecord(s->frame_b, st));
    HIP_TRY(hipGetLastError());
    // a scene that branches more than the arena was sized for gets a larger one for its next frame (within the budget)
    if (s->stats.sliced_levels > 0 && s->arena_factor < 128) s->arena_factor *= 2;
    return RR_OK;
}

extern "C" int rr_render_region_device(rr_scene* s, const rr_camera* cam, const rr_config* cfg, const uint16_t* sample_xy,
                                       const rr_region* rg, const rr_frame* out, void* hip_stream, const volatile int* cancel) try {
    RR_TRY(check_frame_args(s, cam, cfg, sample_xy));
    RR_TRY(check_region(cam->width, cam->height, rg));
    if (!out || !out->rgba8) return fail(RR_ERR_INVALID_ARGUMENT, "out->rgba8 is required");
    RR_TRY(not_in_pass(s, "rr_render_region_device"));
    std::lock_guard<std::mutex> lk(s->mu);
    return render_region_locked(s, cam, cfg, sample_xy, rg, out, false, (hipStream_t)hip_stream, cancel);
} RR_GUARD_END("rr_render_region_device")

static int render_to_host(rr_scene* s, const rr_camera* cam, const rr_config* cfg, const uint16_t* sample_xy, const rr_frame* out,
                          const volatile int* cancel, rr_pass_fn fn, void* user, uint32_t min_passes) {
    RR_TRY(check_frame_args(s, cam, cfg, sample_xy));
    if (!out || !out->rgba8) return fail(RR_ERR_INVALID_ARGUMENT, "out->rgba8 is required");
    RR_TRY(not_in_pass(s, fn ? "rr_render_progressive" : "rr_render"));
    std::lock_guard<std::mutex> lk(s->mu);
    HIP_TRY(hipSetDevice(s->device));
    const size_t np = (size_t)cam->width * cam->height;
    rr_frame dev{};
    RR_TRY(stage_outputs(s, *out, np, false, &dev));
    rr_region whole{8, 8, 1, 0}; // 8x8 tiles: one wave = one tile of primary rays
    PassHook hook{fn, user, min_passes, out};
    RR_TRY(render_region_locked(s, cam, cfg, sample_xy, &whole, &dev, true, nullptr, cancel, fn ? &hook : nullptr));
    HIP_TRY(hipStreamSynchronize(nullptr));
    return copy_outputs(*out, dev, np, nullptr);
}

extern "C" int rr_render(rr_scene* s, const rr_camera* cam, const rr_config* cfg, const uint16_t* sample_xy, const rr_frame* out,
                         const volatile int* cancel) try {
    return render_to_host(s, cam, cfg, sample_xy, out, cancel, nullptr, nullptr, 0);
} RR_GUARD_END("rr_render")

extern "C" int rr_render_progressive(rr_scene* s, const rr_camera* cam, const rr_config* cfg, const uint16_t* sample_xy, const rr_frame* out,
                                     uint32_t min_passes, rr_pass_fn on_pass, void* user, const volatile int* cancel) try {
    if (!on_pass) return fail(RR_ERR_INVALID_ARGUMENT, "on_pass is required (use rr_render for a one-shot frame)");
    return render_to_host(s, cam, cfg, sample_xy, out, cancel, on_pass, user, min_passes);
} RR_GUARD_END("rr_render_progressive")

// the device's work counters of the frame (or pass) that ran last, or of the batches so far inside on_pass
static int read_counters(const rr_scene* s, rr_frame_stats* st) {
    unsigned long long c[RR_CNT_WORDS];
    HIP_TRY(hipMemcpy(c, s->counters.p, sizeof c, hipMemcpyDeviceToHost));
    st->primary_rays = c[RR_CNT_PRIMARY]; st->secondary_rays = c[RR_CNT_SECONDARY];
    st->shadow_rays = c[RR_CNT_SHADOW]; st->shaded_hits = c[RR_CNT_SHADED];
    return RR_OK;
}
// the device counters and launch timers of the frame (or pass) that ran last, into s->stats
static int collect_stats_locked(rr_scene* s) {
    float ms = 0.0f;
    if (hipEventSynchronize(s->frame_b) == hipSuccess && hipEventElapsedTime(&ms, s->frame_a, s->frame_b) == hipSuccess) s->stats.ms_total = ms;
    resolve_timers(s);
    return read_counters(s, &s->stats);
}
extern "C" int rr_scene_overlap_stages(const rr_scene* cs, uint32_t* out) try {
    if (!cs || !out) return fail(RR_ERR_INVALID_ARGUMENT, "NULL argument");
    *out = cs->overlap_stages;
    return RR_OK;
} RR_GUARD_END("rr_scene_overlap_stages")

extern "C" int rr_scene_last_stats(const rr_scene* cs, rr_frame_stats* out) try {
    if (!cs || !out) return fail(RR_ERR_INVALID_ARGUMENT, "NULL argument");
    if (tl_in_pass == cs) { // inside on_pass of this scene: its frame holds s->mu on this thread and the stream is idle -- the passes so far
        rr_frame_stats st = cs->stats;
        if (!cs->stats_final) RR_TRY(read_counters(cs, &st));
        *out = st;
        return RR_OK;
    }
    rr_scene* s = const_cast<rr_scene*>(cs);
    std::lock_guard<std::mutex> lk(s->mu);
    HIP_TRY(hipSetDevice(s->device));
    if (!s->stats_final) { const int rc = collect_stats_locked(s); if (rc != RR_OK) return rc; }
    *out = s->stats;
    return RR_OK;
} RR_GUARD_END("rr_scene_last_stats")

// The frame filled in TILE BY TILE, every pixel final when it appears: what the reference's GUI shows (shuffled 2x2 cells, each rendered with all of
// its samples: src/renderer.rs:125-172, drained by Run::apply_pixels, src/run.rs:506-545).  Pass k of n_passes renders the 32x8-pixel tiles with
// tile_index % n_passes == k -- an interleaved subset, like the shuffled cell list -- straight into their places in the frame.
extern "C" int rr_render_progressive_tiles(rr_scene* s, const rr_camera* cam, const rr_config* cfg, const uint16_t* sample_xy, const rr_frame* out,
                                           uint32_t n_passes, rr_pass_fn on_pass, void* user, const volatile int* cancel) try {
    if (!on_pass) return fail(RR_ERR_INVALID_ARGUMENT, "on_pass is required (use rr_render for a one-shot frame)");
    RR_TRY(check_frame_args(s, cam, cfg, sample_xy));
    if (!out || !out->rgba8) return fail(RR_ERR_INVALID_ARGUMENT, "out->rgba8 is required");
    RR_TRY(not_in_pass(s, "rr_render_progressive_tiles"));
    std::lock_guard<std::mutex> lk(s->mu);
    HIP_TRY(hipSetDevice(s->device));
    const uint32_t W = cam->width, H = cam->height, TW = 32, TH = 8;
    const size_t np = (size_t)W * H;
    for (int k = 0; k < 4; k++) // pixels not rendered yet are zero, also when the frame stops before its first pass
        if (out_buffer(*out, k)) memset(out_buffer(*out, k), 0, np * OUT_ELEM[k]);
    rr_frame dev{};
    RR_TRY(stage_outputs(s, *out, np, true, &dev));
    const uint32_t n_tiles = ((W + TW - 1) / TW) * ((H + TH - 1) / TH);
    const uint32_t P = std::max(1u, std::min(n_passes ? n_passes : 16u, n_tiles));
    rr_frame_stats sum{};
    uint64_t done = 0;
    for (uint32_t k = 0; k < P; k++) {
        if (cancel && *cancel) return fail(RR_ERR_CANCELLED, "cancelled");
        const rr_region rg{TW, TH, P, k};
        RR_TRY(render_region_locked(s, cam, cfg, sample_xy, &rg, &dev, true, nullptr, cancel));
        HIP_TRY(hipStreamSynchronize(nullptr));
        RR_TRY(collect_stats_locked(s));
        {   // the frame's statistics are the sums over its passes
            const rr_frame_stats& a = s->stats;
            sum.primary_rays += a.primary_rays; sum.secondary_rays += a.secondary_rays; sum.shadow_rays += a.shadow_rays; sum.shaded_hits += a.shaded_hits;
            sum.ms_total += a.ms_total; sum.ms_trace_closest += a.ms_trace_closest; sum.ms_trace_shadow += a.ms_trace_shadow; sum.ms_shade += a.ms_shade;
            sum.launches_trace_closest += a.launches_trace_closest; sum.launches_trace_shadow += a.launches_trace_shadow; sum.launches_shade += a.launches_shade;
            sum.batches += a.batches; sum.sliced_levels += a.sliced_levels; sum.binned_rays += a.binned_rays; sum.ms_binning += a.ms_binning;
            sum.ms_trace_closest_level1 += a.ms_trace_closest_level1; sum.launches_trace_closest_level1 += a.launches_trace_closest_level1;
            sum.ms_shade_level1 += a.ms_shade_level1; sum.launches_shade_level1 += a.launches_shade_level1;
            sum.ms_trace_shadow_level1 += a.ms_trace_shadow_level1; sum.launches_trace_shadow_level1 += a.launches_trace_shadow_level1;
        }
        RR_TRY(copy_outputs(*out, dev, np, nullptr));
        done += rr_region_pixel_count(W, H, &rg);
        s->stats = sum; s->stats_final = true;
        if (k + 1 < P) {
            InPass in_pass(s);
            if (on_pass(user, done * cfg->samples, (uint64_t)np * cfg->samples) != 0) return fail(RR_ERR_CANCELLED, "stopped by the pass callback");
        }
    }
    return RR_OK;
} RR_GUARD_END("rr_render_progressive_tiles")

extern "C" int rr_scene_set_compat(rr_scene* s, uint32_t flags) try {
    if (!s) return fail(RR_ERR_INVALID_ARGUMENT, "NULL argument");
    if (flags & ~RR_COMPAT_OCCLUDER_ALPHA_SHADOWS) return fail(RR_ERR_INVALID_ARGUMENT, "unknown compatibility flags 0x%x", flags);
    RR_TRY(not_in_pass(s, "rr_scene_set_compat"));
    std::lock_guard<std::mutex> lk(s->mu);
    s->view.compat = (s->view.compat & RR_VIEW_NAN_BALLS) | flags; // the scene view is passed to the kernels by value with every launch
    return RR_OK;
} RR_GUARD_END("rr_scene_set_compat")

extern "C" int rr_scene_set_tuning(rr_scene* s, const rr_tuning* t) try {
    if (!s || !t) return fail(RR_ERR_INVALID_ARGUMENT, "NULL argument");
    if (t->struct_size != sizeof(rr_tuning)) return fail(RR_ERR_INVALID_ARGUMENT, "rr_tuning::struct_size %u, library expects %zu", t->struct_size, sizeof(rr_tuning));
    if (t->sample_group > 64u || (t->sample_group & (t->sample_group - 1u))) return fail(RR_ERR_INVALID_ARGUMENT, "sample_group %u is not 0 or a power of two <= 64", t->sample_group);
    RR_TRY(not_in_pass(s, "rr_scene_set_tuning"));
    std::lock_guard<std::mutex> lk(s->mu);
    s->tuning = *t;
    s->profiling = t->kernel_timing != 0;
    return RR_OK;
} RR_GUARD_END("rr_scene_set_tuning")
extern "C" int rr_scene_get_tuning(const rr_scene* s, rr_tuning* t) try {
    if (!s || !t) return fail(RR_ERR_INVALID_ARGUMENT, "NULL argument");
    *t = s->tuning;
    t->struct_size = (uint32_t)sizeof(rr_tuning);
    return RR_OK;
} RR_GUARD_END("rr_scene_get_tuning")

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
        if (!s->multi_stream) HIP_TRY(hipStreamCreateWithFlags(&s->multi_stream, hipStreamNonBlocking));
        return RR_OK;
    };
    // device 0: the concatenation of the compact buffers (rank order) and the frame-order buffers
    HIP_TRY(hipSetDevice(s0->device));
    RR_TRY(own_stream(s0));
    for (int k = 0; k < 4; k++)
        if (host[k]) HIP_TRY(s0->multi_cat[k].reserve(np * OUT_ELEM[k]));
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
                if (i == 0) *devp[k] = (char*)s0->multi_cat[k].p + offset[0] * OUT_ELEM[k]; // device 0 renders straight into its slot
                else { HIP_TRY(s->multi_part[k].reserve(std::max<uint64_t>(count[i], 1) * OUT_ELEM[k])); *devp[k] = s->multi_part[k].p; }
            }
            rr_region rg{TW, TH, n_scenes, i};
            RR_TRY(render_region_locked(s, cam, cfg, sample_xy, &rg, &dev, false, s->multi_stream, cancel));
            if (i != 0)
                for (int k = 0; k < 4; k++) {
                    if (!host[k] || !count[i]) continue;
                    const size_t bytes = count[i] * OUT_ELEM[k];
                    void* dst = (char*)s0->multi_cat[k].p + offset[i] * OUT_ELEM[k];
                    if (direct[i] && s->device == s0->device) HIP_TRY(hipMemcpyAsync(dst, s->multi_part[k].p, bytes, hipMemcpyDeviceToDevice, s->multi_stream));
                    else if (direct[i]) HIP_TRY(hipMemcpyPeerAsync(dst, s0->device, s->multi_part[k].p, s->device, bytes, s->multi_stream));
                    else { // no peer access: device -> pinned host here, host -> device 0 after the join
                        if (s->multi_stage_bytes[k] < bytes) {
                            if (s->multi_stage[k]) { (void)hipHostFree(s->multi_stage[k]); s->multi_stage[k] = nullptr; s->multi_stage_bytes[k] = 0; }
                            HIP_TRY(hipHostMalloc(&s->multi_stage[k], bytes, hipHostMallocPortable));
                            s->multi_stage_bytes[k] = bytes;
                        }
                        HIP_TRY(hipMemcpyAsync(s->multi_stage[k], s->multi_part[k].p, bytes, hipMemcpyDeviceToHost, s->multi_stream));
                    }
                }
            HIP_TRY(hipStreamSynchronize(s->multi_stream));
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
                HIP_TRY(hipMemcpyAsync((char*)s0->multi_cat[k].p + offset[i] * OUT_ELEM[k], scenes[i]->multi_stage[k], count[i] * OUT_ELEM[k], hipMemcpyHostToDevice, s0->multi_stream));
    }
    for (int k = 0; k < 4; k++)
        if (host[k]) RR_TRY(rr_deinterleave_device(W, H, TW, TH, n_scenes, (uint32_t)OUT_ELEM[k], s0->multi_cat[k].p, out_buffer(frame_dev, k), s0->device, s0->multi_stream));
    RR_TRY(copy_outputs(*out, frame_dev, np, s0->multi_stream));
    s0->stats.multi_devices = n_scenes; s0->stats.multi_peer_links = n_peer; s0->stats.multi_staged_links = n_staged;
    s0->stats.ms_multi_exchange = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_joined).count();
    return RR_OK;
} RR_GUARD_END("rr_render_multi")

// ---------------------------------------------------------------------------
// post-processing (reference src/post_processing.rs:123-181)
// ---------------------------------------------------------------------------
extern "C" int rr_post_process_device(uint32_t width, uint32_t height, int cavity, int outline, const uint8_t* rgba_in,
                                      const float* normal, const uint32_t* object_id, uint8_t* rgba_out, int device, void* hip_stream) try {
    if (width == 0 || height == 0) return fail(RR_ERR_INVALID_ARGUMENT, "bad frame size %ux%u", width, height);
    if (!rgba_in || !rgba_out || rgba_in == rgba_out) return fail(RR_ERR_INVALID_ARGUMENT, "rgba_in / rgba_out must be distinct non-NULL buffers");
    if ((cavity && !normal) || (outline && !object_id)) return fail(RR_ERR_INVALID_ARGUMENT, "cavity needs the normal buffer, outline the object-id buffer");
    HIP_TRY(hipSetDevice(device));
    const uint64_t n = (uint64_t)width * height;
    hipLaunchKernelGGL(k_post_process, dim3((uint32_t)((n + RR_BLOCK - 1) / RR_BLOCK)), dim3(RR_BLOCK), 0, (hipStream_t)hip_stream, width, height,
                       cavity ? 1u : 0u, outline ? 1u : 0u, (const uint32_t*)rgba_in, normal, object_id, (uint32_t*)rgba_out);
    HIP_TRY(hipGetLastError());
    return RR_OK;
} RR_GUARD_END("rr_post_process_device")

extern "C" int rr_post_process(uint32_t width, uint32_t height, int cavity, int outline, const uint8_t* rgba_in, const float* normal,
                               const uint32_t* object_id, uint8_t* rgba_out, int device) try {
    if (width == 0 || height == 0) return fail(RR_ERR_INVALID_ARGUMENT, "bad frame size %ux%u", width, height);
    if (!rgba_in || !rgba_out) return fail(RR_ERR_INVALID_ARGUMENT, "NULL image");
    if ((cavity && !normal) || (outline && !object_id)) return fail(RR_ERR_INVALID_ARGUMENT, "cavity needs the normal buffer, outline the object-id buffer");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(RR_ERR_NO_DEVICE, "no HIP device available");
    HIP_TRY(hipSetDevice(device));
    const size_t n = (size_t)width * height;
    DevBuf in, out, nrm, ids;
    HIP_TRY(in.reserve(n * 4)); HIP_TRY(out.reserve(n * 4));
    HIP_TRY(hipMemcpy(in.p, rgba_in, n * 4, hipMemcpyHostToDevice));
    if (normal) { HIP_TRY(nrm.reserve(n * 12)); HIP_TRY(hipMemcpy(nrm.p, normal, n * 12, hipMemcpyHostToDevice)); }
    if (object_id) { HIP_TRY(ids.reserve(n * 4)); HIP_TRY(hipMemcpy(ids.p, object_id, n * 4, hipMemcpyHostToDevice)); }
    int rc = rr_post_process_device(width, height, cavity, outline, in.as<uint8_t>(), nrm.as<float>(), ids.as<uint32_t>(), out.as<uint8_t>(), device, nullptr);
    if (rc == RR_OK) {
        hipError_t e = hipMemcpy(rgba_out, out.p, n * 4, hipMemcpyDeviceToHost);
        if (e != hipSuccess) rc = fail(RR_ERR_DEVICE, "copy back: %s", hipGetErrorString(e));
    }
    in.release(); out.release(); nrm.release(); ids.release();
    return rc;
} RR_GUARD_END("rr_post_process")

// ---------------------------------------------------------------------------
// pick (reference src/raytracing.rs:237-273): pixel-centre ray, one closest-hit query
// ---------------------------------------------------------------------------
extern "C" int rr_pick(rr_scene* s, const rr_camera* cam, int x, int y, rr_pick_result* out) try {
    if (!s || !cam || !out) return fail(RR_ERR_INVALID_ARGUMENT, "NULL argument");
    if (x < 0 || y < 0 || (uint32_t)x >= cam->width || (uint32_t)y >= cam->height) return fail(RR_ERR_INVALID_ARGUMENT, "pixel (%d,%d) outside %ux%u", x, y, cam->width, cam->height);
    RR_TRY(not_in_pass(s, "rr_pick"));
    std::lock_guard<std::mutex> lk(s->mu);
    RR_TRY(check_intact(s));
    HIP_TRY(hipSetDevice(s->device));
    RR_TRY(ensure_camera_reach(s, cam, nullptr));
    const rr_config none{}; // a pick has no frame config
    DFrame fr = make_frame(cam, &none);
    fr.samples = 1; fr.cell_size = 1; fr.n_region_pixels = 1;
    DevBuf scratch;
    HIP_TRY(scratch.reserve(256 + sizeof(DShadeConst)));
    // layout: [0] slot_c (the pixel's centre), [8] sample_tr (the one sample's offset), [64] hit, [96] count, [100] head, [128] counters, [256] scene view + frame constants
    char* b = scratch.as<char>();
    const uint32_t h_xy = (uint32_t)x | ((uint32_t)y << 16);
    const uint16_t h_sample[2] = {0, 0};
    float h_tables[4]; // the one-entry tables of a frame of one pixel and one sample: the launch takes the frames' code path
    primary_slot_centres(&h_xy, 1, fr.width, fr.height, h_tables);
    primary_sample_offsets(h_sample, PrimarySampleKey{fr.width, fr.height, fr.cell_size, fr.dof, fr.samples, fr.aperture_size}, h_tables + 2);
    HIP_TRY(hipMemset(b, 0, 256));
    HIP_TRY(hipMemcpy(b, h_tables, sizeof h_tables, hipMemcpyHostToDevice));
    DRayQueue q{nullptr, nullptr, nullptr, (uint4*)(b + 64)};
    DPrimary pr{(const float*)(b + 8), primary_launch(0, 1u, 1u), 1u};
    DShadeConst hc;
    hc.sc = s->view; hc.fr = fr; hc.ps = primary_frame((const float*)b, 1u, 1u);
    HIP_TRY(hipMemcpy(b + 256, &hc, sizeof hc, hipMemcpyHostToDevice));
    RR_TRY(launch_trace_closest(s, true, q, (uint32_t*)(b + 96), (uint32_t*)(b + 100), 1, (const DShadeConst*)(b + 256), pr, (unsigned long long*)(b + 128), nullptr));
    uint32_t hit[4];
    HIP_TRY(hipMemcpy(hit, b + 64, 16, hipMemcpyDeviceToHost));
    scratch.release();
    memset(out, 0, sizeof *out);
    if ((int32_t)hit[1] >= 0) {
        out->hit = 1; out->item_index = hit[1]; out->object_id = s->h_items[hit[1]].id;
        memcpy(&out->distance, &hit[0], 4);
    }
    return RR_OK;
} RR_GUARD_END("rr_pick")

// ---------------------------------------------------------------------------
// ray queries: Raytracing::trace for caller-supplied rays (rr_pick generalised), closest-hit and shadow form, and
// Raytracing::get_color_depth_normal_id for them (rr_shade_rays).  Each query has ONE body, which works on buffers the scene's
// device can address and on a stream: the *_device entry points check the caller's pointers and run it in place; the host entry
// points are the device forms behind a staging copy -- the caller's arrays go into buffers of the call as they are, the body runs
// on the null stream, and the copy of the answers into `out` is the synchronisation.
// The streaming kernels of rr_kernels.hip (5d .. 5g) turn the caller's 12-byte rays into the walks' records and the walks' raw
// hits into the 20-byte records of the ABI; the walks and their launch sites are the frames' own.
// A closest-hit or shadow query waits ONCE for the device, for the 16 bytes of query_words[QW_REACH]: the largest finite |origin|
// per axis (the top level must be padded for it BEFORE the walk is enqueued: ensure_tlas_reach, * 1.001 in double) and the first
// bad max_distance.  A radiance query additionally waits where a frame's level walk does (the level sizes).
// Everything the launches of a device form touch after the call has returned is the caller's or the handle's (rr_scene::query_*,
// the arena): a scene edit waits for the device before it overwrites what they read, and rr_scene_destroy before it frees.
// ---------------------------------------------------------------------------
enum : size_t { QW_COUNT = 0, QW_HEAD = 4, QW_REACH = 64, QW_COUNTERS = 128, QW_CONST = 256 }; // byte offsets into rr_scene::query_words
static_assert(sizeof(rr_ray_hit) == 20 && sizeof(rr_shadow_hit) == 20, "k_unpack_hits writes five words per ray");
static_assert(sizeof(rr_surface_hit) == 128 && offsetof(rr_surface_hit, position) == 16 && offsetof(rr_surface_hit, normal) == 32 &&
              offsetof(rr_surface_hit, shading_normal) == 48 && offsetof(rr_surface_hit, base_color) == 64 && offsetof(rr_surface_hit, ambient_color) == 80 &&
              offsetof(rr_surface_hit, specular_color) == 96 && offsetof(rr_surface_hit, uv) == 112, "k_surface_hits writes rr_surface_hit as eight 16-byte rows");

// `p` (argument `arg` of `fn`) must be memory the scene's device can address: decided by query_pointer_ok (rr_query_pointers.h)
static int check_query_pointer(const rr_scene* s, const void* p, const char* fn, const char* arg) {
    hipPointerAttribute_t at;
    memset(&at, 0, sizeof at);
    QueryMemKind kind = RR_QMEM_UNREGISTERED;
    int owner = -1;
    if (hipPointerGetAttributes(&at, p) != hipSuccess) (void)hipGetLastError(); // a pointer the runtime has never seen
    else {
        switch (at.type) {
        case hipMemoryTypeHost: kind = RR_QMEM_HOST; break;
        case hipMemoryTypeDevice: kind = RR_QMEM_DEVICE; owner = at.device; break;
        case hipMemoryTypeManaged: case hipMemoryTypeUnified: kind = RR_QMEM_MANAGED; break;
        case hipMemoryTypeArray: kind = RR_QMEM_ARRAY; break;
        default: kind = RR_QMEM_UNREGISTERED; break;
        }
    }
    bool peer = false;
    if (kind == RR_QMEM_DEVICE && owner != s->device) { // only what this library has enabled itself (rr_render_multi) counts
        std::lock_guard<std::mutex> lk(g_peer_mu);
        const auto it = g_peer_state.find({s->device, owner});
        peer = it != g_peer_state.end() && it->second;
    }
    if (!query_pointer_ok(kind, owner, s->device, peer))
        return fail(RR_ERR_INVALID_ARGUMENT, "%s: %s is %s%s the scene's device %d cannot address", fn, arg, query_mem_kind_name(kind),
                    kind == RR_QMEM_DEVICE ? " of another device without peer access, which" : ", which", s->device);
    return RR_OK;
}

// the handle's record buffers for n rays (grow-only; a failed growth leaves an empty buffer that the next call allocates anew)
static int reserve_query_records(rr_scene* s, uint32_t n, bool shadow) {
    const size_t elem[4] = {16, 16, 8, 16};
    for (int k = 0; k < 4; k++)
        if (!(shadow && k == 2)) HIP_TRY(s->query_rec[k].reserve((size_t)n * elem[k]));
    HIP_TRY(s->query_words.reserve(QW_CONST + sizeof(DShadeConst)));
    return RR_OK;
}

static int take_stream(rr_scene* s, hipStream_t st) { // the handle's query buffers are shared: queries on different streams are serialised, as frames are
    if (st != s->last_stream) { HIP_TRY(hipStreamSynchronize(s->last_stream)); s->last_stream = st; }
    return RR_OK;
}

// the reach words, preset; the caller enqueues the kernel that merges into them and then calls await_reach
static int preset_reach(rr_scene* s, hipStream_t st) {
    char* w = s->query_words.as<char>();
    HIP_TRY(hipMemsetAsync(w, 0, QW_CONST, st));
    HIP_TRY(hipMemsetAsync(w + QW_REACH + 12, 0xff, 4, st));
    return RR_OK;
}
// THE wait of a query on device buffers: reads the reach words back (pinned, s->h_count[4 .. 7]) and pads the top level for them.
// *first_bad = the first index with a bad limit, or 0xffffffff.
static int await_reach(rr_scene* s, hipStream_t st, uint32_t* first_bad) {
    uint32_t* h = s->h_count + 4;
    HIP_TRY(hipMemcpyAsync(h, s->query_words.as<char>() + QW_REACH, 16, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    *first_bad = h[3];
    if (h[3] != 0xffffffffu) return RR_OK; // the caller refuses: nothing is rebuilt for a call that does nothing
    double need[3];
    for (int c = 0; c < 3; c++) {
        float a;
        memcpy(&a, &h[c], 4);
        need[c] = (double)a * 1.001;
    }
    return ensure_tlas_reach(s, need);
}

static int query_grid(const rr_scene* s, uint64_t n) { return (int)std::min<uint64_t>((n + RR_BLOCK - 1) / RR_BLOCK, (uint64_t)s->n_cus * 8u); }

// a host array of the caller's in a device buffer of the call (blocking)
static int stage_in(DevBuf* b, const void* src, size_t bytes) {
    HIP_TRY(b->reserve(bytes));
    HIP_TRY(hipMemcpy(b->p, src, bytes, hipMemcpyHostToDevice));
    return RR_OK;
}

// ---- closest-hit and shadow queries
// Shadow queries: Raytracing::trace(ray, true, true, depth) and `in_light = toi > len` (reference src/raytracing.rs:429-490,
// :883-892) through the walk the frames' shadow kernel uses (k_query_shadow); closest-hit queries: the closest-hit kernel of the
// deeper levels on a queue that k_pack_rays fills.

// The argument checks of the four entry points, in the order the tests pin; `device`: the alignment rule of the device forms.
// n == 0 passes: the caller returns RR_OK before it touches anything.
static int check_trace_args(const char* fn, bool device, const rr_scene* s, const float* origins, const float* directions, const float* max_distance,
                            uint32_t n, uint32_t depth, const void* out, uintptr_t out_align = 4u) {
    if (!s || (n && (!origins || !directions || !out))) return fail(RR_ERR_INVALID_ARGUMENT, "NULL argument");
    if (depth == 0 || depth > 255u) return fail(RR_ERR_INVALID_ARGUMENT, "depth %u (1 .. 255)", depth);
    if (n == 0) return RR_OK;
    if (n > 0x7fffff00u) return fail(RR_ERR_UNSUPPORTED, "%u rays in one call", n);
    if (device && (((uintptr_t)origins | (uintptr_t)directions | (uintptr_t)max_distance | (uintptr_t)out) & 3u))
        return fail(RR_ERR_INVALID_ARGUMENT, "%s: a buffer is not 4-byte aligned", fn);
    if (device && ((uintptr_t)out & (out_align - 1u))) return fail(RR_ERR_INVALID_ARGUMENT, "%s: out_dev is not %u-byte aligned", fn, (unsigned)out_align);
    return RR_OK;
}

// One query on device buffers, in stream order (the caller holds the lock): Q_SHADOW = limits (or NULL) and the shadow walk into
// rr_shadow_hit records, else the closest-hit walk, whose raw hits end as rr_ray_hit records (Q_CLOSEST) or, with the packed rays
// they answer, as rr_surface_hit records (Q_SURFACE).  The only wait is await_reach.
enum QueryKind { Q_CLOSEST, Q_SHADOW, Q_SURFACE };
template <QueryKind KIND> struct QueryRecord { static const size_t bytes = 20; };
template <> struct QueryRecord<Q_SURFACE> { static const size_t bytes = sizeof(rr_surface_hit); };
template <QueryKind KIND>
static int trace_rays_locked(rr_scene* s, const float* origins, const float* directions, const float* max_distance, uint32_t n, uint32_t depth, void* out,
                             hipStream_t st) {
    constexpr bool SHADOW = KIND == Q_SHADOW;
    RR_TRY(take_stream(s, st));
    RR_TRY(reserve_query_records(s, n, SHADOW));
    char* w = s->query_words.as<char>();
    const DRayQueue q{s->query_rec[0].as<float4>(), s->query_rec[1].as<float4>(), SHADOW ? nullptr : s->query_rec[2].as<uint2>(), s->query_rec[3].as<uint4>()};
    RR_TRY(preset_reach(s, st));
    hipLaunchKernelGGL(k_pack_rays<SHADOW>, dim3(query_grid(s, n)), dim3(RR_BLOCK), 0, st, origins, directions, max_distance, n, depth, q.r0, q.r1, q.r2,
                       (uint32_t*)(w + QW_COUNT), (uint32_t*)(w + QW_REACH));
    HIP_TRY(hipGetLastError());
    uint32_t first_bad = 0;
    RR_TRY(await_reach(s, st, &first_bad));
    if (SHADOW && first_bad != 0xffffffffu) { // (the stream is idle: the value for the message comes with one more small copy)
        float v = 0.0f;
        HIP_TRY(hipMemcpy(&v, max_distance + first_bad, 4, hipMemcpyDefault));
        return fail(RR_ERR_INVALID_ARGUMENT, "max_distance[%u] = %g (a distance >= 0, or +inf for no limit)", first_bad, (double)v);
    }
    if (SHADOW) RR_TRY(launch_query_shadow(s, q.r0, q.r1, n, (uint32_t*)(w + QW_HEAD), q.hit, st));
    else { // (the <false> build reads neither the frame constants nor the work counters; both pointers name the handle's words all the same)
        const DPrimary pr{nullptr, PrimaryLaunch{0u, 0u, 0u, 6u}, 0u};
        RR_TRY(launch_trace_closest(s, false, q, (uint32_t*)(w + QW_COUNT), (uint32_t*)(w + QW_HEAD), n, (const DShadeConst*)(w + QW_CONST), pr,
                                    (unsigned long long*)(w + QW_COUNTERS), st));
    }
    if (KIND == Q_SURFACE) hipLaunchKernelGGL(k_surface_hits, dim3(query_grid(s, n)), dim3(RR_BLOCK), 0, st, s->view, q.r0, q.r1, q.hit, n, (uint4*)out);
    else hipLaunchKernelGGL(k_unpack_hits<SHADOW>, dim3(query_grid(s, n)), dim3(RR_BLOCK), 0, st, q.hit, n, s->view.items, s->view.n_items, s->view.trix, (uint32_t*)out);
    HIP_TRY(hipGetLastError());
    return RR_OK;
}

// The host form: the caller's arrays as they are (12 + 12 B per ray, 4 B of limit) and the 20-byte (128-byte) answers in buffers of the
// call, freed on return (hipFree waits for what a failed call left in flight); trace_rays_locked on the null stream between them.
template <QueryKind KIND>
static int trace_rays_staged(rr_scene* s, const float* origins, const float* directions, const float* max_distance, uint32_t n, uint32_t depth, void* out) {
    DevBuf d_origins, d_dirs, d_limits, d_out;
    RR_TRY(stage_in(&d_origins, origins, 12ull * n));
    RR_TRY(stage_in(&d_dirs, directions, 12ull * n));
    if (max_distance) RR_TRY(stage_in(&d_limits, max_distance, 4ull * n));
    const size_t out_bytes = QueryRecord<KIND>::bytes * n;
    HIP_TRY(d_out.reserve(out_bytes));
    RR_TRY(trace_rays_locked<KIND>(s, d_origins.as<float>(), d_dirs.as<float>(), d_limits.as<float>(), n, depth, d_out.p, nullptr));
    HIP_TRY(hipMemcpy(out, d_out.p, out_bytes, hipMemcpyDeviceToHost)); // waits for the launches: `out` is written by a finished query only
    return RR_OK;
}

extern "C" int rr_trace_rays(rr_scene* s, const float* origins, const float* directions, uint32_t n, uint32_t depth, rr_ray_hit* out) try {
    RR_TRY(check_trace_args("rr_trace_rays", false, s, origins, directions, nullptr, n, depth, out));
    if (n == 0) return RR_OK;
    RR_TRY(not_in_pass(s, "rr_trace_rays"));
    std::lock_guard<std::mutex> lk(s->mu);
    RR_TRY(check_intact(s));
    HIP_TRY(hipSetDevice(s->device));
    RR_FAULT_POINT("trace_rays.host");
    return trace_rays_staged<Q_CLOSEST>(s, origins, directions, nullptr, n, depth, out);
} RR_GUARD_END("rr_trace_rays")

extern "C" int rr_trace_shadow_rays(rr_scene* s, const float* origins, const float* directions, const float* max_distance,
                                    uint32_t n, uint32_t depth, rr_shadow_hit* out) try {
    RR_TRY(check_trace_args("rr_trace_shadow_rays", false, s, origins, directions, max_distance, n, depth, out));
    if (n == 0) return RR_OK;
    if (max_distance) // (the body refuses the same limits; here the refusal costs no upload)
        for (uint32_t i = 0; i < n; i++)
            if (!(max_distance[i] >= 0.0f)) return fail(RR_ERR_INVALID_ARGUMENT, "max_distance[%u] = %g (a distance >= 0, or +inf for no limit)", i, (double)max_distance[i]);
    RR_TRY(not_in_pass(s, "rr_trace_shadow_rays"));
    std::lock_guard<std::mutex> lk(s->mu);
    RR_TRY(check_intact(s));
    HIP_TRY(hipSetDevice(s->device));
    RR_FAULT_POINT("trace_shadow_rays.host");
    return trace_rays_staged<Q_SHADOW>(s, origins, directions, max_distance, n, depth, out);
} RR_GUARD_END("rr_trace_shadow_rays")

extern "C" int rr_trace_rays_device(rr_scene* s, const float* origins, const float* directions, uint32_t n, uint32_t depth, rr_ray_hit* out,
                                    void* hip_stream) try {
    RR_TRY(check_trace_args("rr_trace_rays_device", true, s, origins, directions, nullptr, n, depth, out));
    if (n == 0) return RR_OK;
    RR_TRY(not_in_pass(s, "rr_trace_rays_device"));
    std::lock_guard<std::mutex> lk(s->mu);
    RR_TRY(check_intact(s));
    HIP_TRY(hipSetDevice(s->device));
    RR_FAULT_POINT("trace_rays_device.host");
    RR_TRY(check_query_pointer(s, origins, "rr_trace_rays_device", "origins_dev"));
    RR_TRY(check_query_pointer(s, directions, "rr_trace_rays_device", "directions_dev"));
    RR_TRY(check_query_pointer(s, out, "rr_trace_rays_device", "out_dev"));
    return trace_rays_locked<Q_CLOSEST>(s, origins, directions, nullptr, n, depth, out, (hipStream_t)hip_stream);
} RR_GUARD_END("rr_trace_rays_device")

extern "C" int rr_trace_shadow_rays_device(rr_scene* s, const float* origins, const float* directions, const float* max_distance, uint32_t n, uint32_t depth,
                                           rr_shadow_hit* out, void* hip_stream) try {
    RR_TRY(check_trace_args("rr_trace_shadow_rays_device", true, s, origins, directions, max_distance, n, depth, out));
    if (n == 0) return RR_OK;
    RR_TRY(not_in_pass(s, "rr_trace_shadow_rays_device"));
    std::lock_guard<std::mutex> lk(s->mu);
    RR_TRY(check_intact(s));
    HIP_TRY(hipSetDevice(s->device));
    RR_FAULT_POINT("trace_shadow_rays_device.host");
    RR_TRY(check_query_pointer(s, origins, "rr_trace_shadow_rays_device", "origins_dev"));
    RR_TRY(check_query_pointer(s, directions, "rr_trace_shadow_rays_device", "directions_dev"));
    if (max_distance) RR_TRY(check_query_pointer(s, max_distance, "rr_trace_shadow_rays_device", "max_distance_dev"));
    RR_TRY(check_query_pointer(s, out, "rr_trace_shadow_rays_device", "out_dev"));
    return trace_rays_locked<Q_SHADOW>(s, origins, directions, max_distance, n, depth, out, (hipStream_t)hip_stream);
} RR_GUARD_END("rr_trace_shadow_rays_device")

// ---- surface queries: the closest-hit query with its third ending (k_surface_hits): what get_color_depth_normal_id evaluates at the
// hit before its light loop.  No config, no generator, nothing of a frame's state is touched.
extern "C" int rr_surface_rays(rr_scene* s, const float* origins, const float* directions, uint32_t n, uint32_t depth, rr_surface_hit* out) try {
    RR_TRY(check_trace_args("rr_surface_rays", false, s, origins, directions, nullptr, n, depth, out));
    if (n == 0) return RR_OK;
    RR_TRY(not_in_pass(s, "rr_surface_rays"));
    std::lock_guard<std::mutex> lk(s->mu);
    RR_TRY(check_intact(s));
    HIP_TRY(hipSetDevice(s->device));
    RR_FAULT_POINT("surface_rays.host");
    return trace_rays_staged<Q_SURFACE>(s, origins, directions, nullptr, n, depth, out);
} RR_GUARD_END("rr_surface_rays")

extern "C" int rr_surface_rays_device(rr_scene* s, const float* origins, const float* directions, uint32_t n, uint32_t depth, rr_surface_hit* out,
                                      void* hip_stream) try {
    RR_TRY(check_trace_args("rr_surface_rays_device", true, s, origins, directions, nullptr, n, depth, out, 16u));
    if (n == 0) return RR_OK;
    RR_TRY(not_in_pass(s, "rr_surface_rays_device"));
    std::lock_guard<std::mutex> lk(s->mu);
    RR_TRY(check_intact(s));
    HIP_TRY(hipSetDevice(s->device));
    RR_FAULT_POINT("surface_rays_device.host");
    RR_TRY(check_query_pointer(s, origins, "rr_surface_rays_device", "origins_dev"));
    RR_TRY(check_query_pointer(s, directions, "rr_surface_rays_device", "directions_dev"));
    RR_TRY(check_query_pointer(s, out, "rr_surface_rays_device", "out_dev"));
    return trace_rays_locked<Q_SURFACE>(s, origins, directions, nullptr, n, depth, out, (hipStream_t)hip_stream);
} RR_GUARD_END("rr_surface_rays_device")

// ---- radiance queries: Raytracing::get_color_depth_normal_id(scene, ray, 1) (reference src/raytracing.rs:720-998) for caller-supplied
// rays -- what `render` calls per sample, without its pinhole / DOF camera.  The caller's rays are seeded as depth level 1 of the
// frame's own level walk (k_seed_rays, run_level's seeded form), batch by batch (rr_frame_plan.h plan_ray_batches), into one
// accumulator slot per result; k_resolve_rays returns what k_resolve computes before its clamp.
// Per-frame state of the handle this call shares with rr_render, and why the next frame does not see it: the shade constants, the
// accumulators and the counter pool are rewritten by every frame; the arena and the shadow queue only grow (a frame takes what it
// needs from the front); the slot -> pixel map is this call's own buffer (FrameRun::slot_xy), so the cached region map, the
// sub-sample table and arena_factor are not touched at all.
static_assert(sizeof(rr_radiance) == 32 && offsetof(rr_radiance, depth) == 12 && offsetof(rr_radiance, normal) == 16 && offsetof(rr_radiance, object_id) == 28,
              "k_resolve_rays writes rr_radiance as two float4");
static const uint32_t RESOLVE_RAYS_CHUNK = 1u << 22; // results per k_resolve_rays launch and, in the host form, read-back (128 MB of staging at most)

// Where the rays, the stream ids (or NULL) and the results of one radiance query live: `host` = the caller's host arrays, which
// shade_rays_locked stages batch by batch and chunk by chunk; else buffers the scene's device can address, used where they are.
struct RayIo { const float* origins; const float* directions; const uint32_t* stream_ids; rr_radiance* out; bool host; };

// The argument checks of the two entry points, in the order the tests pin; `device`: the alignment rule of the device form.
// n_results == 0 passes: the caller returns RR_OK before it touches anything.
static int check_shade_args(const char* fn, bool device, const rr_scene* s, const rr_config* cfg, const float* origins, const float* directions,
                            const uint32_t* stream_ids, const rr_radiance* out, uint32_t n_results, uint32_t rays_per_result) {
    if (!s || !cfg) return fail(RR_ERR_INVALID_ARGUMENT, "NULL argument");
    if (rays_per_result == 0) return fail(RR_ERR_INVALID_ARGUMENT, "rays_per_result must be >= 1");
    if (rays_per_result > RR_MAX_SAMPLES_WITH_TABLE) return fail(RR_ERR_UNSUPPORTED, "rays_per_result %u > %u", rays_per_result, RR_MAX_SAMPLES_WITH_TABLE);
    if (cfg->max_recursion > RR_MAX_RECURSION) return fail(RR_ERR_UNSUPPORTED, "max_recursion %u > %u", cfg->max_recursion, RR_MAX_RECURSION);
    if (n_results == 0) return RR_OK;
    if (n_results > 0x7fffff00u) return fail(RR_ERR_UNSUPPORTED, "%u results in one call", n_results);
    if (!origins || !directions || !out) return fail(RR_ERR_INVALID_ARGUMENT, "NULL argument");
    if (device && ((((uintptr_t)origins | (uintptr_t)directions | (uintptr_t)stream_ids) & 3u) || ((uintptr_t)out & 15u)))
        return fail(RR_ERR_INVALID_ARGUMENT, "%s: the ray buffers must be 4-byte aligned and out_dev 16-byte aligned", fn);
    return RR_OK;
}

// the top level padded for host origins (n_words = 3 x rays): what k_ray_reach and await_reach do for rays on the device
static int ensure_host_ray_reach(rr_scene* s, const float* origins, uint64_t n_words) {
    double need[3] = {0.0, 0.0, 0.0};
    for (uint64_t g = 0; g < n_words; g++) {
        const double a = std::fabs((double)origins[g]) * 1.001;
        if (std::isfinite(a)) need[g % 3] = std::max(need[g % 3], a);
    }
    return ensure_tlas_reach(s, need);
}

// the frame constants k_shade reads: `samples` decides which ray of a result carries its object id; a width of 65536 makes
// k_shade's RNG pixel (xy >> 16) * width + (xy & 0xffff) the 32-bit id itself
static DFrame make_ray_frame(const rr_config* cfg, uint32_t rays_per_result, uint32_t n_results) {
    DFrame fr;
    memset(&fr, 0, sizeof fr);
    fr.width = 65536u; fr.height = 65536u; fr.samples = rays_per_result; fr.cell_size = 1u;
    fr.max_recursion = cfg->max_recursion; fr.monte_carlo = cfg->monte_carlo ? 1u : 0u;
    fr.fog_density = cfg->fog_density;
    for (int k = 0; k < 3; k++) fr.fog_color[k] = cfg->fog_color[k];
    fr.seed_lo = (uint32_t)cfg->seed; fr.seed_hi = (uint32_t)(cfg->seed >> 32);
    fr.n_region_pixels = n_results;
    return fr;
}

// the batches of one call, in order; d_origins / d_dirs: the host form's staging for one batch (plan.B rays)
static int run_ray_batches(FrameRun& f, const RayIo& io, uint32_t rays_per_result, float* d_origins, float* d_dirs) {
    rr_scene* s = f.s;
    const uint64_t B = f.plan.B, n_rays = f.plan.total_primary;
    for (uint64_t first = 0; first < n_rays; first += B) {
        if (f.cancel && *f.cancel) return fail(RR_ERR_CANCELLED, "cancelled");
        const uint32_t nb = (uint32_t)std::min<uint64_t>(B, n_rays - first);
        RR_TRY(f.pool.start_batch());
        uint32_t* level1_count = f.pool.take(1);
        if (!level1_count) return counters_exhausted();
        const float *origins = io.origins + 3ull * first, *dirs = io.directions + 3ull * first;
        if (io.host) { // (stream-ordered: the copies wait for the kernels of the batch before, which read the same staging buffers)
            HIP_TRY(hipMemcpyAsync(d_origins, origins, 12ull * nb, hipMemcpyHostToDevice, f.st));
            HIP_TRY(hipMemcpyAsync(d_dirs, dirs, 12ull * nb, hipMemcpyHostToDevice, f.st));
            origins = d_origins; dirs = d_dirs;
        }
        hipLaunchKernelGGL(k_seed_rays, dim3((nb + RR_BLOCK - 1) / RR_BLOCK), dim3(RR_BLOCK), 0, f.st, origins, dirs, (unsigned long long)first, nb, rays_per_result,
                           f.queue_at(0), level1_count, s->counters.as<unsigned long long>());
        HIP_TRY(hipGetLastError());
        s->stats.batches++;
        RR_TRY(run_level(f, 1, 0, nb, level1_count));
        HIP_TRY(hipGetLastError());
        if (f.cancel && first + B < n_rays) { // only a caller that can cancel needs the host to keep pace
            if (io.host) HIP_TRY(hipStreamSynchronize(f.st));
            else if (hipStreamSynchronize(f.st) != hipSuccess) return fail(RR_ERR_DEVICE, "rr_shade_rays_device: the stream failed");
        }
    }
    return RR_OK;
}

// One radiance query (the caller holds the lock).  Host rays: staging of the call, bounded by plan.B rays and RESOLVE_RAYS_CHUNK
// results, and the stream is idle when the call returns, whatever ended it (the staging goes, `out` is the caller's to read).
// Device rays: nothing is the call's own, so nothing is freed behind launches in flight, and only a call that ends early waits.
static int shade_rays_locked(rr_scene* s, const rr_config* cfg, const RayIo& io, uint32_t n_results, uint32_t rays_per_result, hipStream_t st,
                             const volatile int* cancel) {
    RR_TRY(take_stream(s, st));
    resolve_timers(s);
    memset(&s->stats, 0, sizeof s->stats);
    s->stats_final = false;
    s->overlap_stages = 0;
    const uint64_t n_rays = (uint64_t)n_results * rays_per_result;
    if (io.host) RR_TRY(ensure_host_ray_reach(s, io.origins, 3ull * n_rays));
    else {
        HIP_TRY(s->query_words.reserve(QW_CONST + sizeof(DShadeConst)));
        RR_TRY(preset_reach(s, st));
        hipLaunchKernelGGL(k_ray_reach, dim3(query_grid(s, 3ull * n_rays)), dim3(RR_BLOCK), 0, st, io.origins, (unsigned long long)(3ull * n_rays),
                           (uint32_t*)(s->query_words.as<char>() + QW_REACH));
        HIP_TRY(hipGetLastError());
        uint32_t first_bad = 0;
        RR_TRY(await_reach(s, st, &first_bad));
    }
    RR_TRY(upload_shade_const(s, make_ray_frame(cfg, rays_per_result, n_results), PrimaryFrame{}, st)); // (level 1 is ray records here: nothing is derived)
    DevBuf d_ids, d_origins, d_dirs, d_out; // the host form's staging
    const uint32_t* ids = io.stream_ids;
    if (io.host || !ids) { // the caller's host ids uploaded, or 0 .. n - 1: into the call's buffer (host form) or the handle's
        DevBuf& b = io.host ? d_ids : s->query_ids;
        HIP_TRY(b.reserve((size_t)n_results * 4));
        if (ids) HIP_TRY(hipMemcpy(b.p, ids, (size_t)n_results * 4, hipMemcpyHostToDevice));
        else {
            hipLaunchKernelGGL(k_iota, dim3((n_results + RR_BLOCK - 1) / RR_BLOCK), dim3(RR_BLOCK), 0, st, b.as<uint32_t>(), n_results);
            HIP_TRY(hipGetLastError());
        }
        ids = b.as<uint32_t>();
    }
    DAccum acc;
    RR_TRY(reset_accumulators(s, n_results, true, true, true, st, &acc));
    uint64_t budget = 0;
    RR_TRY(queue_budget(s, &budget));
    const FramePlan plan = plan_ray_batches(n_rays, cfg->max_recursion, budget, s->n_enabled_lights, s->tuning.shade_chunk_rays);
    RR_TRY(grow_ray_queues(s, plan.M, plan.sq_need, 0));
    if (io.host) {
        HIP_TRY(d_origins.reserve(12ull * plan.B));
        HIP_TRY(d_dirs.reserve(12ull * plan.B));
        HIP_TRY(d_out.reserve(32ull * std::min<uint32_t>(n_results, RESOLVE_RAYS_CHUNK)));
    }
    FrameRun f{s, st, plan, cfg->max_recursion, DShadowQueue{s->sq[0].as<float4>(), s->sq[1].as<float4>(), s->sq[2].as<float4>()}, acc,
               CounterPool{s, st}, DPrimary{nullptr, PrimaryLaunch{0u, 0u, 0u, 6u}, 0u}, cancel, s->n_cus * RR_SHADOW_GRID_WG, s->n_cus * RR_SHADE_GRID_WG};
    f.slot_xy = ids;
    f.seeded = true;
    HIP_TRY(hipEventRecord(s->frame_a, st));
    int rc = run_ray_batches(f, io, rays_per_result, d_origins.as<float>(), d_dirs.as<float>());
    for (uint32_t r0 = 0; r0 < n_results && rc == RR_OK; r0 += RESOLVE_RAYS_CHUNK) {
        const uint32_t n = std::min<uint32_t>(RESOLVE_RAYS_CHUNK, n_results - r0);
        hipLaunchKernelGGL(k_resolve_rays, dim3((n + RR_BLOCK - 1) / RR_BLOCK), dim3(RR_BLOCK), 0, st, acc, r0, n, rays_per_result,
                           io.host ? d_out.as<float4>() : (float4*)(io.out + r0));
        if (!io.host) continue;
        const hipError_t e = hipMemcpyAsync(io.out + r0, d_out.p, 32ull * n, hipMemcpyDeviceToHost, st);
        if (e != hipSuccess) rc = fail(RR_ERR_DEVICE, "rr_shade_rays: %s", hipGetErrorString(e));
    }
    (void)hipEventRecord(s->frame_b, st);
    const hipError_t e = (io.host || rc != RR_OK) ? hipStreamSynchronize(st) : hipSuccess;
    if (rc != RR_OK) return rc;
    HIP_TRY(e);
    HIP_TRY(hipGetLastError());
    return RR_OK;
}

extern "C" int rr_shade_rays(rr_scene* s, const rr_config* cfg, const float* origins, const float* directions, uint32_t n_results, uint32_t rays_per_result,
                             const uint32_t* stream_ids, rr_radiance* out, const volatile int* cancel) try {
    RR_TRY(check_shade_args("rr_shade_rays", false, s, cfg, origins, directions, stream_ids, out, n_results, rays_per_result));
    if (n_results == 0) return RR_OK;
    RR_TRY(not_in_pass(s, "rr_shade_rays"));
    std::lock_guard<std::mutex> lk(s->mu);
    RR_TRY(check_intact(s));
    HIP_TRY(hipSetDevice(s->device));
    RR_FAULT_POINT("shade_rays.host");
    return shade_rays_locked(s, cfg, RayIo{origins, directions, stream_ids, out, true}, n_results, rays_per_result, nullptr, cancel);
} RR_GUARD_END("rr_shade_rays")

extern "C" int rr_shade_rays_device(rr_scene* s, const rr_config* cfg, const float* origins, const float* directions, uint32_t n_results, uint32_t rays_per_result,
                                    const uint32_t* stream_ids, rr_radiance* out, void* hip_stream, const volatile int* cancel) try {
    RR_TRY(check_shade_args("rr_shade_rays_device", true, s, cfg, origins, directions, stream_ids, out, n_results, rays_per_result));
    if (n_results == 0) return RR_OK;
    RR_TRY(not_in_pass(s, "rr_shade_rays_device"));
    std::lock_guard<std::mutex> lk(s->mu);
    RR_TRY(check_intact(s));
    HIP_TRY(hipSetDevice(s->device));
    RR_FAULT_POINT("shade_rays_device.host");
    RR_TRY(check_query_pointer(s, origins, "rr_shade_rays_device", "origins_dev"));
    RR_TRY(check_query_pointer(s, directions, "rr_shade_rays_device", "directions_dev"));
    if (stream_ids) RR_TRY(check_query_pointer(s, stream_ids, "rr_shade_rays_device", "stream_ids_dev"));
    RR_TRY(check_query_pointer(s, out, "rr_shade_rays_device", "out_dev"));
    return shade_rays_locked(s, cfg, RayIo{origins, directions, stream_ids, out, false}, n_results, rays_per_result, (hipStream_t)hip_stream, cancel);
} RR_GUARD_END("rr_shade_rays_device")

// ---------------------------------------------------------------------------
// device arithmetic probe (tests/test_device_math.py): runs rr_math.h functions on the GPU
// ---------------------------------------------------------------------------
extern "C" int rr_math_probe(int op, const float* a, const float* b, const float* c, int n, float* out0, float* out1, float* out2,
                             uint64_t seed, int device) try {
    if (n <= 0 || !a || !out0) return fail(RR_ERR_INVALID_ARGUMENT, "bad arguments");
    if (op == 11) { // the HOST build of the per-triangle shading constants (tri_shading_constants): a, b, c hold n / 3 triangles' vertices, xyz interleaved
        for (int t = 0; t + 2 < n; t += 3) {
            float ng[3], area;
            tri_shading_constants(a + t, b + t, c + t, ng, &area);
            for (int k = 0; k < 3; k++) { out0[t + k] = ng[k]; if (out1) out1[t + k] = area; }
        }
        return RR_OK;
    }
    if (op == 6) { // the HOST build of rr_cos, as make_dmaterial uses it for DMaterial::cos_*: out0[i] = rr_cos(a[i] * pi); needs no device
        for (int i = 0; i < n; i++) out0[i] = rr_cos(a[i] * RR_PI_F);
        return RR_OK;
    }
    HIP_TRY(hipSetDevice(device));
    DevBuf in[3], o[3];
    const float* src[3] = {a, b, c};
    float* dst[3] = {out0, out1, out2};
    for (int k = 0; k < 3; k++) {
        HIP_TRY(in[k].reserve((size_t)n * 4)); HIP_TRY(o[k].reserve((size_t)n * 4));
        if (src[k]) HIP_TRY(hipMemcpy(in[k].p, src[k], (size_t)n * 4, hipMemcpyHostToDevice));
        else HIP_TRY(hipMemset(in[k].p, 0, (size_t)n * 4));
        HIP_TRY(hipMemset(o[k].p, 0, (size_t)n * 4));
    }
    hipLaunchKernelGGL(k_math_probe, dim3((n + 255) / 256), dim3(256), 0, nullptr, op, in[0].as<float>(), in[1].as<float>(), in[2].as<float>(), n,
                       o[0].as<float>(), o[1].as<float>(), o[2].as<float>(), (uint32_t)seed, (uint32_t)(seed >> 32));
    HIP_TRY(hipDeviceSynchronize());
    for (int k = 0; k < 3; k++) {
        if (dst[k]) HIP_TRY(hipMemcpy(dst[k], o[k].p, (size_t)n * 4, hipMemcpyDeviceToHost));
        in[k].release(); o[k].release();
    }
    return RR_OK;
} RR_GUARD_END("rr_math_probe")

#ifdef RR_EXP_UTIL
extern "C" int rr_exp_util(unsigned long long* out64, int reset) {
    if (out64 && hipMemcpyFromSymbol(out64, HIP_SYMBOL(g_util), sizeof(g_util)) != hipSuccess) return RR_ERR_DEVICE;
    if (reset) { unsigned long long z[64] = {0}; if (hipMemcpyToSymbol(HIP_SYMBOL(g_util), z, sizeof(z)) != hipSuccess) return RR_ERR_DEVICE; }
    return RR_OK;
}
#endif
