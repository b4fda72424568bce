// Host-only test of rustray_amd/csrc/rr_primary_setup.h (built with g++ -ffp-contract=off -fsanitize=address,undefined by
// tests/test_primary_setup.py): the primary ray a kernel builds from the host's tables and index constants against the per-ray
// formula those replaced, as bit patterns, over every (pixel, sample) of small frames; and the exact division by a run-time
// constant against the machine's own division.
#include "../../rustray_amd/csrc/rr_frame_plan.h"
#include "../../rustray_amd/csrc/rr_primary_setup.h"

#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <thread>
#include <vector>

#define CHECK(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

struct V3 { float x, y, z; };
struct V4 { float x, y, z, w; };
static V3 mk3(float x, float y, float z) { return V3{x, y, z}; }
static V4 make_v4(float x, float y, float z, float w) { return V4{x, y, z, w}; }
static float dot3(V3 a, V3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
static float norm3(V3 a) { return sqrtf(dot3(a, a)); }
static V3 normalize3(V3 a) { const float n = norm3(a); return mk3(a.x / n, a.y / n, a.z / n); }
static V4 mat4_mul(const float* m, float x, float y, float z, float w) {
    return make_v4(((m[0] * x + m[4] * y) + m[8] * z) + m[12] * w,
                   ((m[1] * x + m[5] * y) + m[9] * z) + m[13] * w,
                   ((m[2] * x + m[6] * y) + m[10] * z) + m[14] * w,
                   ((m[3] * x + m[7] * y) + m[11] * z) + m[15] * w);
}

struct Ray { V3 o, d; uint32_t pix, sample; };

// THE REFERENCE: primary_ray as the kernels evaluated it per ray before the set-up moved to the host (rr_kernels.hip), restated
// line for line: run-time divisions of the index, the pixel's centre and the sample's offset from (x, y) and (x_i, y_i).
static Ray ref_primary_ray(const DFrame& fr, const uint32_t* slot_xy, const uint16_t* sample_xy, unsigned long long first, uint32_t group, uint32_t i) {
    uint32_t pix, s;
    if (group <= 1u) {
        const unsigned long long gi = first + i;
        pix = (uint32_t)(gi % fr.n_region_pixels);
        s = (uint32_t)(gi / fr.n_region_pixels);
    } else {
        const uint32_t ppp = RR_WAVE / group;
        const uint32_t packets_per_group = fr.n_region_pixels / ppp;
        const uint32_t pkt = i / RR_WAVE, lane = i % RR_WAVE;
        pix = (pkt % packets_per_group) * ppp + lane / group;
        s = (uint32_t)(first / fr.n_region_pixels) + (pkt / packets_per_group) * group + lane % group;
    }
    uint32_t xy = slot_xy[pix];
    float x_f = (float)(xy & 0xffffu), y_f = (float)(xy >> 16);
    float w = (float)fr.width, h = (float)fr.height;
    float x_step = 2.0f / w, y_step = 2.0f / h;
    float x_i = (float)sample_xy[2u * s], y_i = (float)sample_xy[2u * s + 1u];
    float inv_cell = 1.0f / (float)fr.cell_size;
    float x_trans = x_step * x_i * inv_cell;
    float y_trans = y_step * y_i * inv_cell;
    if (fr.dof && fr.samples > 1u) { x_trans -= x_step / 2.0f; y_trans -= y_step / 2.0f; }
    V3 origin, dir;
    if (fr.dof) {
        float aperture_scale = (float)fr.width / 800.0f;
        x_trans *= fr.aperture_size * aperture_scale;
        y_trans *= fr.aperture_size * aperture_scale;
        float cx = ((x_f + 0.5f) / w) * 2.0f - 1.0f;
        float cy = 1.0f - ((y_f + 0.5f) / h) * 2.0f;
        V4 cpp = mat4_mul(fr.proj_inv, cx, cy, -1.0f, 1.0f);
        V3 rd = mk3(cpp.x - 0.0f, cpp.y - 0.0f, cpp.z - 0.0f);
        V4 eye = mat4_mul(fr.view_inv, 0.0f, 0.0f, 0.0f, 1.0f);
        V4 dv = mat4_mul(fr.view_inv, rd.x, rd.y, rd.z, 0.0f);
        float dn = sqrtf((dv.x * dv.x + dv.z * dv.z) + (dv.y * dv.y + dv.w * dv.w));
        V4 dvn = make_v4(dv.x / dn, dv.y / dn, dv.z / dn, dv.w / dn);
        float dist = norm3(rd);
        float f = 1.0f / (dist / (dist + fr.focal_length));
        V3 p = mk3(eye.x + f * dvn.x, eye.y + f * dvn.y, eye.z + f * dvn.z);
        float sx = (((x_f + 0.5f) / w) * 2.0f - 1.0f) + x_trans;
        float sy = (1.0f - ((y_f + 0.5f) / h) * 2.0f) + y_trans;
        V4 pp = mat4_mul(fr.proj_inv, sx, sy, -1.0f, 1.0f);
        V4 ro = mat4_mul(fr.view_inv, pp.x, pp.y, pp.z, 1.0f);
        origin = mk3(ro.x, ro.y, ro.z);
        dir = mk3(p.x - ro.x, p.y - ro.y, p.z - ro.z);
    } else {
        float sx = (((x_f + 0.5f) / w) * 2.0f - 1.0f) + x_trans;
        float sy = (1.0f - ((y_f + 0.5f) / h) * 2.0f) + y_trans;
        V4 pp = mat4_mul(fr.proj_inv, sx, sy, -1.0f, 1.0f);
        V4 o = mat4_mul(fr.view_inv, pp.x, pp.y, pp.z, 1.0f);
        V4 d = mat4_mul(fr.view_inv, pp.x - 0.0f, pp.y - 0.0f, pp.z - 0.0f, 0.0f);
        origin = mk3(o.x, o.y, o.z);
        dir = mk3(d.x, d.y, d.z);
    }
    dir = normalize3(dir);
    return Ray{origin, dir, pix, s};
}

// The kernels' primary_ray of today on the host: the index from primary_index, two table reads, then the arithmetic that does
// depend on the ray.
static Ray new_primary_ray(const DFrame& fr, const PrimaryFrame& pf, const float* sample_tr, const PrimaryLaunch& at, uint32_t i) {
    uint32_t pix, s;
    primary_index(pf, at, i, &pix, &s);
    const float cx = pf.slot_c[2u * pix], cy = pf.slot_c[2u * pix + 1u];
    const float x_trans = sample_tr[2u * s], y_trans = sample_tr[2u * s + 1u];
    V3 origin, dir;
    if (fr.dof) {
        V4 cpp = mat4_mul(fr.proj_inv, cx, cy, -1.0f, 1.0f);
        V3 rd = mk3(cpp.x - 0.0f, cpp.y - 0.0f, cpp.z - 0.0f);
        V4 eye = mat4_mul(fr.view_inv, 0.0f, 0.0f, 0.0f, 1.0f);
        V4 dv = mat4_mul(fr.view_inv, rd.x, rd.y, rd.z, 0.0f);
        float dn = sqrtf((dv.x * dv.x + dv.z * dv.z) + (dv.y * dv.y + dv.w * dv.w));
        V4 dvn = make_v4(dv.x / dn, dv.y / dn, dv.z / dn, dv.w / dn);
        float dist = norm3(rd);
        float f = 1.0f / (dist / (dist + fr.focal_length));
        V3 p = mk3(eye.x + f * dvn.x, eye.y + f * dvn.y, eye.z + f * dvn.z);
        float sx = cx + x_trans;
        float sy = cy + y_trans;
        V4 pp = mat4_mul(fr.proj_inv, sx, sy, -1.0f, 1.0f);
        V4 ro = mat4_mul(fr.view_inv, pp.x, pp.y, pp.z, 1.0f);
        origin = mk3(ro.x, ro.y, ro.z);
        dir = mk3(p.x - ro.x, p.y - ro.y, p.z - ro.z);
    } else {
        float sx = cx + x_trans;
        float sy = cy + y_trans;
        V4 pp = mat4_mul(fr.proj_inv, sx, sy, -1.0f, 1.0f);
        V4 o = mat4_mul(fr.view_inv, pp.x, pp.y, pp.z, 1.0f);
        V4 d = mat4_mul(fr.view_inv, pp.x - 0.0f, pp.y - 0.0f, pp.z - 0.0f, 0.0f);
        origin = mk3(o.x, o.y, o.z);
        dir = mk3(d.x, d.y, d.z);
    }
    dir = normalize3(dir);
    return Ray{origin, dir, pix, s};
}

static uint64_t g_state = 0x9e3779b97f4a7c15ull; // splitmix64, fixed seed
static uint64_t rnd() {
    uint64_t z = (g_state += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

// a perspective camera looking down at an angle: the inverse projection and the inverse view as the callers pass them
static void camera(uint32_t w, uint32_t h, DFrame* fr) {
    const float t = 0.41421357f, a = (float)w / (float)h, zn = 0.1f, zf = 1000.0f;
    const float pi[16] = {a * t, 0, 0, 0, 0, t, 0, 0, 0, 0, 0, (zn - zf) / (2.0f * zf * zn), 0, 0, -1.0f, (zf + zn) / (2.0f * zf * zn)};
    const float c = 0.8660254f, s = 0.5f;
    const float vi[16] = {c, 0, -s, 0, 0.25f, 0.9375f, 0.4330127f, 0, s * 0.9375f, -0.25f, c * 0.9375f, 0, 3.5f, 7.25f, -12.125f, 1.0f};
    std::memcpy(fr->proj_inv, pi, sizeof pi);
    std::memcpy(fr->view_inv, vi, sizeof vi);
}

static uint64_t g_rays = 0;

// every primary index of the batches (first, n) of one frame: the new derivation against the reference, bit for bit, and every
// (slot, sample) exactly once
static int check_batches(const DFrame& fr, const std::vector<uint32_t>& slot_xy, const std::vector<uint16_t>& sample_xy, const FramePlan& plan,
                         const std::vector<float>& slot_c, const std::vector<float>& sample_tr, uint64_t B, bool want_group, bool want_mid_slice) {
    const uint32_t npix = fr.n_region_pixels;
    const PrimaryFrame pf = primary_frame(slot_c.data(), npix, plan.G);
    std::vector<uint8_t> seen((size_t)npix * fr.samples, 0);
    bool grouped = false, mid_slice = false, later = false;
    for (uint64_t first = 0; first < plan.total_primary; first += B) {
        const uint32_t n = (uint32_t)std::min<uint64_t>(B, plan.total_primary - first);
        const uint32_t G = batch_group(plan, npix, first, n);
        const PrimaryLaunch at = primary_launch(first, npix, G);
        CHECK((1u << at.lg_group) == G && (1u << at.lg_pixels) == 64u / G);
        CHECK(at.first_sample == first / npix && at.first_pix == first % npix);
        grouped |= G > 1; mid_slice |= first % npix != 0; later |= first != 0;
        for (uint32_t i = 0; i < n; i++) {
            const Ray a = ref_primary_ray(fr, slot_xy.data(), sample_xy.data(), first, G, i);
            const Ray b = new_primary_ray(fr, pf, sample_tr.data(), at, i);
            if (std::memcmp(&a, &b, sizeof a) != 0) {
                std::printf("FAILED: %ux%u slots %u cell %u samples %u dof %u G %u first %llu i %u: (%a %a %a | %a %a %a | %u %u) != (%a %a %a | %a %a %a | %u %u)\n",
                            fr.width, fr.height, npix, fr.cell_size, fr.samples, fr.dof, G, (unsigned long long)first, i,
                            a.o.x, a.o.y, a.o.z, a.d.x, a.d.y, a.d.z, a.pix, a.sample, b.o.x, b.o.y, b.o.z, b.d.x, b.d.y, b.d.z, b.pix, b.sample);
                return 1;
            }
            CHECK(a.pix < npix && a.sample < fr.samples);
            seen[(size_t)a.sample * npix + a.pix]++;
        }
        g_rays += n;
    }
    for (uint8_t c : seen) CHECK(c == 1);
    if (want_group) CHECK(grouped);
    if (want_mid_slice) CHECK(mid_slice);
    if (B < plan.total_primary) CHECK(later);
    return 0;
}

static int check_frames() {
    struct Size { uint32_t w, h, rx, ry, rw, rh; }; // the frame, and a region of it that does not start at the origin
    const Size sizes[] = {{7, 5, 2, 1, 4, 3}, {64, 48, 8, 16, 24, 16}, {70, 50, 6, 10, 64, 32}};
    const uint32_t cells[] = {1, 2, 16}, sample_counts[] = {1, 3, 6, 64, 128}, groups[] = {0, 1, 2, 64};
    for (const Size& z : sizes) for (int region = 0; region < 2; region++) {
        const uint32_t x0 = region ? z.rx : 0, y0 = region ? z.ry : 0, rw = region ? z.rw : z.w, rh = region ? z.rh : z.h;
        // the region's slots in a scrambled order (the frame driver's order, 8x8 blocks inside tiles, is one such order)
        std::vector<uint32_t> slot_xy;
        for (uint32_t y = 0; y < rh; y++) for (uint32_t x = 0; x < rw; x++) slot_xy.push_back((x0 + x) | ((y0 + y) << 16));
        for (size_t j = slot_xy.size(); j > 1; j--) std::swap(slot_xy[j - 1], slot_xy[rnd() % j]);
        const uint32_t npix = (uint32_t)slot_xy.size();
        std::vector<float> slot_c(2 * (size_t)npix);
        primary_slot_centres(slot_xy.data(), npix, z.w, z.h, slot_c.data());
        for (uint32_t cell : cells) for (uint32_t samples : sample_counts) for (int dof = 0; dof < 2; dof++) {
            DFrame fr;
            std::memset(&fr, 0, sizeof fr);
            camera(z.w, z.h, &fr);
            fr.width = z.w; fr.height = z.h; fr.samples = samples; fr.cell_size = cell; fr.n_region_pixels = npix;
            fr.dof = (uint32_t)dof; fr.aperture_size = dof ? 16.0f : 0.0f; fr.focal_length = dof ? 20.0f : 0.0f;
            std::vector<uint16_t> sample_xy(2 * (size_t)samples);
            for (uint16_t& v : sample_xy) v = (uint16_t)(rnd() % (2 * cell + 1));
            std::vector<float> sample_tr(2 * (size_t)samples);
            primary_sample_offsets(sample_xy.data(), PrimarySampleKey{z.w, z.h, cell, (uint32_t)dof, samples, fr.aperture_size}, sample_tr.data());
            for (uint32_t forced : groups) for (int small_budget = 0; small_budget < 2; small_budget++) {
                // a budget that holds the frame in one batch, and one that cuts it into batches of one whole group (at least 4096 rays)
                const uint64_t small = 128ull * npix * (forced ? forced : 64u);
                const FramePlan plan = plan_frame(FramePlanInputs{npix, samples, 4, small_budget ? small : 1ull << 34, forced, 0, 2, 1, 0});
                const bool allowed = forced >= 2 && samples % forced == 0 && npix % (64 / forced) == 0;
                if (forced >= 2) CHECK((plan.G == forced) == allowed);
                if (forced == 0 && samples % 64 == 0) CHECK(plan.G == 64);
                if (check_batches(fr, slot_xy, sample_xy, plan, slot_c, sample_tr, plan.B, plan.G > 1, false)) return 1;
            }
            // batches that start in the middle of a sample slice: one sample of 64 pixels per packet is then the only form
            const FramePlan whole = plan_frame(FramePlanInputs{npix, samples, 4, 1ull << 34, 1, 0, 2, 1, 0});
            const uint64_t odd = std::max<uint64_t>(1, whole.total_primary / 3) + 7;
            if (check_batches(fr, slot_xy, sample_xy, whole, slot_c, sample_tr, odd, false, whole.total_primary > odd && odd % npix != 0)) return 1;
        }
    }
    return 0;
}

// ---- the exact division ---------------------------------------------------------------------------------------------------------
static std::vector<uint32_t> divisors() {
    std::vector<uint32_t> d = {1, 2, 3, 7, 640, 14400, 921600};
    for (uint32_t k = 1; k <= 31; k++) { d.push_back((1u << k) - 1u); d.push_back(1u << k); d.push_back((1u << k) + 1u); }
    d.push_back(0xffffffffu); // 2^32 - 1
    std::sort(d.begin(), d.end());
    d.erase(std::unique(d.begin(), d.end()), d.end());
    return d;
}

// work items [0, n) on up to 16 threads; false when one of them failed
template <class F> static bool parallel(size_t n, F f) {
    std::atomic<size_t> next{0};
    std::atomic<bool> ok{true};
    const unsigned nt = std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
    std::vector<std::thread> pool;
    for (unsigned t = 0; t < nt; t++) pool.emplace_back([&] { for (size_t j; (j = next++) < n;) if (!f(j)) ok = false; });
    for (auto& t : pool) t.join();
    return ok;
}

static int check_division() {
    const std::vector<uint32_t> ds = divisors();
    // packet indices: every dividend below 2^25 (quotient and remainder follow the dividend by counting: no division in the loop)
    CHECK(parallel(ds.size(), [&](size_t j) {
        const RrDiv dv = rr_div_make_small(ds[j]);
        uint32_t q = 0, r = 0;
        for (uint32_t n = 0; n < (1u << RR_DIV_SMALL_BITS); n++) {
            if (rr_div_small(n, dv) != q) { std::printf("FAILED: rr_div_small(%u, %u) = %u, not %u\n", n, ds[j], rr_div_small(n, dv), q); return false; }
            if (++r == ds[j]) { r = 0; q++; }
        }
        return true;
    }));
    // any 32-bit dividend: every multiple of the divisor and its two neighbours, and the top of the range; in slices of 2^24 multiples
    struct Slice { uint32_t d; uint64_t k0, k1; };
    std::vector<Slice> slices;
    for (uint32_t d : ds) {
        const uint64_t last = 0xffffffffull / d; // multiples k * d, k = 0 .. last
        for (uint64_t k0 = 0; k0 <= last; k0 += 1ull << 24) slices.push_back(Slice{d, k0, std::min<uint64_t>(last + 1, k0 + (1ull << 24))});
    }
    CHECK(parallel(slices.size(), [&](size_t j) {
        const Slice& sl = slices[j];
        const uint32_t d = sl.d;
        const RrDiv dv = rr_div_make_wide(d);
        for (uint64_t k = sl.k0; k < sl.k1; k++) {
            const uint32_t m = (uint32_t)(k * d);
            bool good = rr_div_wide(m, dv) == (uint32_t)k;
            if (k > 0) good &= rr_div_wide(m - 1u, dv) == (uint32_t)(k - 1);
            if ((uint64_t)m + 1 <= 0xffffffffull) good &= rr_div_wide(m + 1u, dv) == (uint32_t)(d == 1 ? k + 1 : k);
            if (!good) { std::printf("FAILED: rr_div_wide near %u / %u\n", m, d); return false; }
        }
        return true;
    }));
    for (uint32_t d : ds) {
        const RrDiv dv = rr_div_make_wide(d);
        for (uint32_t n = 0xffffffffu; n > 0xffffffffu - 4096u; n--) CHECK(rr_div_wide(n, dv) == n / d);
    }
    for (uint32_t k = 0; k < 10000000u; k++) { // 10^7 random pairs; the divisors of all magnitudes
        const uint32_t n = (uint32_t)rnd();
        uint32_t d = (uint32_t)rnd() >> (rnd() % 32);
        if (d == 0) d = 1;
        const RrDiv dv = rr_div_make_wide(d);
        if (rr_div_wide(n, dv) != n / d) { std::printf("FAILED: rr_div_wide(%u, %u) = %u, not %u\n", n, d, rr_div_wide(n, dv), n / d); return 1; }
        const RrDiv ds_ = rr_div_make_small(d);
        const uint32_t n25 = n >> 7;
        if (rr_div_small(n25, ds_) != n25 / d) { std::printf("FAILED: rr_div_small(%u, %u) = %u, not %u\n", n25, d, rr_div_small(n25, ds_), n25 / d); return 1; }
    }
    return 0;
}

int main() {
    if (check_frames()) return 1;
    std::printf("%llu primary rays equal bit for bit\n", (unsigned long long)g_rays);
    if (check_division()) return 1;
    std::printf("primary setup test OK\n");
    return 0;
}
