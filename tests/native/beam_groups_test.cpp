// Host-only test of the packet top level's two-level candidate search (rustray_amd/csrc/rr_beam.h: the box test and the group rule;
// rr_scene_build.h: build_item_groups, build_tlas), built with g++ -fsanitize=address,undefined by tests/test_beam_groups.py and
// linked with rr_bvh.cpp.  The grouped search below restates rr_trace.h beam_candidates lane by lane: one group box per lane, then
// the members of the surviving groups, each against its own box.  Over seeded box sets of 17 .. 512 items -- infinite and NaN
// bounds, lo > hi, boxes around the origins -- and intervals of all eight sign combinations, zero-width origins, reciprocals at
// the float limits and exactly zero, it must name exactly the items of the flat search, each with the flat search's key bits.
#include <cstdarg>
#include <cstdio>
#include <limits>
#include <map>
#include <random>
#include <string>

#include "../../rustray_amd/csrc/rr_scene_build.h"

static std::string g_error;
static int fail(int code, const char* fmt, ...) noexcept {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    try { g_error = buf; } catch (...) { }
    return code;
}
#define CHECK(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s (last error: %s)\n", __FILE__, __LINE__, #c, g_error.c_str()); return 1; } } while (0)
typedef std::mt19937_64 Rng;
static const float INF = std::numeric_limits<float>::infinity(), QNAN = std::numeric_limits<float>::quiet_NaN();
static double U(Rng& rng, double a, double b) { return std::uniform_real_distribution<double>(a, b)(rng); }
static uint32_t bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }

typedef std::map<uint32_t, uint32_t> Found; // item -> key bits
static const float* lo3(const float4& v) { return &v.x; }

// the flat pass of beam_candidates: every item's box of set `set`
static Found flat_search(const std::vector<float4>& boxes, uint32_t n, uint32_t set, const BeamRay& br, float far) {
    Found out;
    for (uint32_t j = 0; j < n; j++) {
        const float4 lo = boxes[2 * ((size_t)n * set + j)], hi = boxes[2 * ((size_t)n * set + j) + 1];
        float key, tf;
        beam_box_test(br, lo.x, lo.y, lo.z, hi.x, hi.y, hi.z, &key, &tf);
        if (beam_item_passes(key, tf, far)) out[j] = bits(key);
    }
    return out;
}
// the grouped passes; *bad is set when a padding slot, an item out of range or a repeated item shows up
static Found grouped_search(const std::vector<float4>& rec, uint32_t n, uint32_t set, const BeamRay& br, float far, bool* bad, uint32_t* n_member_tests) {
    Found out;
    const uint32_t g = beam_group_count(n);
    const float4* members = rec.data() + 2 * (size_t)n * set;
    const float4* groups = rec.data() + 4 * (size_t)n + 2 * (size_t)g * set;
    std::vector<uint32_t> survivors;
    for (uint32_t lane = 0; lane < g; lane++) {
        float key, tf;
        beam_box_test(br, groups[2 * lane].x, groups[2 * lane].y, groups[2 * lane].z, groups[2 * lane + 1].x, groups[2 * lane + 1].y, groups[2 * lane + 1].z, &key, &tf);
        if (beam_group_passes(key, tf, far)) survivors.push_back(lane);
    }
    const uint32_t n_slots = (uint32_t)survivors.size() << RR_BEAM_GROUP_SHIFT;
    for (uint32_t s = 0; s < n_slots; s++) {
        const uint32_t slot = (survivors[s >> RR_BEAM_GROUP_SHIFT] << RR_BEAM_GROUP_SHIFT) + (s & ((1u << RR_BEAM_GROUP_SHIFT) - 1u));
        if (slot >= n) continue; // the last group is short
        ++*n_member_tests;
        const float4 lo = members[2 * (size_t)slot], hi = members[2 * (size_t)slot + 1];
        float key, tf;
        beam_box_test(br, lo.x, lo.y, lo.z, hi.x, hi.y, hi.z, &key, &tf);
        if (!beam_item_passes(key, tf, far)) continue;
        const uint32_t item = bits(lo.w);
        if (item >= n || out.count(item)) { *bad = true; continue; }
        out[item] = bits(key);
    }
    return out;
}

// ---- inputs ----------------------------------------------------------------------------------------------------------------
// 4 n float4 as build_tlas lays them out: corner boxes, then surface boxes (inside the corner boxes where both are ordinary)
static std::vector<float4> random_boxes(Rng& rng, uint32_t n, int flavour) {
    std::vector<float4> b(4 * (size_t)n);
    const double extent = flavour == 2 ? 1e30 : (flavour == 3 ? 1e-3 : 100.0);
    for (uint32_t i = 0; i < n; i++) {
        float lo[3], hi[3], slo[3], shi[3];
        for (int c = 0; c < 3; c++) {
            const double m = U(rng, -extent, extent), h = std::fabs(U(rng, 0.0, 1.0)) * extent * (rng() % 8 == 0 ? 2.0 : 0.05);
            lo[c] = (float)(m - h); hi[c] = (float)(m + h);
            slo[c] = (float)(m - 0.5 * h); shi[c] = (float)(m + 0.5 * h);
        }
        const unsigned odd = (unsigned)(rng() % 16);
        const int c = (int)(rng() % 3);
        if (flavour >= 1) {
            if (odd == 0) { lo[c] = -INF; slo[c] = -INF; }
            if (odd == 1) { hi[c] = INF; shi[c] = INF; }
            if (odd == 2) { lo[c] = INF; hi[c] = -INF; }                 // the form of an unused slot
            if (odd == 3) { lo[c] = QNAN; }
            if (odd == 4) { shi[c] = QNAN; hi[c] = QNAN; }
            if (odd == 5) { std::swap(lo[c], hi[c]); }                   // lo > hi
            if (odd == 6) { for (int k = 0; k < 3; k++) { lo[k] = -INF; hi[k] = INF; slo[k] = (float)-extent; shi[k] = (float)extent; } } // holds every origin
            if (odd == 7) { hi[c] = -INF; }                              // hi alone at -inf
            if (odd == 8) { slo[c] = INF; }
        }
        b[2 * (size_t)i] = make_float4(lo[0], lo[1], lo[2], 0.0f); b[2 * (size_t)i + 1] = make_float4(hi[0], hi[1], hi[2], 0.0f);
        b[2 * ((size_t)n + i)] = make_float4(slo[0], slo[1], slo[2], 0.0f); b[2 * ((size_t)n + i) + 1] = make_float4(shi[0], shi[1], shi[2], 0.0f);
    }
    return b;
}
static float random_reciprocal(Rng& rng) {
    const unsigned k = (unsigned)(rng() % 24);
    if (k == 0) return 0.0f;                                                                         // a reciprocal that flushed to zero
    if (k <= 2) return std::numeric_limits<float>::min() * (float)U(rng, 1.0, 4.0);
    if (k <= 4) return 1.00001e30f * (float)U(rng, 0.5, 1.0);                                        // |d| > 1e-30
    if (k <= 6) return std::numeric_limits<float>::denorm_min() * (float)(2 + rng() % 100);
    return (float)std::pow(10.0, U(rng, -3.0, 3.0));
}
static BeamRay random_ray(Rng& rng, unsigned signs, int flavour) {
    BeamRay r;
    r.negx = signs & 1u; r.negy = (signs >> 1) & 1u; r.negz = (signs >> 2) & 1u;
    const double extent = flavour == 2 ? 1e30 : (flavour == 3 ? 1e-3 : 100.0);
    float* o[3][2] = {{&r.oxl, &r.oxh}, {&r.oyl, &r.oyh}, {&r.ozl, &r.ozh}};
    float* a[3][2] = {{&r.axl, &r.axh}, {&r.ayl, &r.ayh}, {&r.azl, &r.azh}};
    const bool point = rng() % 2 == 0; // zero-width origins: the rays of one pixel
    for (int c = 0; c < 3; c++) {
        const float m = (float)U(rng, -1.5 * extent, 1.5 * extent);
        *o[c][0] = m; *o[c][1] = point ? m : m + (float)(std::fabs(U(rng, 0.0, 0.1)) * extent);
        const float x = random_reciprocal(rng), y = rng() % 2 ? x : random_reciprocal(rng);
        *a[c][0] = std::min(x, y) * 0.99999f; *a[c][1] = std::max(x, y) * 1.00001f;
    }
    return r;
}

// ---- 1. the grouped search against the flat search ---------------------------------------------------------------------------
static int test_searches() {
    Rng rng(2024);
    unsigned long long cases = 0, grouped_cases = 0, flat_tests = 0, member_tests = 0, candidates = 0, zero_reciprocal = 0;
    const uint32_t sizes[] = {17u, 40u, 64u, 65u, 72u, 73u, 128u, 129u, 194u, 200u, 256u, 257u, 505u, 511u, 512u}; // 65, 73, 129, 257, 505: one more than whole groups
    for (uint32_t n : sizes) {
        for (int set_no = 0; set_no < 24; set_no++) {
            const int flavour = set_no % 4; // 0 ordinary, 1 with odd boxes, 2 huge (differences overflow), 3 tiny
            const std::vector<float4> boxes = random_boxes(rng, n, flavour);
            std::vector<float4> rec, again;
            build_item_groups(boxes, n, &rec);
            build_item_groups(boxes, n, &again);
            CHECK(rec.size() == beam_group_records(n) && rec.size() == again.size() && (rec.empty() || memcmp(rec.data(), again.data(), rec.size() * sizeof(float4)) == 0));
            CHECK(beam_grouped(n) == (n > 64u) && (rec.empty() == !beam_grouped(n)));
            if (beam_grouped(n)) {
                const uint32_t g = beam_group_count(n);
                CHECK(g <= 64u && (g << RR_BEAM_GROUP_SHIFT) >= n && ((g - 1u) << RR_BEAM_GROUP_SHIFT) < n && rec.size() == 4 * (size_t)n + 4 * (size_t)g);
                for (uint32_t set = 0; set < 2; set++) {
                    std::vector<bool> seen(n, false);
                    for (uint32_t slot = 0; slot < n; slot++) { // the members: a permutation of the items, each with its own box, bit for bit
                        const float4 lo = rec[2 * ((size_t)n * set + slot)], hi = rec[2 * ((size_t)n * set + slot) + 1];
                        const uint32_t item = bits(lo.w);
                        CHECK(item < n && !seen[item]);
                        seen[item] = true;
                        CHECK(item == bits(rec[2 * (size_t)slot].w)); // one membership for both box sets
                        CHECK(memcmp(&lo, &boxes[2 * ((size_t)n * set + item)], 12) == 0 && memcmp(&hi, &boxes[2 * ((size_t)n * set + item) + 1], 12) == 0);
                        const float4 glo = rec[4 * (size_t)n + 2 * ((size_t)g * set + (slot >> RR_BEAM_GROUP_SHIFT))], ghi = rec[4 * (size_t)n + 2 * ((size_t)g * set + (slot >> RR_BEAM_GROUP_SHIFT)) + 1];
                        for (int c = 0; c < 3; c++) { // the group box contains it, and is never NaN; a bound that is not finite opens the side
                            const float ml = lo3(lo)[c], mh = lo3(hi)[c], gl = lo3(glo)[c], gh = lo3(ghi)[c];
                            CHECK(gl == gl && gh == gh);
                            CHECK(std::isfinite(ml) ? gl <= ml : gl == -INF);
                            CHECK(std::isfinite(mh) ? gh >= mh : gh == INF);
                        }
                    }
                }
            }
            for (int k = 0; k < 480; k++) {
                const BeamRay br = random_ray(rng, (unsigned)k & 7u, flavour);
                const uint32_t set = (uint32_t)(k >> 3) & 1u;
                const float far = k % 5 == 0 ? std::numeric_limits<float>::max() : (k % 5 == 1 ? INF : (float)std::pow(10.0, U(rng, -2.0, 3.0)));
                const Found flat = flat_search(boxes, n, set, br, far);
                cases++; flat_tests += n; candidates += flat.size();
                const bool zero = !beam_ray_takes_groups(br);
                zero_reciprocal += zero;
                CHECK(zero == (br.axl == 0.0f || br.ayl == 0.0f || br.azl == 0.0f));
                if (!beam_grouped(n) || zero) continue; // beam_candidates takes the flat pass: nothing to compare
                bool bad = false;
                uint32_t tested = 0;
                const Found grouped = grouped_search(rec, n, set, br, far, &bad, &tested);
                grouped_cases++; member_tests += tested;
                CHECK(!bad);
                if (grouped != flat) {
                    std::printf("n %u set %u case %d: flat %zu grouped %zu candidates\n", n, set, k, flat.size(), grouped.size());
                    for (const auto& f : flat) if (!grouped.count(f.first)) std::printf("  item %u lost\n", f.first);
                }
                CHECK(grouped == flat); // the same items, and per item the same key bits
            }
        }
    }
    std::printf("searches: %llu cases (%llu grouped, %llu with a zero reciprocal bound), %.1f candidates per case, member tests %.1f%% of the flat pass's\n", cases, grouped_cases, zero_reciprocal,
                (double)candidates / (double)cases, grouped_cases ? 100.0 * (double)member_tests / ((double)flat_tests * (double)grouped_cases / (double)cases) : 0.0);
    CHECK(grouped_cases >= 100000 && zero_reciprocal >= 1000);
    return 0;
}

// ---- 2. a group test that is NaN lets the group through -------------------------------------------------------------------
static int test_nan_group_passes() {
    CHECK(beam_group_passes(1.0f, QNAN, 10.0f) && !beam_item_passes(1.0f, QNAN, 10.0f));
    CHECK(beam_group_passes(QNAN, 2.0f, 10.0f) && beam_group_passes(1.0f, 2.0f, QNAN));
    CHECK(!beam_group_passes(3.0f, 2.0f, 10.0f) && !beam_group_passes(1.0f, 2.0f, 0.5f) && beam_group_passes(1.0f, 2.0f, 10.0f));
    // the real thing: an open group box against a packet whose reciprocals all flushed to zero: every product is inf * 0
    BeamRay br;
    br.negx = false; br.negy = true; br.negz = false;
    br.oxl = br.oxh = 1.0f; br.oyl = br.oyh = 2.0f; br.ozl = br.ozh = 3.0f;
    br.axl = br.axh = br.ayl = br.ayh = br.azl = br.azh = 0.0f;
    float key, tf;
    beam_box_test(br, -INF, -INF, -INF, INF, INF, INF, &key, &tf);
    CHECK(tf != tf && beam_group_passes(key, tf, 1.0f) && !beam_item_passes(key, tf, 1.0f));
    CHECK(!beam_ray_takes_groups(br)); // (and such a packet does not search the groups to begin with)
    return 0;
}

// ---- 3. build_tlas: the appended records, their sizes, determinism --------------------------------------------------------------
static int test_build_tlas() {
    const double none[3] = {0, 0, 0};
    for (uint32_t n : {17u, 64u, 65u, 512u}) {
        Rng rng(n);
        rr_material m;
        memset(&m, 0, sizeof m);
        for (int k = 0; k < 3; k++) m.base_color[k] = 0.5f;
        m.alpha = 1.0f; m.shininess = 8.0f; m.refraction_index = 1.0f; m.shadow_softness = 0.01f; m.roughness = 0.2f;
        for (int k = 0; k < RR_TEX_COUNT; k++) m.texture[k] = -1;
        m.cast_shadow = m.receive_shadow = m.smooth_shading = m.backface_cullig = 1;
        std::vector<rr_item> items(n);
        for (uint32_t i = 0; i < n; i++) { // balls of many sizes, scattered
            rr_item& it = items[i];
            memset(&it, 0, sizeof it);
            it.kind = RR_ITEM_SPHERE; it.id = i + 1u; it.mesh = -1; it.radius = 1.0f; it.visible = 1;
            const float s = (float)std::pow(10.0, U(rng, -1.0, 1.0)), t[3] = {(float)U(rng, -50, 50), (float)U(rng, -5, 5), (float)U(rng, -50, 50)};
            it.trans[0] = it.trans[5] = it.trans[10] = s; it.trans[15] = 1.0f;
            it.trans_inv[0] = it.trans_inv[5] = it.trans_inv[10] = 1.0f / s; it.trans_inv[15] = 1.0f;
            for (int k = 0; k < 3; k++) { it.trans[12 + k] = t[k]; it.trans_inv[12 + k] = -t[k] / s; it.bbox_min[k] = -1.0f; it.bbox_max[k] = 1.0f; }
        }
        rr_flat_scene fs;
        memset(&fs, 0, sizeof fs);
        fs.abi_version = RR_ABI_VERSION;
        fs.n_items = n; fs.items = items.data(); fs.n_materials = 1; fs.materials = &m;
        SceneRecords r;
        CHECK(validate_scene(&fs) == RR_OK && build_scene_records(&fs, &r) == RR_OK);
        TlasTrees a, b;
        CHECK(build_tlas(r.items, std::vector<double>(), r.tlas_depth_limit, none, &a) == RR_OK);
        CHECK(build_tlas(r.items, std::vector<double>(), r.tlas_depth_limit, none, &b) == RR_OK);
        CHECK(a.item_boxes.size() == 4 * (size_t)n && memcmp(a.item_boxes.data(), b.item_boxes.data(), a.item_boxes.size() * sizeof(float4)) == 0);
        const size_t want = n <= 64u ? 0 : 4 * (size_t)n + 4 * (size_t)((n + 7u) / 8u); // 65: 260 + 36, 512: 2048 + 256
        CHECK(a.item_groups.size() == want && a.item_groups.size() == beam_group_records(n) && b.item_groups.size() == want);
        CHECK(want == 0 || memcmp(a.item_groups.data(), b.item_groups.data(), want * sizeof(float4)) == 0);
        std::vector<float4> direct;
        build_item_groups(a.item_boxes, n, &direct);
        CHECK(direct.size() == want && (want == 0 || memcmp(direct.data(), a.item_groups.data(), want * sizeof(float4)) == 0));
        if (want == 0) continue;
        // a scattered scene: the sort is spatial -- the groups' boxes are small beside the scene, so a thin packet passes few of them
        BeamRay br;
        br.negx = br.negy = br.negz = false;
        br.oxl = br.oxh = -60.0f; br.oyl = br.oyh = 0.0f; br.ozl = br.ozh = -60.0f;
        br.axl = 0.99f; br.axh = 1.01f; br.ayl = 50.0f; br.ayh = 100.0f; br.azl = 0.99f; br.azh = 1.01f; // along the diagonal of the floor plan
        bool bad = false;
        uint32_t tested = 0;
        const Found g = grouped_search(a.item_groups, n, 0u, br, std::numeric_limits<float>::max(), &bad, &tested);
        CHECK(!bad && g == flat_search(a.item_boxes, n, 0u, br, std::numeric_limits<float>::max()));
        std::printf("build_tlas n %u: %zu group records, diagonal packet: %u member tests, %zu candidates\n", n, want, tested, g.size());
        CHECK(tested < n); // fewer box tests than the flat pass, which makes n
    }
    return 0;
}

int main() {
    if (test_searches() || test_nan_group_passes() || test_build_tlas()) return 1;
    std::printf("beam groups test OK\n");
    return 0;
}
