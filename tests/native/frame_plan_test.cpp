// Host-only test of rustray_amd/csrc/rr_frame_plan.h (built with g++ -fsanitize=address,undefined by tests/test_frame_plan.py):
// the batch / arena / shade-chunk sizing of a frame against a table of expected plans, and its invariants over a sweep.
#include "../../rustray_amd/csrc/rr_frame_plan.h"

#include <cstdio>

#define CHECK(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

struct Case { const char* name; FramePlanInputs in; uint64_t B; uint32_t G; uint64_t M, chunk, sq_need; };

// Expected plans, computed with the sizing arithmetic as it stood inside the frame driver before it moved into rr_frame_plan.h.
static const uint64_t GB64 = 64ull << 30;
static const uint32_t P720 = 1280 * 720;
static const Case k_cases[] = {
    // name                        npix    spp   R  budget           group passes af lights chunk      B           G   M            chunk      sq_need
    {"contract 1280x720 128 spp",  {P720,  128,  6, GB64,            0,    0,     2,  1,    0},        117964800, 64, 306786962,  67108864, 67117056},
    {"queue budget 1 B",           {P720,  128,  6, 1,               0,    0,     2,  1,    0},        4096,      1,  11776,      67108864, 19968},
    {"min_passes 4",               {P720,  128,  6, GB64,            0,    4,     2,  1,    0},        29491200,  32, 206441984,  67108864, 67117056},
    {"min_passes 16",              {P720,  128,  6, GB64,            0,    16,    2,  1,    0},        7372800,   8,  51613184,   67108864, 51621376},
    {"sample_group 1",             {P720,  128,  6, GB64,            1,    0,     2,  1,    0},        117964800, 1,  306786962,  67108864, 67117056},
    {"sample_group 4",             {P720,  128,  6, GB64,            4,    0,     2,  1,    0},        117964800, 4,  306786962,  67108864, 67117056},
    {"sample_group 64, 96 spp",    {P720,  96,   6, GB64,            64,   0,     2,  1,    0},        88473600,  1,  306786962,  67108864, 67117056},
    {"0 lights",                   {P720,  128,  6, GB64,            0,    0,     2,  0,    0},        117964800, 64, 306786962,  67108864, 67117056},
    {"40 lights",                  {P720,  128,  6, GB64,            0,    0,     2,  40,   0},        117964800, 64, 306786962,  8945664,  358154240},
    {"arena_factor 128",           {P720,  128,  6, GB64,            0,    0,     128, 1,   0},        117964800, 64, 1193432868, 67108864, 67117056},
    {"1x1, 1 spp",                 {1,     1,    6, GB64,            0,    0,     2,  1,    0},        1,         1,  3591,       67108864, 11783},
    {"1x1, 128 spp",               {1,     128,  6, GB64,            0,    0,     2,  1,    0},        128,       64, 4480,       67108864, 12672},
    {"lopsided 4097x3",            {12291, 6,    12, 1ull << 28,     0,    0,     2,  3,    100000},   73746,     1,  522878,     100000,   324576},
    {"tiles pass of 1280x720",     {57600, 32,   4, 1ull << 24,      0,    0,     8,  2,    0},        115200,    2,  269238,     67108864, 554860},
    {"shade_chunk_rays 1",         {P720,  128,  6, GB64,            0,    0,     2,  1,    1},        117964800, 64, 306786962,  65536,    73728},
};

static int check_invariants(const FramePlanInputs& in) {
    const FramePlan p = plan_frame(in);
    CHECK(p.total_primary == (uint64_t)in.npix * in.samples);
    CHECK(p.B >= 1 && p.B <= p.total_primary && p.B <= RR_LEVEL_MAX);
    CHECK(p.M <= RR_LEVEL_MAX && p.M >= 2ull * RR_BLOCK * (in.max_recursion + 1));
    CHECK(p.chunk >= 65536 && p.sq_need >= 1);
    CHECK(p.G >= 1 && p.G <= 64 && (p.G & (p.G - 1)) == 0 && in.samples % p.G == 0);
    if (in.sample_group) CHECK(p.G == in.sample_group || p.G == 1);
    if (p.G > 1) CHECK(in.npix % (RR_WAVE / p.G) == 0 && p.B % ((uint64_t)in.npix * p.G) == 0);
    // the batch loop of the frame driver: every batch but the last holds exactly B rays, and with G > 1 whole sample groups
    uint64_t batches = 0;
    for (uint64_t first = 0; first < p.total_primary && batches < 4096; first += p.B, batches++) {
        const uint64_t n = std::min<uint64_t>(p.B, p.total_primary - first);
        CHECK(n == p.B || first + n == p.total_primary);
        if (p.G > 1) CHECK(n % ((uint64_t)in.npix * p.G) == 0 && batch_group(p, in.npix, first, n) == p.G);
        else CHECK(batch_group(p, in.npix, first, n) == 1);
    }
    return 0;
}

static int check_level_slice(uint64_t M, uint64_t child_base, uint64_t n, uint32_t d, uint32_t R) {
    const uint64_t slice = level_slice(M, child_base, n, d, R);
    if (d > R) { CHECK(slice == n); return 0; }
    const uint64_t keep = 2ull * RR_BLOCK * (R - d), room = M - child_base;
    if (slice == 0) { CHECK(room < keep + 2ull * RR_BLOCK); return 0; } // the arena is too small: the error
    CHECK(slice == n || (slice < n && slice % RR_BLOCK == 0));
    CHECK(2 * slice <= room - keep || slice == n); // a slice's children fit behind the level, with room left for the levels below
    if (slice == n) CHECK(2 * n <= room - keep);
    return 0;
}

// The shadow-queue geometry of one shade chunk of `len` rays (plan_shade_chunk: what k_shade writes by and k_trace_shadow reads by) against
// the allocations the plans ask for: the frame's queue p.sq_need with its sq_need / 64 + 1 validity words (rr_api_frame.h grow_ray_queues)
// and, for a chunk that is a stage of level 1, a stage buffer.  `checked` counts the cases.
static int check_shade_chunk(const FramePlanInputs& in, const FramePlan& p, uint64_t len, uint64_t* checked) {
    const uint32_t L = in.n_enabled_lights;
    for (const bool fixed : {false, true}) {
        const uint64_t c0 = 12345 * RR_BLOCK; // (a chunk anywhere in its level: only the length counts)
        const ShadeChunk g = plan_shade_chunk(c0, c0 + len, L, fixed);
        CHECK(g.fixed == fixed && g.groups == (len + RR_BLOCK - 1) / RR_BLOCK && g.groups * RR_BLOCK >= len);
        CHECK(g.sq_cap == (fixed ? g.groups * RR_BLOCK : 0) && g.sq_packets * RR_WAVE == L * g.sq_cap);
        CHECK(g.shadow_wg * RR_BLOCK >= (fixed ? L * g.sq_cap : len * L) && g.shadow_wg <= (fixed ? L * g.sq_cap : len * L) / RR_BLOCK + 1);
        CHECK(g.segcap <= 0xffffffffull && L * g.sq_cap <= 0xffffffffull); // the kernels' arguments and slot indices are 32-bit
        CHECK(RR_SQ_SHARDS * g.segcap <= p.sq_need);                       // every shard's share of the dense queue lies inside it
        CHECK(RR_SQ_SHARDS * g.segcap >= len * std::max(L, 1u));           // ... and the shards together hold every ray the chunk can write
        if (len % ((uint64_t)RR_BLOCK * RR_SQ_SHARDS) == 0) CHECK(RR_SQ_SHARDS * g.segcap == len * std::max(L, 1u)); // whole rounds: equal shares
        if (fixed && L >= 1 && L <= 32 && len <= p.B) {                    // level 1 with fixed slots (RR_FIXED_SLOT_LIGHTS, rr_kernels.hip)
            CHECK(L * g.sq_cap <= p.sq_need);
            CHECK(g.sq_packets <= p.sq_need / RR_WAVE + 1);
        }
    }
    ++*checked;
    return 0;
}

// ... and every stage of level 1 in stages (plan_level1_stages, as rr_api_frame.h asks for it: the batch's B hits): L x sq_cap slots fit a buffer
static int check_stage_chunks(const FramePlanInputs& in, const FramePlan& p) {
    const uint32_t L = in.n_enabled_lights;
    if (L < 1 || L > 32) return 0;
    for (const uint32_t n_buf : {2u, 3u}) {
        const Level1Stages sp = plan_level1_stages({p.B, L, in.shade_chunk_rays, 20ull << 20, n_buf});
        for (uint32_t k = 0; k < sp.n_stages; k++) {
            const uint64_t c0 = sp.begin_of(k), c1 = std::min<uint64_t>(c0 + sp.stage, p.B);
            const ShadeChunk g = plan_shade_chunk(c0, c1, L, true);
            CHECK(L * g.sq_cap <= sp.buf_rays && g.sq_packets <= sp.buf_rays / RR_WAVE && g.segcap <= 0xffffffffull);
            if (k > 2 && k + 3 < sp.n_stages) k = sp.n_stages - 3; // (the middle of a long level is all alike)
        }
    }
    return 0;
}

int main() {
    // the geometry of a shade chunk by hand: 257 rays are 2 groups, so 512 fixed slots per light; a shard holds ceil(2 / 32) groups x 3 lights
    {
        const ShadeChunk g = plan_shade_chunk(1000, 1257, 3, true), d = plan_shade_chunk(1000, 1257, 3, false), none = plan_shade_chunk(0, 65536, 0, true);
        CHECK(g.groups == 2 && g.sq_cap == 512 && g.segcap == 768 && g.sq_packets == 24 && g.shadow_wg == 6);
        CHECK(d.groups == 2 && d.sq_cap == 0 && d.segcap == 768 && d.sq_packets == 0 && d.shadow_wg == 4); // 771 rays at most: 4 workgroups
        CHECK(none.groups == 256 && none.sq_cap == 65536 && none.segcap == 2048 && none.sq_packets == 0 && none.shadow_wg == 0); // no light: nothing to trace
        CHECK(shade_chunk(1, 0) == 64ull << 20 && shade_chunk(1, 1) == 65536 && shade_chunk(1, 100000) == 100000 && shade_chunk(40, 0) == 8945664);
    }
    // ... and over a sweep of frames, against what their plans allocate
    {
        uint64_t checked = 0;
        for (uint32_t npix : {1u, 64u, 9216u, 18240u, 921600u})
            for (uint32_t spp : {1u, 2u, 8u, 16u, 128u})
                for (uint32_t L : {0u, 1u, 2u, 32u, 33u, 300u})
                    for (uint64_t chunk_rays : {0ull, 1ull, 65536ull, 100000ull, 1ull << 22})
                        for (uint64_t budget : {150000ull * 128, 1ull << 30, 1ull << 36})
                            for (uint32_t R : {0u, 4u, 15u}) {
                                const FramePlanInputs in{npix, spp, R, budget, 0, 0, 2, L, chunk_rays};
                                const FramePlan p = plan_frame(in);
                                const uint64_t longest = std::min<uint64_t>(p.chunk, std::max<uint64_t>(p.M, p.B)); // no level holds more rays
                                for (uint64_t len : {(uint64_t)1, (uint64_t)255, (uint64_t)256, (uint64_t)257, (uint64_t)8191, (uint64_t)8193, longest})
                                    if (len <= longest && check_shade_chunk(in, p, len, &checked)) {
                                        std::printf("  npix %u spp %u lights %u chunk %llu budget %llu R %u len %llu\n", npix, spp, L, (unsigned long long)chunk_rays,
                                                    (unsigned long long)budget, R, (unsigned long long)len);
                                        return 1;
                                    }
                                if (check_stage_chunks(in, p)) return 1;
                            }
        CHECK(checked == 44190); // (the sweep ran: 47 250 combinations, less the lengths no level of their frame can hold)
    }
    for (const Case& c : k_cases) {
        const FramePlan p = plan_frame(c.in);
        if (p.B != c.B || p.G != c.G || p.M != c.M || p.chunk != c.chunk || p.sq_need != c.sq_need) {
            std::printf("FAILED plan %s: B %llu G %u M %llu chunk %llu sq_need %llu\n", c.name, (unsigned long long)p.B, p.G, (unsigned long long)p.M,
                        (unsigned long long)p.chunk, (unsigned long long)p.sq_need);
            return 1;
        }
        if (check_invariants(c.in)) { std::printf("  in case %s\n", c.name); return 1; }
    }
    // level slices by hand: the arena of the "queue budget 1 B" plan (11776 rays, R = 6)
    CHECK(level_slice(11776, 0, 4096, 1, 6) == 4096);   // 2 x 4096 children fit in 11776 - 5 x 512
    CHECK(level_slice(11776, 0, 8192, 1, 6) == 4608);   // they do not: (11776 - 2560) / 2, whole workgroups
    CHECK(level_slice(11776, 11000, 16, 2, 6) == 0);    // 776 rays of room < 4 x 512 kept + 512: the arena is too small
    CHECK(level_slice(11776, 11000, 16, 7, 6) == 16);   // the deepest level spawns nothing
    CHECK(level_slice(11776, 11000, 1000, 6, 6) == 256); // R - d = 0: the children of one workgroup fit in 776
    // invariants over a sweep
    const uint32_t npixs[] = {1, 7, 64, 100, 4096, 12291, 57600, P720};
    const uint32_t spps[] = {1, 3, 6, 16, 96, 128, 1024};
    const uint64_t budgets[] = {1, 1ull << 20, 1ull << 27, 1ull << 32, GB64};
    const uint32_t groups[] = {0, 1, 4, 64};
    const uint32_t passes[] = {0, 2, 16};
    for (uint32_t npix : npixs)
        for (uint32_t spp : spps)
            for (uint64_t budget : budgets)
                for (uint32_t g : groups)
                    for (uint32_t mp : passes)
                        for (uint32_t R : {0u, 6u, 16u}) {
                            const FramePlanInputs in{npix, spp, R, budget, g, mp, (npix & 1) ? 128u : 2u, npix % 3 ? 1u : 40u, spp == 3 ? 70000ull : 0ull};
                            if (check_invariants(in)) {
                                std::printf("  npix %u spp %u R %u budget %llu group %u passes %u\n", npix, spp, R, (unsigned long long)budget, g, mp);
                                return 1;
                            }
                            const FramePlan p = plan_frame(in);
                            for (uint32_t d = 1; d <= R + 1; d++)
                                for (uint64_t n : {(uint64_t)1, p.B / 3 + 1, p.B, 2 * p.B})
                                    for (uint64_t cb : {(uint64_t)0, p.M / 2, p.M - 1})
                                        if (check_level_slice(p.M, cb, n, d, R)) return 1;
                        }
    std::printf("frame plan test OK\n");
    return 0;
}
