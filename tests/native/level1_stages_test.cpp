// Host-only test of plan_level1_stages in rustray_amd/csrc/rr_frame_plan.h (built with g++ -fsanitize=address,undefined by
// tests/test_level1_stages.py): how level 1's hits are cut into stages and shadow-queue buffers for the two-stream path, against a
// table of expected plans, and the invariants the frame driver relies on over a sweep.
#include "../../rustray_amd/csrc/rr_frame_plan.h"

#include <cstdio>

#define CHECK(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

static const uint64_t AUTO = 20ull << 20; // RR_L1_STAGE_RAYS as it ships (rr_kernels.hip)

struct Case { const char* name; Level1StageInputs in; uint64_t stage; uint32_t n_stages, n_buf; uint64_t buf_rays, off1, off2, voff1, voff2, sq_need, valid_need; };

static const Case k_cases[] = {
    // name                          n          lights chunk  auto  bufs   stage    stages bufs buf_rays   off1       off2    voff1   voff2 sq_need    valid_need
    {"contract 1280x720 128 spp",   {117964800, 1,     0,     AUTO, 2},    19660800, 6,    2,   20971520,  20971520,  0,      327680, 0,    41943040,  655360},
    {"contract, 3 buffers",         {117964800, 1,     0,     AUTO, 3},    19660800, 6,    3,   20971520,  20971520,  41943040, 327680, 655360, 62914560, 983040},
    {"65536-ray chunks, 2 lights",  {291840,    2,     65536, AUTO, 3},    65536,   5,     3,   131072,    131072,    262144, 2048,   4096, 393216,    6144},
    {"65536-ray chunks, 1 light",   {291840,    1,     65536, AUTO, 2},    65536,   5,     2,   65536,     65536,     0,      1024,   0,    131072,    2048},
    {"32 lights",                   {117964800, 32,    0,     AUTO, 2},    5365760, 22,    2,   178782208, 178782208, 0,      2793472, 0,   357564416, 5586944},
    {"one ray below two stages",    {65535,     1,     65536, AUTO, 2},    65536,   1,     2,   65536,     65536,     0,      1024,   0,    0,         0},
    {"exactly one stage",           {65536,     1,     65536, AUTO, 2},    65536,   1,     2,   65536,     65536,     0,      1024,   0,    0,         0},
    {"one ray above one stage",     {65537,     1,     65536, AUTO, 2},    65536,   2,     2,   65536,     65536,     0,      1024,   0,    131072,    2048},
    {"n no multiple of the stage",  {200000,    1,     65536, AUTO, 2},    65536,   4,     2,   65536,     65536,     0,      1024,   0,    131072,    2048},
    {"chunk below the floor",       {200000,    1,     1,     AUTO, 2},    65536,   4,     2,   65536,     65536,     0,      1024,   0,    131072,    2048},
    {"chunk no multiple of 8192",   {300000,    1,     100000, AUTO, 2},   98304,   4,     2,   98304,     98304,     0,      1536,   0,    196608,    3072},
    {"0 lights count as one",       {200000,    0,     65536, AUTO, 2},    65536,   4,     2,   65536,     65536,     0,      1024,   0,    131072,    2048},
};

static int check_invariants(const Level1StageInputs& in) {
    const Level1Stages p = plan_level1_stages(in);
    const uint64_t L = std::max<uint32_t>(in.n_enabled_lights, 1u);
    CHECK(p.stage >= 65536 && p.stage % ((uint64_t)RR_BLOCK * RR_SQ_SHARDS) == 0);
    CHECK(p.stage <= std::max<uint64_t>(65536, in.shade_chunk_rays ? in.shade_chunk_rays : in.auto_stage)); // never above the chunk asked for
    CHECK(p.n_buf == 2 || p.n_buf == 3);
    CHECK(p.stage <= p.stage_cap && p.stage_cap % ((uint64_t)RR_BLOCK * RR_SQ_SHARDS) == 0);
    CHECK(p.buf_rays == L * p.stage_cap);
    CHECK(p.stage_cap == plan_level1_stages({1, in.n_enabled_lights, in.shade_chunk_rays, in.auto_stage, in.n_buf}).stage_cap); // the layout does not depend on n
    if (in.shade_chunk_rays) CHECK(p.stage == p.stage_cap); // an explicit chunk IS the stage
    else if (p.n_stages >= 2) CHECK(p.n_stages == (in.n + p.stage_cap - 1) / p.stage_cap && p.stage * p.n_stages - in.n < p.n_stages * (uint64_t)RR_BLOCK * RR_SQ_SHARDS); // the fewest stages, equal to within a unit
    CHECK(p.overlapped() == (p.n_stages >= 2) && p.overlapped() == (in.n > p.stage_cap)); // fewer than 2 stages = the serial loop
    // stages tile [0, n) exactly and in order, none larger than the stage; stage k uses buffer k % n_buf and fits it with every light
    uint64_t at = 0;
    for (uint32_t k = 0; k < p.n_stages; k++) {
        CHECK(p.begin_of(k) == at);
        const uint64_t end = std::min<uint64_t>(at + p.stage, in.n);
        CHECK(end > at && end - at <= p.stage);
        const ShadeChunk g = plan_shade_chunk(at, end, (uint32_t)L, true); // what k_shade and k_trace_shadow are given for the stage
        CHECK(g.sq_cap >= end - at && L * g.sq_cap <= p.buf_rays && g.sq_packets == L * (g.sq_cap / RR_WAVE) && g.sq_packets <= p.buf_rays / RR_WAVE);
        CHECK(p.buffer_of(k) == k % p.n_buf);
        at = end;
        if (k > 4 && k + 4 < p.n_stages) { k = p.n_stages - 4; at = p.begin_of(k + 1); } // (the middle of a long level is all alike)
    }
    CHECK(at == in.n);
    if (!p.overlapped()) { CHECK(p.sq_need == 0 && p.valid_need == 0); return 0; }
    // buffers, and their validity words, are pairwise disjoint and inside the allocation the plan asks for
    for (uint32_t a = 0; a < p.n_buf; a++) {
        CHECK(p.ray_offset[a] + p.buf_rays <= p.sq_need);
        CHECK(p.valid_offset[a] + p.buf_rays / RR_WAVE <= p.valid_need);
        for (uint32_t b = a + 1; b < p.n_buf; b++) {
            CHECK(p.ray_offset[a] + p.buf_rays <= p.ray_offset[b] || p.ray_offset[b] + p.buf_rays <= p.ray_offset[a]);
            CHECK(p.valid_offset[a] + p.buf_rays / RR_WAVE <= p.valid_offset[b] || p.valid_offset[b] + p.buf_rays / RR_WAVE <= p.valid_offset[a]);
        }
    }
    CHECK(p.sq_need * 48ull <= (16ull << 30) || p.stage == 65536); // 16 GB of shadow rays at most, down to the smallest stage
    CHECK(p.sq_need <= 0xffffffffull * 4); // (ray indices inside one buffer are 32-bit: L * stage below 2^32)
    CHECK(p.buf_rays <= 0xffffffffull);
    return 0;
}

int main() {
    for (const Case& c : k_cases) {
        const Level1Stages p = plan_level1_stages(c.in);
        if (p.stage != c.stage || p.n_stages != c.n_stages || p.n_buf != c.n_buf || p.buf_rays != c.buf_rays || p.ray_offset[0] != 0 || p.valid_offset[0] != 0 ||
            p.ray_offset[1] != c.off1 || p.ray_offset[2] != c.off2 || p.valid_offset[1] != c.voff1 || p.valid_offset[2] != c.voff2 || p.sq_need != c.sq_need ||
            p.valid_need != c.valid_need) {
            std::printf("FAILED plan %s: stage %llu stages %u bufs %u buf_rays %llu off %llu %llu voff %llu %llu sq_need %llu valid_need %llu\n", c.name,
                        (unsigned long long)p.stage, p.n_stages, p.n_buf, (unsigned long long)p.buf_rays, (unsigned long long)p.ray_offset[1], (unsigned long long)p.ray_offset[2],
                        (unsigned long long)p.valid_offset[1], (unsigned long long)p.valid_offset[2], (unsigned long long)p.sq_need, (unsigned long long)p.valid_need);
            return 1;
        }
        if (check_invariants(c.in)) { std::printf("  in case %s\n", c.name); return 1; }
    }
    // the layout of the buffers does not depend on n: the allocation made for a frame's largest batch serves every smaller one
    {
        const Level1Stages a = plan_level1_stages({117964800, 3, 0, AUTO, 3}), b = plan_level1_stages({50000000, 3, 0, AUTO, 3});
        for (int k = 0; k < 3; k++) CHECK(a.ray_offset[k] == b.ray_offset[k] && a.valid_offset[k] == b.valid_offset[k]);
        CHECK(a.stage_cap == b.stage_cap && a.buf_rays == b.buf_rays && b.sq_need == a.sq_need);
    }
    // invariants over a sweep: n in [1, 2^31 - 256] (every size around a stage boundary and a sample in between), lights, chunks, buffers
    const uint64_t n_max = RR_LEVEL_MAX;
    const uint64_t chunks[] = {0, 1, 65536, 65537, 100000, 1ull << 20, 4ull << 20, 16ull << 20, 64ull << 20, 1ull << 33};
    const uint64_t autos[] = {4ull << 20, 8ull << 20, 16ull << 20};
    for (uint32_t L = 1; L <= 32; L++)
        for (uint64_t chunk : chunks)
            for (uint64_t au : autos)
                for (uint32_t nb : {2u, 3u}) {
                    const uint64_t stage = plan_level1_stages({1, L, chunk, au, nb}).stage_cap;
                    uint64_t ns[40]; int m = 0;
                    for (uint64_t k : {1ull, 2ull, 3ull, 7ull}) for (int64_t dlt : {-1ll, 0ll, 1ll}) ns[m++] = k * stage + dlt;
                    ns[m++] = 1; ns[m++] = 255; ns[m++] = 256; ns[m++] = 65535; ns[m++] = 291840; ns[m++] = 117964800; ns[m++] = n_max - 1; ns[m++] = n_max;
                    for (uint64_t x = 12345, i = 0; i < 12; i++) { x = x * 6364136223846793005ull + 1442695040888963407ull; ns[m++] = 1 + (x >> 33) % n_max; }
                    for (int i = 0; i < m; i++) {
                        if (ns[i] < 1 || ns[i] > n_max) continue;
                        if (check_invariants({ns[i], L, chunk, au, nb})) {
                            std::printf("  n %llu lights %u chunk %llu auto %llu bufs %u\n", (unsigned long long)ns[i], L, (unsigned long long)chunk, (unsigned long long)au, nb);
                            return 1;
                        }
                    }
                }
    std::printf("level-1 stages test OK\n");
    return 0;
}
