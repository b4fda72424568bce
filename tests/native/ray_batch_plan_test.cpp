// Host-only test of plan_ray_batches (rustray_amd/csrc/rr_frame_plan.h), built with g++ -fsanitize=address,undefined by
// tests/test_ray_batch_plan.py: how rr_shade_rays cuts the caller's rays into device batches and sizes the ray arena for them.
#include "../../rustray_amd/csrc/rr_frame_plan.h"

#include <cstdio>

#define CHECK(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s (n %llu R %u budget %llu lights %u chunk %llu)\n", __FILE__, __LINE__, #c, \
    (unsigned long long)n, R, (unsigned long long)budget, L, (unsigned long long)chunk_in); return 1; } } while (0)

static int check(uint64_t n, uint32_t R, uint64_t budget, uint32_t L, uint64_t chunk_in) {
    const FramePlan p = plan_ray_batches(n, R, budget, L, chunk_in);
    const uint64_t slack = 2ull * RR_BLOCK * (R + 1);
    CHECK(p.total_primary == n && p.G == 1);
    CHECK(p.B >= 1 && p.B <= n && p.B <= RR_LEVEL_MAX);
    // the batches of rr_shade_rays' loop partition [0, n): consecutive, non-empty, none beyond B, equal but for the last
    const uint64_t batches = (n + p.B - 1) / p.B;
    if (batches <= (1u << 20)) { // (walked where that stays quick; beyond, the arithmetic below says the same)
        uint64_t covered = 0, walked = 0;
        for (uint64_t first = 0; first < n; first += p.B, walked++) {
            const uint64_t nb = std::min<uint64_t>(p.B, n - first);
            CHECK(first == covered && nb >= 1 && nb <= RR_LEVEL_MAX);
            CHECK(nb == p.B || first + nb == n);
            covered += nb;
        }
        CHECK(covered == n && walked == batches);
    }
    CHECK(p.B * batches >= n && p.B * (batches - 1) < n);
    CHECK(p.B - (n - (batches - 1) * p.B) < batches); // equal batches: the last one is short by less than one ray per batch
    // the arena: the batch's own records, two children per ray, the slack of the spawning levels; inside 32-bit ray indices
    CHECK(p.M >= 3 * p.B + slack && p.M <= RR_LEVEL_MAX);
    CHECK(level_slice(p.M, p.B, p.B, 1, R) == p.B);           // the children of a whole seeded level fit behind it
    // within the budget, except at the 4096-ray floor
    if (budget >= 56ull * (3ull * 4096 + slack)) CHECK(56ull * p.M <= budget);
    else CHECK(p.B <= 4096);
    // the shade chunk and the dense shadow queue, as plan_frame sizes them
    CHECK(p.chunk >= 65536 && (chunk_in < 65536 || p.chunk <= chunk_in));
    CHECK(p.sq_need >= (std::min<uint64_t>(p.chunk, p.M) + (uint64_t)RR_BLOCK * RR_SQ_SHARDS) * std::max<uint32_t>(L, 1u));
    CHECK(48ull * p.sq_need <= (17ull << 30) || L > 1024);
    return 0;
}

int main() {
    const uint64_t counts[] = {1, 63, 4096, 4097, 5700, 291840, (1ull << 31) + 5, 0x7fffff00ull * 32766ull};
    const uint64_t budgets[] = {0, 1, 4096, 1ull << 20, 1ull << 24, 1ull << 28, 1ull << 32, 64ull << 30};
    const uint32_t recursion[] = {0, 4, 30};
    const uint32_t lights[] = {0, 1, 4, 40};
    const uint64_t chunks[] = {0, 1, 65536, 100000};
    for (uint64_t n : counts)
        for (uint64_t b : budgets)
            for (uint32_t R : recursion)
                for (uint32_t L : lights)
                    for (uint64_t c : chunks)
                        if (check(n, R, b, L, c)) return 1;
    // a tiny budget cuts even a small call into several batches (what the batching test on the GPU relies on)
    const uint64_t tiny_counts[] = {4097ull * 3, 291840ull, (1ull << 31) + 5};
    for (uint64_t n : tiny_counts)
        for (uint32_t R : recursion) {
            const FramePlan p = plan_ray_batches(n, R, 1, 4, 0);
            if (p.B != (n + ((n + 4095) / 4096) - 1) / ((n + 4095) / 4096) || (n + p.B - 1) / p.B < 3) { std::printf("FAILED: tiny budget, n %llu: B %llu\n", (unsigned long long)n, (unsigned long long)p.B); return 1; }
        }
    // expected plans, worked out by hand: 5700 rays fit one batch under any budget at or above the floor; 4097 rays under a tiny budget are two batches
    { const FramePlan p = plan_ray_batches(5700, 4, 64ull << 30, 4, 0); if (p.B != 5700 || p.M != 3 * 5700 + 2560 || p.chunk != (64ull << 20) || p.sq_need != (17100 + 2560 + 8192) * 4ull) { std::printf("FAILED: 5700-ray plan\n"); return 1; } }
    { const FramePlan p = plan_ray_batches(4097, 0, 1, 1, 0); if (p.B != 2049 || p.M != 3 * 2049 + 512) { std::printf("FAILED: 4097-ray plan\n"); return 1; } }
    { const FramePlan p = plan_ray_batches(291840, 4, 56ull * (3 * 65536 + 2560), 4, 65536); if (p.B != 58368 || p.chunk != 65536) { std::printf("FAILED: 291840-ray plan: B %llu\n", (unsigned long long)p.B); return 1; } }
    std::printf("ray batch plan test OK\n");
    return 0;
}
