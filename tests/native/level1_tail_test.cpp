// Host-only test of level1_tail and chunk_clear_of_tail in rustray_amd/csrc/rr_frame_plan.h (built with g++ -fsanitize=address,undefined by
// tests/test_level1_tail.py): which rays of the shadow-queue allocation the last two shadow stages of a staged level 1 still read when the
// frame's stream goes on, which chunks of the serial loop may be shaded beside them, and which earlier stage's shadow launch such a chunk
// has to wait for instead, because it read the buffer the chunk writes.
#include "../../rustray_amd/csrc/rr_frame_plan.h"

#include <cstdio>

#define CHECK(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

static const uint64_t AUTO = 20ull << 20; // RR_L1_STAGE_RAYS as it ships (rr_kernels.hip)

// the rays a chunk of the serial loop may write, from ray 0 of the allocation on: every shard of the dense queue, or every light's fixed slots
static uint64_t chunk_extent(const ShadeChunk& g, uint32_t lights) { return g.fixed ? g.sq_cap * lights : g.segcap * RR_SQ_SHARDS; }

static int check(const Level1StageInputs& in, uint64_t m) {
    const Level1Stages sp = plan_level1_stages(in);
    if (!sp.overlapped()) return 0; // the serial loop: nothing is ever pending
    const uint32_t L = std::max<uint32_t>(in.n_enabled_lights, 1u);
    const Level1Tail t = level1_tail(sp);
    // the tail covers the buffers of the last two stages entirely and lies inside the allocation
    for (uint32_t k = sp.n_stages - 2; k < sp.n_stages; k++) {
        const uint64_t at = sp.ray_offset[sp.buffer_of(k)];
        CHECK(t.lo <= at && at + sp.buf_rays <= t.hi);
    }
    CHECK(t.lo < t.hi && t.hi <= sp.sq_need);
    // the buffer at rest is in front of the tail exactly where there are three buffers and a multiple of three stages
    CHECK((t.lo > 0) == (sp.n_buf == 3 && sp.n_stages % 3 == 0));
    if (t.lo > 0) CHECK(t.lo == sp.buf_rays && t.hi == 3 * sp.buf_rays);
    // ORDER.  [0, lo) is not at rest by itself: shadow launches of earlier stages read it, and a shade launch of the level waits for shadow
    // k - n_buf only.  rest_stage is the LAST stage whose buffer lies in [0, lo): every stage that used such a buffer is rest_stage or an
    // earlier one (all of them on the second stream, in order, so a wait for rest_stage's launch covers them), the event of its buffer is
    // not recorded again by a later stage, and no stage of the level was shaded behind a wait for it (the wait is not redundant).
    if (t.lo == 0) CHECK(t.rest_stage == -1 && t.rest_buffer == -1);
    else {
        CHECK(t.rest_stage == (int32_t)sp.n_stages - 3 && t.rest_stage >= 0 && t.rest_buffer == (int32_t)sp.buffer_of((uint32_t)t.rest_stage));
        CHECK(sp.ray_offset[t.rest_buffer] + sp.buf_rays <= t.lo);
        for (uint32_t k = 0; k < sp.n_stages; k++) {
            const bool below = sp.ray_offset[sp.buffer_of(k)] < t.lo;
            if (below) CHECK((int32_t)k <= t.rest_stage && (int32_t)sp.buffer_of(k) == t.rest_buffer); // one buffer in front of the tail, last used by rest_stage
            if ((int32_t)k > t.rest_stage) CHECK((int32_t)sp.buffer_of(k) != t.rest_buffer);           // its event still is rest_stage's
            if (k >= sp.n_buf) CHECK((int32_t)(k - sp.n_buf) < t.rest_stage);                          // shade k waited for an earlier launch only
        }
        CHECK(t.rest_stage + 1 < (int32_t)sp.n_stages - 1); // rest_stage's launch is on the second stream (only the last stage's is on the third)
    }
    // a chunk that is let through writes no ray of the tail; one with fixed slots never is (it writes validity words from word 0 on)
    const ShadeChunk dense = plan_shade_chunk(0, m, in.n_enabled_lights, false), fixed = plan_shade_chunk(0, m, in.n_enabled_lights, true);
    CHECK(!chunk_clear_of_tail(fixed, t));
    if (chunk_clear_of_tail(dense, t)) CHECK(chunk_extent(dense, L) <= t.lo && m * L <= chunk_extent(dense, L));
    else CHECK(t.lo == 0 || chunk_extent(dense, L) > t.lo);
    return 0;
}

int main() {
    // the contract frame: six stages in three buffers of 20 Mi rays, buffers 1 and 2 in use at the end; level 2's 4.47 M rays fit into buffer 0
    {
        const Level1Stages sp = plan_level1_stages({117964800, 1, 0, AUTO, 3});
        const Level1Tail t = level1_tail(sp);
        CHECK(sp.n_stages == 6 && t.lo == 20971520 && t.hi == 62914560);
        CHECK(t.rest_stage == 3 && t.rest_buffer == 0); // stage 3's shadow launch read buffer 0 last, and shade 5 waited for shadow 2 only
        CHECK(chunk_clear_of_tail(plan_shade_chunk(0, 4468685, 1, false), t));
        CHECK(chunk_clear_of_tail(plan_shade_chunk(0, 20971520, 1, false), t));    // exactly one buffer
        CHECK(!chunk_clear_of_tail(plan_shade_chunk(0, 20971521, 1, false), t));   // one more workgroup iteration in every shard
        CHECK(!chunk_clear_of_tail(plan_shade_chunk(0, 4468685, 1, true), t));
        const Level1Tail two = level1_tail(plan_level1_stages({117964800, 1, 0, AUTO, 2})); // two buffers: both in use
        CHECK(two.lo == 0 && two.hi == 41943040 && two.rest_stage == -1 && !chunk_clear_of_tail(plan_shade_chunk(0, 256, 1, false), two));
    }
    // 153 600 hits in 65 536-ray stages with two lights (tests/test_gpu_tail_overlap.py): three stages, buffer 0 at rest, 131 072 rays each
    {
        const Level1Tail t = level1_tail(plan_level1_stages({153600, 2, 65536, AUTO, 3}));
        CHECK(t.lo == 131072 && t.hi == 393216);
        CHECK(t.rest_stage == 0 && t.rest_buffer == 0); // three stages: no shade launch waits for any shadow launch, stage 0's read buffer 0
        CHECK(chunk_clear_of_tail(plan_shade_chunk(0, 47143, 2, false), t));    // level 4 of that frame's scene
        CHECK(chunk_clear_of_tail(plan_shade_chunk(0, 65536, 2, false), t));    // a full chunk of level 2: 65 536 rays per light
        CHECK(!chunk_clear_of_tail(plan_shade_chunk(0, 65537, 2, false), t));
        const Level1Tail t2 = level1_tail(plan_level1_stages({76800, 2, 65536, AUTO, 3})); // one of two batches: two stages, buffers 0 and 1
        CHECK(t2.lo == 0 && t2.hi == 262144 && !chunk_clear_of_tail(plan_shade_chunk(0, 256, 2, false), t2));
    }
    // a sweep: level sizes around the stage boundaries, lights, chunks, buffers, and chunks of the serial loop from one ray to a whole stage and beyond
    for (uint32_t L : {1u, 2u, 3u, 7u, 32u})
        for (uint64_t chunk : {0ull, 65536ull, 100000ull, 1ull << 20})
            for (uint32_t nb : {2u, 3u}) {
                const uint64_t stage = plan_level1_stages({1, L, chunk, AUTO, nb}).stage_cap;
                for (uint64_t k = 1; k <= 8; k++)
                    for (int64_t dlt : {-1ll, 0ll, 1ll})
                        for (uint64_t m : {(uint64_t)1, (uint64_t)255, (uint64_t)256, (uint64_t)2049, stage / 3, stage - 8192, stage - 1, stage, stage + 1, 4 * stage}) {
                            if (check({k * stage + dlt, L, chunk, AUTO, nb}, m)) {
                                std::printf("  n %llu lights %u chunk %llu bufs %u m %llu\n", (unsigned long long)(k * stage + dlt), L, (unsigned long long)chunk, nb, (unsigned long long)m);
                                return 1;
                            }
                        }
            }
    std::printf("level-1 tail test OK\n");
    return 0;
}
