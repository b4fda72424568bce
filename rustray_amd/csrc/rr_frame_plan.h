// rr_frame_plan.h — how a frame is cut into device batches and how its ray memory is sized: plain host arithmetic,
// no HIP calls.  rr_api_frame.h runs it: render_region_locked (plan_frame), run_level (level_slice, plan_level1_stages and, for the
// serial loop and the staged path alike, plan_shade_chunk); rr_api_query.h rr_shade_rays (plan_ray_batches).
// tests/native/frame_plan_test.cpp and level1_stages_test.cpp check it on the CPU.
//
// All live depth levels of a batch sit in ONE arena of ray records (56 B each), level d + 1 stacked behind level d.
// A level of n rays spawns at most 2 n children; if they fit behind it the level is shaded in one go, otherwise in
// slices whose children fit, each slice's subtree finished (depth first) before the next slice starts.  So capacity
// never limits correctness, only how large the launches can be -- and launch size matters: the persistent trace
// kernels lose 8-15 % to ramp-up and tail per launch at 12 M rays (reserving the worst case 2^(d-1) growth per
// level, as the first version did, capped batches there).
#pragma once
#include "rr_device.h"

#include <algorithm>
#include <cstdint>

struct FramePlanInputs {
    uint32_t npix;             // accumulator slots of the region (>= 1)
    uint32_t samples;          // per pixel (>= 1)
    uint32_t max_recursion;    // R
    uint64_t queue_budget;     // bytes for level 1's hit records and the arena (rr_api_frame.h queue_budget)
    uint32_t sample_group;     // rr_tuning::sample_group: 0 = automatic
    uint32_t min_passes;       // progressive passes asked for; 0 without a pass hook
    uint32_t arena_factor;     // arena rays per primary ray after a frame that had to slice levels
    uint32_t n_enabled_lights;
    uint64_t shade_chunk_rays; // rr_tuning::shade_chunk_rays: 0 = 64 Mi
};

struct FramePlan {
    uint64_t total_primary; // npix * samples
    uint64_t B;             // primary rays per batch (every batch but the last holds exactly B)
    uint32_t G;             // samples of one pixel per 64-ray packet
    uint64_t M;             // arena rays (levels 2 and deeper)
    uint64_t chunk;         // rays per shade launch
    uint64_t sq_need;       // shadow queue rays
};

static const uint64_t RR_LEVEL_MAX = 0x7fffff00ull; // ray indices are 32-bit

// Rays per shade launch: rr_tuning::shade_chunk_rays, at least 65536 (0 = 64 Mi).  The shadow queue holds one 48-B ray per hit of the
// chunk and ENABLED light: with many lights the chunk shrinks so that the queue stays within 16 GB -- the reference has no limit on
// lights, src/raytracing.rs:814.
inline uint64_t shade_chunk(uint32_t n_enabled_lights, uint64_t shade_chunk_rays) {
    const uint64_t by_lights = std::max<uint64_t>(65536, ((16ull << 30) / (48ull * std::max<uint32_t>(n_enabled_lights, 1u))) / (RR_BLOCK * RR_SQ_SHARDS) * (RR_BLOCK * RR_SQ_SHARDS));
    return std::min<uint64_t>(shade_chunk_rays ? std::max<uint64_t>(65536, shade_chunk_rays) : (64ull << 20), by_lights);
}

inline FramePlan plan_frame(const FramePlanInputs& in) {
    const uint32_t npix = in.npix, R = in.max_recursion, L = in.n_enabled_lights;
    const uint64_t budget = in.queue_budget;
    const uint64_t total_primary = (uint64_t)npix * in.samples;
    // Level 1 (the primary rays) needs only its 16-B hit records: the rays themselves are derived from their index
    // (primary_ray).  The arena holds the deeper levels; 2 arena rays per primary ray cover every level of a typical
    // frame at once (sponza_syn: all deeper levels together hold 4 % of the primaries), sliced when a scene branches more.
    const uint64_t per_primary = 16ull + 2ull * 56ull;
    uint64_t B = std::max<uint64_t>(budget / per_primary, 4096);
    B = std::min<uint64_t>(B, std::min<uint64_t>(total_primary, RR_LEVEL_MAX));
    if (in.min_passes > 1) B = std::min<uint64_t>(B, std::max<uint64_t>(npix, (total_primary + in.min_passes - 1) / in.min_passes));
    // equal batches (a frame that needs 1.2 batches would otherwise end with a small, poorly filled one)
    { const uint64_t nb = (total_primary + B - 1) / B; B = (total_primary + nb - 1) / nb; }
    if (B > npix) B = ((B + npix - 1) / npix) * npix; // whole sample slices when possible
    // Sample grouping: a packet of 64 primary rays = 64/G neighbouring pixels x G samples of each (primary_ray), so the
    // rays of a wave - and the shadow rays and children they spawn - start almost identical and their walks stay
    // together.  The largest group the sample count allows is best (closest-hit -30 % on sponza_syn at G = 64 against
    // one sample of 64 pixels), given that the wave merges its accumulator adds per pixel first (accum_merged): 64
    // lanes adding to one address otherwise cost more than the walks gain.  Needs whole groups per batch.
    uint32_t G = 1;
    {
        const uint32_t forced = in.sample_group; // 0 = automatic
        for (uint32_t g = forced ? forced : 64u; g >= 2; g >>= 1)
            if (g <= 64 && !(g & (g - 1)) && in.samples % g == 0 && npix % (RR_WAVE / g) == 0 && (uint64_t)npix * g <= B) { G = g; break; }
        if (forced && G != forced) G = 1;
    }
    if (G > 1) {
        // whole groups per batch, batches as equal as whole groups allow
        const uint64_t unit = (uint64_t)npix * G, units_max = B / unit, total_units = total_primary / unit;
        const uint64_t nb = (total_units + units_max - 1) / units_max;
        B = ((total_units + nb - 1) / nb) * unit;
    }
    B = std::min<uint64_t>(B, total_primary);
    // arena (levels 2 and deeper): 2 rays per primary ray, or 7 where that stays under 16 GB (a branching scene then fits
    // on its first frame too), or `arena_factor` after a frame that had to slice -- always within the budget
    const uint64_t after_hits = budget > 16ull * B ? (budget - 16ull * B) / 56ull : 0ull;
    const uint64_t roomy = std::min<uint64_t>(7 * B, (16ull << 30) / 56ull);
    const uint64_t want = std::max<uint64_t>(std::max<uint64_t>(2 * B, roomy), (uint64_t)in.arena_factor * B);
    const uint64_t M = std::min<uint64_t>(std::min<uint64_t>(want, std::max<uint64_t>(2 * B, after_hits)) + 2ull * RR_BLOCK * (R + 1), RR_LEVEL_MAX);
    const uint64_t chunk = shade_chunk(L, in.shade_chunk_rays);
    // level 1: fixed shadow slots, (enabled light, hit of the chunk), the chunk padded to whole workgroup iterations;
    // deeper levels: the dense sharded queue (a shard's static share of the chunk, one slack group per shard)
    const uint64_t sq_need = std::max<uint64_t>(1, (std::min<uint64_t>(chunk, std::max<uint64_t>(M, B)) + RR_BLOCK * RR_SQ_SHARDS) * std::max<uint32_t>(L, 1u));
    return FramePlan{total_primary, B, G, M, chunk, sq_need};
}

// ---- caller-supplied rays (rr_api_query.h rr_shade_rays) ----------------------------------------------------------------------
// The rays of such a call are depth level 1 as RECORDS: a batch of B rays sits at the front of the arena (56 B each, where a
// frame keeps 16-B hit records only), its children behind it.  2 arena rays per ray for the children, as plan_frame allows per
// primary ray, plus the slack every spawning level needs to make progress; level_slice covers a scene that branches more.
// B <= RR_LEVEL_MAX / 3, so that the children's room stays inside 32-bit ray indices; at least 4096 rays, as plan_frame.
// The batches are equal: batch k = rays [k * B, min((k + 1) * B, n_rays)), a result's rays cut anywhere (the accumulators are
// integers and live across the batches).  Returned as a FramePlan (total_primary = n_rays, G = 1): the level walk reads it.
inline FramePlan plan_ray_batches(uint64_t n_rays, uint32_t max_recursion, uint64_t budget, uint32_t n_enabled_lights, uint64_t shade_chunk_rays) {
    const uint64_t slack = 2ull * RR_BLOCK * (max_recursion + 1);
    const uint64_t per_ray = 3ull * 56ull;
    uint64_t B = std::max<uint64_t>(budget > 56ull * slack ? (budget - 56ull * slack) / per_ray : 0ull, 4096);
    B = std::min<uint64_t>(B, std::min<uint64_t>(std::max<uint64_t>(n_rays, 1), (RR_LEVEL_MAX - slack) / 3));
    { const uint64_t nb = (std::max<uint64_t>(n_rays, 1) + B - 1) / B; B = (std::max<uint64_t>(n_rays, 1) + nb - 1) / nb; }
    const uint64_t M = 3 * B + slack;
    const uint64_t chunk = shade_chunk(n_enabled_lights, shade_chunk_rays);
    // every level takes the dense sharded shadow queue (no fixed slots: the rays of a packet need not belong together)
    const uint64_t sq_need = std::max<uint64_t>(1, (std::min<uint64_t>(chunk, M) + RR_BLOCK * RR_SQ_SHARDS) * std::max<uint32_t>(n_enabled_lights, 1u));
    return FramePlan{n_rays, B, 1u, M, chunk, sq_need};
}

// ---- level 1 in stages (rr_api_frame.h run_level, the two-stream path) -------------------------------------------------------
// Level 1 of a scene with fixed shadow slots may be cut into STAGES of hits: k_shade<true> of stage k + 1 then runs on one
// stream while k_trace_shadow<true> of stage k runs on a second one.  Stage k writes its shadow rays into buffer
// k % n_buf of the shadow-queue allocation, so a buffer is rewritten only after the shadow launch that read it.
// A buffer holds the fixed slots of one whole stage: (enabled light, hit of the stage), with one validity word per 64 slots.
// With an explicit rr_tuning::shade_chunk_rays a stage is that chunk.  Otherwise the level is cut into the fewest EQUAL
// stages of at most `auto_stage` hits (a short last stage would shade beside a full stage of shadow rays and then leave
// them the GPU at the reduced grid).  The buffer layout depends on the largest stage allowed, the lights and n_buf alone,
// never on the number of hits: the allocation made for one batch of a frame serves every batch and every slice of it.
struct Level1StageInputs {
    uint64_t n;                // hits of the level (or of a slice of it): [0, n)
    uint32_t n_enabled_lights;
    uint64_t shade_chunk_rays; // rr_tuning::shade_chunk_rays: 0 = automatic
    uint64_t auto_stage;       // largest stage when automatic (RR_L1_STAGE_RAYS, rr_kernels.hip)
    uint32_t n_buf;            // shadow-queue buffers: 2 or 3 (RR_L1_BUFFERS)
};

struct Level1Stages {
    uint64_t stage;           // hits per stage, a multiple of RR_BLOCK * RR_SQ_SHARDS; the last stage may hold fewer
    uint64_t stage_cap;       // the largest stage these inputs allow for any n (>= stage): what a buffer is sized for
    uint32_t n_stages;        // ceil(n / stage); fewer than 2 = the serial loop
    uint32_t n_buf;           // 2 or 3
    uint64_t buf_rays;        // capacity of one buffer in shadow rays: lights * stage_cap
    uint64_t ray_offset[3];   // buffer b starts at this ray of the shadow-queue allocation
    uint64_t valid_offset[3]; // ... and at this word of sq_valid
    uint64_t sq_need;         // shadow-queue rays the buffers need together (0 when serial)
    uint64_t valid_need;      // sq_valid words they need together (0 when serial)
    bool overlapped() const { return n_stages >= 2; }
    uint32_t buffer_of(uint32_t k) const { return k % n_buf; }
    uint64_t begin_of(uint32_t k) const { return (uint64_t)k * stage; }
};

static const uint64_t RR_STAGE_UNIT = (uint64_t)RR_BLOCK * RR_SQ_SHARDS;

inline Level1Stages plan_level1_stages(const Level1StageInputs& in) {
    const uint64_t L = std::max<uint32_t>(in.n_enabled_lights, 1u);
    const uint32_t n_buf = in.n_buf >= 3 ? 3u : 2u;
    // all buffers together stay within 16 GB of 48-B rays, as plan_frame's chunk does with many lights
    const uint64_t by_lights = std::max<uint64_t>(65536, ((16ull << 30) / (48ull * L * n_buf)) / RR_STAGE_UNIT * RR_STAGE_UNIT);
    uint64_t stage = in.shade_chunk_rays ? in.shade_chunk_rays : in.auto_stage;
    stage = std::max<uint64_t>(65536, stage / RR_STAGE_UNIT * RR_STAGE_UNIT); // whole workgroup iterations of every shard
    stage = std::min<uint64_t>(stage, by_lights);
    Level1Stages p{};
    p.stage_cap = stage;
    if (!in.shade_chunk_rays && in.n > stage) { // automatic: equal stages
        const uint64_t n_st = (in.n + stage - 1) / stage;
        stage = std::max<uint64_t>(65536, ((in.n + n_st - 1) / n_st + RR_STAGE_UNIT - 1) / RR_STAGE_UNIT * RR_STAGE_UNIT); // (<= stage_cap, itself whole units)
    }
    p.stage = stage;
    p.n_stages = (uint32_t)((in.n + stage - 1) / stage);
    p.n_buf = n_buf;
    p.buf_rays = L * p.stage_cap;
    for (uint32_t b = 0; b < 3; b++) {
        p.ray_offset[b] = b < n_buf ? b * p.buf_rays : 0ull;
        p.valid_offset[b] = b < n_buf ? b * (p.buf_rays / RR_WAVE) : 0ull;
    }
    p.sq_need = p.overlapped() ? n_buf * p.buf_rays : 0ull;
    p.valid_need = p.overlapped() ? n_buf * (p.buf_rays / RR_WAVE) : 0ull;
    return p;
}

// ---- the shadow queue of one shade chunk (rr_api_frame.h: the serial loop of run_level and every stage of the staged path) ------
// Where k_shade writes the shadow rays of the hits [c0, c1) and how far k_trace_shadow reads: both launches of a chunk take these
// numbers, and nothing else computes them.  Level 1 with fixed slots: slot (light, hit of the chunk), the chunk padded to whole
// workgroup iterations, one validity word per 64 slots, walked as packets.  Otherwise the dense queue: a shard gets the 256-ray groups
// with (group % RR_SQ_SHARDS == shard), at most `lights` rays per hit.  64-bit, so that the launch sites can refuse what the kernels'
// 32-bit arguments cannot hold; what the allocations of plan_frame and plan_level1_stages must cover: tests/native/frame_plan_test.cpp.
struct ShadeChunk {
    bool fixed;
    uint64_t groups;     // 256-ray groups of the chunk: k_shade's workgroup iterations, dealt round-robin to the shards
    uint64_t sq_cap, sq_packets; // fixed slots per light (0 when dense), and the 64-slot packets of all lights together
    uint64_t segcap;     // rays a shard of the dense queue holds at most
    uint64_t shadow_wg;  // workgroups with one thread per shadow ray there can be, before the caller's cap
};

inline ShadeChunk plan_shade_chunk(uint64_t c0, uint64_t c1, uint32_t n_enabled_lights, bool fixed) {
    const uint64_t L = n_enabled_lights, groups = (c1 - c0 + RR_BLOCK - 1) / RR_BLOCK;
    const uint64_t sq_cap = fixed ? groups * RR_BLOCK : 0ull, sq_packets = (sq_cap / RR_WAVE) * L;
    const uint64_t segcap = ((groups + RR_SQ_SHARDS - 1) / RR_SQ_SHARDS) * RR_BLOCK * std::max<uint64_t>(L, 1);
    const uint64_t shadow_rays = fixed ? sq_packets * RR_WAVE : (c1 - c0) * L; // the most there can be
    return ShadeChunk{fixed, groups, sq_cap, sq_packets, segcap, (shadow_rays + RR_BLOCK - 1) / RR_BLOCK};
}

// ---- the end of a staged level 1 (rr_api_frame.h join_shadow) ------------------------------------------------------------------
// When the last stage has been shaded, the shadow launches of the last TWO stages may still run (stage n - 2 trails the shade launches by
// one stage, stage n - 1 has only just begun), and the frame's stream goes on to level 2 beside them.  [lo, hi) = the rays of the
// shadow-queue allocation they read: the hull of the two buffers (of the one buffer where the level has a single stage).
// The rays [0, lo) in front of them belong to the buffers the two do not use, and those are not at rest by themselves: the shadow launch
// of an EARLIER stage read them, and no shade launch of the level has waited for the latest of those (shade k waits for shadow k - n_buf
// only).  rest_stage = that stage, the last one before n - 2 whose buffer lies in [0, lo) (-1: there is none), rest_buffer = its buffer:
// whoever writes [0, lo) without waiting for the two launches of the tail must wait for the shadow launch of rest_stage instead.
struct Level1Tail { uint64_t lo, hi; int32_t rest_stage, rest_buffer; };
inline Level1Tail level1_tail(const Level1Stages& sp) {
    const uint64_t a = sp.ray_offset[sp.buffer_of(sp.n_stages - 1)], b = sp.n_stages >= 2 ? sp.ray_offset[sp.buffer_of(sp.n_stages - 2)] : a;
    Level1Tail t{std::min(a, b), std::max(a, b) + sp.buf_rays, -1, -1};
    for (int64_t k = (int64_t)sp.n_stages - 3; k >= 0 && t.rest_stage < 0; k--)
        if (sp.ray_offset[sp.buffer_of((uint32_t)k)] < t.lo) { t.rest_stage = (int32_t)k; t.rest_buffer = (int32_t)sp.buffer_of((uint32_t)k); }
    return t;
}
// A chunk of the serial loop writes its shadow rays from ray 0 of the allocation on.  May its shade launch run while the launches of
// `tail` still read their buffers?  Only a chunk of the dense queue (a chunk with fixed slots writes the validity words as well, from word
// 0 on) whose shards all end in front of the tail: with three buffers and a stage count that is a multiple of three the last two stages
// use buffers 1 and 2, and a deeper level that fits into buffer 0 need only wait for the shadow launch of rest_stage, which read it last.
inline bool chunk_clear_of_tail(const ShadeChunk& g, const Level1Tail& tail) {
    return !g.fixed && g.segcap * RR_SQ_SHARDS <= tail.lo;
}

// The sample group of the batch [first, first + n): G where the batch holds whole groups of whole sample slices, else 1.
inline uint32_t batch_group(const FramePlan& p, uint32_t npix, uint64_t first, uint64_t n) {
    return (n % ((uint64_t)npix * p.G) == 0 && first % npix == 0) ? p.G : 1u;
}

// Rays per slice of depth level d (n rays, its children from arena index child_base on), in an arena of M rays for
// R = max_recursion: n when the children of the whole level fit, else a positive whole number of workgroups;
// 0 = the arena is too small for level d.  The deepest level (d > R) spawns nothing (k_shade: depth <= max_recursion).
// Children of a slice may use the space behind this level minus what the deeper levels need to make progress
// themselves (one 256-ray slice = 512 children per spawning level below): the recursion can then never get stuck.
inline uint64_t level_slice(uint64_t M, uint64_t child_base, uint64_t n, uint32_t d, uint32_t R) {
    if (d > R) return n;
    const uint64_t keep = 2ull * RR_BLOCK * (R - d); // spawning levels below d + 1's parent: d + 1 .. R
    const uint64_t room = M - child_base;
    if (room < keep + 2ull * RR_BLOCK) return 0;
    return 2 * n > room - keep ? ((room - keep) / 2 / RR_BLOCK) * RR_BLOCK : n;
}
