// rr_kernels.hip — the trace loop of rustray as a wavefront path tracer for gfx950.
//
// Replaces, for a whole frame, Raytracing::render / trace /
// get_color_depth_normal_id (reference src/raytracing.rs:275-998) and the
// Shape implementations under it (src/shape/mesh.rs, src/shape/sphere.rs,
// src/shape/mod.rs:510-629, :755-761).
//
// The reference recursion (every hit may spawn a reflection AND a refraction
// child, src/raytracing.rs:938-971) is flattened breadth-first: all path nodes
// of one recursion depth form a ray queue in HBM, and one depth level is
//     trace_closest  ->  shade  ->  trace_shadow
// `shade` appends the next level's rays (wave ballot + prefix compaction, one
// atomic per wave) and the shadow rays of its lights.  A node's colour is an
// affine function of its children (c = A + wR*R + wT*T with scalar weights), so
// each ray carries one scalar throughput and every node adds throughput * A into
// per-pixel fixed-point accumulators: integer adds commute, hence the frame is
// bit-identical for any scheduling, batching, tiling or GPU count.
//
// The trace kernels are persistent: a fixed grid of 256-thread workgroups walks
// the queue in 64-ray packets, half of them dealt round-robin, half pulled from a
// shared head; the queue length is read on the device.
#include "rr_device.h"
#include "rr_math.h"
#include "rr_primary_setup.h"
#include "rr_adaptive.h" // half_error and the 8x8-block order of a refinement list (kernels 5l .. 5p)
#include "rr_denoise.h"  // the arithmetic of the a-trous filter (kernels 7a .. 7d)
#include "rr_temporal.h" // the arithmetic of the temporal reprojection (kernel 7e)
#include "rr_history_clamp.h" // the neighbourhood clamp of the history (kernel 7e'')
#include "rr_motion.h"   // the per-pixel motion of moved items and the call's table (kernel 7f)
#include "rr_upsample.h" // the arithmetic of the joint-bilateral upsampler (kernel 7g)

// ---------------------------------------------------------------------------
// The numeric knobs of the build, all of them: every one can be overridden with -D (tools/variant.sh, tools/resusage.sh);
// the values here are the ones that were measured fastest and that ship.
// ---------------------------------------------------------------------------
#ifndef RR_SQ_STRIDE
#define RR_SQ_STRIDE 16 // words between two append counters: 64 B apart (packed into one line they cost k_shade 13-20 %)
#endif
#ifndef RR_TRACE_WAVES
#define RR_TRACE_WAVES 4 // waves per SIMD the trace kernels are built for (bounds VGPRs; LDS stack: RR_STACK_DEPTH KB per workgroup)
#endif
#ifndef RR_CLOSEST_WAVES
#define RR_CLOSEST_WAVES RR_TRACE_WAVES // k_trace_closest alone
#endif
#ifndef RR_SHADOW_WAVES
#define RR_SHADOW_WAVES RR_TRACE_WAVES // k_trace_shadow alone
#endif
#ifndef RR_SHADE_WAVES
#define RR_SHADE_WAVES 4 // waves per SIMD k_shade is built for
#endif
// Launch sizes (host side, rr_api_frame.h): workgroups per CU of a k_shade and of a k_trace_shadow launch that has the GPU to itself.
#ifndef RR_SHADE_GRID_WG
#define RR_SHADE_GRID_WG (2 * RR_SHADE_WAVES) // two rounds of resident workgroups
#endif
#ifndef RR_SHADOW_GRID_WG
#define RR_SHADOW_GRID_WG RR_SHADOW_WAVES // exactly the resident workgroups (RR_STACK_DEPTH KB of LDS stack each)
#endif
// Level 1 in stages on three streams (rr_api_frame.h run_level1_stages, rr_frame_plan.h plan_level1_stages): k_shade<true> of stage
// k + 1 beside k_trace_shadow<true> of stage k and, where the level is one slice, beside k_trace_closest<true> over the packets of stage
// k + 2 (round 15: before, one closest-hit launch traced the whole level alone, a third of the level-1 work at rate 1.0).  The numbers of
// the first two knob blocks: the contract frame (sponza_syn 1280x720 128 spp) in round 5, serial loop 19.2 ms on the same box
// (profiles/r05_level1_share_rates.txt, profiles/r05_dropped.txt, profiles/r05_ab_level1_overlap.txt).
//   0 = never in stages; 1 = only where the caller asks for shade chunks (rr_tuning::shade_chunk_rays != 0: a stage is that
//   chunk); 2 = also with automatic tuning, in equal stages of at most RR_L1_STAGE_RAYS.
#ifndef RR_L1_OVERLAP
#define RR_L1_OVERLAP 2
#endif
#ifndef RR_L1_STAGE_RAYS
#define RR_L1_STAGE_RAYS (20ull << 20) // largest automatic stage: the contract frame in 6 equal stages 18.6 ms; 8 stages 18.6, 5: 18.6, 4: 18.65, 3: 18.7, 2: 19.0;
#endif                                 // unequal 8 Mi stages (15) 19.7 ms, 16 Mi (8) 18.75 ms, 32 Mi (4) 18.6 ms
#ifndef RR_L1_BUFFERS
#define RR_L1_BUFFERS 3 // shadow-queue buffers the stages rotate through (2 or 3): with 2, 16 Mi stages 19.55 ms against 18.75, 32 Mi 19.1 against 18.6
#endif
// Workgroups per CU of the two launches while they share the GPU.  4 workgroups of either kernel are resident on a CU, and a
// split of those 4 (3 + 1 24.2 ms, 2 + 2 21.3 ms, 1 + 3 24.0 ms; 2 + 2 with 3 buffers and 16 Mi stages 19.6 ms) LOSES to the
// serial loop: a stage's shade and shadow costs differ by up to 4 x with the part of the picture it covers, so one of the two
// launches always ends early and leaves its slots idle.  Grids of SEVERAL rounds of workgroups share the CUs instead: a
// workgroup that ends frees its slot for whichever launch has workgroups waiting, no slot is ever idle, and the mix follows
// the work.  16 + 16: 18.6 ms; 8 + 8 19.2, 12 + 12 18.65, 24 + 24 18.5 - 18.8, 32 + 32 18.75 - 19.2, 64 + 64 25.1 ms; 16 + 8
// 19.45, 8 + 16 19.2, 24 + 16 19.05, 16 + 24 19.0 ms; 8 + 4 (the grids of the serial loop) 19.65 ms.
#ifndef RR_L1_SHADE_WG
#define RR_L1_SHADE_WG 16 // 0 = one workgroup per 256 hits: k_shade then takes 40 ms instead of 6.3 (the dispatcher starts ~11 workgroups per microsecond)
#endif
#ifndef RR_L1_SHADOW_WG
#define RR_L1_SHADOW_WG 16
#endif
// ... and of the closest-hit launches of the stages, which share the CUs with both (round 15, parent 17.07 - 17.10 ms on the same box;
// profiles/r15_ab_closest_stages.txt, profiles/r15_dropped.txt): 24: 16.78 - 16.84 ms; 4 (exactly the resident workgroups: a slot is never
// handed over) 17.02 - 17.05, 8: 16.88 - 16.89, 16: 16.98 - 17.00, 20: 16.84 - 16.94, 32: 17.02 - 17.06, 48: 19.6 - 19.8.  With the closest-hit
// launches at 24, shade and shadow at 12 + 12: 16.98 - 17.01, 24 + 24: 17.29; 4 stages instead of 6: 16.74 - 16.78 (no better), 5: 17.2,
// 8: 17.2 - 17.3, 12: 19.1 - 19.2.  The launch of stage 0 runs alone: the grid of the serial loop, 16.66 - 16.74 against 16.78 - 16.81 at 24.
#ifndef RR_L1_CLOSEST_WG
#define RR_L1_CLOSEST_WG 24
#endif
#ifndef RR_L1_CLOSEST_FIRST_WG
#define RR_L1_CLOSEST_FIRST_WG RR_CLOSEST_WAVES // stage 0 (8: 16.71 - 16.76)
#endif
// The end of the staged level 1 (round 27, rr_api_frame.h join_shadow; profiles/r27_ab_tail_overlap.txt, profiles/r27_dropped.txt): the shadow
// launches of the last two stages run beside each other and beside level 2, so the last stage's launch takes RR_L1_SHADOW_WG like the
// stages before it.  On the serial loop's grid (exactly the resident workgroups), which it had while it ran alone, the medians are the same
// to 0.03 ms (15.32 - 15.43 against 15.31 - 15.36 ms in the same calls) and the runs spread twice as far.
#ifndef RR_DYN_FETCH
#define RR_DYN_FETCH 4 // packets per fetch from the shared head on large launches (more costs locality: +4 % at 8, +10 % at 16)
#endif
// Share of a launch's packets that is dealt to the waves round-robin, without an atomic (see PacketStream).
#ifndef RR_STATIC_NUM
#define RR_STATIC_NUM 1
#define RR_STATIC_DEN 2
#endif
#ifndef RR_SHADOW_FIXED_STATIC_NUM
#define RR_SHADOW_FIXED_STATIC_NUM 7 // level 1 (fixed slots): sponza_syn shadow 6.3 -> 6.0 ms against one half
#define RR_SHADOW_FIXED_STATIC_DEN 8
#endif
#ifndef RR_SHADOW_STATIC_NUM
#define RR_SHADOW_STATIC_NUM 1 // the dense shadow queue of the deeper levels keeps half of its packets dynamic
#define RR_SHADOW_STATIC_DEN 2
#endif
// A per-mesh walk tests its parked leaves once this share of the wave's unfinished lanes holds one (rr_walk.h, blas_closest:
// before, node steps ran with ~27 of 64 lanes and triangle tests with 7-15).
#ifndef RR_PEND_NUM
#define RR_PEND_NUM 2
#define RR_PEND_DEN 3
#endif

#define RR_DEPTH_WIDE ((int)0x80000000) // k_shade: this lane's depth term does not fit its 32-bit sum (accum_depth_wide_merged)
#define RR_FIXED_SLOT_LIGHTS 32u // level 1 keeps fixed shadow slots for up to this many enabled lights (one bit per light in k_shade's sq_wrote)

// The layers under the kernels, bottom-up (each header says what it offers and un-defines the macros that are its own):
#include "rr_primitives.h" // exact ray / box, triangle and ball tests in item-local space
#include "rr_walk.h"       // the BVH4 node step; walks of one mesh, per lane and per packet
#include "rr_trace.h"      // a ray or a packet against the scene: closest hit, shadow query
#include "rr_surface.h"    // textures, materials, uv, jitter, fresnel
#include "rr_accumulate.h" // fixed-point per-pixel sums, merged per wave

// ---------------------------------------------------------------------------
// primary rays (reference src/raytracing.rs:319-396)
// ---------------------------------------------------------------------------
RR_DEV float4 mat4_mul(const float* m, float x, float y, float z, float w) {
    return make_float4(((m[0] * x + m[4] * y) + m[8] * z) + m[12] * w,
                       ((m[1] * x + m[5] * y) + m[9] * z) + m[13] * w,
                       ((m[2] * x + m[6] * y) + m[10] * z) + m[14] * w,
                       ((m[3] * x + m[7] * y) + m[11] * z) + m[15] * w);
}

// Primary rays are a pure function of (pixel slot, sample): the level-1 trace and shade kernels both DERIVE them
// instead of reading ray records that a ray-generation kernel wrote (round 1: k_raygen wrote 40 B per primary ray,
// 4.7 GB per sponza_syn frame, that the trace kernel read straight back and the shade kernel read a third time).
// Both kernels run the same instruction sequence on the same inputs, so they see the same ray, bit for bit.
// What the derivation does not owe to the ray is set up on the host (rr_primary_setup.h): the screen point of a pixel's
// centre per accumulator slot, the sub-sample's offset per sample, and the constants of the index arithmetic.
struct DPrimary {
    const float* sample_tr; // (x_trans, y_trans) per sample: primary_sample_offsets
    PrimaryLaunch at;       // where the batch starts and how its packets are grouped
    uint32_t n;             // primary rays in the batch
    uint32_t lg_parts;      // log2 of the accumulator slots per pixel: 0 but for rr_render_pixel_parts (primary_part_sample)
};
RR_DEV void primary_ray(const DFrame& fr, const PrimaryFrame& pf, const DPrimary& pr, uint32_t i,
                        f3* origin_out, f3* dir_out, uint32_t* pix_out, uint32_t* sample_out) {
    uint32_t pix, s; // accumulator slot (slots enumerate 8x8 blocks of the region's tiles) and sample
    primary_index(pf, pr.at, pr.lg_parts, i, &pix, &s);
    const float2 c = rr_global(reinterpret_cast<const float2*>(pf.slot_c))[pix]; // (a pointer read from a device record: rr_global)
    const float2 tr = reinterpret_cast<const float2*>(pr.sample_tr)[s];
    const float cx = c.x, cy = c.y, x_trans = tr.x, y_trans = tr.y;
    f3 origin, dir;
    if (fr.dof) {
        float4 cpp = mat4_mul(fr.proj_inv, cx, cy, -1.0f, 1.0f);
        f3 rd = mk3(cpp.x - 0.0f, cpp.y - 0.0f, cpp.z - 0.0f);
        float4 eye = mat4_mul(fr.view_inv, 0.0f, 0.0f, 0.0f, 1.0f);
        float4 dv = mat4_mul(fr.view_inv, rd.x, rd.y, rd.z, 0.0f);
        float dn = sqrtf((dv.x * dv.x + dv.z * dv.z) + (dv.y * dv.y + dv.w * dv.w)); // nalgebra 4-lane dot order
        float4 dvn = make_float4(dv.x / dn, dv.y / dn, dv.z / dn, dv.w / dn);
        float dist = norm3(rd);
        float f = 1.0f / (dist / (dist + fr.focal_length));
        f3 p = mk3(eye.x + f * dvn.x, eye.y + f * dvn.y, eye.z + f * dvn.z);
        float sx = cx + x_trans;
        float sy = cy + y_trans;
        float4 pp = mat4_mul(fr.proj_inv, sx, sy, -1.0f, 1.0f);
        float4 ro = mat4_mul(fr.view_inv, pp.x, pp.y, pp.z, 1.0f);
        origin = mk3(ro.x, ro.y, ro.z);
        dir = mk3(p.x - ro.x, p.y - ro.y, p.z - ro.z);
    } else {
        float sx = cx + x_trans;
        float sy = cy + y_trans;
        float4 pp = mat4_mul(fr.proj_inv, sx, sy, -1.0f, 1.0f);
        float4 o = mat4_mul(fr.view_inv, pp.x, pp.y, pp.z, 1.0f);
        float4 d = mat4_mul(fr.view_inv, pp.x - 0.0f, pp.y - 0.0f, pp.z - 0.0f, 0.0f);
        origin = mk3(o.x, o.y, o.z);
        dir = mk3(d.x, d.y, d.z);
    }
    dir = normalize3(dir); // get_color_depth_normal_id normalises on entry (:723)
    *origin_out = origin; *dir_out = dir; *pix_out = pix; *sample_out = s;
}

// The ray record (DRayQueue: r0, r1, r2) of the ROOT of a path -- a primary ray of a frame (k_shade<true>) or a caller's ray as depth
// level 1 (k_seed_rays): throughput 1, depth 1, carries the object id, path node 1.  `pix`: the accumulator slot.
RR_DEV void root_record(f3 origin, f3 dir, uint32_t pix, uint32_t sample, float4* r0, float4* r1, uint2* r2) {
    *r0 = make_float4(origin.x, origin.y, origin.z, 1.0f);
    *r1 = make_float4(dir.x, dir.y, dir.z, __uint_as_float(pix));
    *r2 = make_uint2(sample | (1u << 16) | (1u << 24), 1u);
}

// ---------------------------------------------------------------------------
// the packet stream of the walk kernels (k_trace_closest, k_trace_shadow, k_query_shadow): which 64-ray packet a wave takes next
// ---------------------------------------------------------------------------
// Work distribution.  Locality decides here: the waves that run side by side must walk neighbouring
// packets (runs of consecutive packets per wave cost 1.8x, measured), and one head word sustains only ~90
// fetches per microsecond.  So num / den of the packets (the static share: RR_STATIC_*, RR_SHADOW_*STATIC_*) are dealt
// round-robin with no atomic at all, and the rest is pulled a few packets at a time from the shared head word to absorb
// expensive packets.  Blocks b and b + 8 share an XCD (and its L2): when the grid is a multiple of 8 the blocks of one XCD
// take one contiguous run of packets per round instead of every eighth group.
struct PacketStream {
    uint32_t n_packets, n_waves, wave_id, rounds, n_static, round, dyn_next, dyn_left, dyn_k;
    uint32_t* head;
    static RR_DEV uint32_t waves() { return gridDim.x * (RR_BLOCK / RR_WAVE); } // of the launch
    // num / den: the static share; head: the launch's head word (the host zeroes it), counted in packets behind the static ones
    RR_DEV PacketStream(uint32_t n_packets_, uint32_t num, uint32_t den, uint32_t* head_) : n_packets(n_packets_), head(head_) {
        n_waves = waves();
        uint32_t blk = blockIdx.x;
        if ((gridDim.x & 7u) == 0u) blk = (blockIdx.x & 7u) * (gridDim.x >> 3) + (blockIdx.x >> 3);
        wave_id = blk * (RR_BLOCK / RR_WAVE) + threadIdx.x / RR_WAVE;
        rounds = (uint32_t)(((unsigned long long)n_packets * num / den) / n_waves);
        n_static = rounds * n_waves;
        round = 0; dyn_next = 0; dyn_left = 0;
        // packets per fetch of the dynamic part: RR_DYN_FETCH on large launches (more costs locality: +4 % at 8, +10 % at 16), fewer when
        // the launch has only a few packets per wave
        dyn_k = n_packets >= 8u * n_waves ? (uint32_t)RR_DYN_FETCH : (n_packets >= 2u * n_waves ? 2u : 1u);
    }
    // the stream hands out p0 + its packets from here on: once, before the first next() (nothing of p0 stays live in the walk)
    RR_DEV void start_at(uint32_t p0) { wave_id += p0; n_static += p0; n_packets += p0; }
    // false: the stream has ended for this wave (wave-uniform)
    RR_DEV bool next(uint32_t* pkt) {
        uint32_t p;
        if (round < rounds) { p = round * n_waves + wave_id; round++; }
        else {
            if (dyn_left == 0u) { // several packets per atomic: the head word sustains only ~90 fetches per microsecond
                uint32_t f = 0;
                if ((threadIdx.x & (RR_WAVE - 1)) == 0) f = atomicAdd(head, dyn_k);
                dyn_next = n_static + __shfl(f, 0); dyn_left = dyn_k;
            }
            p = dyn_next++; dyn_left--;
        }
        *pkt = p;
        return p < n_packets;
    }
};

// ---------------------------------------------------------------------------
// kernel 2: closest hit for a queue of rays
// ---------------------------------------------------------------------------
// Scene view + frame constants of k_shade as one device record.  As by-value kernel arguments all 90 dwords stayed live
// in SGPRs across the kernel's loop and 117 of them were spilled into VGPR lanes; read through a pointer, only what is
// in use is kept (k_shade -4 %).  The trace kernels keep their by-value arguments: their walks use the same few fields
// in every step, and re-reading those costs more than the spills did (closest-hit +4 %, shadow +10 %, measured).
struct DShadeConst { DSceneView sc; DFrame fr; PrimaryFrame ps; };

// PRIMARY: depth level 1.  The rays are derived from their index (primary_ray), only the 16-B hit record is written;
// block 0 publishes the level's size for the shade kernel and counts the rays.
// A launch walks the packets [p0, p0 + np) of the level, as far as the level has them (RR_ALL_PACKETS from 0: the whole level).  A ray
// and its hit record depend on the ray's index alone, so the launches of a level cut into ranges write what one launch would: level 1
// in stages (rr_api_frame.h) traces stage k + 1 while stage k is shaded.  Every launch publishes the LEVEL's size and counts its own rays;
// its packet stream (static share, small_launch) is dealt over its own packets, and the head word is its own.
#define RR_ALL_PACKETS 0xffffffffu
template <bool PRIMARY>
__global__ __launch_bounds__(RR_BLOCK, RR_CLOSEST_WAVES) void k_trace_closest(DSceneView sc, DRayQueue q, uint32_t* __restrict__ q_count,
                                                            uint32_t* head, const DShadeConst* __restrict__ kc, DPrimary pr,
                                                            unsigned long long* counters, uint32_t p0, uint32_t np) {
    __shared__ int s_stack[RR_STACK_DEPTH * RR_BLOCK];
    RR_UTIL_KIND(PRIMARY ? 0u : 1u)
    const uint32_t n = PRIMARY ? pr.n : *q_count;
    const uint32_t level_packets = (n + RR_WAVE - 1) / RR_WAVE;
    const uint32_t n_packets = p0 < level_packets ? min(np, level_packets - p0) : 0u; // of this launch
    if (PRIMARY && blockIdx.x == 0 && threadIdx.x == 0) {
        *q_count = n;
        atomicAdd(&counters[RR_CNT_PRIMARY], (unsigned long long)(min(n, (p0 + n_packets) * RR_WAVE) - min(n, p0 * RR_WAVE)));
    }
    const uint32_t lane = threadIdx.x & (RR_WAVE - 1);
    // (a launch with few packets per wave -- one rank's share of a frame tiled over 4 or 8 GPUs -- deals three quarters statically:
    // closest-hit 2.36 -> 2.29 ms on a quarter of the contract frame, 1.36 -> 1.32 ms on an eighth; the whole frame loses 5 % to it)
    const bool small_launch = n_packets < 160u * PacketStream::waves();
    PacketStream stream(n_packets, small_launch ? 3u : (uint32_t)RR_STATIC_NUM, small_launch ? 4u : (uint32_t)RR_STATIC_DEN, head);
    stream.start_at(p0);
    for (uint32_t pkt; stream.next(&pkt);) { // a packet of the LEVEL
        const uint32_t i = pkt * RR_WAVE + lane;
        const uint32_t ii = min(i, n - 1u); // the lanes past the end of the last packet repeat its last ray, so that the packet form below runs with all lanes
        f3 ro, rd; uint32_t depth;
        if constexpr (PRIMARY) { // the frame constants are read once per packet (not worth 49 SGPRs across the walks); kc is NULL in the <false> build's launches
            uint32_t pix_, smp_; primary_ray(kc->fr, kc->ps, pr, ii, &ro, &rd, &pix_, &smp_); depth = 1u;
        } else {
            const float4 r0 = q.r0[ii], r1 = q.r1[ii];
            ro = mk3(r0.x, r0.y, r0.z); rd = mk3(r1.x, r1.y, r1.z);
            depth = (q.r2[ii].x >> 16) & 0xffu;
        }
        Closest best;
        if (!trace_closest_packet(sc, ro, rd, depth, s_stack, &best))
        {
            if (ray_nonfinite(ro, rd)) trace_closest_nonfinite(sc, ro, rd, depth, &best);
            else trace_closest_ray(sc, ro, rd, depth, s_stack, &best);
        }
        if (best.nan_seen) trace_closest_ordered(sc, ro, rd, depth, s_stack, &best); // (rare: a ball whose arithmetic overflows)
        if (i < n) q.hit[i] = make_uint4(__float_as_uint(best.t), (uint32_t)(best.found ? best.item : -1), best.face, 0u);
    }
}

// ---------------------------------------------------------------------------
// wave-level queue allocation: ballot + prefix, one atomic per wave.  Must be
// reached by every lane that may set `want` in the same control-flow region.
// ---------------------------------------------------------------------------
RR_DEV uint32_t wave_alloc(uint32_t* counter, bool want, uint32_t lane) {
    unsigned long long mask = __ballot(want);
    if (mask == 0ull) return 0u;
    int leader = __ffsll((long long)mask) - 1;
    uint32_t base = 0u;
    if ((int)lane == leader) base = atomicAdd(counter, (uint32_t)__popcll(mask));
    base = __shfl(base, leader);
    return base + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
}

// ---------------------------------------------------------------------------
// kernel 3: shade one depth level (reference src/raytracing.rs:734-995)
// ---------------------------------------------------------------------------
// SPLIT (rr_render_pixel_split, level 1 only): next to every light term of a depth-1 hit its DIFFUSE part -- the same product with the
// specular summand left out -- goes to three planes of its own (`diffuse`, laid out as acc.rgb: channel k at diffuse + k * acc.n) through
// the same fix_add / accum_merged, and for a receiver that takes shadows into a fourth queue array (sq_s3, next to sq.s2) that
// k_trace_shadow<*, true> scales by the ray's factor.  The two pointers are the arguments `split` of the SPLIT builds ALONE (long long*
// diffuse, float4* sq_s3): the other builds take no argument more than they took, so their kernel-argument segment and with it their code
// are what they were.
RR_DEV long long* split_planes() { return nullptr; }
template <class Q> RR_DEV long long* split_planes(long long* planes, Q*) { return planes; }
RR_DEV float4* split_queue() { return nullptr; }
template <class Q> RR_DEV Q* split_queue(long long*, Q* queue) { return queue; }
// The record of light `li` in scalar registers.  The index is the light loop's counter, the same in every lane of either build, and the
// record arrived as seven vector loads of 64 equal addresses, fetched where the fields are used.  Here its three 16-byte groups are
// requested together through the constant address space and waited for once, as item_rec_uniform (rr_primitives.h) does for the walks;
// the empty asm statement reads them where they are loaded.  No kernel writes the lights; edits happen between launches.
static_assert(sizeof(DLight) == 48 && offsetof(DLight, intensity) == 12 && offsetof(DLight, dir) == 16 && offsetof(DLight, max_angle) == 28 &&
              offsetof(DLight, color) == 32 && offsetof(DLight, type) == 44, "light_uniform: three 16-byte groups");
RR_DEV DLight light_uniform(const DLight* lights, uint32_t li) {
    const __attribute__((address_space(4))) char* p = (const __attribute__((address_space(4))) char*)(uintptr_t)lights + (unsigned long long)li * sizeof(DLight);
    const rr_f4v g0 = *(const __attribute__((address_space(4))) rr_f4v*)p, g1 = *(const __attribute__((address_space(4))) rr_f4v*)(p + 16),
                 g2 = *(const __attribute__((address_space(4))) rr_f4v*)(p + 32);
    asm volatile("" :: "s"(g0), "s"(g1), "s"(g2));
    DLight L;
    L.pos[0] = g0.x; L.pos[1] = g0.y; L.pos[2] = g0.z; L.intensity = g0.w;
    L.dir[0] = g1.x; L.dir[1] = g1.y; L.dir[2] = g1.z; L.max_angle = g1.w;
    L.color[0] = g2.x; L.color[1] = g2.y; L.color[2] = g2.z; L.type = __float_as_uint(g2.w);
    return L;
}

// The arguments of k_shade as its kernel-argument segment holds them (every member is naturally aligned, so the segment's layout is this
// struct's; the SPLIT builds' two pointers follow it).  What the packet loop uses in every packet and every light -- the hit records, the
// chunk bounds, the shadow queue -- the kernel takes from its parameters as before, and those stay in SGPRs.  Everything else it reads
// from the segment WHERE IT IS USED, through the scalar cache: about 60 dwords of parameters held across the loop, on a target with 102
// SGPRs, were spilled into VGPR lanes, and every use of a spilled one is a v_readlane on the vector port, which is what bounds this
// kernel.  A parameter that is not named in the body is not loaded at the kernel's entry either.
struct ShadeArgs {
    const DShadeConst* kc; const uint32_t* slot_xy; DPrimary pr; DRayQueue qin; const uint32_t* qin_count; uint32_t chunk_begin, chunk_end;
    DRayQueue qout; uint32_t* qout_count; DShadowQueue sq; uint32_t* sq_counts; uint32_t sq_segcap; unsigned long long* sq_valid; uint32_t sq_cap;
    DAccum acc; unsigned long long* counters;
};
typedef const __attribute__((address_space(4))) char* rr_kernarg_ptr;
// The segment's address as a value the compiler cannot see through (the empty asm statement): loads behind it are neither hoisted out of
// the loop the statement stands in nor merged with the entry's own loads of the parameters.
RR_DEV rr_kernarg_ptr kernarg_segment() {
    rr_kernarg_ptr p = (rr_kernarg_ptr)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(p));
    return p;
}
template <class T> RR_DEV T* rr_global_mut(T* p) { return (T*)(__attribute__((address_space(1))) T*)(uintptr_t)p; }
template <class T> RR_DEV T kernarg_at(rr_kernarg_ptr ka, uint32_t offset) {
    static_assert(std::is_scalar<T>::value, "member by member: a record's copy constructor takes no reference into the constant address space");
    const T v = *(const __attribute__((address_space(4))) T*)(ka + offset);
    if constexpr (std::is_pointer<T>::value) return rr_global_mut(v); // (a pointer loaded from memory is generic: rr_walk.h rr_global)
    else return v;
}
#define RR_SHADE_ARG(ka, member) kernarg_at<decltype(((ShadeArgs*)nullptr)->member)>(ka, (uint32_t)__builtin_offsetof(ShadeArgs, member))
RR_DEV DAccum shade_arg_accum(rr_kernarg_ptr ka) { // the whole record, for the merges at a packet's end
    DAccum a;
    a.rgb = RR_SHADE_ARG(ka, acc.rgb); a.normal = RR_SHADE_ARG(ka, acc.normal); a.depth = RR_SHADE_ARG(ka, acc.depth); a.object_id = RR_SHADE_ARG(ka, acc.object_id);
    a.n = RR_SHADE_ARG(ka, acc.n); a.flags = RR_SHADE_ARG(ka, acc.flags);
    return a;
}
RR_DEV DPrimary shade_arg_primary(rr_kernarg_ptr ka) {
    DPrimary p;
    p.sample_tr = RR_SHADE_ARG(ka, pr.sample_tr);
    p.at.first_sample = RR_SHADE_ARG(ka, pr.at.first_sample); p.at.first_pix = RR_SHADE_ARG(ka, pr.at.first_pix);
    p.at.lg_group = RR_SHADE_ARG(ka, pr.at.lg_group); p.at.lg_pixels = RR_SHADE_ARG(ka, pr.at.lg_pixels);
    p.n = RR_SHADE_ARG(ka, pr.n); p.lg_parts = RR_SHADE_ARG(ka, pr.lg_parts);
    return p;
}
template <bool PRIMARY, bool SPLIT = false, class... Split>
__global__ __launch_bounds__(RR_BLOCK, RR_SHADE_WAVES) void k_shade(const DShadeConst* __restrict__ kc, const uint32_t* __restrict__ /* slot_xy */, DPrimary /* pr */,
                                                    DRayQueue qin, const uint32_t* __restrict__ qin_count,
                                                    uint32_t chunk_begin, uint32_t chunk_end,
                                                    DRayQueue /* qout */, uint32_t* /* qout_count */,
                                                    DShadowQueue sq, uint32_t* /* sq_counts */, uint32_t /* sq_segcap */, unsigned long long* __restrict__ /* sq_valid */, uint32_t sq_cap,
                                                    DAccum /* acc */, unsigned long long* /* counters */, Split... split) { // (the unnamed ones: ShadeArgs)
    static_assert(sizeof...(Split) == (SPLIT ? 2 : 0), "the SPLIT builds take (long long* diffuse, float4* sq_s3), the others nothing");
    [[maybe_unused]] float4* const sq_s3 = split_queue(split...);
    [[maybe_unused]] long long* const dif_rgb = split_planes(split...); // SPLIT: the diffuse planes, laid out as acc.rgb
    // The scene view and the frame constants (90 dwords) are read from a small device record where they are needed
    // instead of arriving as kernel arguments: as arguments they were all live in SGPRs across the whole loop and the
    // kernel spilled 117 of them into VGPR lanes.
    const DSceneView& sc = kc->sc;
    const DFrame& fr = kc->fr;
    const uint32_t n = min(*qin_count, chunk_end);
    const uint32_t lane = threadIdx.x & (RR_WAVE - 1);
    const bool gw = sc.general_w != 0u;
    uint32_t n_shaded = 0, n_shadow = 0, n_secondary = 0;
    // the four waves of a workgroup walk four neighbouring packets per iteration and allocate their children together
    // (one atomic per workgroup iteration: a single append counter sustains ~90 returning atomics per microsecond, which
    // made it THE limiter of this kernel on scenes where most hits spawn children)
    __shared__ uint32_t s_child_n[2][RR_BLOCK / RR_WAVE];
    __shared__ float s_lut[256]; // the u8 -> f32 table next to the lanes: a texel decodes with four LDS reads
    s_lut[threadIdx.x] = c_u8_to_f32[threadIdx.x];
    __syncthreads();
    __shared__ uint32_t s_child_base[2];
    const uint32_t wave_in_block = threadIdx.x / RR_WAVE;
    uint32_t parity = 0;
    for (uint32_t block_base = chunk_begin + blockIdx.x * RR_BLOCK; block_base < n; block_base += gridDim.x * RR_BLOCK, parity ^= 1u) {
        const uint32_t base = block_base + wave_in_block * RR_WAVE;
        const uint32_t i = base + lane;
        const rr_kernarg_ptr ka = kernarg_segment(); // (per packet: what is read behind it is read in this packet, where it is used)
        // the colour, diffuse and normal planes of channel ch, fetched by the rare term that goes to its plane directly (fix_add_at)
        const auto rgb_plane = [=](uint32_t ch) { return [=] { return RR_SHADE_ARG(ka, acc.rgb) + ch * RR_SHADE_ARG(ka, acc.n); }; };
        [[maybe_unused]] const auto dif_plane = [=](uint32_t ch) { return [=] { return dif_rgb + ch * RR_SHADE_ARG(ka, acc.n); }; };
        const auto normal_plane = [=](uint32_t ch) { return [=] { long long* const p = RR_SHADE_ARG(ka, acc.normal); return p ? p + ch * RR_SHADE_ARG(ka, acc.n) : nullptr; }; };
        uint4 hit = make_uint4(0u, 0xffffffffu, 0u, 0u);
        if (i < n) hit = qin.hit[i];
        const int item_idx = (int)hit.y;
        const bool active = i < n && item_idx >= 0; // miss: colour 0, depth 0, normal 0, id 0 (:728-732); buffers are pre-zeroed
        // LEVEL 1: shadow rays have FIXED slots.  The ray of hit i towards the k-th enabled light sits at k * sq_cap +
        // (i - chunk_begin), and one 64-bit word per (light, packet) says which lanes hold one (sq_valid).  A packet of the
        // shadow kernel is then the shadow rays of one packet of hits -- 64 samples of one pixel towards one light, all or
        // none of them as a rule -- which is what its packet form of the top level needs, and nothing is allocated.
        // DEEPER LEVELS: appended densely (ballot + prefix, one atomic per wave and light) to one of RR_SQ_SHARDS sub-queues
        // chosen by the input packet group (256 consecutive rays; a single append counter is a hot word, ~90 returning
        // atomics per microsecond; shard capacity is static: a shard receives at most its share of the chunk's packets).
        // There only some lanes of a packet spawn a shadow ray, and fixed slots would trace packets a fifth full
        // (monkey: shadow 2.1 -> 3.5 ms); so do the level-1 packets of scenes too small for the packet form (+3 .. 15 %).
        const bool sq_fixed = PRIMARY && sq_cap != 0u; // (the host's choice: level 1 of a scene whose top level has a packet form)
        const uint32_t sq_slot = i - chunk_begin;
        uint32_t sq_wrote = 0u; // bit k: this lane wrote a ray for the k-th enabled light
        const uint32_t shard = ((base - chunk_begin) / RR_BLOCK) % RR_SQ_SHARDS; // the 4 packets of a workgroup iteration stay together
        uint32_t* sq_count = nullptr; uint32_t sq_base = 0u; // (dead with fixed slots)
        if (!sq_fixed) { sq_count = RR_SHADE_ARG(ka, sq_counts) + shard * RR_SQ_STRIDE; sq_base = shard * RR_SHADE_ARG(ka, sq_segcap); }
        int sum_r = 0, sum_g = 0, sum_b = 0; // this hit's direct adds (32-bit fixed point, fix_add), merged with its neighbours' at the end
        [[maybe_unused]] int dif_r = 0, dif_g = 0, dif_b = 0; // SPLIT: the same for the diffuse parts of a depth-1 hit's unshadowed light terms
        [[maybe_unused]] uint32_t dif_pix = 0xffffffffu;
        // children of this hit (emitted after the hit is shaded, by all waves of the workgroup together)
        bool spawn_refl = false, spawn_refr = false;
        float4 c1_r0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), c1_r1 = c1_r0, c2_r0 = c1_r0, c2_r1 = c1_r0;
        uint2 c1_r2 = make_uint2(0u, 0u), c2_r2 = c1_r2;
        uint32_t sum_pix = 0xffffffffu, aux_pix = 0xffffffffu, nf = 0u, pix_of_nf = 0u;
        int aux_nx = 0, aux_ny = 0, aux_nz = 0, aux_d = 0;
        if (active) {
        n_shaded++;
        float4 r0, r1; uint2 r2;
        if (PRIMARY) { // the root node of a path
            f3 po, pd; uint32_t ppix, psmp;
            primary_ray(fr, kc->ps, shade_arg_primary(ka), i, &po, &pd, &ppix, &psmp);
            root_record(po, pd, ppix, psmp, &r0, &r1, &r2);
        } else { r0 = RR_SHADE_ARG(ka, qin.r0)[i]; r1 = RR_SHADE_ARG(ka, qin.r1)[i]; r2 = RR_SHADE_ARG(ka, qin.r2)[i]; }
        const uint32_t pix = __float_as_uint(r1.w);
        pix_of_nf = pix;
        const uint32_t meta = r2.x, node = r2.y;
        const uint32_t sample = meta & 0xffffu, depth = (meta >> 16) & 0xffu;
        const bool idc = ((meta >> 24) & 1u) != 0u;
        const float thr = r0.w;
        const DItem& it = rr_global(sc.items)[item_idx];
        // The item's words and the material, in registers (HitItem, MatR).  A level-1 packet is 64 samples of one pixel: as a rule every hit of
        // it is on ONE item, and then the wave asks for both records once, through the scalar cache -- two dependent requests of a few groups each
        // instead of hit -> item -> material per lane.  Lanes that missed are outside this region and never supply the index.  Packets at an
        // item's edge, of several pixels (sample_group < 64) and all deeper levels load per lane.  One shading body follows either loader.
        HitItem hi; MatR m;
        bool one_item = false;
        if constexpr (PRIMARY) one_item = __ballot(item_idx != __builtin_amdgcn_readfirstlane(item_idx)) == 0ull;
        if (one_item) {
            hi = load_hit_item_uniform(sc.items, item_idx);
            m = load_material_uniform(sc.materials, hi.material, s_lut);
        } else {
            hi = load_hit_item(it);
            m = load_material(&rr_global(sc.materials)[hi.material], s_lut);
        }
        const uint32_t it_flags = hi.flags, it_id = hi.id;
        const f3 ro = mk3(r0.x, r0.y, r0.z), rd = mk3(r1.x, r1.y, r1.z);
        const float hit_dist = __uint_as_float(hit.x);
        const f3 hit_point = ro + (rd * hit_dist);

        // ---- world normal: Shape::intersect (mesh.rs:76-98, sphere.rs:61-65)
        HitWeights hw;
        const f3 normal = hit_normal(sc, it, hi, m, ro, rd, hit_point, hit.z, gw, &hw);
        // ---- aux outputs of the root node (:742-744, :400-402): summed per pixel below, with the wave's other root hits
        if (depth == 1u) {
            aux_pix = pix;
            {   // (a term beyond the 32-bit lane sum is marked and taken in 64 bits with the wave's other wide terms, after the light loop)
                const float dx = hit_dist * RR_DEPTH_SCALE;
                aux_d = rr_abs(dx) < 33554432.0f ? __float2int_rn(dx) : RR_DEPTH_WIDE;
            }
            fix_add_at(aux_nx, normal.x, RR_FIX_SCALE, RR_FIX_CLAMP, normal_plane(0u), pix);
            fix_add_at(aux_ny, normal.y, RR_FIX_SCALE, RR_FIX_CLAMP, normal_plane(1u), pix);
            fix_add_at(aux_nz, normal.z, RR_FIX_SCALE, RR_FIX_CLAMP, normal_plane(2u), pix);
            if ((normal.x - normal.x) + (normal.y - normal.y) + (normal.z - normal.z) + (hit_dist - hit_dist) != 0.0f) { // rare: something is not finite
                if (hit_dist != hit_dist) nf |= RR_NF_DEPTH_NAN;
                if (normal.x != normal.x) nf |= RR_NF_NORMAL_NAN;
                if (normal.y != normal.y) nf |= RR_NF_NORMAL_NAN << 1;
                if (normal.z != normal.z) nf |= RR_NF_NORMAL_NAN << 2;
            }
        }
        // ---- uv (:749-754)
        f2 uv;
        const bool has_uv = hit_uv(it, it_flags, m, hit_point, gw, hw, &uv);
        // ---- normal mapping (:757-784)
        f3 surface_normal = mapped_normal(sc, m, has_uv, uv, normal, flat_frame_entry(hi, hit.z));
        // the generator is keyed on the FRAME pixel (y * width + x), never on the accumulator slot
        const uint32_t xy = RR_SHADE_ARG(ka, slot_xy)[pix];
        RngKey rk; rk.seed_lo = fr.seed_lo; rk.seed_hi = fr.seed_hi;
        rk.pixel = (xy >> 16) * fr.width + (xy & 0xffffu); rk.sample = sample; rk.node = node;
        const bool mc = fr.monte_carlo != 0u && (m.flags & RR_MF_MONTE_CARLO) != 0u;
        // ---- roughness (:787-798)
        {
            float roughness;
            const bool has_rtc = roughness_spread(sc, m, has_uv, uv, &roughness);
            if (mc && (m.roughness > 0.0f || has_rtc))
                surface_normal = jitter(surface_normal, roughness, has_rtc ? rr_cos(roughness * RR_PI_F) : m.cos_roughness, rk, 0u);
        }
        // ---- colours and alpha (:801-811)
        const HitColors col = hit_colors(sc, m, has_uv, uv);
        const float4 ambient_color = col.ambient, base_color = col.base, specular_color = col.specular;
        const float alpha = col.alpha;

        // ---- everything after the light loop that does not depend on it (:922-991)
        const float reflectivity = hit_reflectivity(sc, m, has_uv, uv);
        const bool may_recurse = depth <= fr.max_recursion;
        spawn_refl = reflectivity > 0.0f && may_recurse;
        f3 refr_o = mk3(0.0f, 0.0f, 0.0f), refr_d = mk3(0.0f, 0.0f, 0.0f);
        float a_mul = 1.0f; // the factor `color * alpha` applies to what is already in `color`
        if (alpha < 1.0f && may_recurse) {
            // create_transmission (:500-533)
            f3 ref_n = surface_normal;
            float eta_t = m.refraction_index, eta_i = 1.0f;
            float i_dot_n = dot3(rd, surface_normal);
            if (i_dot_n < 0.0f) { i_dot_n = -i_dot_n; }
            else { ref_n = -surface_normal; eta_t = 1.0f; eta_i = m.refraction_index; }
            float eta = eta_i / eta_t;
            float k = 1.0f - (eta * eta) * (1.0f - i_dot_n * i_dot_n);
            if (!(k < 0.0f)) {
                spawn_refr = true;
                refr_o = hit_point + (ref_n * -0.001f);
                refr_d = ((rd + i_dot_n * ref_n) * eta) - (ref_n * sqrtf(k));
                a_mul = alpha;
            }
        } else if (alpha < 1.0f) {
            a_mul = alpha;
        }
        const float fog_amount = rs_min(fr.fog_density * hit_dist, 1.0f);
        const float ao = hit_ambient_occlusion(sc, m, has_uv, uv);
        const float g = (1.0f - fog_amount) * ao;
        const float w_light = thr * ((1.0f - reflectivity) * a_mul * g);
        const float w_refl = thr * (reflectivity * a_mul * g);
        float w_refr = 0.0f; // only a refraction child carries it: fresnel() is evaluated for the hits that spawn one
        if (spawn_refr) {
            const float kr = fresnel(rd, surface_normal, m.refraction_index);
            w_refr = thr * (((kr < 1.0f) ? ((1.0f - kr) * (1.0f - alpha)) : (1.0f - alpha)) * g);
        }

        // The reference multiplies the light sum by (1 - reflectivity), alpha, (1 - fog) and the AO texel AFTER the light
        // loop (:922-991): a NaN in any of them (a map sampled at a NaN uv: acos beyond 1 at a sphere's pole) poisons the
        // pixel even when the light sum is exactly zero or there is no light at all, where no contribution carries it here.
        if (w_light != w_light) nf |= RR_NF_NAN * 7u;
        // ---- constant part: fog colour and ambient / emissive (:977-994)
        {
            float fa = fog_amount * ao;
            sum_pix = pix;
            const float kr_ = thr * (fr.fog_color[0] * fa + ambient_color.x), kg_ = thr * (fr.fog_color[1] * fa + ambient_color.y), kb_ = thr * (fr.fog_color[2] * fa + ambient_color.z);
            nf |= nonfinite_flags(kr_, kg_, kb_);
            fix_add_at(sum_r, kr_, RR_FIX_SCALE, RR_FIX_CLAMP, rgb_plane(0u), pix); fix_add_at(sum_g, kg_, RR_FIX_SCALE, RR_FIX_CLAMP, rgb_plane(1u), pix);
            fix_add_at(sum_b, kb_, RR_FIX_SCALE, RR_FIX_CLAMP, rgb_plane(2u), pix);
        }
        // ---- object id (:744, :966-969): the last sample's id, passed through fully transparent hits
        const bool child_idc = idc && spawn_refr && approx_equal(alpha, 0.0f);
        if (idc && !child_idc && sample + 1u == fr.samples) {
            uint32_t* const object_id = RR_SHADE_ARG(ka, acc.object_id);
            if (object_id) object_id[pix] = it_id;
        }

        // ---- lights (:814-920)
        const f3 view_dir = normalize3(-rd);
        uint32_t lk = 0xffffffffu; // ordinal among the enabled lights
        for (uint32_t li = 0; li < sc.n_lights; li++) {
            const DLight L = light_uniform(sc.lights, li); // (all three groups are requested before the type is tested)
            if (L.type & 0x80u) continue; // disabled
            lk++;
            const f3 lpos = mk3(L.pos[0], L.pos[1], L.pos[2]), ldir = mk3(L.dir[0], L.dir[1], L.dir[2]);
            f3 to_light;
            if (L.type == 0u) to_light = normalize3(-ldir);
            else to_light = normalize3(lpos - hit_point);
            const float dot_light = rs_max(dot3(surface_normal, to_light), 0.0f);
            const f3 ml = -to_light;
            const f3 reflect_dir = ml - ((2.0f * dot3(surface_normal, ml)) * surface_normal);
            const float spec_dot = rs_max(dot3(reflect_dir, view_dir), 0.0f);
            const float light_power = powf(spec_dot, m.shininess);
            float intensity;
            float limit = RR_FLT_MAX;
            if (L.type == 0u) {
                intensity = L.intensity;
            } else {
                const float r2 = norm3(lpos - hit_point);
                limit = r2;
                intensity = L.intensity / (4.0f * RR_PI_F * r2);
                if (L.type == 2u) {
                    const float dd = dot3(-to_light, normalize3(ldir));
                    if (rr_acos(dd) > L.max_angle) intensity = 0.0f;
                }
            }
            const float cr = ((L.color[0] * (specular_color.x * light_power + base_color.x * dot_light)) * intensity) * w_light;
            const float cg = ((L.color[1] * (specular_color.y * light_power + base_color.y * dot_light)) * intensity) * w_light;
            const float cb = ((L.color[2] * (specular_color.z * light_power + base_color.z * dot_light)) * intensity) * w_light;
            const bool nonzero = (cr != 0.0f) || (cg != 0.0f) || (cb != 0.0f);
            [[maybe_unused]] float dr = 0.0f, dg = 0.0f, db = 0.0f; // SPLIT: the term without its specular summand, for the hits of depth 1
            if constexpr (SPLIT) {
                if (depth == 1u) {
                    dr = ((L.color[0] * (base_color.x * dot_light)) * intensity) * w_light;
                    dg = ((L.color[1] * (base_color.y * dot_light)) * intensity) * w_light;
                    db = ((L.color[2] * (base_color.z * dot_light)) * intensity) * w_light;
                }
            }
            // A light term that is exactly zero stays zero whatever the shadow query says, so its ray is not traced -- unless
            // an occluder with an alpha map exists AND this receiver's uv can be non-finite: the reference samples that map at the
            // RECEIVER's uv of the OCCLUDER's hit point (:905), which for a sphere receiver is acos of a value beyond 1 = NaN (for
            // a mesh receiver: the 0 / 0 area weights of a zero-area face), and 0 * NaN = NaN reaches the pixel (found by
            // tools/fuzz_parity.py: a white pixel in the reference, a dark one here).  Every other receiver's uv is finite, the
            // attenuation is finite, and zero stays zero: a scene with alpha-mapped foliage does not pay for the corner case.
            const bool want_shadow = (m.flags & RR_MF_RECEIVE_SHADOW) != 0u && (nonzero || (sc.any_alpha_occluder != 0u && (it_flags & RR_IF_UV_MAY_BE_NAN) != 0u));
            if (!(m.flags & RR_MF_RECEIVE_SHADOW) && nonzero) {
                nf |= nonfinite_flags(cr, cg, cb);
                fix_add_at(sum_r, cr, RR_FIX_SCALE, RR_FIX_CLAMP, rgb_plane(0u), pix); fix_add_at(sum_g, cg, RR_FIX_SCALE, RR_FIX_CLAMP, rgb_plane(1u), pix);
                fix_add_at(sum_b, cb, RR_FIX_SCALE, RR_FIX_CLAMP, rgb_plane(2u), pix);
                if constexpr (SPLIT) {
                    if (depth == 1u) {
                        dif_pix = pix;
                        fix_add_at(dif_r, dr, RR_FIX_SCALE, RR_FIX_CLAMP, dif_plane(0u), pix); fix_add_at(dif_g, dg, RR_FIX_SCALE, RR_FIX_CLAMP, dif_plane(1u), pix);
                        fix_add_at(dif_b, db, RR_FIX_SCALE, RR_FIX_CLAMP, dif_plane(2u), pix);
                    }
                }
            }
            // Hundreds of unshadowed lights: the 32-bit sums are flushed every 32 enabled lights, whether or not THIS light added a term
            // (inside the branch above a light 31 or 63 with a zero term skipped its flush, and 96 terms can pass 2^31).
            if (!(m.flags & RR_MF_RECEIVE_SHADOW) && (lk & 31u) == 31u) {
                if (sum_r) atomicAdd((unsigned long long*)rgb_plane(0u)() + pix, (unsigned long long)(long long)sum_r);
                if (sum_g) atomicAdd((unsigned long long*)rgb_plane(1u)() + pix, (unsigned long long)(long long)sum_g);
                if (sum_b) atomicAdd((unsigned long long*)rgb_plane(2u)() + pix, (unsigned long long)(long long)sum_b);
                sum_r = sum_g = sum_b = 0;
                if constexpr (SPLIT) {
                    if (dif_r) atomicAdd((unsigned long long*)dif_plane(0u)() + pix, (unsigned long long)(long long)dif_r);
                    if (dif_g) atomicAdd((unsigned long long*)dif_plane(1u)() + pix, (unsigned long long)(long long)dif_g);
                    if (dif_b) atomicAdd((unsigned long long*)dif_plane(2u)() + pix, (unsigned long long)(long long)dif_b);
                    dif_r = dif_g = dif_b = 0;
                }
            }
            const uint32_t si = sq_fixed ? lk * sq_cap + sq_slot : sq_base + wave_alloc(sq_count, want_shadow, lane);
            if (want_shadow) {
                if (sq_fixed) sq_wrote |= 1u << lk; // (fixed slots are only chosen for <= RR_FIXED_SLOT_LIGHTS enabled lights)
                f3 so = hit_point + (surface_normal * 0.001f);
                f3 sd = to_light;
                if (mc) sd = jitter(sd, m.shadow_softness, m.cos_shadow_softness, rk, 1u + li);
                sq.s0[si] = make_float4(so.x, so.y, so.z, limit);
                sq.s1[si] = make_float4(sd.x, sd.y, sd.z, __uint_as_float((uint32_t)item_idx | (depth << 27)));
                sq.s2[si] = make_float4(cr, cg, cb, __uint_as_float(pix));
                if constexpr (SPLIT) sq_s3[si] = make_float4(dr, dg, db, 0.0f); // (zeros for a hit that is not of depth 1)
                n_shadow++;
            }
        }

        // ---- children (:938-971): prepared here, compacted into the next level's queue below
        const uint32_t child_meta = sample | ((depth + 1u) << 16);
        if (spawn_refl) {
            // create_reflection (:492-498)
            f3 o2 = hit_point + (surface_normal * 0.001f);
            f3 d2 = normalize3(rd - ((2.0f * dot3(rd, surface_normal)) * surface_normal));
            c1_r0 = make_float4(o2.x, o2.y, o2.z, w_refl);
            c1_r1 = make_float4(d2.x, d2.y, d2.z, __uint_as_float(pix));
            c1_r2 = make_uint2(child_meta, node * 2u);
            n_secondary++;
        }
        if (spawn_refr) {
            f3 d2 = normalize3(refr_d);
            c2_r0 = make_float4(refr_o.x, refr_o.y, refr_o.z, w_refr);
            c2_r1 = make_float4(d2.x, d2.y, d2.z, __uint_as_float(pix));
            c2_r2 = make_uint2(child_meta | (child_idc ? (1u << 24) : 0u), node * 2u + 1u);
            n_secondary++;
        }
        } // active
        if (sq_fixed) { // which lanes of this packet hold a shadow ray, per enabled light (zero words too: the shadow kernel reads them all)
            const uint32_t pk = (base - chunk_begin) / RR_WAVE, n_pk = sq_cap / RR_WAVE;
            unsigned long long* const sq_valid = RR_SHADE_ARG(ka, sq_valid);
            for (uint32_t k = 0; k < sc.n_enabled_lights; k++) {
                const unsigned long long mk = __ballot((sq_wrote >> k) & 1u);
                if (lane == 0) sq_valid[k * n_pk + pk] = mk;
            }
        }
        if (nf) atomicOr(&RR_SHADE_ARG(ka, acc.flags)[pix_of_nf], nf); // rare: a non-finite term
        const DAccum acc = shade_arg_accum(ka); // the planes of the merges below, in SGPRs from here to the packet's end only
        [[maybe_unused]] DAccum dacc = acc; // SPLIT: the diffuse planes behind the colour planes' own interface (accum_merged_runs)
        if constexpr (SPLIT) dacc.rgb = dif_rgb;
        // One-pixel packets exist on level 1 only, so only the PRIMARY build asks for them (accum_hit_merged: one test, seven wave sums, one
        // atomic instruction); the deeper levels' compacted waves would pay for the test and never pass it.  The SPLIT builds sit at 128
        // VGPRs and spill to scratch with the test in them: they keep the segmented forms too.
        const bool with_aux = (acc.normal || acc.depth) && __ballot(aux_pix != 0xffffffffu) != 0ull;
        if (with_aux && __ballot(aux_d == RR_DEPTH_WIDE) != 0ull) { // hits beyond 512 units: their depth terms in 64 bits, merged per pixel
            long long wide = 0ll;
            if (aux_d == RR_DEPTH_WIDE) { wide = to_fix(__uint_as_float(qin.hit[i].x), RR_DEPTH_SCALE, 1.0e9f); aux_d = 0; }
            if constexpr (SPLIT || !PRIMARY) accum_depth_wide_merged_runs(acc, wide != 0ll ? aux_pix : 0xffffffffu, wide);
            else accum_depth_wide_merged(acc, wide != 0ll ? aux_pix : 0xffffffffu, wide);
        }
        if constexpr (SPLIT || !PRIMARY) {
            accum_merged_runs(acc, sum_pix, sum_r, sum_g, sum_b);
            if constexpr (SPLIT) accum_merged_runs(dacc, dif_pix, dif_r, dif_g, dif_b);
            if (with_aux) accum_aux_merged_runs(acc, aux_pix, aux_nx, aux_ny, aux_nz, aux_d);
        } else if (with_aux) accum_hit_merged(acc, sum_pix, sum_r, sum_g, sum_b, aux_pix, aux_nx, aux_ny, aux_nz, aux_d); // (colour and aux sums in one merge)
        else accum_merged(acc, sum_pix, sum_r, sum_g, sum_b);
        {
            // one allocation for all children of the workgroup iteration: per wave the reflection rays first, then the refraction rays
            const unsigned long long m_refl = __ballot(spawn_refl), m_refr = __ballot(spawn_refr);
            const uint32_t n_refl = (uint32_t)__popcll(m_refl), n_both = n_refl + (uint32_t)__popcll(m_refr);
            if (lane == 0) s_child_n[parity][wave_in_block] = n_both;
            __syncthreads();
            if (threadIdx.x == 0) {
                uint32_t total = 0;
                for (uint32_t w2 = 0; w2 < RR_BLOCK / RR_WAVE; w2++) total += s_child_n[parity][w2];
                s_child_base[parity] = total ? atomicAdd(RR_SHADE_ARG(ka, qout_count), total) : 0u;
            }
            __syncthreads();
            uint32_t obase = s_child_base[parity];
            for (uint32_t w2 = 0; w2 < wave_in_block; w2++) obase += s_child_n[parity][w2];
            const unsigned long long below = (1ull << lane) - 1ull;
            if (spawn_refl) {
                const uint32_t oi = obase + (uint32_t)__popcll(m_refl & below);
                RR_SHADE_ARG(ka, qout.r0)[oi] = c1_r0; RR_SHADE_ARG(ka, qout.r1)[oi] = c1_r1; RR_SHADE_ARG(ka, qout.r2)[oi] = c1_r2;
            }
            if (spawn_refr) {
                const uint32_t oi = obase + n_refl + (uint32_t)__popcll(m_refr & below);
                RR_SHADE_ARG(ka, qout.r0)[oi] = c2_r0; RR_SHADE_ARG(ka, qout.r1)[oi] = c2_r1; RR_SHADE_ARG(ka, qout.r2)[oi] = c2_r2;
            }
        }
    }
    // per-wave reduction of the work counters
    for (int off = 32; off > 0; off >>= 1) {
        n_shaded += __shfl_down(n_shaded, off);
        n_shadow += __shfl_down(n_shadow, off);
        n_secondary += __shfl_down(n_secondary, off);
    }
    if (lane == 0) {
        unsigned long long* const counters = RR_SHADE_ARG(kernarg_segment(), counters);
        if (n_shaded) atomicAdd(&counters[RR_CNT_SHADED], (unsigned long long)n_shaded);
        if (n_shadow) atomicAdd(&counters[RR_CNT_SHADOW], (unsigned long long)n_shadow);
        if (n_secondary) atomicAdd(&counters[RR_CNT_SECONDARY], (unsigned long long)n_secondary);
    }
}

// The flat world normals of every mesh item (DSceneView::flat_normals): one workgroup per item, both signs of every triangle's
// normal through the item's transform.  Run at scene creation and after rr_scene_update_transforms.
// One workgroup per CHUNK of an item's triangles (`chunks`: (item, first triangle) per workgroup, RR_ITEM_CHUNK triangles each, laid out by
// rr_scene_create: a mesh of a million triangles is 123 workgroups, not one).
#define RR_ITEM_CHUNK 8192u
// Triangle `slot` of mesh item `it`: both signs of its flat normal through the item's transform, each with its tangent frame
RR_DEV void flat_world_entry(f3 n, float4* e) {
    const TangentFrame f = tangent_frame(n);
    e[0] = make_float4(n.x, n.y, n.z, 0.0f);
    e[1] = make_float4(f.tangent.x, f.tangent.y, f.tangent.z, 0.0f);
    e[2] = make_float4(f.bitangent.x, f.bitangent.y, f.bitangent.z, 0.0f);
}
RR_DEV void flat_world_normals(const DItem& it, uint32_t slot, const DTri* tris, float4* out) {
    const float4 v3 = tris[it.tri_base + slot].v3;
    const f3 ng = mk3(v3.x, v3.y, v3.z);
    float4* const e = out + (uint64_t)(it.wn_base + 2u * slot) * RR_FLAT_ENTRY_F4;
    flat_world_entry(to_world_normal(it, ng), e);
    flat_world_entry(to_world_normal(it, -ng), e + RR_FLAT_ENTRY_F4);
}
__global__ __launch_bounds__(RR_BLOCK) void k_world_normals(const DItem* __restrict__ items, const uint2* __restrict__ chunks, const DTri* __restrict__ tris, float4* __restrict__ out) {
    const uint2 ch = chunks[blockIdx.x];
    const DItem& it = items[ch.x];
    if (it.flags & RR_IF_SPHERE) return;
    const uint32_t end = min(it.n_tris, ch.y + RR_ITEM_CHUNK);
    for (uint32_t slot = ch.y + threadIdx.x; slot < end; slot += blockDim.x) flat_world_normals(it, slot, tris, out);
}

// The flat world normals of an EDITED item list (rr_scene_set_items), into the new arena: one workgroup per chunk of the new chunk
// map, as k_world_normals.  An item whose matrices, mesh records and flag word are bit for bit those of an item of the list before
// (rr_scene_build.h: plan_item_reuse) takes that item's normals -- chunk_src[chunk] = the old item's wn_base: the chunk's run of
// 2 * triangles entries is copied from `old` at the same offset behind that base -- and every other chunk (RR_CHUNK_DERIVE) evaluates
// them as k_world_normals does.  The copied bits are those the evaluation gives: it is a pure function of what was compared.
// The host bounds both runs: a kept item has the triangle count of the old one, whose run lies inside the old arena.
#define RR_CHUNK_DERIVE 0xffffffffu // never a wn_base: bases are even
__global__ __launch_bounds__(RR_BLOCK) void k_world_normals_edit(const DItem* __restrict__ items, const uint2* __restrict__ chunks, const uint32_t* __restrict__ chunk_src,
                                                                 const DTri* __restrict__ tris, const float4* __restrict__ old, float4* __restrict__ out) {
    const uint2 ch = chunks[blockIdx.x];
    const DItem& it = items[ch.x];
    if (it.flags & RR_IF_SPHERE) return;
    const uint32_t end = min(it.n_tris, ch.y + RR_ITEM_CHUNK);
    const uint32_t src = chunk_src[blockIdx.x];
    if (src != RR_CHUNK_DERIVE) {
        const uint64_t per_tri = 2ull * RR_FLAT_ENTRY_F4, to = (uint64_t)it.wn_base * RR_FLAT_ENTRY_F4, from = (uint64_t)src * RR_FLAT_ENTRY_F4;
        for (uint64_t k = per_tri * ch.y + threadIdx.x; k < per_tri * end; k += blockDim.x) out[to + k] = old[from + k];
        return;
    }
    for (uint32_t slot = ch.y + threadIdx.x; slot < end; slot += blockDim.x) flat_world_normals(it, slot, tris, out);
}

// The extent of every mesh item's SURFACE along the rows of its transform (rr_scene_build.h: exact_world_box): one workgroup per item over
// the vertices of the mesh's triangles, which are resident (DTri), in double -- per row r the minimum and maximum of
// tr_r.x * p.x + tr_r.y * p.y + tr_r.z * p.z, and the largest |coordinate| per local axis.  Products and sums are IEEE binary64
// without contraction and minimum / maximum are exact, so the host evaluation this replaces (one thread, every vertex of every
// item, three passes: a transform update of sponza_syn spent its time there) gives the same numbers.  A non-finite vertex makes a
// span non-finite; the host then keeps the box of the local box's corners for that item.
// One workgroup per chunk of an item's triangles, as k_world_normals; the host takes the minimum / maximum over an item's chunks.
// out[9 * chunk + (0..2)] = minima, (3..5) = maxima, (6..8) = largest |coordinate|; spheres and empty meshes: +inf / -inf / 0.
__global__ __launch_bounds__(RR_BLOCK) void k_item_spans(const DItem* __restrict__ items, const uint2* __restrict__ chunks, const DTri* __restrict__ tris, double* __restrict__ out) {
    const uint2 ch = chunks[blockIdx.x];
    const DItem& it = items[ch.x];
    const bool mesh = !(it.flags & RR_IF_SPHERE);
    const double inf = __builtin_inf();
    double lo[3] = {inf, inf, inf}, hi[3] = {-inf, -inf, -inf}, ext[3] = {0.0, 0.0, 0.0};
    bool bad = false; // a NaN coordinate (minimum / maximum would drop it)
    if (mesh) {
        const double m[3][3] = {{(double)it.tr0.x, (double)it.tr0.y, (double)it.tr0.z}, {(double)it.tr1.x, (double)it.tr1.y, (double)it.tr1.z},
                                {(double)it.tr2.x, (double)it.tr2.y, (double)it.tr2.z}};
        const uint32_t end = min(it.n_tris, ch.y + RR_ITEM_CHUNK);
        for (uint32_t slot = ch.y + threadIdx.x; slot < end; slot += RR_BLOCK) {
            const DTri& t = tris[it.tri_base + slot];
            const float4 vs[3] = {t.v0, t.v1, t.v2};
#pragma unroll
            for (int k = 0; k < 3; k++) {
                const double p[3] = {(double)vs[k].x, (double)vs[k].y, (double)vs[k].z};
                if (p[0] != p[0] || p[1] != p[1] || p[2] != p[2]) bad = true;
#pragma unroll
                for (int r = 0; r < 3; r++) {
                    const double v = m[r][0] * p[0] + m[r][1] * p[1] + m[r][2] * p[2];
                    lo[r] = fmin(lo[r], v); hi[r] = fmax(hi[r], v);
                    ext[r] = fmax(ext[r], fabs(p[r]));
                }
            }
        }
    }
    __shared__ double s_red[RR_BLOCK / RR_WAVE][9];
    __shared__ int s_bad;
    if (threadIdx.x == 0) s_bad = 0;
    __syncthreads();
    if (bad) s_bad = 1;
#pragma unroll
    for (int r = 0; r < 3; r++)
        for (int off = 32; off > 0; off >>= 1) {
            lo[r] = fmin(lo[r], __shfl_down(lo[r], off)); hi[r] = fmax(hi[r], __shfl_down(hi[r], off)); ext[r] = fmax(ext[r], __shfl_down(ext[r], off));
        }
    if ((threadIdx.x & (RR_WAVE - 1)) == 0)
        for (int r = 0; r < 3; r++) { s_red[threadIdx.x / RR_WAVE][r] = lo[r]; s_red[threadIdx.x / RR_WAVE][3 + r] = hi[r]; s_red[threadIdx.x / RR_WAVE][6 + r] = ext[r]; }
    __syncthreads();
    if (threadIdx.x < 9) {
        const int k = (int)threadIdx.x;
        double v = s_red[0][k];
        for (int w = 1; w < RR_BLOCK / RR_WAVE; w++) v = k < 3 ? fmin(v, s_red[w][k]) : fmax(v, s_red[w][k]);
        if (s_bad) v = __builtin_nan("");
        out[9ull * blockIdx.x + k] = v;
    }
}

// ---------------------------------------------------------------------------
// kernel 4: shadow rays of one shade chunk (reference src/raytracing.rs:872-914)
// ---------------------------------------------------------------------------
// FIXED (level 1): packet p = the shadow rays of hit packet (p % packets per light) towards enabled light (p / packets per
// light), slots p * 64 .. p * 64 + 63, lanes by sq_valid[p]; n_packets given.  Otherwise the dense sharded queue of the
// deeper levels (k_shade), n_packets from the shard counts.
// SPLIT (rr_render_pixel_split, level 1): sq_s3[i] is the diffuse part of ray i's term (k_shade<true, true>); it is scaled by the ray's
// factor and summed in the planes `diffuse` as the term itself is in acc.rgb, in the same packet pass.
template <bool FIXED, bool SPLIT = false, class... Split>
__global__ __launch_bounds__(RR_BLOCK, RR_SHADOW_WAVES) void k_trace_shadow(DSceneView sc, DShadowQueue sq, const uint32_t* __restrict__ sq_counts, uint32_t sq_segcap,
                                                           const unsigned long long* __restrict__ sq_valid, uint32_t n_fixed_packets,
                                                           uint32_t* head, DAccum acc, Split... split) {
    static_assert(sizeof...(Split) == (SPLIT ? 2 : 0), "the SPLIT builds take (long long* diffuse, const float4* sq_s3), the others nothing");
    DAccum dacc = acc;
    [[maybe_unused]] const float4* const sq_s3 = split_queue(split...);
    if constexpr (SPLIT) dacc.rgb = split_planes(split...);
    __shared__ int s_stack[RR_STACK_DEPTH * RR_BLOCK];
    __shared__ uint32_t s_prefix[RR_SQ_SHARDS + 1];
    RR_UTIL_KIND(2u)
    uint32_t n = 0;
    if (!FIXED) { // dense index space over the shards: prefix sums of their counts
        if (threadIdx.x < RR_WAVE) {
            uint32_t c = threadIdx.x < RR_SQ_SHARDS ? sq_counts[threadIdx.x * RR_SQ_STRIDE] : 0u;
            uint32_t incl = c;
            for (int off = 1; off < RR_SQ_SHARDS; off <<= 1) { uint32_t v = __shfl_up(incl, off); if ((int)threadIdx.x >= off) incl += v; }
            if (threadIdx.x < RR_SQ_SHARDS) s_prefix[threadIdx.x + 1] = incl;
            if (threadIdx.x == 0) s_prefix[0] = 0u;
        }
        __syncthreads();
        n = s_prefix[RR_SQ_SHARDS];
    }
    const uint32_t n_packets = FIXED ? n_fixed_packets : (n + RR_WAVE - 1) / RR_WAVE;
    const uint32_t lane = threadIdx.x & (RR_WAVE - 1);
    const bool gw = sc.general_w != 0u;
    // (level 1's aligned packets cost much the same and are mostly dealt statically; the dense queue of the deeper levels keeps half dynamic)
    PacketStream stream(n_packets, FIXED ? RR_SHADOW_FIXED_STATIC_NUM : RR_SHADOW_STATIC_NUM, FIXED ? RR_SHADOW_FIXED_STATIC_DEN : RR_SHADOW_STATIC_DEN, head);
    for (uint32_t p; stream.next(&p);) {
        unsigned long long valid;
        if (FIXED) valid = sq_valid[p]; // (the same word in every lane)
        else { const uint32_t left = n - p * RR_WAVE; valid = left >= RR_WAVE ? ~0ull : (1ull << left) - 1ull; }
        if (valid == 0ull) continue;
        {
        int sum_r = 0, sum_g = 0, sum_b = 0;
        [[maybe_unused]] int dif_r = 0, dif_g = 0, dif_b = 0;
        uint32_t sum_pix = 0xffffffffu;
        const bool live = ((valid >> lane) & 1ull) != 0ull;
        {
            // lanes without a ray repeat the packet's first one (the packet form runs with all lanes) and add nothing
            const uint32_t j = p * RR_WAVE + (live ? lane : (uint32_t)__ffsll((long long)valid) - 1u);
            uint32_t i = j;
            if (!FIXED) {
                uint32_t lo = 0, hi = RR_SQ_SHARDS; // largest shard with prefix <= j
                while (hi - lo > 1u) { uint32_t mid = (lo + hi) >> 1; if (s_prefix[mid] <= j) lo = mid; else hi = mid; }
                i = lo * sq_segcap + (j - s_prefix[lo]);
            }
            const float4 s0 = sq.s0[i];
            const float4 s1 = sq.s1[i], s2 = sq.s2[i];
            [[maybe_unused]] float4 s3 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if constexpr (SPLIT) s3 = sq_s3[i];
            const uint32_t rcv_item = __float_as_uint(s1.w) & 0x07ffffffu, rcv_depth = __float_as_uint(s1.w) >> 27;
            const f3 o = mk3(s0.x, s0.y, s0.z), d = mk3(s1.x, s1.y, s1.z);
            ShadowSel sel;
            if (!FIXED || !trace_shadow_packet(sc, o, d, rcv_depth, s0.w, s_stack, &sel)) { if (live) trace_shadow_ray(sc, o, d, rcv_depth, s0.w, s_stack, &sel); }
            if (live) {
            const bool occluded = sel.found && sel.within;
            float factor = 1.0f;
            if (occluded) {
                const DItem& occ = rr_global(sc.items)[sel.item];
                // the RECEIVER's material.alpha (:898); the 2022-05 binary took the occluder's (RR_COMPAT_OCCLUDER_ALPHA_SHADOWS, wave-uniform)
                float shadow_source_alpha = rr_global(sc.materials)[(sc.compat & 1u) ? occ.material : rr_global(sc.items)[rcv_item].material].alpha;
                if (occ.flags & RR_IF_OCCLUDER_ALPHA_TEX) {
                    // the reference evaluates the RECEIVER's get_uv with the occluder's face id (:905)
                    const DItem& rcv = rr_global(sc.items)[rcv_item];
                    const f3 shp = o + (d * sel.t);
                    f2 uv;
                    if (rcv.flags & RR_IF_SPHERE) uv = sphere_uv(rcv, shp, gw);
                    else if (rcv.n_tris != 0u) uv = mesh_uv(sc, rcv, rr_global(sc.face_slot)[rcv.tri_base + sel.face % rcv.n_tris], shp, gw);
                    else { uv.x = 0.0f; uv.y = 0.0f; }
                    float4 tc;
                    if (tex_color(sc, rr_global(sc.materials)[occ.material], true, uv, 4, &tc)) shadow_source_alpha *= tc.x;
                }
                factor = 1.0f - shadow_source_alpha;
            }
            sum_pix = __float_as_uint(s2.w);
            const float vr_ = s2.x * factor, vg_ = s2.y * factor, vb_ = s2.z * factor;
            const uint32_t nf = nonfinite_flags(vr_, vg_, vb_);
            fix_add(sum_r, vr_, RR_FIX_SCALE, RR_FIX_CLAMP, acc.rgb, sum_pix); fix_add(sum_g, vg_, RR_FIX_SCALE, RR_FIX_CLAMP, acc.rgb + acc.n, sum_pix);
            fix_add(sum_b, vb_, RR_FIX_SCALE, RR_FIX_CLAMP, acc.rgb + 2ull * acc.n, sum_pix);
            if (nf) atomicOr(&acc.flags[sum_pix], nf);
            if constexpr (SPLIT) {
                fix_add(dif_r, s3.x * factor, RR_FIX_SCALE, RR_FIX_CLAMP, dacc.rgb, sum_pix); fix_add(dif_g, s3.y * factor, RR_FIX_SCALE, RR_FIX_CLAMP, dacc.rgb + dacc.n, sum_pix);
                fix_add(dif_b, s3.z * factor, RR_FIX_SCALE, RR_FIX_CLAMP, dacc.rgb + 2ull * dacc.n, sum_pix);
            }
            }
        }
        // (fixed slots: a packet is the shadow rays of one pixel's hits, and asks for the one-pixel form; the dense queue's packets are
        // compacted, and the SPLIT builds spill to scratch with the test in them: both keep the segmented form)
        if constexpr (FIXED && !SPLIT) accum_merged(acc, sum_pix, sum_r, sum_g, sum_b);
        else accum_merged_runs(acc, sum_pix, sum_r, sum_g, sum_b);
        if constexpr (SPLIT) accum_merged_runs(dacc, sum_pix, dif_r, dif_g, dif_b);
        }
    }
}

// ---------------------------------------------------------------------------
// kernel 4b: shadow QUERIES for caller-supplied rays (rr_trace_shadow_rays): Raytracing::trace(ray, true, true, depth) and
// `in_light = toi > len` (reference src/raytracing.rs:429-490, :883-892), with no receiver and no colour
// ---------------------------------------------------------------------------
// Ray i: r0[i] = (origin, limit), r1[i] = (direction, depth as bits).  Packet p = rays 64 p .. 64 p + 63 in the caller's order.
// The decision is k_trace_shadow's own: trace_shadow_packet where the scene has a packet form and the packet is coherent,
// trace_shadow_ray otherwise.  out[i] = (toi bits, deciding item, reference face id, occluded) -- (0, 0xffffffff, 0, 0) for a ray
// that is lit -- written once per ray with one 16-byte vector store.
__global__ __launch_bounds__(RR_BLOCK, RR_SHADOW_WAVES) void k_query_shadow(DSceneView sc, const float4* __restrict__ r0, const float4* __restrict__ r1, uint32_t n,
                                                           uint32_t* head, uint4* __restrict__ out) {
    __shared__ int s_stack[RR_STACK_DEPTH * RR_BLOCK];
    RR_UTIL_KIND(2u)
    const uint32_t n_packets = (n + RR_WAVE - 1) / RR_WAVE;
    const uint32_t lane = threadIdx.x & (RR_WAVE - 1);
    PacketStream stream(n_packets, RR_SHADOW_STATIC_NUM, RR_SHADOW_STATIC_DEN, head); // the static share of k_trace_shadow's dense queue
    for (uint32_t p; stream.next(&p);) {
        const uint32_t i = p * RR_WAVE + lane;
        const bool live = i < n;
        // lanes past the end repeat the packet's first ray (the packet form runs with all lanes) and write nothing
        const uint32_t j = live ? i : p * RR_WAVE;
        const float4 s0 = r0[j], s1 = r1[j];
        const f3 o = mk3(s0.x, s0.y, s0.z), d = mk3(s1.x, s1.y, s1.z);
        const uint32_t depth = __float_as_uint(s1.w);
        ShadowSel sel;
        if (!trace_shadow_packet(sc, o, d, depth, s0.w, s_stack, &sel)) trace_shadow_ray(sc, o, d, depth, s0.w, s_stack, &sel);
        const bool occluded = sel.found && sel.within;
        if (occluded) shadow_deciding_hit(sc, o, d, s_stack, &sel);
        if (live) out[i] = occluded ? make_uint4(__float_as_uint(sel.t), (uint32_t)sel.item, sel.face, 1u) : make_uint4(0u, 0xffffffffu, 0u, 0u);
    }
}

// ---------------------------------------------------------------------------
// ray binning between depth levels (counting sort of a level's rays by origin cell x direction octant)
//
// OFF by default (rr_tuning::bin_min_rays).  A deeper level's rays can be re-ordered before they are traced so that a
// wave holds rays that start in the same cell of an 8 x 8 x 8 grid over the level's origins and point into the same
// octant: bounds -> histogram -> prefix -> scatter, 4096 bins.  The order of rays never changes a bit of the frame
// (fixed-point accumulators), so the sort may be unstable: positions inside a bin come from an atomic cursor.
// Measured: it does not pay on this renderer's rays.  Children are spawned in the order of their parents,
// and a packet of parents is 64 samples of ONE pixel: the children of a wave already share their origin to within a
// pixel footprint and differ only by the roughness jitter of their normals (up to +-28 degrees on helmet_syn), which
// no bin of practical size separates.  helmet_syn deeper levels: node steps 21.5 -> 23.1 active lanes of 64, triangle
// tests 11.8 -> 12.9, closest-hit time -2 %, for +2.4 ms of sorting; lotus_syn (refraction, no jitter) gets slower.
// ---------------------------------------------------------------------------
#define RR_BIN_AXIS 8u
#define RR_BIN_COUNT (RR_BIN_AXIS * RR_BIN_AXIS * RR_BIN_AXIS * 8u)
RR_DEV int float_ordered(float f) { const int i = __float_as_int(f); return i ^ ((i >> 31) & 0x7fffffff); } // monotone map f32 -> i32
RR_DEV float ordered_float(int i) { return __int_as_float(i ^ ((i >> 31) & 0x7fffffff)); }

// bounds[0..2] = min, bounds[3..5] = max of the finite ray origins, as ordered ints (host presets +max / -max)
__global__ __launch_bounds__(RR_BLOCK) void k_bin_bounds(DRayQueue q, uint32_t n, int* bounds) {
    float lo[3] = {RR_FLT_MAX, RR_FLT_MAX, RR_FLT_MAX}, hi[3] = {-RR_FLT_MAX, -RR_FLT_MAX, -RR_FLT_MAX};
    for (uint32_t i = blockIdx.x * RR_BLOCK + threadIdx.x; i < n; i += gridDim.x * RR_BLOCK) {
        const float4 r0 = q.r0[i];
        const float o[3] = {r0.x, r0.y, r0.z};
#pragma unroll
        for (int k = 0; k < 3; k++)
            if (rr_abs(o[k]) <= RR_FLT_MAX) { lo[k] = fminf(lo[k], o[k]); hi[k] = fmaxf(hi[k], o[k]); }
    }
#pragma unroll
    for (int k = 0; k < 3; k++) {
        for (int off = 32; off > 0; off >>= 1) { lo[k] = fminf(lo[k], __shfl_down(lo[k], off)); hi[k] = fmaxf(hi[k], __shfl_down(hi[k], off)); }
        if ((threadIdx.x & 63u) == 0u) { atomicMin(&bounds[k], float_ordered(lo[k])); atomicMax(&bounds[3 + k], float_ordered(hi[k])); }
    }
}
RR_DEV uint32_t bin_cell(float o, float lo, float inv_step) { // NaN -> 0
    const float c = fminf(fmaxf((o - lo) * inv_step, 0.0f), (float)(RR_BIN_AXIS - 1u));
    return (uint32_t)c;
}
RR_DEV uint32_t spread3(uint32_t v) { return (v & 1u) | ((v & 2u) << 2) | ((v & 4u) << 4); } // 3 bits -> every third bit
RR_DEV uint32_t bin_key(float4 r0, float4 r1, const int* __restrict__ bounds) {
    const float lx = ordered_float(bounds[0]), ly = ordered_float(bounds[1]), lz = ordered_float(bounds[2]);
    const float ex = ordered_float(bounds[3]) - lx, ey = ordered_float(bounds[4]) - ly, ez = ordered_float(bounds[5]) - lz;
    const float sx = ex > 0.0f ? (float)RR_BIN_AXIS / ex : 0.0f, sy = ey > 0.0f ? (float)RR_BIN_AXIS / ey : 0.0f, sz = ez > 0.0f ? (float)RR_BIN_AXIS / ez : 0.0f;
    const uint32_t cell = spread3(bin_cell(r0.x, lx, sx)) | (spread3(bin_cell(r0.y, ly, sy)) << 1) | (spread3(bin_cell(r0.z, lz, sz)) << 2); // Morton order
    const uint32_t oct = (__float_as_uint(r1.x) >> 31) | ((__float_as_uint(r1.y) >> 31) << 1) | ((__float_as_uint(r1.z) >> 31) << 2);
    return (cell << 3) | oct;
}
// One add per DISTINCT key of a wave instead of one per lane (neighbouring rays mostly share their bin, and 64 lanes
// adding to one word serialise): the lanes are peeled off key by key; returns this lane's slot when `ret`.
RR_DEV uint32_t wave_add_by_key(uint32_t* table, uint32_t key, bool valid, bool ret) {
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t slot = 0u;
    unsigned long long todo = __ballot(valid);
    while (todo != 0ull) {
        const int leader = __ffsll((long long)todo) - 1;
        const uint32_t k = (uint32_t)__shfl((int)key, leader);
        const unsigned long long same = __ballot(valid && key == k);
        uint32_t base = 0u;
        if ((int)lane == leader) base = atomicAdd(&table[k], (uint32_t)__popcll(same));
        if (ret) { base = (uint32_t)__shfl((int)base, leader); if (valid && key == k) slot = base + (uint32_t)__popcll(same & ((1ull << lane) - 1ull)); }
        todo &= ~same;
    }
    return slot;
}
// keys into the (still unused) hit records of the level, histogram through LDS
__global__ __launch_bounds__(RR_BLOCK) void k_bin_count(DRayQueue q, uint32_t n, const int* __restrict__ bounds, uint32_t* hist) {
    __shared__ uint32_t s_hist[RR_BIN_COUNT];
    for (uint32_t b = threadIdx.x; b < RR_BIN_COUNT; b += RR_BLOCK) s_hist[b] = 0u;
    __syncthreads();
    const uint32_t n_up = ((n + RR_BLOCK - 1) / RR_BLOCK) * RR_BLOCK; // whole waves take part in the peeling loop
    for (uint32_t i = blockIdx.x * RR_BLOCK + threadIdx.x; i < n_up; i += gridDim.x * RR_BLOCK) {
        uint32_t key = 0u;
        if (i < n) { key = bin_key(q.r0[i], q.r1[i], bounds); q.hit[i] = make_uint4(key, 0u, 0u, 0u); }
        wave_add_by_key(s_hist, key, i < n, false);
    }
    __syncthreads();
    for (uint32_t b = threadIdx.x; b < RR_BIN_COUNT; b += RR_BLOCK) { const uint32_t c = s_hist[b]; if (c) atomicAdd(&hist[b], c); }
}
// exclusive prefix of the histogram, in place (one workgroup of 1024 threads, 4 bins each)
__global__ __launch_bounds__(1024) void k_bin_prefix(uint32_t* hist) {
    __shared__ uint32_t s_part[1024];
    const uint32_t t = threadIdx.x;
    uint32_t v[RR_BIN_COUNT / 1024], sum = 0;
#pragma unroll
    for (uint32_t k = 0; k < RR_BIN_COUNT / 1024; k++) { v[k] = hist[t * (RR_BIN_COUNT / 1024) + k]; sum += v[k]; }
    s_part[t] = sum;
    __syncthreads();
    for (uint32_t off = 1; off < 1024; off <<= 1) { // Hillis-Steele inclusive scan
        const uint32_t add = t >= off ? s_part[t - off] : 0u;
        __syncthreads();
        s_part[t] += add;
        __syncthreads();
    }
    uint32_t run = s_part[t] - sum;
#pragma unroll
    for (uint32_t k = 0; k < RR_BIN_COUNT / 1024; k++) { hist[t * (RR_BIN_COUNT / 1024) + k] = run; run += v[k]; }
}
// every ray takes the next free slot of its bin (`cursor` = the exclusive prefix, advanced atomically)
__global__ __launch_bounds__(RR_BLOCK) void k_bin_scatter(DRayQueue src, DRayQueue dst, uint32_t n, uint32_t* cursor) {
    const uint32_t n_up = ((n + RR_BLOCK - 1) / RR_BLOCK) * RR_BLOCK;
    for (uint32_t i = blockIdx.x * RR_BLOCK + threadIdx.x; i < n_up; i += gridDim.x * RR_BLOCK) {
        const uint32_t pos = wave_add_by_key(cursor, i < n ? src.hit[i].x : 0u, i < n, true);
        if (i < n) { dst.r0[pos] = src.r0[i]; dst.r1[pos] = src.r1[i]; dst.r2[pos] = src.r2[i]; }
    }
}

// ---------------------------------------------------------------------------
// kernel 5: resolve accumulators into PixelData (reference src/raytracing.rs:406-426)
// ---------------------------------------------------------------------------
// The four bytes of a frame's pixel from the resolved, unclamped colour (:410-424): f32::min (NaN.min(1.0) = 1.0), the gamma curve when
// the config asks for it, truncation to u8, alpha 255.  k_resolve and k_resolve_pixels both write what this returns.
RR_DEV uint32_t frame_bytes(const float* color, uint32_t gamma) {
    float c[3];
#pragma unroll
    for (int k = 0; k < 3; k++) c[k] = rs_min(color[k], 1.0f);
    uint32_t r, g, b;
    if (gamma) {
        const float ig = 1.0f / 2.2f;
        r = as_u8(powf(c[0], ig) * 255.0f); g = as_u8(powf(c[1], ig) * 255.0f); b = as_u8(powf(c[2], ig) * 255.0f);
    } else {
        r = as_u8(c[0] * 255.0f); g = as_u8(c[1] * 255.0f); b = as_u8(c[2] * 255.0f);
    }
    return r | (g << 8) | (b << 16) | (255u << 24);
}

__global__ __launch_bounds__(RR_BLOCK) void k_resolve(DFrame fr, const uint32_t* __restrict__ slot_xy,
                                                      const uint32_t* __restrict__ slot_out, DAccum acc,
                                                      uint8_t* rgba8, float* normal, float* depth, uint32_t* object_id,
                                                      uint32_t frame_layout) {
    uint32_t p = blockIdx.x * blockDim.x + threadIdx.x; // accumulator slot
    if (p >= fr.n_region_pixels) return;
    uint32_t o;
    if (frame_layout) o = frame_index(slot_xy[p], fr.width);
    else o = slot_out[p]; // position in the region's compact output order
    const float n = (float)fr.samples;
    const uint32_t nf = acc.flags[p];
    float c[3];
#pragma unroll
    for (int k = 0; k < 3; k++) c[k] = resolve_color(acc, p, nf, k, n);
    ((uint32_t*)rgba8)[o] = frame_bytes(c, fr.gamma);
    if (normal && acc.normal) {
        const f3 nn = resolve_normal(acc, p, nf, n);
        normal[3ull * o] = nn.x; normal[3ull * o + 1] = nn.y; normal[3ull * o + 2] = nn.z;
    }
    if (depth && acc.depth) depth[o] = resolve_depth(acc, p, nf, n);
    if (object_id && acc.object_id) object_id[o] = acc.object_id[p];
}

// ---------------------------------------------------------------------------
// kernels 5b, 5c: caller-supplied rays as depth level 1 (rr_shade_rays): get_color_depth_normal_id(scene, ray, 1) per ray
// ---------------------------------------------------------------------------
// One batch of the caller's rays -> level-1 RECORDS at the front of the ray arena: root_record, as for a frame's primary ray.
// Record i is the caller's ray first + i = sample (first + i) % rays_per_result of result (first + i) / rays_per_result, whose
// accumulator slot is the result's index: the samples of a result sit in neighbouring lanes and accum_merged merges their adds.
// origins / dirs: the batch's 3 n floats each.  The direction is normalised as primary_ray does it (get_color_depth_normal_id, :723).
// Thread 0 publishes the level's size and counts the rays.
__global__ __launch_bounds__(RR_BLOCK) void k_seed_rays(const float* __restrict__ origins, const float* __restrict__ dirs, unsigned long long first, uint32_t n,
                                                        uint32_t rays_per_result, DRayQueue q, uint32_t* __restrict__ q_count, unsigned long long* counters) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i == 0u) { *q_count = n; atomicAdd(&counters[RR_CNT_PRIMARY], (unsigned long long)n); }
    if (i >= n) return;
    const unsigned long long g = first + i;
    const uint32_t slot = (uint32_t)(g / rays_per_result), sample = (uint32_t)(g % rays_per_result);
    const f3 d = normalize3(mk3(dirs[3ull * i], dirs[3ull * i + 1], dirs[3ull * i + 2]));
    root_record(mk3(origins[3ull * i], origins[3ull * i + 1], origins[3ull * i + 2]), d, slot, sample, &q.r0[i], &q.r1[i], &q.r2[i]);
}

// What k_resolve computes BEFORE its clamp, per accumulator slot [first, first + n): two float4 per result =
// (colour rgb, depth), (normal xyz, bits(object id)) -- rr_radiance: resolve_record (rr_accumulate.h).
__global__ __launch_bounds__(RR_BLOCK) void k_resolve_rays(DAccum acc, uint32_t first, uint32_t n, uint32_t samples, float4* __restrict__ out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    store_record(out, i, resolve_record(acc, first + i, (float)samples));
}

// ---------------------------------------------------------------------------
// kernels 5i, 5j: the frame's camera for pixels of the caller's choice, ending in floats (rr_render_pixels)
// ---------------------------------------------------------------------------
// 5i: the caller's pixel list on the device -> the handle's slot table: entry i becomes accumulator slot i (slot_xy[i], and its centre
// slot_c[i] = pixel_centre, rr_pixel_list.h: what primary_slot_centres writes for a region's slot).  One entry per lane, grid-stride:
// a wave instruction reads 256 consecutive bytes and writes 256 and 512.  *first_bad: the first index whose pixel lies outside the
// frame (the host presets 0xffffffff); one atomicMin per wave that has one to report, as reach_merge does for the limits.  Such an
// entry is copied like any other -- its centre is plain arithmetic -- and the host refuses the call before a walk reads the table.
// With parts (rr_render_pixel_parts, lg_parts > 0) entry i becomes the K = 2^lg_parts slots i * K .. i * K + K - 1, all with the entry's pixel
// and centre: K neighbouring lanes read one word and every store stays as wide as it was.
RR_DEV void first_bad_merge(uint32_t bad, uint32_t* __restrict__ first_bad) { // every lane's first bad index (0xffffffff = none) -> *first_bad
#pragma unroll
    for (int off = RR_WAVE / 2; off > 0; off >>= 1) bad = min(bad, (uint32_t)__shfl_xor((int)bad, off));
    if ((threadIdx.x & (RR_WAVE - 1)) == 0u && bad != 0xffffffffu) atomicMin(first_bad, bad);
}
__global__ __launch_bounds__(RR_BLOCK) void k_pixel_slots(const uint32_t* __restrict__ pixel_xy, uint32_t n, uint32_t lg_parts, uint32_t width, uint32_t height,
                                                          uint32_t* __restrict__ slot_xy, float2* __restrict__ slot_c, uint32_t* __restrict__ first_bad) {
    const float w = (float)width, h = (float)height;
    const unsigned long long n_slots = (unsigned long long)n << lg_parts; // <= 2^30 (the host)
    uint32_t bad = 0xffffffffu;
    for (unsigned long long j = (unsigned long long)blockIdx.x * RR_BLOCK + threadIdx.x; j < n_slots; j += (unsigned long long)gridDim.x * RR_BLOCK) {
        const uint32_t i = (uint32_t)(j >> lg_parts);
        const uint32_t xy = pixel_xy[i];
        if (!pixel_in_frame(xy, width, height)) bad = min(bad, i);
        float2 c;
        pixel_centre(xy, w, h, &c.x, &c.y);
        slot_xy[j] = xy;
        slot_c[j] = c;
    }
    first_bad_merge(bad, first_bad);
}

// 5j: what k_resolve computes BEFORE its clamp, per accumulator slot of a frame, as k_resolve_rays writes it (two float4 = rr_radiance),
// and on request the frame's own bytes of the pixel next to it (frame_bytes: the device's powf is not the host's).  Record index:
// the slot itself for a pixel list (out[i] is list entry i), y * width + x of the slot's pixel for a whole frame (from_xy).
__global__ __launch_bounds__(RR_BLOCK) void k_resolve_pixels(DFrame fr, const uint32_t* __restrict__ slot_xy, DAccum acc, uint32_t from_xy,
                                                             float4* __restrict__ out, uint32_t* __restrict__ rgba8) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x; // accumulator slot
    if (p >= fr.n_region_pixels) return;
    const uint32_t o = from_xy ? frame_index(slot_xy[p], fr.width) : p;
    const Record r = resolve_record(acc, p, (float)fr.samples);
    store_record(out, o, r);
    const float c[3] = {r.color_depth.x, r.color_depth.y, r.color_depth.z};
    if (rgba8) rgba8[o] = frame_bytes(c, fr.gamma);
}

// 5k: the K = 2^lg_parts slots of a pixel (rr_render_pixel_parts; slot i * K + h = part h of entry i) -> K part records and the pixel's full record.
// One lane per slot: a lane resolves its own part over the part's S / K samples (loads of consecutive lanes are consecutive, 8 B per
// accumulator word; so are the 32-B stores of a list, and those of a whole frame in runs of 8 pixels x K parts, a row of an 8x8 block).  The K lanes of a pixel are an aligned power-of-two group inside the wave (K <= 64 and the
// block starts on a multiple of 64), so log2 K butterfly steps of __shfl_xor leave in every lane of the group the group's integer sums and
// the OR of its flags; the group's first lane resolves them over all S samples through the functions k_resolve_pixels uses -- integer
// adds commute, so these are the sums one slot would have held and the record has k_resolve_pixels' bytes.  The object id sits in the
// slot that received sample S - 1, the group's last (K divides S); every record of the pixel carries it.  Lanes behind the last slot
// belong to groups that lie behind it as a whole: they take part in the shuffles with zeros and store nothing.
// Record index o of the pixel: the entry itself for a list, y * width + x for a whole frame (from_xy), as k_resolve_pixels; part h goes to o * K + h.
RR_DEV long long shfl_xor_ll(long long v, int mask) {
    const int lo = __shfl_xor((int)(uint32_t)(unsigned long long)v, mask), hi = __shfl_xor((int)(uint32_t)((unsigned long long)v >> 32), mask);
    return (long long)(((unsigned long long)(uint32_t)hi << 32) | (uint32_t)lo);
}
// SPLIT: the end of rr_render_pixel_split: records and part records as above -- the same body -- and next to them the diffuse planes
// (`diffuse`: three planes of acc.n words, laid out as acc.rgb) resolved the same way, as floats: dif_out[3 o + c] over all S samples,
// dif_parts[3 (o K + h) + c] over the part's S / K.  The flags are the colour's: a channel whose record colour is not finite holds the
// record's value here too.  There lg_parts == 0 (no halves wanted) is one slot per pixel: `parts` and `dif_parts` are NULL and not
// written, and the record has k_resolve_pixels' bytes.  Without SPLIT the three diffuse arguments are NULL and nothing of them is compiled.
template <bool SPLIT>
__global__ __launch_bounds__(RR_BLOCK) void k_resolve_pixel_parts(DFrame fr, const uint32_t* __restrict__ slot_xy, DAccum acc, const long long* __restrict__ diffuse,
                                                                  uint32_t lg_parts, uint32_t from_xy, float4* __restrict__ out, float4* __restrict__ parts,
                                                                  float* __restrict__ dif_out, float* __restrict__ dif_parts) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x; // accumulator slot
    const bool live = p < fr.n_region_pixels;                 // (n_region_pixels: the slots, n_pixels * K)
    const uint32_t K = 1u << lg_parts;
    long long w[RECORD_SUMS] = {0ll, 0ll, 0ll, 0ll, 0ll, 0ll, 0ll}, dw[3] = {0ll, 0ll, 0ll}; // rgb, normal, depth; diffuse rgb
    uint32_t nf = 0u, id = 0u;
    if (live) {
        load_slot_sums(acc, p, w);
        if (SPLIT) {
#pragma unroll
            for (int k = 0; k < 3; k++) dw[k] = diffuse[(unsigned long long)k * acc.n + p];
        }
        nf = acc.flags[p];
        id = acc.object_id[p];
    }
    id = (uint32_t)__shfl((int)id, (int)((threadIdx.x & (RR_WAVE - 1)) | (K - 1u))); // the group's last slot holds sample S - 1
    const float n_part = (float)(fr.samples >> lg_parts), n = (float)fr.samples;
    const Record part = resolve_record_sums(w, nf, id, n_part);
    float dc[3] = {0.0f, 0.0f, 0.0f};
    if (SPLIT) {
#pragma unroll
        for (int k = 0; k < 3; k++) dc[k] = resolve_color_sum(dw[k], nf, k, n_part);
    }
    for (uint32_t off = 1u; off < K; off <<= 1) { // (wave-uniform trip count)
#pragma unroll
        for (int k = 0; k < RECORD_SUMS; k++) w[k] += shfl_xor_ll(w[k], (int)off);
        if (SPLIT) {
#pragma unroll
            for (int k = 0; k < 3; k++) dw[k] += shfl_xor_ll(dw[k], (int)off);
        }
        nf |= (uint32_t)__shfl_xor((int)nf, (int)off);
    }
    if (!live) return;
    const uint32_t o = from_xy ? frame_index(slot_xy[p], fr.width) : p >> lg_parts; // the pixel's record index; its parts follow each other at o * K
    if (!SPLIT || parts) {
        const unsigned long long q = ((unsigned long long)o << lg_parts) + (p & (K - 1u));
        store_record(parts, q, part);
        if (SPLIT) {
#pragma unroll
            for (int k = 0; k < 3; k++) dif_parts[3ull * q + k] = dc[k];
        }
    }
    if ((p & (K - 1u)) != 0u) return;
    store_record(out, o, resolve_record_sums(w, nf, id, n));
    if (SPLIT) {
#pragma unroll
        for (int k = 0; k < 3; k++) dif_out[3ull * o + k] = resolve_color_sum(dw[k], nf, k, n);
    }
}

// ---------------------------------------------------------------------------
// kernels 5l .. 5p: find the noisy entries of a frame or of a list and refine them on the device (rr_refine_list_device,
// rr_refine_sublist_device, rr_render_adaptive, rr_render_adaptive_levels)
// ---------------------------------------------------------------------------
// The lists of adaptive.refine_list and adaptive.refine_sublist (rustray_amd/adaptive.py) as an order-preserving stream compaction in
// three launches, and the passes that put a refined frame together.  One body per launch serves both lists: what differs is the entry
// SOURCE (rr_adaptive.h), which tells lane l of wave w whether it has an entry, where the entry's part records lie and which word it
// adds to the list.  FrameSource: the frame's 8x8 blocks, row-major, ARE the list's order, and on wave64 one wave is one block: lane l
// is the block's pixel l, __ballot of the lanes' flags is the block's 64-bit refine mask, and a set lane's place inside its block is the
// number of set bits below it.  ListSource: one wave per 64 consecutive entries of a list; the entries' coordinates are not
// interpreted: there is no frame there.  No kernel waits for another workgroup: the scan between the two wave kernels is a launch of its own.
//
// the tail of every masks kernel (5l, 5t): the wave's ballot of `flag` and its popcount, stored by lane 0
RR_DEV void store_wave_mask(bool flag, uint32_t lane, uint32_t w, unsigned long long* __restrict__ masks, uint32_t* __restrict__ counts) {
    const unsigned long long mask = __ballot(flag);
    if (lane == 0u) { masks[w] = mask; counts[w] = (uint32_t)__popcll(mask); }
}

// 5l: parts = the K = 2 part records of the source (k_resolve_pixel_parts: two float4 per part; a frame's at (y * width + x) * 2 + h, a
// list's entry i at 2 i + h).  A lane loads the colour of its entry's two halves (the 8 lanes of a block row: 512 consecutive bytes; the
// lanes of a list's wave: 4 KB), error_out (or NULL) gets half_error at the entry's index, and lane 0 stores the wave's mask and its
// popcount.  Lanes without an entry -- outside the frame, behind `count` -- load nothing and flag nothing: what lies behind a list, the
// caller's own pad, is never looked at.
template <class Source>
__global__ __launch_bounds__(RR_BLOCK) void k_refine_masks(const Source src, const float4* __restrict__ parts, float threshold, float* __restrict__ error_out,
                                                           unsigned long long* __restrict__ masks, uint32_t* __restrict__ counts) {
    const uint32_t lane = threadIdx.x & (RR_WAVE - 1), waves = gridDim.x * (RR_BLOCK / RR_WAVE), n_waves = src.waves();
    for (uint32_t w = blockIdx.x * (RR_BLOCK / RR_WAVE) + threadIdx.x / RR_WAVE; w < n_waves; w += waves) { // (wave-uniform)
        uint32_t i = 0u, word = 0u;
        bool flag = false;
        if (src.entry(w, lane, &i, &word)) {
            const float e = half_error_of_parts(parts, i);
            if (error_out) error_out[i] = e;
            flag = e > threshold;
        }
        store_wave_mask(flag, lane, w, masks, counts);
    }
}

// 5m: the exclusive prefix of the n block counts, in place, and their sum in *total.  ONE workgroup of 1024 threads walks the array in
// steps of 1024 with a carry (14 400 blocks at 1280x720: 15 steps): a shuffle scan inside each wave, the 16 wave sums through LDS.
__global__ __launch_bounds__(1024) void k_refine_scan(uint32_t* __restrict__ counts, uint32_t n, uint32_t* __restrict__ total) {
    __shared__ uint32_t s_wave[1024 / RR_WAVE];
    const uint32_t t = threadIdx.x, lane = t & (RR_WAVE - 1), wv = t / RR_WAVE;
    uint32_t carry = 0u;
    for (uint32_t base = 0u; base < n; base += 1024u) { // (uniform over the workgroup)
        const uint32_t i = base + t;
        const uint32_t v = i < n ? counts[i] : 0u;
        uint32_t incl = v;
#pragma unroll
        for (int off = 1; off < RR_WAVE; off <<= 1) {
            const uint32_t u = (uint32_t)__shfl_up((int)incl, off);
            if (lane >= (uint32_t)off) incl += u;
        }
        if (lane == RR_WAVE - 1) s_wave[wv] = incl;
        __syncthreads();
        uint32_t before = 0u, all = 0u;
#pragma unroll
        for (uint32_t k = 0; k < 1024 / RR_WAVE; k++) { const uint32_t w = s_wave[k]; before += k < wv ? w : 0u; all += w; }
        if (i < n) counts[i] = carry + before + incl - v;
        carry += all;
        __syncthreads(); // s_wave is written again in the next step
    }
    if (t == 0u) *total = carry;
}

// 5n: one wave per block or per 64 entries again.  A lane whose bit is set writes its word -- its pixel x | y << 16, or its entry
// list[64 w + l] -- at offset + (set bits below the lane).  The wave that holds the list's last entry -- the last one with any bit set:
// its offset plus its popcount is the total -- also writes the pad: copies of that entry up to the next multiple of 64 (fewer than 64:
// one per lane); only that wave knows the entry, and it writes nothing another wave writes.  With a ListSource list_out does not
// overlap the source's list (the host refuses it): a wave may write where another has yet to read.
template <class Source>
__global__ __launch_bounds__(RR_BLOCK) void k_refine_scatter(const Source src, const unsigned long long* __restrict__ masks, const uint32_t* __restrict__ offsets,
                                                             const uint32_t* __restrict__ total, uint32_t* __restrict__ list_out) {
    const uint32_t lane = threadIdx.x & (RR_WAVE - 1), waves = gridDim.x * (RR_BLOCK / RR_WAVE), n_waves = src.waves();
    const uint32_t taken = *total;
    for (uint32_t w = blockIdx.x * (RR_BLOCK / RR_WAVE) + threadIdx.x / RR_WAVE; w < n_waves; w += waves) { // (wave-uniform)
        const unsigned long long mask = masks[w];
        if (mask == 0ull) continue;
        const uint32_t off = offsets[w];
        uint32_t i = 0u, word = 0u;
        (void)src.entry(w, lane, &i, &word);
        if ((mask >> lane) & 1ull) list_out[off + refine_mask_rank(mask, lane)] = word; // (a set bit is a lane with an entry: k_refine_masks)
        if (!sublist_wave_is_last(mask, off, taken)) continue;
        const uint32_t last = (uint32_t)__shfl((int)word, (int)sublist_last_lane(mask));
        uint32_t at = 0u;
        if (sublist_pad_word(taken, lane, &at)) list_out[at] = last;
    }
}

// 5o: a pass's records over the frame: full record i (two float4) -> out at the pixel of list entry i, for the n entries before the
// pad; samples_out (or NULL) gets the pass's sample count there and error_out (or NULL) half_error of the entry's two halves at this
// count, the bits k_refine_masks computes from the same floats (`parts` is read for error_out only: rr_render_adaptive passes neither).
// The entries before the pad are distinct pixels of the frame: k_refine_scatter's list, or a sub-sequence of it.
__global__ __launch_bounds__(RR_BLOCK) void k_scatter_level(const uint32_t* __restrict__ list, uint32_t n, const float4* __restrict__ fine, const float4* __restrict__ parts,
                                                            uint32_t width, uint16_t samples, float4* __restrict__ out, uint16_t* __restrict__ samples_out,
                                                            float* __restrict__ error_out) {
    for (uint32_t i = blockIdx.x * RR_BLOCK + threadIdx.x; i < n; i += gridDim.x * RR_BLOCK) {
        const uint32_t o = frame_index(list[i], width);
        store_record(out, o, load_record(fine, i));
        if (samples_out) samples_out[o] = samples;
        if (error_out) error_out[o] = half_error_of_parts(parts, i);
    }
}

// 5p: the frame's own bytes of n finished records: frame_bytes on the record's colour, the function and the floats of k_resolve_pixels
__global__ __launch_bounds__(RR_BLOCK) void k_record_bytes(const float4* __restrict__ out, uint32_t n, uint32_t gamma, uint32_t* __restrict__ rgba8) {
    for (uint32_t o = blockIdx.x * RR_BLOCK + threadIdx.x; o < n; o += gridDim.x * RR_BLOCK) {
        const float4 r = out[2ull * o];
        const float c[3] = {r.x, r.y, r.z};
        rgba8[o] = frame_bytes(c, gamma);
    }
}

// ---------------------------------------------------------------------------
// kernels 5t, 5u: a level of a frame whose refined pixels KEEP their samples (rr_render_adaptive_prefix)
// ---------------------------------------------------------------------------
// The accumulators of a level stay on the device from level to level: entry i of the level's list owns slots 2 i and 2 i + 1 of `acc`
// (rr_adaptive.h: the halves s mod 2 of rr_render_pixel_parts at K = 2), and the next level adds only the samples the entry does not have
// yet.  So nothing here reads a float that another kernel wrote: the records, the error and the refine mask of an entry all come from its
// integer sums in one pass, where k_resolve_pixel_parts, k_scatter_level and k_refine_masks hand two part records per entry through HBM.
// One wave per 64 consecutive entries, k_refine_scan between the two wave kernels as it is, no kernel waiting for another workgroup.
// Level 0 is the whole frame in the region's slot order, which IS the list order of a frame (8x8 blocks row-major, row-major inside);
// there the pixel of entry i is the slot table's word 2 i (xy_stride 2: k_pixel_slots wrote every entry twice), for a list it is list[i]
// (xy_stride 1).  No block shape is assumed: a partial block's pixels are wherever the table says.
//
// the two slots of an entry: one 16-byte access per 8-byte plane, one 8-byte access for the ids and the flags
struct PrefixEntry { long long w[2][PREFIX_PLANES]; uint32_t id[2], nf[2]; };
static_assert(PREFIX_PLANES == RECORD_SUMS, "a set's planes are a slot's sums in resolve_record_sums' order");
RR_DEV void prefix_load_entry(const DAccum& acc, uint32_t i, PrefixEntry* e) {
    const unsigned long long p = prefix_entry_slot(i);
#pragma unroll
    for (int k = 0; k < PREFIX_PLANES; k++) {
        const long long* plane = k < 3 ? acc.rgb + (unsigned long long)k * acc.n : k < 6 ? acc.normal + (unsigned long long)(k - 3) * acc.n : acc.depth;
        const longlong2 v = *(const longlong2*)(plane + p);
        e->w[0][k] = v.x; e->w[1][k] = v.y;
    }
    const uint2 id = *(const uint2*)(acc.object_id + p), nf = *(const uint2*)(acc.flags + p);
    e->id[0] = id.x; e->id[1] = id.y; e->nf[0] = nf.x; e->nf[1] = nf.y;
}
// The ids are NOT carried: a level's pass writes the id of its last sample where that sample's path ends in a hit, and a pixel whose
// last sample hits nothing reports 0, as a frame rendered from cleared accumulators does.
RR_DEV void prefix_store_entry(const DAccum& acc, uint32_t j, const PrefixEntry& e) {
    const unsigned long long p = prefix_entry_slot(j);
#pragma unroll
    for (int k = 0; k < PREFIX_PLANES; k++) {
        long long* plane = k < 3 ? acc.rgb + (unsigned long long)k * acc.n : k < 6 ? acc.normal + (unsigned long long)(k - 3) * acc.n : acc.depth;
        longlong2 v; v.x = e.w[0][k]; v.y = e.w[1][k];
        *(longlong2*)(plane + p) = v;
    }
    *(uint2*)(acc.object_id + p) = make_uint2(0u, 0u);
    *(uint2*)(acc.flags + p) = make_uint2(e.nf[0], e.nf[1]);
}

// 5t: lane l of wave w resolves entry 64 w + l at `samples` samples: its halves over samples / 2 and its full record over `samples`,
// through the functions k_resolve_pixel_parts uses on the same integers (the sum of the two slots and the OR of their flags are what one
// slot would have held; the id lies in the slot of the last sample, the odd one).  The record goes to out at the entry's pixel, with
// samples_out and error_out (either may be NULL) beside it as k_scatter_level writes them, and lane 0 stores the wave's mask of
// half_error > threshold and its popcount.  Lanes behind `count` load nothing and flag nothing: the pad is never looked at, so every
// pixel is written once.
__global__ __launch_bounds__(RR_BLOCK) void k_prefix_masks(DAccum acc, const uint32_t* __restrict__ xy_table, uint32_t xy_stride, uint32_t count, uint32_t samples,
                                                           float threshold, uint32_t width, float4* __restrict__ out, uint16_t* __restrict__ samples_out,
                                                           float* __restrict__ error_out, unsigned long long* __restrict__ masks, uint32_t* __restrict__ counts) {
    const uint32_t lane = threadIdx.x & (RR_WAVE - 1), waves = gridDim.x * (RR_BLOCK / RR_WAVE), n_waves = sublist_waves(count);
    const float n_half = (float)(samples >> 1), n_full = (float)samples;
    for (uint32_t w = blockIdx.x * (RR_BLOCK / RR_WAVE) + threadIdx.x / RR_WAVE; w < n_waves; w += waves) { // (wave-uniform)
        uint32_t i = 0u;
        bool flag = false;
        if (sublist_lane_entry(w, lane, count, &i)) {
            PrefixEntry e;
            prefix_load_entry(acc, i, &e);
            float ca[3], cb[3];
            long long sum[RECORD_SUMS];
#pragma unroll
            for (int k = 0; k < 3; k++) {
                ca[k] = resolve_color_sum(e.w[0][k], e.nf[0], k, n_half);
                cb[k] = resolve_color_sum(e.w[1][k], e.nf[1], k, n_half);
            }
#pragma unroll
            for (int k = 0; k < RECORD_SUMS; k++) sum[k] = e.w[0][k] + e.w[1][k];
            const uint32_t o = frame_index(xy_table[(unsigned long long)i * xy_stride], width);
            store_record(out, o, resolve_record_sums(sum, e.nf[0] | e.nf[1], e.id[1], n_full));
            const float err = half_error(ca, cb);
            if (samples_out) samples_out[o] = (uint16_t)samples;
            if (error_out) error_out[o] = err;
            flag = err > threshold;
        }
        store_wave_mask(flag, lane, w, masks, counts);
    }
}

// 5u: one wave per 64 entries again.  A lane whose bit is set moves its entry to place offset + (set bits below the lane) of the next
// level: the pixel into list_out, the two slots of every plane and the flags into `dst`, the set of the next list (dst.n = twice its
// padded length, which the host knows: it has waited for *total).  The wave that holds the last taken entry also writes the pad: every
// pad lane copies that entry once more, from `src`, up to the next multiple of 64.  `dst` and list_out overlap nothing that is read here.
__global__ __launch_bounds__(RR_BLOCK) void k_prefix_compact(DAccum src, const uint32_t* __restrict__ xy_table, uint32_t xy_stride, uint32_t count,
                                                             const unsigned long long* __restrict__ masks, const uint32_t* __restrict__ offsets,
                                                             const uint32_t* __restrict__ total, uint32_t* __restrict__ list_out, DAccum dst) {
    const uint32_t lane = threadIdx.x & (RR_WAVE - 1), waves = gridDim.x * (RR_BLOCK / RR_WAVE), n_waves = sublist_waves(count);
    const uint32_t taken = *total;
    if (prefix_set_slots(taken) != dst.n) return; // (the host sized `dst` by this very word)
    for (uint32_t w = blockIdx.x * (RR_BLOCK / RR_WAVE) + threadIdx.x / RR_WAVE; w < n_waves; w += waves) { // (wave-uniform)
        const unsigned long long mask = masks[w];
        if (mask == 0ull) continue;
        const uint32_t off = offsets[w];
        uint32_t j = 0u;
        if (prefix_survivor_entry(mask, off, lane, &j)) { // (a set bit is an entry before `count`: k_prefix_masks)
            const uint32_t i = (w << 6) | lane;
            PrefixEntry e;
            prefix_load_entry(src, i, &e);
            list_out[j] = xy_table[(unsigned long long)i * xy_stride];
            prefix_store_entry(dst, j, e);
        }
        if (!sublist_wave_is_last(mask, off, taken)) continue;
        uint32_t i = 0u;
        if (prefix_pad_entry(w, mask, taken, lane, &i, &j)) {
            PrefixEntry e;
            prefix_load_entry(src, i, &e);
            list_out[j] = xy_table[(unsigned long long)i * xy_stride];
            prefix_store_entry(dst, j, e);
        }
    }
}

// ---------------------------------------------------------------------------
// kernels 5d .. 5h: the streaming passes around the walks of the DEVICE-BUFFER ray queries (rr_trace_rays_device,
// rr_trace_shadow_rays_device, rr_shade_rays_device, rr_surface_rays_device): the caller's 12-byte and 20-byte records are not a power of two, so a
// workgroup moves its 256 rays' 768 or 1280 consecutive dwords with lane-strided dword accesses (every wave instruction covers 64
// consecutive dwords = two 128-B lines) and turns them into per-ray records through LDS, where a stride of 3 or 5 dwords meets
// every bank once.  Ray i of the caller's order stays record i: packet p of the walks is rays 64 p .. 64 p + 63.
// ---------------------------------------------------------------------------
// reach[0 .. 2]: the largest finite |origin| per axis as float bits (non-negative floats order as their bits: atomicMax);
// reach[3]: the first index whose limit is NaN or negative (atomicMin; 0xffffffff = none).  One atomic per wave and word, and none
// for a wave that has nothing to report.  The host presets the words (0, 0, 0, 0xffffffff).
RR_DEV void reach_merge(uint32_t* __restrict__ reach, float ax, float ay, float az, uint32_t bad, uint32_t lane) {
#pragma unroll
    for (int off = RR_WAVE / 2; off > 0; off >>= 1) {
        ax = fmaxf(ax, __shfl_xor(ax, off)); ay = fmaxf(ay, __shfl_xor(ay, off)); az = fmaxf(az, __shfl_xor(az, off));
        bad = min(bad, (uint32_t)__shfl_xor((int)bad, off));
    }
    if (lane == 0u) {
        if (ax > 0.0f) atomicMax(&reach[0], __float_as_uint(ax));
        if (ay > 0.0f) atomicMax(&reach[1], __float_as_uint(ay));
        if (az > 0.0f) atomicMax(&reach[2], __float_as_uint(az));
        if (bad != 0xffffffffu) atomicMin(&reach[3], bad);
    }
}
RR_DEV float finite_abs(float v) { const float a = fabsf(v); return a <= RR_FLT_MAX ? a : 0.0f; } // NaN and inf: ignored (0)

// 5d: the caller's rays -> the records the walks read, and what the host must learn before it may enqueue the walk.
//   SHADOW: r0[i] = (origin, min(limit, FLT_MAX)), r1[i] = (direction, bits(depth));  limits == NULL: no limit
//   else:   r0[i] = (origin, 1), r1[i] = (direction, 0), r2[i] = (depth << 16, 1); thread 0 publishes the level's size in *q_count
template <bool SHADOW>
__global__ __launch_bounds__(RR_BLOCK) void k_pack_rays(const float* __restrict__ origins, const float* __restrict__ dirs, const float* __restrict__ limits,
                                                        uint32_t n, uint32_t depth, float4* __restrict__ r0, float4* __restrict__ r1, uint2* __restrict__ r2,
                                                        uint32_t* __restrict__ q_count, uint32_t* __restrict__ reach) {
    __shared__ float s_o[3 * RR_BLOCK], s_d[3 * RR_BLOCK];
    const uint32_t tid = threadIdx.x, lane = tid & (RR_WAVE - 1);
    if (!SHADOW && blockIdx.x == 0 && tid == 0) *q_count = n;
    const unsigned long long n_words = 3ull * n;
    float ax = 0.0f, ay = 0.0f, az = 0.0f;
    uint32_t bad = 0xffffffffu;
    for (unsigned long long base = (unsigned long long)blockIdx.x * RR_BLOCK; base < n; base += (unsigned long long)gridDim.x * RR_BLOCK) { // block-uniform
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const uint32_t w = k * RR_BLOCK + tid;
            const unsigned long long g = 3ull * base + w;
            if (g < n_words) { s_o[w] = origins[g]; s_d[w] = dirs[g]; }
        }
        __syncthreads();
        const unsigned long long i = base + tid;
        if (i < n) {
            const float ox = s_o[3 * tid], oy = s_o[3 * tid + 1], oz = s_o[3 * tid + 2];
            const float dx = s_d[3 * tid], dy = s_d[3 * tid + 1], dz = s_d[3 * tid + 2];
            ax = fmaxf(ax, finite_abs(ox)); ay = fmaxf(ay, finite_abs(oy)); az = fmaxf(az, finite_abs(oz));
            if (SHADOW) {
                float limit = RR_FLT_MAX;
                if (limits) {
                    const float l = limits[i];
                    if (!(l >= 0.0f)) bad = min(bad, (uint32_t)i);
                    limit = fminf(l, RR_FLT_MAX);
                }
                r0[i] = make_float4(ox, oy, oz, limit);
                r1[i] = make_float4(dx, dy, dz, __uint_as_float(depth));
            } else {
                r0[i] = make_float4(ox, oy, oz, 1.0f);
                r1[i] = make_float4(dx, dy, dz, 0.0f);
                r2[i] = make_uint2(depth << 16, 1u);
            }
        }
        __syncthreads(); // the next round overwrites the staging
    }
    reach_merge(reach, ax, ay, az, bad, lane);
}

// 5e: the reach alone, for rays that k_seed_rays reads where they are (rr_shade_rays_device): n_words = 3 x rays, which may pass 2^32
__global__ __launch_bounds__(RR_BLOCK) void k_ray_reach(const float* __restrict__ origins, unsigned long long n_words, uint32_t* __restrict__ reach) {
    float a[3] = {0.0f, 0.0f, 0.0f};
    const unsigned long long stride = (unsigned long long)gridDim.x * RR_BLOCK;
    unsigned long long g = (unsigned long long)blockIdx.x * RR_BLOCK + threadIdx.x;
    uint32_t c = (uint32_t)(g % 3ull);
    const uint32_t dc = (uint32_t)(stride % 3ull);
    for (; g < n_words; g += stride) {
        const float v = finite_abs(origins[g]);
        a[0] = fmaxf(a[0], c == 0u ? v : 0.0f); a[1] = fmaxf(a[1], c == 1u ? v : 0.0f); a[2] = fmaxf(a[2], c == 2u ? v : 0.0f);
        c += dc; if (c >= 3u) c -= 3u;
    }
    reach_merge(reach, a[0], a[1], a[2], 0xffffffffu, threadIdx.x & (RR_WAVE - 1));
}

// 5f: the walks' raw 16-byte hit records -> the 20-byte records of the ABI, as rr_trace_rays / rr_trace_shadow_rays build them on the host.
//   closest (k_trace_closest): (bits(toi), item or -1, leaf-order slot | side bits, 0) -> rr_ray_hit {hit, item, id, face, toi}; face:
//     reference_face_id (rr_trace.h)
//   SHADOW (k_query_shadow): (bits(toi), item, reference face id, occluded) -> rr_shadow_hit {occluded, item, id, face, toi}
template <bool SHADOW>
__global__ __launch_bounds__(RR_BLOCK) void k_unpack_hits(const uint4* __restrict__ hits, uint32_t n, const DItem* __restrict__ items, uint32_t n_items,
                                                          const DTriX* __restrict__ trix, uint32_t* __restrict__ out) {
    __shared__ uint32_t s_w[5 * RR_BLOCK];
    const uint32_t tid = threadIdx.x;
    const unsigned long long n_words = 5ull * n;
    for (unsigned long long base = (unsigned long long)blockIdx.x * RR_BLOCK; base < n; base += (unsigned long long)gridDim.x * RR_BLOCK) { // block-uniform
        const unsigned long long i = base + tid;
        if (i < n) {
            const uint4 h = hits[i];
            uint32_t w0 = 0u, w1 = 0xffffffffu, w2 = 0u, w3 = 0u, w4 = 0u;
            if (SHADOW ? (h.w != 0u && h.y < n_items) : ((int32_t)h.y >= 0 && h.y < n_items)) {
                const DItem* it = &items[h.y];
                w0 = 1u; w1 = h.y; w2 = it->id; w4 = h.x;
                if (SHADOW) w3 = h.z;
                else w3 = reference_face_id(it, trix, h.z);
            }
            s_w[5 * tid] = w0; s_w[5 * tid + 1] = w1; s_w[5 * tid + 2] = w2; s_w[5 * tid + 3] = w3; s_w[5 * tid + 4] = w4;
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 5; k++) {
            const uint32_t w = k * RR_BLOCK + tid;
            const unsigned long long g = 5ull * base + w;
            if (g < n_words) out[g] = s_w[w];
        }
        __syncthreads();
    }
}

// 5h: the walks' raw closest hits and the packed rays they answer -> the 128-byte records of rr_surface_rays: rr_ray_hit's four words,
// then surface_at (rr_surface.h) as eight 16-byte rows.  One ray per lane, grid-stride over groups of 256 rays like 5f; the gathers of
// surface_at are divergent by nature, the stores are not: a lane puts its eight rows into the workgroup's LDS image (32 KB, the 256
// records in output order) and the workgroup then moves the image out 16 bytes per lane, every wave instruction covering 1 KB of
// consecutive bytes -- never eight lane-strided stores of 64 lines with 16 bytes each.  Inside the image row r of ray t sits in
// 16-byte unit 8 t + (r ^ (t & 7)): the eight lanes a ds_write_b128 serves together then meet every bank once (unswizzled, all eight
// would share four banks), and so do the lanes of the ds_read_b128 on the way out, which read 8 consecutive units of one ray.
//   r0[i] = (origin, .), r1[i] = (direction, .): k_pack_rays' records; hits[i]: k_trace_closest's
//   a miss, or an item index out of range: {0, 0xffffffff, 0, 0} and 112 zero bytes
//
// The eight rows of ray i's rr_surface_hit, the miss record included (5h and 5w).  ALL_ROWS = false (the albedo-only build of 5w): a hit
// fills only row 4, base_color; surface_at is evaluated in full either way and the compiler drops what nothing stores.
template <bool ALL_ROWS>
RR_DEV void surface_rows(const DSceneView& sc, const float4* __restrict__ r0, const float4* __restrict__ r1, const uint4* __restrict__ hits, unsigned long long i,
                         const float* s_lut, uint4 (&row)[8]) {
    const uint4 h = hits[i];
    row[0] = make_uint4(0u, 0xffffffffu, 0u, 0u);
#pragma unroll
    for (int k = 1; k < 8; k++) row[k] = make_uint4(0u, 0u, 0u, 0u);
    if (!((int32_t)h.y >= 0 && h.y < sc.n_items)) return;
    const DItem& it = rr_global(sc.items)[h.y];
    const MatR m = load_material(&rr_global(sc.materials)[it.material], s_lut);
    const float4 a = r0[i], b = r1[i];
    const SurfaceAt s = surface_at(sc, it, m, mk3(a.x, a.y, a.z), mk3(b.x, b.y, b.z), __uint_as_float(h.x), h.z);
    row[4] = make_uint4(__float_as_uint(s.base_color.x), __float_as_uint(s.base_color.y), __float_as_uint(s.base_color.z), __float_as_uint(s.base_color.w));
    if (!ALL_ROWS) return;
    const uint32_t face = reference_face_id(&it, rr_global(sc.trix), h.z);
    row[0] = make_uint4(1u, h.y, it.id, face);
    row[1] = make_uint4(__float_as_uint(s.position.x), __float_as_uint(s.position.y), __float_as_uint(s.position.z), h.x);
    row[2] = make_uint4(__float_as_uint(s.normal.x), __float_as_uint(s.normal.y), __float_as_uint(s.normal.z), (uint32_t)it.material);
    row[3] = make_uint4(__float_as_uint(s.shading_normal.x), __float_as_uint(s.shading_normal.y), __float_as_uint(s.shading_normal.z), s.has_uv ? 1u : 0u);
    row[5] = make_uint4(__float_as_uint(s.ambient_color.x), __float_as_uint(s.ambient_color.y), __float_as_uint(s.ambient_color.z), __float_as_uint(s.alpha));
    row[6] = make_uint4(__float_as_uint(s.specular_color.x), __float_as_uint(s.specular_color.y), __float_as_uint(s.specular_color.z), __float_as_uint(s.reflectivity));
    row[7] = make_uint4(__float_as_uint(s.uv.x), __float_as_uint(s.uv.y), __float_as_uint(s.roughness), __float_as_uint(s.ambient_occlusion));
}
// where row r of ray t of a round sits in the workgroup's LDS image, in 16-byte units (the swizzle above)
RR_DEV uint32_t surface_row_unit(uint32_t t, uint32_t r) { return 8u * t + (r ^ (t & 7u)); }

__global__ __launch_bounds__(RR_BLOCK) void k_surface_hits(DSceneView sc, const float4* __restrict__ r0, const float4* __restrict__ r1, const uint4* __restrict__ hits,
                                                           uint32_t n, uint4* __restrict__ out) {
    __shared__ uint4 s_rows[8 * RR_BLOCK];
    __shared__ float s_lut[256]; // the u8 -> f32 table next to the lanes, as in k_shade
    const uint32_t tid = threadIdx.x;
    s_lut[tid] = c_u8_to_f32[tid];
    __syncthreads();
    const unsigned long long n_rows = 8ull * n;
    for (unsigned long long base = (unsigned long long)blockIdx.x * RR_BLOCK; base < n; base += (unsigned long long)gridDim.x * RR_BLOCK) { // block-uniform
        const unsigned long long i = base + tid;
        if (i < n) {
            uint4 row[8];
            surface_rows<true>(sc, r0, r1, hits, i, s_lut, row);
#pragma unroll
            for (uint32_t k = 0; k < 8u; k++) s_rows[surface_row_unit(tid, k)] = row[k];
        }
        __syncthreads();
#pragma unroll
        for (uint32_t k = 0; k < 8u; k++) {
            const uint32_t u = k * RR_BLOCK + tid;      // unit of the output image: row u % 8 of ray u / 8
            const unsigned long long g = 8ull * base + u;
            if (g < n_rows) out[g] = s_rows[surface_row_unit(u >> 3, u & 7u)];
        }
        __syncthreads(); // the next round overwrites the image
    }
}

// ---------------------------------------------------------------------------
// kernels 5v, 5w: the camera's surface per pixel (rr_surface_pixels): the rays of 5d made on the device from the camera, the
// closest-hit walk on them unchanged, and the ending of 5h with a target per record
// ---------------------------------------------------------------------------
// the camera's two inverses, a kernel argument: 32 floats in SGPRs, as TpFrame in kernels 7e and 7f
struct PixelCam { float proj_inv[16], view_inv[16]; };

// 5v: the records k_pack_rays<false> would have written for the pinhole rays through pixel centres (pixel_ray, rr_pixel_list.h) at depth 1:
// r0[i] = (origin, 1), r1[i] = (direction, 0), r2[i] = (1 << 16, 1), *q_count = n.  Ray i is the ray of list entry i (pixel_xy, n entries;
// *first_bad: the first index whose pixel lies outside the frame, one atomicMin per wave that has one to report, the host presets
// 0xffffffff and refuses the call before a walk -- the ray of such an entry is plain arithmetic) or, without a list, of slot i of the whole
// frame in the frame's own slot order (pixel_of_block_slot, n = width * height: a wave's 64 rays are one 8x8 block of the screen), and then
// target[i] = y * width + x: where the ending puts its record.  One ray per lane, grid-stride; every store of a wave is consecutive.
__global__ __launch_bounds__(RR_BLOCK) void k_pixel_rays(const PixelCam cam, uint32_t width, uint32_t height, const uint32_t* __restrict__ pixel_xy, uint32_t n,
                                                         float4* __restrict__ r0, float4* __restrict__ r1, uint2* __restrict__ r2, uint32_t* __restrict__ q_count,
                                                         uint32_t* __restrict__ target, uint32_t* __restrict__ first_bad) {
    const float w = (float)width, h = (float)height;
    if (blockIdx.x == 0 && threadIdx.x == 0) *q_count = n;
    uint32_t bad = 0xffffffffu;
    for (unsigned long long j = (unsigned long long)blockIdx.x * RR_BLOCK + threadIdx.x; j < n; j += (unsigned long long)gridDim.x * RR_BLOCK) {
        const uint32_t i = (uint32_t)j;
        uint32_t xy;
        if (pixel_xy) {
            xy = pixel_xy[i];
            if (!pixel_in_frame(xy, width, height)) bad = min(bad, i);
        } else {
            xy = pixel_of_block_slot(i, width, height);
            target[i] = frame_index(xy, width);
        }
        float o[3], d[3];
        pixel_ray(cam.proj_inv, cam.view_inv, xy, w, h, o, d);
        r0[i] = make_float4(o[0], o[1], o[2], 1.0f);
        r1[i] = make_float4(d[0], d[1], d[2], 0.0f);
        r2[i] = make_uint2(1u << 16, 1u);
    }
    if (pixel_xy) first_bad_merge(bad, first_bad); // (kernel-uniform)
}

// 5w: the ending of 5h for these rays.  Ray i answers record target[i] (target == NULL: record i): with RECORDS its rr_surface_hit goes to
// out[target[i]], with ALBEDO the bits of its base_color[0 .. 2] to albedo[3 target[i] ..] -- three zeros for a miss.  The evaluation is
// k_surface_hits': surface_at in full in every build, so the albedo has the record's bits by construction (in the albedo-only build the
// compiler drops what nothing stores: the normal map, the roughness, the other colours).  Records leave through the LDS image and swizzle of
// 5h: the eight lanes that hold the eight 16-byte units of one record store its whole 128-byte line at the record's own address, so a wave
// store instruction covers eight whole lines wherever the targets lie.  The albedo leaves lane-strided through a 3 KB image as 5f's words
// do: consecutive dwords for a list, runs of 24 dwords (a row of an 8x8 block) for a whole frame.
//   a miss, or an item index out of range: {0, 0xffffffff, 0, 0} and 112 zero bytes; albedo 0, 0, 0
//
// The way out of a 3 KB image (5w and 5y).  A workgroup's 3-word-per-entry image (s_albedo: entry t of the round at words 3 t .. 3 t + 2; s_target[t]: its record) ->
// albedo[3 target + c], lane-strided, for the first in_round entries.  The caller has synchronised behind the image's last store.
RR_DEV void store_albedo_image(const uint32_t* s_albedo, const uint32_t* s_target, uint32_t tid, uint32_t in_round, uint32_t* __restrict__ albedo) {
#pragma unroll
    for (uint32_t k = 0; k < 3u; k++) {
        const uint32_t word = k * RR_BLOCK + tid; // word of the image: channel word % 3 of entry word / 3 of this round
        const uint32_t t = word / 3u;
        if (t < in_round) albedo[3ull * s_target[t] + (word - 3u * t)] = s_albedo[word];
    }
}
template <bool RECORDS, bool ALBEDO>
__global__ __launch_bounds__(RR_BLOCK) void k_surface_pixels(DSceneView sc, const float4* __restrict__ r0, const float4* __restrict__ r1, const uint4* __restrict__ hits,
                                                             uint32_t n, const uint32_t* __restrict__ target, uint4* __restrict__ out, uint32_t* __restrict__ albedo) {
    __shared__ uint4 s_rows[RECORDS ? 8 * RR_BLOCK : 1];
    __shared__ uint32_t s_albedo[ALBEDO ? 3 * RR_BLOCK : 1];
    __shared__ uint32_t s_target[RR_BLOCK];
    __shared__ float s_lut[256]; // the u8 -> f32 table next to the lanes, as in k_shade
    const uint32_t tid = threadIdx.x;
    s_lut[tid] = c_u8_to_f32[tid];
    __syncthreads();
    for (unsigned long long base = (unsigned long long)blockIdx.x * RR_BLOCK; base < n; base += (unsigned long long)gridDim.x * RR_BLOCK) { // block-uniform
        const unsigned long long i = base + tid;
        const uint32_t in_round = (uint32_t)(n - base < RR_BLOCK ? n - base : RR_BLOCK); // rays of this round
        if (i < n) {
            uint4 row[8];
            surface_rows<RECORDS>(sc, r0, r1, hits, i, s_lut, row);
            if (RECORDS) {
#pragma unroll
                for (uint32_t k = 0; k < 8u; k++) s_rows[surface_row_unit(tid, k)] = row[k];
            }
            if (ALBEDO) { s_albedo[3u * tid] = row[4].x; s_albedo[3u * tid + 1u] = row[4].y; s_albedo[3u * tid + 2u] = row[4].z; }
            s_target[tid] = target ? target[i] : (uint32_t)i;
        }
        __syncthreads();
        if (RECORDS) {
#pragma unroll
            for (uint32_t k = 0; k < 8u; k++) {
                const uint32_t u = k * RR_BLOCK + tid; // unit of the image: row u % 8 of ray u / 8 of this round
                const uint32_t t = u >> 3;
                if (t < in_round) out[8ull * s_target[t] + (u & 7u)] = s_rows[surface_row_unit(t, u & 7u)];
            }
        }
        if (ALBEDO) store_albedo_image(s_albedo, s_target, tid, in_round, albedo);
        __syncthreads(); // the next round overwrites the images
    }
}

// ---------------------------------------------------------------------------
// kernels 5x, 5y: the frame's albedo per pixel (rr_albedo_pixels): the base colour at the first hit of every primary ray of the frame,
// summed per pixel in the frame's own accumulators
// ---------------------------------------------------------------------------
// 5x: the ending of depth level 1 for this call, where k_shade<true> stands in a frame.  Hit i of [chunk_begin, min(*count, chunk_end)) is
// the hit record k_trace_closest<true> wrote for primary index i of the batch; the ray is derived again (primary_ray: the inputs and the
// instruction sequence of the closest-hit kernel, so the same bits), the evaluation is k_surface_pixels' -- item and material per lane,
// surface_at in full, of which only base_color.xyz is used (the compiler drops the normal map, the roughness and the other colours) -- and
// the term goes the way every colour term of a frame goes: fix_add at scale 2^24 with the colour clamp (to_fix for a term beyond 2^25),
// the non-finite flags, accum_merged.  The samples of a pixel sit in neighbouring lanes, so the segmented merge applies unchanged.
// All 64 lanes of every wave reach accum_merged (the loop bound is block-uniform): lanes past the end, misses and item indices out of
// range pass pix = 0xffffffff.  No children, no shadow slots, no counters: RR_CNT_PRIMARY is the closest-hit kernel's.
__global__ __launch_bounds__(RR_BLOCK) void k_albedo_level1(const DShadeConst* __restrict__ kc, DPrimary pr, const uint4* __restrict__ hit1,
                                                            const uint32_t* __restrict__ count, uint32_t chunk_begin, uint32_t chunk_end, DAccum acc) {
    const DSceneView& sc = kc->sc;
    const DFrame& fr = kc->fr;
    const uint32_t n = min(*count, chunk_end);
    __shared__ float s_lut[256]; // the u8 -> f32 table next to the lanes, as in k_shade
    s_lut[threadIdx.x] = c_u8_to_f32[threadIdx.x];
    __syncthreads();
    for (uint32_t base = chunk_begin + blockIdx.x * RR_BLOCK; base < n; base += gridDim.x * RR_BLOCK) { // block-uniform
        const uint32_t i = base + threadIdx.x;
        uint32_t sum_pix = 0xffffffffu;
        int sum_r = 0, sum_g = 0, sum_b = 0;
        if (i < n) {
            const uint4 h = hit1[i];
            if ((int32_t)h.y >= 0 && h.y < sc.n_items) {
                f3 ro, rd; uint32_t pix, smp;
                primary_ray(fr, kc->ps, pr, i, &ro, &rd, &pix, &smp);
                const DItem& it = rr_global(sc.items)[h.y];
                const MatR m = load_material(&rr_global(sc.materials)[it.material], s_lut);
                const SurfaceAt s = surface_at(sc, it, m, ro, rd, __uint_as_float(h.x), h.z);
                const float ar = s.base_color.x, ag = s.base_color.y, ab = s.base_color.z;
                sum_pix = pix;
                const uint32_t nf = nonfinite_flags(ar, ag, ab);
                fix_add(sum_r, ar, RR_FIX_SCALE, RR_FIX_CLAMP, acc.rgb, pix); fix_add(sum_g, ag, RR_FIX_SCALE, RR_FIX_CLAMP, acc.rgb + acc.n, pix);
                fix_add(sum_b, ab, RR_FIX_SCALE, RR_FIX_CLAMP, acc.rgb + 2ull * acc.n, pix);
                if (nf) atomicOr(&acc.flags[pix], nf); // rare: a non-finite base colour
            }
        }
        accum_merged_runs(acc, sum_pix, sum_r, sum_g, sum_b); // (the segmented form: the one-pixel test's scalars take this kernel from 8 waves per SIMD to 7)
    }
}

// 5y: the colour sums of every accumulator slot -> three floats per pixel through resolve_color, what k_resolve_pixels puts into
// rr_radiance.color.  Index o of slot p: the slot itself for a pixel list, y * width + x of the slot's pixel for a whole frame (from_xy),
// as k_resolve_pixels.  The floats leave through a 3 KB image as the albedo of k_surface_pixels does: consecutive dwords for a list, runs
// of 24 dwords (a row of an 8x8 block) for a whole frame.  One workgroup per 256 slots.
__global__ __launch_bounds__(RR_BLOCK) void k_resolve_albedo(DFrame fr, const uint32_t* __restrict__ slot_xy, DAccum acc, uint32_t from_xy, uint32_t* __restrict__ albedo) {
    __shared__ uint32_t s_albedo[3 * RR_BLOCK];
    __shared__ uint32_t s_target[RR_BLOCK];
    const uint32_t tid = threadIdx.x, base = blockIdx.x * RR_BLOCK, npix = fr.n_region_pixels;
    const uint32_t p = base + tid; // accumulator slot
    const uint32_t in_round = base < npix ? min(npix - base, (uint32_t)RR_BLOCK) : 0u; // slots of this workgroup
    if (p < npix) {
        const float n = (float)fr.samples;
        const uint32_t nf = acc.flags[p];
#pragma unroll
        for (int k = 0; k < 3; k++) s_albedo[3u * tid + k] = __float_as_uint(resolve_color(acc, p, nf, k, n));
        s_target[tid] = from_xy ? frame_index(slot_xy[p], fr.width) : p;
    }
    __syncthreads();
    store_albedo_image(s_albedo, s_target, tid, in_round, albedo);
}

// 5g: stream ids 0 .. n - 1 (rr_shade_rays_device without the caller's)
__global__ __launch_bounds__(RR_BLOCK) void k_iota(uint32_t* __restrict__ ids, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) ids[i] = i;
}

// ---------------------------------------------------------------------------
// kernel 6: gather compact per-rank buffers into frame order (multi-GPU epilogue)
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(RR_BLOCK) void k_gather_frame(const uint32_t* __restrict__ src_index, uint32_t n_pixels,
                                                           uint32_t elem_words, const uint32_t* __restrict__ src, uint32_t* __restrict__ dst) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_pixels * elem_words) return;
    uint32_t p = i / elem_words, w = i % elem_words;
    dst[i] = src[(uint64_t)src_index[p] * elem_words + w];
}

// The same for the gathered PACKS of a multi-rank frame (TiledFrame: every rank's byte buffer holds one section per output buffer,
// each section sized for the largest rank): all four buffers in ONE launch, straight from the gather target -- no concatenation
// pass, no launch per buffer.  src_rank / src_local: for every frame pixel, the rank that rendered it and its position in that
// rank's compact order.  A thread moves one 4-byte word; the words of a pixel are (rgba, normal.xyz, depth, object id) = 6.
struct DPackedGather {
    const uint32_t* src_rank; const uint32_t* src_local;
    const char* packs; unsigned long long pack_stride;   // rank r's pack starts at packs + r * pack_stride
    unsigned long long section[4];                       // byte offset of each buffer's section inside a pack
    uint32_t words[4];                                   // 4-byte words per pixel of each buffer (0 = absent)
    uint32_t* dst[4];
    uint32_t n_pixels, words_total;
};
__global__ __launch_bounds__(RR_BLOCK) void k_gather_packed(DPackedGather g) {
    const unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (unsigned long long)g.n_pixels * g.words_total) return;
    const uint32_t p = (uint32_t)(i / g.words_total);
    uint32_t w = (uint32_t)(i % g.words_total);
    uint32_t b = 0;
    while (w >= g.words[b]) { w -= g.words[b]; b++; } // (absent buffers have 0 words: skipped)
    const uint32_t* src = (const uint32_t*)(g.packs + (unsigned long long)g.src_rank[p] * g.pack_stride + g.section[b]);
    g.dst[b][(unsigned long long)p * g.words[b] + w] = src[(unsigned long long)g.src_local[p] * g.words[b] + w];
}

// ---------------------------------------------------------------------------
// kernel 7: post-processing (reference src/post_processing.rs:24-181), one thread per pixel.
// HBM-bound: 24 algorithmic bytes per pixel (RGBA in + normal + object id + RGBA out; the 4-neighbour
// re-reads come from L1/L2).  Neighbours are addressed by LINEAR index y * width + x and only the linear index is
// range-checked (:40-45), so x + 1 at the right border reads the first pixel of the next row, as in the reference.
// ---------------------------------------------------------------------------
RR_DEV float curvature_soft_clamp(float curvature, float control) {
    if (curvature < 0.5f / control) return curvature * (1.0f - curvature * control);
    return 0.25f / control;
}
__global__ __launch_bounds__(RR_BLOCK) void k_post_process(uint32_t width, uint32_t height, uint32_t cavity, uint32_t outline,
                                                           const uint32_t* __restrict__ rgba_in, const float* __restrict__ normal,
                                                           const uint32_t* __restrict__ object_id, uint32_t* __restrict__ rgba_out) {
    const long long n = (long long)width * height;
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t px = rgba_in[i];
    float r = (float)(px & 255u), g = (float)((px >> 8) & 255u), b = (float)((px >> 16) & 255u);
    const long long w = (long long)width;
    const long long up = i + w, down = i - w, left = i - 1, right = i + 1; // (0,1) (0,-1) (-1,0) (1,0)
    if (outline) {
        const uint32_t c = object_id[i];
        const uint32_t o_up = (up >= 0 && up < n) ? object_id[up] : 0u, o_down = (down >= 0 && down < n) ? object_id[down] : 0u;
        const uint32_t o_l = (left >= 0 && left < n) ? object_id[left] : 0u, o_r = (right >= 0 && right < n) ? object_id[right] : 0u;
        // equal_vec . (0.25, 0.25, 0.25, 0.25) in nalgebra's 4-lane order (x*x' + z*z') + (y*y' + w*w'); lanes = (up, down, -1, +1)
        const float e0 = (o_up == c) ? 1.0f : 0.0f, e1 = (o_down == c) ? 1.0f : 0.0f, e2 = (o_l == c) ? 1.0f : 0.0f, e3 = (o_r == c) ? 1.0f : 0.0f;
        const float opacity = 1.0f - ((e0 * 0.25f + e2 * 0.25f) + (e1 * 0.25f + e3 * 0.25f));
        if (opacity > 0.0f) { r = opacity * 255.0f; g = opacity * 255.0f; b = opacity * 255.0f; }
    }
    if (cavity) {
        // .xz() of the neighbour normals: x -> .x, z -> .y
        const float up_z = (up >= 0 && up < n) ? normal[3 * up + 2] : 0.0f, down_z = (down >= 0 && down < n) ? normal[3 * down + 2] : 0.0f;
        const float left_x = (left >= 0 && left < n) ? normal[3 * left] : 0.0f, right_x = (right >= 0 && right < n) ? normal[3 * right] : 0.0f;
        const float diff = (up_z - down_z) + (right_x - left_x);
        float curvature;
        if (diff < 0.0f) curvature = -2.0f * curvature_soft_clamp(-diff, 1.0f);
        else curvature = 2.0f * curvature_soft_clamp(diff, 1.15f);
        r *= curvature + 1.0f; g *= curvature + 1.0f; b *= curvature + 1.0f;
    }
    // f32::clamp(0, 255) keeps NaN, `as u8` maps NaN to 0
    r = (r < 0.0f) ? 0.0f : ((r > 255.0f) ? 255.0f : r);
    g = (g < 0.0f) ? 0.0f : ((g > 255.0f) ? 255.0f : g);
    b = (b < 0.0f) ? 0.0f : ((b > 255.0f) ? 255.0f : b);
    rgba_out[i] = as_u8(r) | (as_u8(g) << 8) | (as_u8(b) << 16) | (255u << 24);
}

// ---------------------------------------------------------------------------
// kernels 7a .. 7d: the variance-guided a-trous filter over a frame of records (rr_denoise_records; rr_denoise.h has the arithmetic, in
// the order the header states; rustray_amd/denoise.py is the yardstick)
// ---------------------------------------------------------------------------
// Every kernel here works a 32x8 tile of pixels per workgroup, one pixel per lane, a tile row per half wave.  Working data are the
// handle's: the working colour as ping-pong float4 (r, g, b, var), the guide packed once as float4 (normal, depth) and uint2 (id, flags).
// A lane whose pixel lies outside the frame does nothing after the last barrier of its kernel.
//
// 7a: prepare.  Per pixel: the flags, the guide, the (demodulated) colour, and with halves the variance: the seeds of the tile and a
// halo of one pixel go through LDS (34 x 10 floats; a seed is >= 0 or NaN, -1 marks "no tap": outside the frame or colour not finite), then the
// 3x3 prefilter.  halves: the K = 2 layout (part h of pixel o: two float4 at 4 o + 2 h); albedo: 3 floats per pixel; either may be NULL.
RR_DEV uint32_t denoise_record_flags(const float4 r0, const float4 r1) {
    const float c[3] = {r0.x, r0.y, r0.z}, n[3] = {r1.x, r1.y, r1.z};
    return denoise_flags(c, r0.w, n);
}
__global__ __launch_bounds__(RR_BLOCK) void k_denoise_prepare(const float4* __restrict__ records, const float4* __restrict__ halves, const float* __restrict__ albedo,
                                                              uint32_t width, uint32_t height, float4* __restrict__ work, float4* __restrict__ guide,
                                                              uint2* __restrict__ meta) {
    __shared__ float s_v[(DN_TILE_H + 2) * (DN_TILE_W + 2)];
    const int x0 = (int)blockIdx.x * DN_TILE_W, y0 = (int)blockIdx.y * DN_TILE_H;
    if (halves) {
        for (int e = (int)threadIdx.x; e < (DN_TILE_H + 2) * (DN_TILE_W + 2); e += RR_BLOCK) {
            const int qx = x0 - 1 + e % (DN_TILE_W + 2), qy = y0 - 1 + e / (DN_TILE_W + 2);
            float v = -1.0f;
            if (qx >= 0 && qy >= 0 && qx < (int)width && qy < (int)height) {
                const unsigned long long o = (unsigned long long)qy * width + (unsigned int)qx;
                const float4 r0 = records[2ull * o];
                const float c[3] = {r0.x, r0.y, r0.z};
                if (denoise_is_finite(c[0]) && denoise_is_finite(c[1]) && denoise_is_finite(c[2])) {
                    const float4 ha = halves[4ull * o], hb = halves[4ull * o + 2];
                    const float a[3] = {ha.x, ha.y, ha.z}, b[3] = {hb.x, hb.y, hb.z};
                    v = denoise_variance_seed(true, a, b, albedo ? albedo + 3ull * o : nullptr);
                }
            }
            s_v[e] = v;
        }
        __syncthreads();
    }
    const int tx = (int)threadIdx.x & (DN_TILE_W - 1), ty = (int)threadIdx.x / DN_TILE_W;
    const int x = x0 + tx, y = y0 + ty;
    if (x >= (int)width || y >= (int)height) return;
    const unsigned long long o = (unsigned long long)y * width + (unsigned int)x;
    const float4 r0 = records[2ull * o], r1 = records[2ull * o + 1];
    const uint32_t flags = denoise_record_flags(r0, r1);
    float c[3] = {r0.x, r0.y, r0.z}, var = 0.0f;
    if (flags & DN_FIN) {
        if (albedo)
            for (int k = 0; k < 3; k++) c[k] = denoise_demodulate(c[k], albedo[3ull * o + k]);
        if (halves)
            var = denoise_prefilter([&](int dx, int dy, float* v) {
                *v = s_v[(ty + 1 + dy) * (DN_TILE_W + 2) + tx + 1 + dx];
                return !(*v < 0.0f); // (a seed may be NaN -- halves that both overflow at demodulation -- and is a tap all the same)
            });
    }
    work[o] = make_float4(c[0], c[1], c[2], var);
    guide[o] = make_float4(r1.x, r1.y, r1.z, r0.w);
    meta[o] = make_uint2(__float_as_uint(r1.w), flags);
}

RR_DEV DnTap denoise_make_tap(const float4 w, const float4 g, const uint2 m) {
    DnTap t;
    t.c[0] = w.x; t.c[1] = w.y; t.c[2] = w.z; t.var = w.w;
    t.n[0] = g.x; t.n[1] = g.y; t.n[2] = g.z; t.z = g.w;
    t.id = m.x; t.flags = m.y;
    return t;
}

// 7b: one pass, every tap gathered straight from global memory (the form of the large steps: the taps of a lane's neighbours are the
// neighbours of its taps, so each of the 25 loads of a wave is two runs of 512 contiguous bytes).  A tap's id and flags are read first;
// its colour and guide only where it is taken.
__global__ __launch_bounds__(RR_BLOCK) void k_denoise_pass_gather(const float4* __restrict__ in, const float4* __restrict__ guide, const uint2* __restrict__ meta,
                                                                  uint32_t width, uint32_t height, DnPass pass, float4* __restrict__ out) {
    const int x = (int)blockIdx.x * DN_TILE_W + ((int)threadIdx.x & (DN_TILE_W - 1)), y = (int)blockIdx.y * DN_TILE_H + (int)threadIdx.x / DN_TILE_W;
    if (x >= (int)width || y >= (int)height) return;
    const unsigned long long o = (unsigned long long)y * width + (unsigned int)x;
    const float4 w_p = in[o];
    const uint2 m_p = meta[o];
    if (!(m_p.y & DN_FIN)) { out[o] = w_p; return; }
    const DnTap p = denoise_make_tap(w_p, guide[o], m_p);
    float c[3], var;
    denoise_pixel_pass(pass, p, [&](int dx, int dy, DnTap* q) {
        const int qx = x + dx * pass.step, qy = y + dy * pass.step;
        if (qx < 0 || qy < 0 || qx >= (int)width || qy >= (int)height) return false;
        const unsigned long long oq = (unsigned long long)qy * width + (unsigned int)qx;
        const uint2 m_q = meta[oq];
        q->id = m_q.x; q->flags = m_q.y;
        if (!denoise_tap_taken(p, *q)) return false;
        *q = denoise_make_tap(in[oq], guide[oq], m_q);
        return true;
    }, c, &var);
    out[o] = make_float4(c[0], c[1], c[2], var);
}

// 7c: one pass through LDS.  The kernel works on the sub-lattice of period L of the frame -- the pixels (rx + L i, ry + L j) of residue
// class blockIdx.z = ry * L + rx -- on which the pass is a filter of step u = step / L: a 32x8 tile of lattice points plus a halo of
// h = 2 u points is staged in LDS (working colour, guide, id and flags; 40 B per point), and the 25 taps of every lane are LDS reads.
//   L = 1, u = step: the frame itself, for the small steps (h = 2, 4, 8);
//   L = step, u = 1: one dense 36 x 12 tile per residue class, for the large steps, whose halo in the frame would outgrow the tile.
// LDS: float4 arrays in row-major tile order; a wave reads two tile rows, 32 consecutive 16-byte slots each, and the four 16-lane groups
// of a ds_read_b128 each stay inside one row: 16 distinct slots of one 256-byte bank row whatever the tile's pitch, so the reads are
// conflict-free without padding (as are the staging writes, whose lanes walk the tile linearly).  Dynamic LDS: 40 B x (32 + 2h)(8 + 2h).
__global__ __launch_bounds__(RR_BLOCK) void k_denoise_pass_tile(const float4* __restrict__ in, const float4* __restrict__ guide, const uint2* __restrict__ meta,
                                                                uint32_t width, uint32_t height, DnPass pass, int lattice, float4* __restrict__ out) {
    extern __shared__ float4 s_dn[];
    const int L = lattice, u = pass.step / L, h = 2 * u;
    const int rx = (int)blockIdx.z % L, ry = (int)blockIdx.z / L;
    if (rx >= (int)width || ry >= (int)height) return; // (uniform over the workgroup, as the next one: before any barrier)
    const int wl = ((int)width - rx + L - 1) / L, hl = ((int)height - ry + L - 1) / L; // lattice points of this class
    const int i0 = (int)blockIdx.x * DN_TILE_W, j0 = (int)blockIdx.y * DN_TILE_H;
    if (i0 >= wl || j0 >= hl) return;
    const int tw = DN_TILE_W + 2 * h, th = DN_TILE_H + 2 * h, n_e = tw * th;
    float4* s_work = s_dn;
    float4* s_guide = s_dn + n_e;
    uint2* s_meta = (uint2*)(s_dn + 2 * n_e);
    for (int e = (int)threadIdx.x; e < n_e; e += RR_BLOCK) {
        const int i = i0 - h + e % tw, j = j0 - h + e / tw;
        float4 w = make_float4(0.0f, 0.0f, 0.0f, 0.0f), g = w;
        uint2 m = make_uint2(0u, DN_ABSENT);
        if (i >= 0 && j >= 0 && i < wl && j < hl) {
            const unsigned long long oq = (unsigned long long)(ry + L * j) * width + (unsigned int)(rx + L * i);
            w = in[oq]; g = guide[oq]; m = meta[oq];
        }
        s_work[e] = w; s_guide[e] = g; s_meta[e] = m;
    }
    __syncthreads();
    const int tx = (int)threadIdx.x & (DN_TILE_W - 1), ty = (int)threadIdx.x / DN_TILE_W;
    if (i0 + tx >= wl || j0 + ty >= hl) return;
    const unsigned long long o = (unsigned long long)(ry + L * (j0 + ty)) * width + (unsigned int)(rx + L * (i0 + tx));
    const int e_p = (ty + h) * tw + tx + h;
    const uint2 m_p = s_meta[e_p];
    if (!(m_p.y & DN_FIN)) { out[o] = s_work[e_p]; return; }
    const DnTap p = denoise_make_tap(s_work[e_p], s_guide[e_p], m_p);
    float c[3], var;
    denoise_pixel_pass(pass, p, [&](int dx, int dy, DnTap* q) {
        const int e = e_p + dy * u * tw + dx * u;
        const uint2 m_q = s_meta[e];
        q->id = m_q.x; q->flags = m_q.y;
        if (!denoise_tap_taken(p, *q)) return false; // (DN_ABSENT: no pixel there)
        *q = denoise_make_tap(s_work[e], s_guide[e], m_q);
        return true;
    }, c, &var);
    out[o] = make_float4(c[0], c[1], c[2], var);
}

// 7d: finish.  out = the record with the filtered colour, remodulated (a pixel whose colour is not finite keeps its bits: the working
// colour was never touched, but it is the INPUT's bits that are written); depth, normal and id are the input's bits; variance_out
// (or NULL) gets the last variance.  out may be `records` itself: a lane reads and writes its own pixel only.
__global__ __launch_bounds__(RR_BLOCK) void k_denoise_finish(const float4* records, const float* __restrict__ albedo, const float4* __restrict__ work,
                                                             const uint2* __restrict__ meta, uint32_t width, uint32_t height, float4* out,
                                                             float* __restrict__ variance_out) {
    const int x = (int)blockIdx.x * DN_TILE_W + ((int)threadIdx.x & (DN_TILE_W - 1)), y = (int)blockIdx.y * DN_TILE_H + (int)threadIdx.x / DN_TILE_W;
    if (x >= (int)width || y >= (int)height) return;
    const unsigned long long o = (unsigned long long)y * width + (unsigned int)x;
    const float4 r0 = records[2ull * o], r1 = records[2ull * o + 1], w = work[o];
    float c[3] = {r0.x, r0.y, r0.z};
    if (meta[o].y & DN_FIN) {
        c[0] = w.x; c[1] = w.y; c[2] = w.z;
        if (albedo)
            for (int k = 0; k < 3; k++) c[k] = denoise_remodulate(c[k], albedo[3ull * o + k]);
    }
    out[2ull * o] = make_float4(c[0], c[1], c[2], r0.w);
    out[2ull * o + 1] = r1;
    if (variance_out) variance_out[o] = w.w;
}

// 7d', 7d'': the two streaming ends of rr_denoise_split_records (rustray_amd/denoise.py: atrous_denoise_split), one pixel per lane, grid-stride.
// 7d': the two record sets the filter runs on.  Both share depth, normal and id with `records`; `rest` holds colour - diffuse (one binary32
// subtraction per channel), `direct` holds diffuse.  halves / dif_halves (both or neither) are split the same way, part q = 2 o + h.
__global__ __launch_bounds__(RR_BLOCK) void k_denoise_split_sets(const float4* __restrict__ records, const float4* __restrict__ halves, const float* __restrict__ diffuse,
                                                                 const float* __restrict__ dif_halves, uint32_t n, float4* __restrict__ rest, float4* __restrict__ direct,
                                                                 float4* __restrict__ rest_halves, float4* __restrict__ direct_halves) {
    for (uint32_t o = blockIdx.x * RR_BLOCK + threadIdx.x; o < n; o += gridDim.x * RR_BLOCK) {
        const float4 r0 = records[2ull * o], r1 = records[2ull * o + 1];
        const float d0 = diffuse[3ull * o], d1 = diffuse[3ull * o + 1], d2 = diffuse[3ull * o + 2];
        rest[2ull * o] = make_float4(r0.x - d0, r0.y - d1, r0.z - d2, r0.w);
        rest[2ull * o + 1] = r1;
        direct[2ull * o] = make_float4(d0, d1, d2, r0.w);
        direct[2ull * o + 1] = r1;
        if (halves) {
#pragma unroll
            for (uint32_t h = 0; h < 2u; h++) {
                const unsigned long long q = 2ull * o + h;
                const float4 h0 = halves[2ull * q], h1 = halves[2ull * q + 1];
                const float e0 = dif_halves[3ull * q], e1 = dif_halves[3ull * q + 1], e2 = dif_halves[3ull * q + 2];
                rest_halves[2ull * q] = make_float4(h0.x - e0, h0.y - e1, h0.z - e2, h0.w);
                rest_halves[2ull * q + 1] = h1;
                direct_halves[2ull * q] = make_float4(e0, e1, e2, h0.w);
                direct_halves[2ull * q + 1] = h1;
            }
        }
    }
}
// 7d'': out = the record with the sum of the two filtered colours, one binary32 add per channel; a pixel whose record colour is not finite
// keeps the record's colour.  out may be `records` itself: a lane reads and writes its own pixel only.
__global__ __launch_bounds__(RR_BLOCK) void k_denoise_split_sum(const float4* records, const float4* __restrict__ rest, const float4* __restrict__ direct, uint32_t n,
                                                                float4* out) {
    for (uint32_t o = blockIdx.x * RR_BLOCK + threadIdx.x; o < n; o += gridDim.x * RR_BLOCK) {
        const float4 r0 = records[2ull * o], r1 = records[2ull * o + 1];
        float4 c = r0;
        if (denoise_is_finite(r0.x) && denoise_is_finite(r0.y) && denoise_is_finite(r0.z)) {
            const float4 a = rest[2ull * o], b = direct[2ull * o];
            c.x = a.x + b.x; c.y = a.y + b.y; c.z = a.z + b.z;
        }
        out[2ull * o] = c;
        out[2ull * o + 1] = r1;
    }
}

// 7e, 7e': temporal reprojection (rr_accumulate_records, rr_accumulate_split_records; rr_history_clamp.h: temporal_pixel is the step
// of one pixel, with rr_temporal.h's arithmetic behind it in the order the headers state; rustray_amd/temporal.py is the yardstick).
// ONE body, accumulate_pixel_body<HALVES, SPLIT>, behind two entries that keep their names, their arguments and their __restrict__
// promises.  (7e'' and 7e''', the clamped calls, have bodies of their own below, with the step's sequence written out: behind this
// body they measured 1 to 3 % slower than before)
// One pixel per lane, 32x8 tiles as 7a .. 7d, so that the 2x2 taps of neighbouring lanes fall into the same 128-byte lines; no LDS: the
// shifts are sub-tile and the taps hit in cache.  A record is two 16-byte loads and two 16-byte stores.  Of a tap the guide row (normal,
// id) is read and tested first, then the colour row (colour, depth), then the length, and only then the colour rows of its two
// half-histories.  The camera, the previous view and the scalars are the kernel argument f.  HALVES: the one-layer call carries no
// registers for three layers.  history == NULL: the first frame, every pixel takes the no-history path and every layer is copied.
// out may be `records` and halves_out `halves`: a lane reads those at its own pixel only, before it writes.
// SPLIT (7e'): the records, halves and length of the build without it, bit for bit, and the diffuse layers (3 floats a pixel, 3 a half:
// rr_render_pixel_split's layouts) blended over the same taps with the same weights and length.  A 12-byte diffuse row is three dword
// loads; consecutive lanes read consecutive rows.  Of a tap the diffuse rows are read last, after its half rows, and only when it is
// taken.  diffuse_out may be `diffuse` and dif_halves_out `dif_halves`, as halves_out.
struct TpHistory {
    const float4* __restrict__ history;
    const float4* __restrict__ history_halves;
    const float* __restrict__ history_length;
    RR_DEV float length(unsigned long long q) const { return history_length[q]; }
    RR_DEV void guide(unsigned long long q, float* n, unsigned int* id) const {
        const float4 r1 = history[2ull * q + 1];
        n[0] = r1.x; n[1] = r1.y; n[2] = r1.z; *id = __float_as_uint(r1.w);
    }
    RR_DEV void colour(unsigned long long q, float* c, float* z) const {
        const float4 r0 = history[2ull * q];
        c[0] = r0.x; c[1] = r0.y; c[2] = r0.z; *z = r0.w;
    }
    RR_DEV void half(unsigned long long q, int h, float* c) const {
        const float4 r0 = history_halves[4ull * q + 2ull * (unsigned int)h];
        c[0] = r0.x; c[1] = r0.y; c[2] = r0.z;
    }
};
struct TpSplitHistory : TpHistory {
    const float* __restrict__ history_diffuse;
    const float* __restrict__ history_dif_halves;
    RR_DEV void diffuse(unsigned long long q, float* c) const {
        c[0] = history_diffuse[3ull * q]; c[1] = history_diffuse[3ull * q + 1]; c[2] = history_diffuse[3ull * q + 2];
    }
    RR_DEV void diffuse_half(unsigned long long q, int h, float* c) const {
        const unsigned long long r = 3ull * (2ull * q + (unsigned int)h);
        c[0] = history_dif_halves[r]; c[1] = history_dif_halves[r + 1]; c[2] = history_dif_halves[r + 2];
    }
};
struct TpSplitIo { // the diffuse pointers of the call, in the order of its arguments
    const float* diffuse; const float* dif_halves;
    const float* __restrict__ history_diffuse; const float* __restrict__ history_dif_halves;
    float* diffuse_out; float* dif_halves_out;
};
template <bool HALVES, bool SPLIT>
RR_DEV void accumulate_pixel_body(const TpFrame& f, const float4* records, const float4* halves, const float4* history, const float4* history_halves,
                                  const float* history_length, const float* motion, float4* out, float4* halves_out, float* length_out, const TpSplitIo& io) {
    const int x = (int)blockIdx.x * DN_TILE_W + ((int)threadIdx.x & (DN_TILE_W - 1)), y = (int)blockIdx.y * DN_TILE_H + (int)threadIdx.x / DN_TILE_W;
    if (x >= f.width || y >= f.height) return;
    const unsigned long long o = (unsigned long long)y * (unsigned int)f.width + (unsigned int)x;
    const float4 r0 = records[2ull * o], r1 = records[2ull * o + 1];
    float4 a0, a1, b0, b1;
    if (HALVES) { a0 = halves[4ull * o]; a1 = halves[4ull * o + 1]; b0 = halves[4ull * o + 2]; b1 = halves[4ull * o + 3]; }
    TpPixel p;
    p.c[0] = r0.x; p.c[1] = r0.y; p.c[2] = r0.z; p.depth = r0.w;
    p.n[0] = r1.x; p.n[1] = r1.y; p.n[2] = r1.z; p.id = __float_as_uint(r1.w);
    if (HALVES) { p.a[0] = a0.x; p.a[1] = a0.y; p.a[2] = a0.z; p.b[0] = b0.x; p.b[1] = b0.y; p.b[2] = b0.z; }
    if constexpr (SPLIT) {
        p.d[0] = io.diffuse[3ull * o]; p.d[1] = io.diffuse[3ull * o + 1]; p.d[2] = io.diffuse[3ull * o + 2];
        if (HALVES)
            for (int c = 0; c < 3; c++) { p.da[c] = io.dif_halves[6ull * o + c]; p.db[c] = io.dif_halves[6ull * o + 3 + c]; }
    }
    TpSplitHistory hist;
    hist.history = history; hist.history_halves = history_halves; hist.history_length = history_length;
    hist.history_diffuse = io.history_diffuse; hist.history_dif_halves = io.history_dif_halves;
    temporal_pixel<HALVES, SPLIT, false>(f, (unsigned int)x, (unsigned int)y, motion ? motion + 3ull * o : nullptr, history != nullptr, hist, 0, 0.0f, TpNoWindow{},
                                         TpNoWindow{}, &p);
    out[2ull * o] = make_float4(p.c[0], p.c[1], p.c[2], r0.w);
    out[2ull * o + 1] = r1;
    length_out[o] = p.length;
    if constexpr (SPLIT) { io.diffuse_out[3ull * o] = p.d[0]; io.diffuse_out[3ull * o + 1] = p.d[1]; io.diffuse_out[3ull * o + 2] = p.d[2]; }
    if (HALVES) {
        a0.x = p.a[0]; a0.y = p.a[1]; a0.z = p.a[2]; b0.x = p.b[0]; b0.y = p.b[1]; b0.z = p.b[2];
        halves_out[4ull * o] = a0; halves_out[4ull * o + 1] = a1; halves_out[4ull * o + 2] = b0; halves_out[4ull * o + 3] = b1;
        if constexpr (SPLIT)
            for (int c = 0; c < 3; c++) { io.dif_halves_out[6ull * o + c] = p.da[c]; io.dif_halves_out[6ull * o + 3 + c] = p.db[c]; }
    }
}
template <bool HALVES>
__global__ __launch_bounds__(RR_BLOCK) void k_accumulate_records(const TpFrame f, const float4* records, const float4* halves, const float4* __restrict__ history,
                                                                 const float4* __restrict__ history_halves, const float* __restrict__ history_length,
                                                                 const float* __restrict__ motion, float4* out, float4* halves_out, float* __restrict__ length_out) {
    accumulate_pixel_body<HALVES, false>(f, records, halves, history, history_halves, history_length, motion, out, halves_out, length_out, TpSplitIo{});
}
template <bool HALVES>
__global__ __launch_bounds__(RR_BLOCK) void k_accumulate_split_records(const TpFrame f, const float4* records, const float4* halves, const float4* __restrict__ history,
                                                                       const float4* __restrict__ history_halves, const float* __restrict__ history_length,
                                                                       const float* __restrict__ motion, float4* out, float4* halves_out,
                                                                       float* __restrict__ length_out, const TpSplitIo io) {
    accumulate_pixel_body<HALVES, true>(f, records, halves, history, history_halves, history_length, motion, out, halves_out, length_out, io);
}
// 7e'': 7e with the history held to the colours of the current frame (rr_accumulate_clamped_records; the sequence is
// temporal_pixel<HALVES, false, true>'s, which tests/native/temporal_pixel_test.cpp runs on the host, written out here with its stores
// between the blends).  The colour rows of `records` for the tile and a halo of R points go through LDS, one float4 per point: the
// colour and, in w, 1 where the point lies inside the frame with three finite floats, else 0 (34 x 10 at R = 1, 36 x 12 = 6912 B at
// R = 2).  Row-major, as 7c: the lanes of a tile row read consecutive 16-byte slots of one row of the staged tile at each window
// position (the compiler reads a slot as ds_read_b96 for the colour and ds_read_b32 for w); the staging writes are ds_write_b128 and
// walk the tile linearly.  EVERY lane stages and reaches the barrier; a lane outside the frame leaves after it.  Then 7e:
// temporal_history as there, and for a pixel that kept its history the (2R + 1)^2 window reads, the clamp and the length rule before
// the blends.  `out` may NOT be `records` (another workgroup's halo reads them); halves_out may be `halves`, read at the lane's pixel only.
template <bool HALVES, int R>
__global__ __launch_bounds__(RR_BLOCK) void k_accumulate_clamped_records(const TpFrame f, float sigma_scale, const float4* __restrict__ records, const float4* halves,
                                                                         const float4* __restrict__ history, const float4* __restrict__ history_halves,
                                                                         const float* __restrict__ history_length, const float* __restrict__ motion,
                                                                         float4* __restrict__ out, float4* halves_out, float* __restrict__ length_out) {
    constexpr int TW = DN_TILE_W + 2 * R, TH = DN_TILE_H + 2 * R;
    __shared__ float4 s_c[TW * TH];
    const int x0 = (int)blockIdx.x * DN_TILE_W, y0 = (int)blockIdx.y * DN_TILE_H;
    for (int e = (int)threadIdx.x; e < TW * TH; e += RR_BLOCK) {
        const int qx = x0 - R + e % TW, qy = y0 - R + e / TW;
        float4 c = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (qx >= 0 && qy >= 0 && qx < f.width && qy < f.height) {
            c = records[2ull * ((unsigned long long)qy * (unsigned int)f.width + (unsigned int)qx)];
            c.w = (denoise_is_finite(c.x) && denoise_is_finite(c.y) && denoise_is_finite(c.z)) ? 1.0f : 0.0f;
        }
        s_c[e] = c;
    }
    __syncthreads();
    const int tx = (int)threadIdx.x & (DN_TILE_W - 1), ty = (int)threadIdx.x / DN_TILE_W;
    const int x = x0 + tx, y = y0 + ty;
    if (x >= f.width || y >= f.height) return;
    const unsigned long long o = (unsigned long long)y * (unsigned int)f.width + (unsigned int)x;
    const float4 r0 = records[2ull * o], r1 = records[2ull * o + 1];
    float4 a0, a1, b0, b1;
    if (HALVES) { a0 = halves[4ull * o]; a1 = halves[4ull * o + 1]; b0 = halves[4ull * o + 2]; b1 = halves[4ull * o + 3]; }
    const uint32_t flags = denoise_record_flags(r0, r1);
    TpMix m;
    bool kept = false;
    if (history && flags == (uint32_t)(DN_FIN | DN_VALID)) {
        const float n_p[3] = {r1.x, r1.y, r1.z};
        const TpHistory hist{history, history_halves, history_length};
        kept = temporal_history<HALVES>(f, (unsigned int)x, (unsigned int)y, r0.w, n_p, __float_as_uint(r1.w), motion ? motion + 3ull * o : nullptr, hist, &m);
    }
    if (kept) {
        const float4* s_p = s_c + (ty + R) * TW + tx + R;
        history_clamp<HALVES>(R, sigma_scale, [&](int dx, int dy, float* c) {
            const float4 q = s_p[dy * TW + dx];
            c[0] = q.x; c[1] = q.y; c[2] = q.z;
            return q.w != 0.0f;
        }, &m);
    }
    float4 c0 = r0;
    if (kept) { c0.x = temporal_blend(m.h[0], m.a, r0.x); c0.y = temporal_blend(m.h[1], m.a, r0.y); c0.z = temporal_blend(m.h[2], m.a, r0.z); }
    out[2ull * o] = c0;
    out[2ull * o + 1] = r1;
    length_out[o] = kept ? m.length : ((flags & DN_FIN) ? 1.0f : 0.0f);
    if (HALVES) {
        if (kept && denoise_is_finite(a0.x) && denoise_is_finite(a0.y) && denoise_is_finite(a0.z)) {
            a0.x = temporal_blend(m.ha[0], m.a, a0.x); a0.y = temporal_blend(m.ha[1], m.a, a0.y); a0.z = temporal_blend(m.ha[2], m.a, a0.z);
        }
        if (kept && denoise_is_finite(b0.x) && denoise_is_finite(b0.y) && denoise_is_finite(b0.z)) {
            b0.x = temporal_blend(m.hb[0], m.a, b0.x); b0.y = temporal_blend(m.hb[1], m.a, b0.y); b0.z = temporal_blend(m.hb[2], m.a, b0.z);
        }
        halves_out[4ull * o] = a0; halves_out[4ull * o + 1] = a1; halves_out[4ull * o + 2] = b0; halves_out[4ull * o + 3] = b1;
    }
}

// 7e''': 7e'' merged with 7e' (rr_accumulate_clamped_split_records; the sequence is temporal_pixel<HALVES, true, true>'s, written out
// as in 7e'').  Two planes of the tile and its halo of R points go through
// LDS, one float4 per point each: the colour plane of 7e'', and the diffuse plane, the three floats of `diffuse` and, in w, 1 where the
// point lies inside the frame with three finite DIFFUSE floats, else 0 (2 x 5440 B at R = 1, 2 x 6912 = 13 824 B at R = 2).  Lane e stages
// point e of both planes: consecutive lanes read the consecutive 12-byte rows of `diffuse` of one row of the staged tile (the compiler
// merges a lane's three dwords into one global_load_dwordx3, so a wave's load walks that row's bytes without a gap), and write one
// ds_write_b128 per plane; a window position is a ds_read_b96 and a ds_read_b32 per plane.  EVERY lane stages and reaches the one
// barrier; a lane outside the frame leaves after it.  Then 7e': temporal_history with the diffuse means, and for a pixel that kept its
// history the two windows, one after the other, the clamps and the length rule before the blends.  The lane's own diffuse triple is its
// slot of the diffuse plane.  `out` may NOT be `records` and diffuse_out NOT `diffuse` (another workgroup's halo reads them); halves_out
// may be `halves` and dif_halves_out `dif_halves`, read at the lane's pixel only.
template <bool HALVES, int R>
__global__ __launch_bounds__(RR_BLOCK) void k_accumulate_clamped_split_records(const TpFrame f, float sigma_scale, const float4* __restrict__ records, const float4* halves,
                                                                               const float4* __restrict__ history, const float4* __restrict__ history_halves,
                                                                               const float* __restrict__ history_length, const float* __restrict__ motion,
                                                                               float4* __restrict__ out, float4* halves_out, float* __restrict__ length_out,
                                                                               const TpSplitIo io) {
    constexpr int TW = DN_TILE_W + 2 * R, TH = DN_TILE_H + 2 * R;
    __shared__ float4 s_c[TW * TH];
    __shared__ float4 s_d[TW * TH];
    const int x0 = (int)blockIdx.x * DN_TILE_W, y0 = (int)blockIdx.y * DN_TILE_H;
    for (int e = (int)threadIdx.x; e < TW * TH; e += RR_BLOCK) {
        const int qx = x0 - R + e % TW, qy = y0 - R + e / TW;
        float4 c = make_float4(0.0f, 0.0f, 0.0f, 0.0f), g = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (qx >= 0 && qy >= 0 && qx < f.width && qy < f.height) {
            const unsigned long long q = (unsigned long long)qy * (unsigned int)f.width + (unsigned int)qx;
            c = records[2ull * q];
            c.w = (denoise_is_finite(c.x) && denoise_is_finite(c.y) && denoise_is_finite(c.z)) ? 1.0f : 0.0f;
            g.x = io.diffuse[3ull * q]; g.y = io.diffuse[3ull * q + 1]; g.z = io.diffuse[3ull * q + 2];
            g.w = (denoise_is_finite(g.x) && denoise_is_finite(g.y) && denoise_is_finite(g.z)) ? 1.0f : 0.0f;
        }
        s_c[e] = c;
        s_d[e] = g;
    }
    __syncthreads();
    const int tx = (int)threadIdx.x & (DN_TILE_W - 1), ty = (int)threadIdx.x / DN_TILE_W;
    const int x = x0 + tx, y = y0 + ty;
    if (x >= f.width || y >= f.height) return;
    const unsigned long long o = (unsigned long long)y * (unsigned int)f.width + (unsigned int)x;
    const float4 r0 = records[2ull * o], r1 = records[2ull * o + 1];
    float4 a0, a1, b0, b1;
    if (HALVES) { a0 = halves[4ull * o]; a1 = halves[4ull * o + 1]; b0 = halves[4ull * o + 2]; b1 = halves[4ull * o + 3]; }
    const float4* s_p = s_c + (ty + R) * TW + tx + R;
    const float4* s_q = s_d + (ty + R) * TW + tx + R;
    float d[3] = {s_q->x, s_q->y, s_q->z}, da[3], db[3];
    if (HALVES)
        for (int c = 0; c < 3; c++) { da[c] = io.dif_halves[6ull * o + c]; db[c] = io.dif_halves[6ull * o + 3 + c]; }
    const uint32_t flags = denoise_record_flags(r0, r1);
    TpMix m;
    TpSplitMix s;
    bool kept = false;
    if (history && flags == (uint32_t)(DN_FIN | DN_VALID)) {
        const float n_p[3] = {r1.x, r1.y, r1.z};
        TpSplitHistory hist;
        hist.history = history; hist.history_halves = history_halves; hist.history_length = history_length;
        hist.history_diffuse = io.history_diffuse; hist.history_dif_halves = io.history_dif_halves;
        kept = temporal_history<HALVES, TpSplitHistory, true>(f, (unsigned int)x, (unsigned int)y, r0.w, n_p, __float_as_uint(r1.w), motion ? motion + 3ull * o : nullptr,
                                                     hist, &m, &s);
    }
    if (kept) {
        history_clamp_split<HALVES>(R, sigma_scale, [&](int dx, int dy, float* c) {
            const float4 q = s_p[dy * TW + dx];
            c[0] = q.x; c[1] = q.y; c[2] = q.z;
            return q.w != 0.0f;
        }, [&](int dx, int dy, float* c) {
            const float4 q = s_q[dy * TW + dx];
            c[0] = q.x; c[1] = q.y; c[2] = q.z;
            return q.w != 0.0f;
        }, &m, &s);
    }
    float4 c0 = r0;
    if (kept) { c0.x = temporal_blend(m.h[0], m.a, r0.x); c0.y = temporal_blend(m.h[1], m.a, r0.y); c0.z = temporal_blend(m.h[2], m.a, r0.z); }
    out[2ull * o] = c0;
    out[2ull * o + 1] = r1;
    length_out[o] = kept ? m.length : ((flags & DN_FIN) ? 1.0f : 0.0f);
    if (kept) temporal_blend_diffuse(s.d, m.a, d, d);
    io.diffuse_out[3ull * o] = d[0]; io.diffuse_out[3ull * o + 1] = d[1]; io.diffuse_out[3ull * o + 2] = d[2];
    if (HALVES) {
        if (kept && denoise_is_finite(a0.x) && denoise_is_finite(a0.y) && denoise_is_finite(a0.z)) {
            a0.x = temporal_blend(m.ha[0], m.a, a0.x); a0.y = temporal_blend(m.ha[1], m.a, a0.y); a0.z = temporal_blend(m.ha[2], m.a, a0.z);
        }
        if (kept && denoise_is_finite(b0.x) && denoise_is_finite(b0.y) && denoise_is_finite(b0.z)) {
            b0.x = temporal_blend(m.hb[0], m.a, b0.x); b0.y = temporal_blend(m.hb[1], m.a, b0.y); b0.z = temporal_blend(m.hb[2], m.a, b0.z);
        }
        halves_out[4ull * o] = a0; halves_out[4ull * o + 1] = a1; halves_out[4ull * o + 2] = b0; halves_out[4ull * o + 3] = b1;
        if (kept) { temporal_blend_diffuse(s.da, m.a, da, da); temporal_blend_diffuse(s.db, m.a, db, db); }
        for (int c = 0; c < 3; c++) { io.dif_halves_out[6ull * o + c] = da[c]; io.dif_halves_out[6ull * o + 3 + c] = db[c]; }
    }
}

// 7f: the motion of moved items per pixel (rr_motion_records; rr_motion.h has the arithmetic, rustray_amd/temporal.py: motion_records is
// the yardstick).  One pixel per lane, 32x8 tiles as 7a .. 7e; a record is two 16-byte loads, the answer three dword stores (six with
// world_out); no LDS.  The table is sorted by id: a lane whose record is valid looks its id up by binary search and reads the 24 floats
// of its entry.  The camera is the kernel argument f (of TpFrame only the two inverses and the frame's size are set).  n_moved == 0: the
// table is never read (the call with world_out and nothing moved).
__global__ __launch_bounds__(RR_BLOCK) void k_motion_records(const TpFrame f, const float4* __restrict__ records, const MoEntry* __restrict__ table,
                                                             uint32_t n_moved, float* __restrict__ motion_out, float* __restrict__ world_out) {
    const int x = (int)blockIdx.x * DN_TILE_W + ((int)threadIdx.x & (DN_TILE_W - 1)), y = (int)blockIdx.y * DN_TILE_H + (int)threadIdx.x / DN_TILE_W;
    if (x >= f.width || y >= f.height) return;
    const unsigned long long o = (unsigned long long)y * (unsigned int)f.width + (unsigned int)x;
    const float4 r0 = records[2ull * o], r1 = records[2ull * o + 1];
    const float n_p[3] = {r1.x, r1.y, r1.z};
    float world[3], m[3];
    motion_pixel(f, (unsigned int)x, (unsigned int)y, r0.w, n_p, __float_as_uint(r1.w), table, n_moved, world, m);
    motion_out[3ull * o] = m[0]; motion_out[3ull * o + 1] = m[1]; motion_out[3ull * o + 2] = m[2];
    if (world_out) { world_out[3ull * o] = world[0]; world_out[3ull * o + 1] = world[1]; world_out[3ull * o + 2] = world[2]; }
}

// 7g: the joint-bilateral upsampler (rr_upsample_records; rr_upsample.h has the arithmetic, rustray_amd/upsample.py: upsample_records is the
// yardstick).  One full-resolution pixel per lane, 32x8 tiles as 7a .. 7f.  The low-frame pixels a tile's taps touch form a patch of at
// most 34 x 10 (rr_upsample.h: UP_PATCH_W), from the left tap of the tile's first pixel to the right tap of its last: the workgroup stages
// it once in LDS -- colour and flags, (normal, distance), (albedo, id) as three float4 arrays, with HALVES the six half-colour floats as a
// float4 and a float2: 48 or 72 B per patch pixel, 16320 or 24480 B a workgroup -- and every lane takes its four taps from there.  A patch
// pixel outside the low frame carries no flag.  Global loads are 16 bytes each: of a surface record rows 0, 1, 2 and 4 (of the low guide
// by the staging lanes, of the full guide by every lane for its own pixel), of a colour record row 0, of a half record row 0.  LDS reads:
// the lanes of a tile row read entries that are consecutive or, at a ratio above 1, repeated (a broadcast): 16 lanes of a ds_read_b128
// stay inside one patch row, distinct 16-byte slots of it, as in 7c.  The stores go through store_record, two 16-byte stores a record.
// No output may overlap another buffer (the entry points refuse it) and the inputs are only read: every pointer is __restrict__.
// PLANES (rr_upsample_albedo_records with at least one plane): the albedo in use comes from the caller's planes -- the staging lanes fill
// s_a[e].xyz from albedo_low, every lane its own p.albedo from albedo, three dword loads at a 12-byte stride each (a tile row reads 384
// consecutive bytes of `albedo`) in place of the 16-byte load of row 4, which is then not issued; either plane may be NULL, a test of a
// kernel argument that is uniform over the launch.  The LDS layout and everything behind the loads are those of the builds without.
enum { UP_F_FIN = 1u, UP_F_VALID = 2u, UP_F_HIT = 4u, UP_F_INSIDE = 8u };
// A guide as the sum takes it.  PLANES with a `plane` (rr_upsample_albedo_records: 3 floats a pixel, 4-byte aligned and no more, so three
// dword loads and never a wider one) takes the albedo in use from there and leaves row 4 of the surface record unread.
template <bool PLANES>
RR_DEV UpGuide upsample_load_guide(const uint4* __restrict__ guide, unsigned long long o, const float* __restrict__ plane) {
    const uint4 r0 = guide[8ull * o], r1 = guide[8ull * o + 1], r2 = guide[8ull * o + 2];
    const float n[3] = {__uint_as_float(r2.x), __uint_as_float(r2.y), __uint_as_float(r2.z)};
    float a[3];
    if (PLANES && plane) {
        a[0] = plane[3ull * o]; a[1] = plane[3ull * o + 1]; a[2] = plane[3ull * o + 2];
    } else {
        const uint4 r4 = guide[8ull * o + 4];
        a[0] = __uint_as_float(r4.x); a[1] = __uint_as_float(r4.y); a[2] = __uint_as_float(r4.z);
    }
    return upsample_guide(r0.x, r0.z, __uint_as_float(r1.w), n, a);
}
template <bool HALVES, bool PLANES>
__global__ __launch_bounds__(RR_BLOCK) void k_upsample_records(const float4* __restrict__ low, const float4* __restrict__ halves_low, const uint4* __restrict__ guide_low,
                                                               const uint4* __restrict__ guide, const float* __restrict__ albedo_low,
                                                               const float* __restrict__ albedo, uint32_t low_width, uint32_t low_height, uint32_t width,
                                                               uint32_t height, const UpCall call, float4* __restrict__ out, float4* __restrict__ halves_out,
                                                               float* __restrict__ weight_out) {
    __shared__ float4 s_c[UP_PATCH_W * UP_PATCH_H];
    __shared__ float4 s_g[UP_PATCH_W * UP_PATCH_H];
    __shared__ float4 s_a[UP_PATCH_W * UP_PATCH_H];
    __shared__ float4 s_h4[HALVES ? UP_PATCH_W * UP_PATCH_H : 1];
    __shared__ float2 s_h2[HALVES ? UP_PATCH_W * UP_PATCH_H : 1];
    const int X0 = (int)blockIdx.x * UP_TILE_W, Y0 = (int)blockIdx.y * UP_TILE_H;
    const int X1 = min(X0 + UP_TILE_W, (int)width) - 1, Y1 = min(Y0 + UP_TILE_H, (int)height) - 1; // the tile's last pixel inside the frame
    int px0, py0, px1, py1;
    float f_;
    upsample_position(X0, low_width, width, &px0, &f_);
    upsample_position(X1, low_width, width, &px1, &f_);
    upsample_position(Y0, low_height, height, &py0, &f_);
    upsample_position(Y1, low_height, height, &py1, &f_);
    const int pw = min(px1 + 2 - px0, (int)UP_PATCH_W), ph = min(py1 + 2 - py0, (int)UP_PATCH_H); // (the bounds hold by themselves: rr_upsample.h)
    for (int e = (int)threadIdx.x; e < pw * ph; e += RR_BLOCK) {
        const int qx = px0 + e % pw, qy = py0 + e / pw;
        float4 c = make_float4(0.0f, 0.0f, 0.0f, __uint_as_float(0u)), g = c, a = c, h4 = c;
        float2 h2 = make_float2(0.0f, 0.0f);
        if (qx >= 0 && qy >= 0 && qx < (int)low_width && qy < (int)low_height) {
            const unsigned long long oq = (unsigned long long)qy * low_width + (unsigned int)qx;
            const float4 r0 = low[2ull * oq];
            const UpGuide gq = upsample_load_guide<PLANES>(guide_low, oq, albedo_low);
            const float col[3] = {r0.x, r0.y, r0.z};
            const uint32_t flags = UP_F_INSIDE | (upsample_fin(col) ? UP_F_FIN : 0u) | (gq.valid ? UP_F_VALID : 0u) | (gq.hit ? UP_F_HIT : 0u);
            c = make_float4(r0.x, r0.y, r0.z, __uint_as_float(flags));
            g = make_float4(gq.n[0], gq.n[1], gq.n[2], gq.z);
            a = make_float4(gq.albedo[0], gq.albedo[1], gq.albedo[2], __uint_as_float(gq.id));
            if (HALVES) {
                const float4 ha = halves_low[4ull * oq], hb = halves_low[4ull * oq + 2];
                h4 = make_float4(ha.x, ha.y, ha.z, hb.x);
                h2 = make_float2(hb.y, hb.z);
            }
        }
        s_c[e] = c; s_g[e] = g; s_a[e] = a;
        if (HALVES) { s_h4[e] = h4; s_h2[e] = h2; }
    }
    __syncthreads();
    const int x = X0 + ((int)threadIdx.x & (UP_TILE_W - 1)), y = Y0 + (int)threadIdx.x / UP_TILE_W;
    if (x >= (int)width || y >= (int)height) return;
    const unsigned long long o = (unsigned long long)y * width + (unsigned int)x;
    const UpGuide p = upsample_load_guide<PLANES>(guide, o, albedo);
    int x0, y0;
    float fx, fy;
    upsample_position(x, low_width, width, &x0, &fx);
    upsample_position(y, low_height, height, &y0, &fy);
    UpResult res;
    upsample_pixel<HALVES>(call, x0, fx, y0, fy, p, [&](int qx, int qy, UpTap* q) {
        const int i = qx - px0, j = qy - py0;
        if (i < 0 || j < 0 || i >= pw || j >= ph) return false; // (never: x0 is monotone in x; kept so that no index leaves the patch)
        const int e = j * pw + i;
        const float4 c = s_c[e];
        const uint32_t flags = __float_as_uint(c.w);
        if (!(flags & UP_F_INSIDE)) return false;
        const float4 g = s_g[e], a = s_a[e];
        q->c[0] = c.x; q->c[1] = c.y; q->c[2] = c.z;
        q->fin = (flags & UP_F_FIN) != 0u;
        q->g.n[0] = g.x; q->g.n[1] = g.y; q->g.n[2] = g.z; q->g.z = g.w;
        q->g.albedo[0] = a.x; q->g.albedo[1] = a.y; q->g.albedo[2] = a.z;
        q->g.id = __float_as_uint(a.w);
        q->g.hit = (flags & UP_F_HIT) != 0u;
        q->g.valid = (flags & UP_F_VALID) != 0u;
        if (HALVES) {
            const float4 h4 = s_h4[e];
            const float2 h2 = s_h2[e];
            q->h[0][0] = h4.x; q->h[0][1] = h4.y; q->h[0][2] = h4.z;
            q->h[1][0] = h4.w; q->h[1][1] = h2.x; q->h[1][2] = h2.y;
        }
        return true;
    }, &res);
    unsigned int depth, normal[3], id;
    upsample_guide_fields(p, &depth, normal, &id);
    const float4 guide_row = make_float4(__uint_as_float(normal[0]), __uint_as_float(normal[1]), __uint_as_float(normal[2]), __uint_as_float(id));
    store_record(out, o, Record{make_float4(res.c[0], res.c[1], res.c[2], __uint_as_float(depth)), guide_row});
    if (HALVES) {
        store_record(halves_out, 2ull * o, Record{make_float4(res.h[0][0], res.h[0][1], res.h[0][2], __uint_as_float(depth)), guide_row});
        store_record(halves_out, 2ull * o + 1, Record{make_float4(res.h[1][0], res.h[1][1], res.h[1][2], __uint_as_float(depth)), guide_row});
    }
    if (weight_out) weight_out[o] = res.weight;
}

// ---------------------------------------------------------------------------
// kernel 8: device self-test of the arithmetic contract (tests/test_device_math.py)
// op: 0 sincos -> (sin, cos); 1 acos; 2 atan2(a, b); 3 a / b; 4 sqrt(a); 5 jitter(dir = (a, b, c)); 7 cos(a * pi) as jitter() needs it
// (op 6 is the HOST build of the same rr_cos, rr_api_probe.h rr_math_probe)
// op 12: philox4x32_10 of caller-given words, as bit patterns: n = 2 m, entry i < m has the counter (a[i], b[i], c[i], a[m + i]) = (pixel,
// sample, node, stream) and the key (seed_lo, seed_hi); out0[i], out1[i] = the two words jitter() uses.  (op 14 is the HOST build of the same
// function, rr_api_probe.h.)
// op 13: the wave merges of rr_accumulate.h as the kernels call them, words as bit patterns: n = 9 * 256, and lane l of the ONE workgroup
// that works (four waves) takes a[k * 256 + l], k = 0 .. 8: colour pixel, r, g, b, aux pixel, nx, ny, nz, depth (b[l]: the depth's high
// word for entry 3).  A pixel is a slot below 128 or 0xffffffff (anything else counts as that).  seed_lo picks the entry: 0 accum_merged,
// 1 accum_aux_merged, 2 accum_hit_merged, 3 accum_depth_wide_merged.  out0, zeroed by the host, is a DAccum of 128 slots: seven planes of
// 128 64-bit sums (r, g, b, nx, ny, nz, depth).
// ---------------------------------------------------------------------------
__global__ void k_math_probe(int op, const float* a, const float* b, const float* c, int n, float* out0, float* out1, float* out2,
                             uint32_t seed_lo, uint32_t seed_hi) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (op == 0) { float s, co; rr_sincos(a[i], &s, &co); out0[i] = s; out1[i] = co; }
    else if (op == 1) out0[i] = rr_acos(a[i]);
    else if (op == 2) out0[i] = rr_atan2(a[i], b[i]);
    else if (op == 3) out0[i] = a[i] / b[i];
    else if (op == 4) out0[i] = sqrtf(a[i]);
    else if (op == 7) out0[i] = rr_cos(a[i] * RR_PI_F);
    else if (op == 10) { // the per-triangle shading constants as k_shade evaluated them per hit (now DTri::v1.w, v3; op 11 is the host's build)
        const int t = (i / 3) * 3, k = i % 3;
        if (t + 2 < n) {
            const f3 va = mk3(a[t], a[t + 1], a[t + 2]), vb = mk3(b[t], b[t + 1], b[t + 2]), vc = mk3(c[t], c[t + 1], c[t + 2]);
            const f3 ng = normalize3(cross3(vb - va, vc - va));
            out0[i] = k == 0 ? ng.x : (k == 1 ? ng.y : ng.z);
            out1[i] = norm3(cross3(va - vb, va - vc));
        }
    }
    else if (op == 5) {
        RngKey k; k.seed_lo = seed_lo; k.seed_hi = seed_hi; k.pixel = (uint32_t)i; k.sample = (uint32_t)(i & 7); k.node = 1u + (uint32_t)(i % 5);
        f3 r = jitter(mk3(a[i], b[i], c[i]), 0.05f, rr_cos(0.05f * RR_PI_F), k, (uint32_t)(i % 3));
        out0[i] = r.x; out1[i] = r.y; out2[i] = r.z;
    }
    else if (op == 12) {
        const int m = n / 2;
        if (i < m) {
            uint32_t r0, r1;
            philox4x32_10(__float_as_uint(a[i]), __float_as_uint(b[i]), __float_as_uint(c[i]), __float_as_uint(a[m + i]), seed_lo, seed_hi, &r0, &r1);
            out0[i] = __uint_as_float(r0); out1[i] = __uint_as_float(r1);
        }
    }
    else if (op == 13) {
        if (blockIdx.x != 0 || blockDim.x != 256 || n < 9 * 256) return; // (uniform: all 64 lanes of the four waves go on)
        int w[9];
        for (int k = 0; k < 9; k++) w[k] = __float_as_int(a[k * 256 + (int)threadIdx.x]);
        const uint32_t sum_pix = (uint32_t)w[0] < 128u ? (uint32_t)w[0] : 0xffffffffu, aux_pix = (uint32_t)w[4] < 128u ? (uint32_t)w[4] : 0xffffffffu;
        DAccum acc;
        acc.rgb = (long long*)out0; acc.normal = acc.rgb + 3 * 128; acc.depth = acc.rgb + 6 * 128; acc.object_id = nullptr; acc.n = 128ull; acc.flags = nullptr;
        if (seed_lo == 0u) accum_merged(acc, sum_pix, w[1], w[2], w[3]);
        else if (seed_lo == 1u) accum_aux_merged(acc, aux_pix, w[5], w[6], w[7], w[8]);
        else if (seed_lo == 2u) accum_hit_merged(acc, sum_pix, w[1], w[2], w[3], aux_pix, w[5], w[6], w[7], w[8]);
        else if (seed_lo == 3u) accum_depth_wide_merged(acc, aux_pix, (long long)(((unsigned long long)__float_as_uint(b[threadIdx.x]) << 32) | (uint32_t)w[8]));
    }
}
