// rr_accumulate.h — layer 5 of the device code: the per-pixel fixed-point accumulators that stand for the reference's f32 sums
// over samples (src/raytracing.rs:400-417).  Integer adds commute, so the frame does not depend on the order of anything.
//
// Offers: to_fix, fix_add, fix_add_at, nonfinite_flags, accum_merged, accum_aux_merged, accum_depth_wide_merged, accum_hit_merged (the last four
// must be called by all 64 lanes of a wave); from_fix, resolve_color, resolve_normal, resolve_depth (and their *_sum forms); Record, load_record,
// store_record, load_slot_sums, resolve_record, resolve_record_sums: an rr_radiance from a slot or from sums, every pixel ending's way out.
// wave_merge_runs / wave_merge_runs32 / fits25i / fits25 / wave_one_pixel / wave_sum32 / wave_sum64 / totals_to_lanes and the *_runs forms of the merges
// are this layer's own, and so are its DPP macros (RR_DPP_*, RR_SEG_STEP, RR_SEG_STEP32), un-defined at the end.
// Needs: rr_device.h (DAccum, RR_NF_*), rr_math.h.
#pragma once
#include "rr_device.h"
#include "rr_math.h"

// ---------------------------------------------------------------------------
// accumulators
// ---------------------------------------------------------------------------
RR_DEV long long to_fix(float v, float scale, float clampv) {
    if (v != v) return 0ll; // a NaN adds nothing to the fixed-point sum; its pixel is flagged (to_fix_c)
    v = fminf(fmaxf(v, -clampv), clampv);
    return __float2ll_rn(v * scale);
}
// The fixed-point sum of one lane and channel is a 32-bit integer.  Nearly every term is small (a colour term up to 2, a normal
// component, a depth below 512: |v * scale| < 2^25) and converts with v_rndne + v_cvt_i32; __float2ll_rn is eleven instructions and
// a 64-bit add two more, seven to ten times per shaded hit.  A term beyond 2^25 goes straight to its accumulator word as one 64-bit
// atomic of its own (rare: a saturating highlight, a far hit's depth); a NaN adds nothing (its pixel is flagged).  Every term is
// rounded to nearest-even by itself either way, and integer adds commute: the pixel's sum is the same integer.
// fix_add_at: `plane()` names the plane, and is evaluated by a term that goes there only (k_shade fetches the pointer then)
template <class Plane> RR_DEV void fix_add_at(int& n, float v, float scale, float clampv, Plane plane, uint32_t pix) {
    const float x = v * scale;
    if (rr_abs(x) < 33554432.0f) n += __float2int_rn(x); // (inside every clamp in use: |v| < 2 at scale 2^24, < 512 at 2^16)
    else {
        const long long t = to_fix(v, scale, clampv);
        if (t != 0ll) { long long* const p = plane(); if (p) atomicAdd((unsigned long long*)p + pix, (unsigned long long)t); }
    }
}
RR_DEV void fix_add(int& n, float v, float scale, float clampv, long long* plane, uint32_t pix) {
    fix_add_at(n, v, scale, clampv, [=] { return plane; }, pix);
}

// A colour contribution of channel `ch`: non-finite values are recorded in `flags` (RR_NF_*), because the reference's f32
// sum would carry them to the pixel (NaN or +inf -> 255, -inf -> 0, src/raytracing.rs:406-417) while a fixed-point sum cannot.
RR_DEV uint32_t nonfinite_flags(float r, float g, float b) {
    if (((r - r) + (g - g)) + (b - b) == 0.0f) return 0u; // x - x is 0 for every finite x and NaN otherwise: one test for the common case
    uint32_t f = 0u;
    const float v[3] = {r, g, b};
#pragma unroll
    for (int ch = 0; ch < 3; ch++)
        if (!(rr_abs(v[ch]) <= RR_FLT_MAX)) f |= (v[ch] != v[ch] ? RR_NF_NAN : (v[ch] > 0.0f ? RR_NF_PINF : RR_NF_NINF)) << ch;
    return f;
}
// Adds of one wave to the accumulators, merged: neighbouring lanes that add to the same pixel (the samples of one
// pixel sit in neighbouring lanes, primary_ray; compaction keeps lane order) are summed first with a segmented scan over
// the 16-lane DPP rows, and only the last lane of each run issues the atomics.  Integer adds commute, so the frame
// is the same whatever is merged.  Must be called by all 64 lanes of the wave; lanes with nothing to add pass
// pix = 0xffffffff.  (64 lanes adding to one address, or 16, serialise in the L2 atomic units: +10 ms on sponza_syn.)
#define RR_DPP_SHR(x, n) __builtin_amdgcn_update_dpp(0, (int)(x), 0x110 + (n), 0xf, 0xf, true)
#define RR_DPP_SHL(x, n) __builtin_amdgcn_update_dpp(0, (int)(x), 0x100 + (n), 0xf, 0xf, true)
#define RR_DPP_SHR64(x, n) (((unsigned long long)(uint32_t)RR_DPP_SHR((uint32_t)((x) >> 32), n) << 32) | (uint32_t)RR_DPP_SHR((uint32_t)(x), n))
#define RR_SEG_STEP(n)                                                                                         \
    {                                                                                                          \
        const int pf = RR_DPP_SHR(f, n);                                                                       \
        _Pragma("unroll") for (int k_ = 0; k_ < N; k_++) { const unsigned long long p_ = RR_DPP_SHR64(v[k_], n); if (!f) v[k_] += p_; } \
        if (!f) f = pf;                                                                                        \
    }
// Segmented sum over runs of equal `pix` inside the 16-lane DPP rows: afterwards the LAST lane of every run (return
// value true) holds the run's sums in v[0..N).  Must be called by all 64 lanes; lanes with nothing to add pass 0xffffffff.
template <int N> RR_DEV bool wave_merge_runs(uint32_t pix, unsigned long long (&v)[N]) {
    const uint32_t lane16 = threadIdx.x & 15u;
    const uint32_t prev = (uint32_t)RR_DPP_SHR(pix, 1);
    const int head = (lane16 == 0u || prev != pix) ? 1 : 0; // first lane of a run of equal pixels inside its row
    int f = head;
    RR_SEG_STEP(1) RR_SEG_STEP(2) RR_SEG_STEP(4) RR_SEG_STEP(8)
    const int next_head = RR_DPP_SHL(head, 1);
    return (lane16 == 15u || next_head != 0) && pix != 0xffffffffu;
}
// The same over 32-bit values: when every value of the wave is below 2^25 in magnitude (a colour term up to 2, any
// normal) a run of at most 16 of them sums to less than 2^29, and a step is one DPP add per value instead of a
// 64-bit add with its carry and two moves.
#define RR_SEG_STEP32(n)                                                                                       \
    {                                                                                                          \
        const int pf = RR_DPP_SHR(f, n);                                                                       \
        _Pragma("unroll") for (int k_ = 0; k_ < N; k_++) { const int p_ = RR_DPP_SHR(v[k_], n); if (!f) v[k_] += p_; } \
        if (!f) f = pf;                                                                                        \
    }
template <int N> RR_DEV bool wave_merge_runs32(uint32_t pix, int (&v)[N]) {
    const uint32_t lane16 = threadIdx.x & 15u;
    const uint32_t prev = (uint32_t)RR_DPP_SHR(pix, 1);
    const int head = (lane16 == 0u || prev != pix) ? 1 : 0;
    int f = head;
    RR_SEG_STEP32(1) RR_SEG_STEP32(2) RR_SEG_STEP32(4) RR_SEG_STEP32(8)
    const int next_head = RR_DPP_SHL(head, 1);
    return (lane16 == 15u || next_head != 0) && pix != 0xffffffffu;
}
RR_DEV bool fits25i(int a, int b, int c) { // |a|, |b|, |c| < 2^25
    return (((uint32_t)(a + (1 << 25)) | (uint32_t)(b + (1 << 25)) | (uint32_t)(c + (1 << 25))) >> 26) == 0u;
}
RR_DEV void accum_merged_runs(const DAccum& acc, uint32_t pix, int r, int g, int b) {
    unsigned long long* p = (unsigned long long*)acc.rgb + pix; // one plane per channel
    if (__ballot(!fits25i(r, g, b)) == 0ull) {
        int w[3] = {r, g, b};
        if (wave_merge_runs32<3>(pix, w)) {
            if (w[0]) atomicAdd(p, (unsigned long long)(long long)w[0]);
            if (w[1]) atomicAdd(p + acc.n, (unsigned long long)(long long)w[1]);
            if (w[2]) atomicAdd(p + 2ull * acc.n, (unsigned long long)(long long)w[2]);
        }
        return;
    }
    unsigned long long v[3] = {(unsigned long long)(long long)r, (unsigned long long)(long long)g, (unsigned long long)(long long)b};
    if (wave_merge_runs<3>(pix, v)) {
        if (v[0]) atomicAdd(p, v[0]);
        if (v[1]) atomicAdd(p + acc.n, v[1]);
        if (v[2]) atomicAdd(p + 2ull * acc.n, v[2]);
    }
}
// The aux outputs of the root hits (normal and depth sums, reference src/raytracing.rs:400-402), merged the same way:
// the samples of a pixel sit in neighbouring lanes, and 64 lanes adding to one address serialise in the L2 atomic
// units (measured: k_shade 6.5 -> 42.8 ms on sponza_syn when the four aux adds of every primary hit went out unmerged).
RR_DEV void accum_aux_merged_runs(const DAccum& acc, uint32_t pix, int nx, int ny, int nz, int depth) {
    if (__ballot(!fits25i(nx, ny, nz) || !fits25i(depth, 0, 0)) == 0ull) {
        int w[4] = {nx, ny, nz, depth};
        if (wave_merge_runs32<4>(pix, w)) {
            if (acc.normal) {
                unsigned long long* np = (unsigned long long*)acc.normal + pix;
                if (w[0]) atomicAdd(np, (unsigned long long)(long long)w[0]);
                if (w[1]) atomicAdd(np + acc.n, (unsigned long long)(long long)w[1]);
                if (w[2]) atomicAdd(np + 2ull * acc.n, (unsigned long long)(long long)w[2]);
            }
            if (acc.depth && w[3]) atomicAdd((unsigned long long*)acc.depth + pix, (unsigned long long)(long long)w[3]);
        }
        return;
    }
    unsigned long long v[4] = {(unsigned long long)(long long)nx, (unsigned long long)(long long)ny, (unsigned long long)(long long)nz, (unsigned long long)(long long)depth};
    if (wave_merge_runs<4>(pix, v)) {
        if (acc.normal) {
            unsigned long long* np = (unsigned long long*)acc.normal + pix;
            if (v[0]) atomicAdd(np, v[0]);
            if (v[1]) atomicAdd(np + acc.n, v[1]);
            if (v[2]) atomicAdd(np + 2ull * acc.n, v[2]);
        }
        if (acc.depth && v[3]) atomicAdd((unsigned long long*)acc.depth + pix, v[3]);
    }
}

// Depth terms beyond the 32-bit lane sums (|depth * 2^16| >= 2^25: a root hit farther than 512 units -- a scene modelled in centimetres,
// a far background), merged like everything else: round 3 sent each of them to its accumulator word as an atomic of its own, 64 lanes
// of a level-1 packet to ONE word (the cliff accum_aux_merged's comment describes, for depth alone).  All 64 lanes.
RR_DEV void accum_depth_wide_merged_runs(const DAccum& acc, uint32_t pix, long long depth) {
    unsigned long long v[1] = {(unsigned long long)depth};
    if (wave_merge_runs<1>(pix, v) && acc.depth && v[0]) atomicAdd((unsigned long long*)acc.depth + pix, v[0]);
}

// ---------------------------------------------------------------------------
// Waves of ONE pixel.  With a sample group of 64 every level-1 packet is 64 samples of one pixel, and the segmented scan above is the
// general answer to a special question: four runs, one per DPP row, each with a head flag, a flag shift, a select and an add per value
// and step, and four atomics to the SAME word per channel.  Such a wave needs a plain sum: six DPP adds per value (four inside the rows,
// row_bcast:15, row_bcast:31) leave it in lane 63; lane k then takes channel k's total, and the packet's adds leave as ONE atomic
// instruction, one lane per channel.  (Lane 63 issuing one instruction per channel was measured first and is slower than the scan: what
// a packet pays for is the number of atomic instructions)  The entries below test for the case (two ballots and a
// readlane) and hand every other wave -- several pixels, smaller sample groups -- to the *_runs forms above, unchanged; the kernels call
// them where a one-pixel packet can occur and the registers allow it (k_shade<true, false>, k_trace_shadow<true, false>), and the *_runs
// forms everywhere else.  Integer adds commute: the pixel's sum is the same integer either way.
// ---------------------------------------------------------------------------
#define RR_DPP_ADD(v, ctrl) (v) += __builtin_amdgcn_update_dpp(0, (v), ctrl, 0xf, 0xf, true)
#define RR_DPP_ADD_ROWS(v, ctrl, rows) (v) += __builtin_amdgcn_update_dpp(0, (v), ctrl, rows, 0xf, false) // (the other rows add 0)
// Do the lanes that have a pixel (a, or b where a lane has no a) all have the same one?  0: no lane has a pixel; 1: yes, *p0; 2: no.
RR_DEV int wave_one_pixel(uint32_t a, uint32_t b, uint32_t* p0) {
    const uint32_t any = a != 0xffffffffu ? a : b;
    const unsigned long long live = __ballot(any != 0xffffffffu);
    if (live == 0ull) return 0;
    const uint32_t first = (uint32_t)__builtin_amdgcn_readlane((int)any, (int)__builtin_ctzll(live));
    *p0 = first;
    return __ballot((a != 0xffffffffu && a != first) || (b != 0xffffffffu && b != first)) == 0ull ? 1 : 2;
}
// The sums of v[0..N) over the 64 lanes, in lane 63 (the other lanes are left with partial sums).  Wraps like any 32-bit add: the
// callers bound their terms (fits25).
template <int N> RR_DEV void wave_sum32(int (&v)[N]) {
#pragma unroll
    for (int k = 0; k < N; k++) RR_DPP_ADD(v[k], 0xB1); // quad_perm [1,0,3,2]
#pragma unroll
    for (int k = 0; k < N; k++) RR_DPP_ADD(v[k], 0x4E); // quad_perm [2,3,0,1]
#pragma unroll
    for (int k = 0; k < N; k++) RR_DPP_ADD(v[k], 0x141); // row_half_mirror
#pragma unroll
    for (int k = 0; k < N; k++) RR_DPP_ADD(v[k], 0x140); // row_mirror: every lane holds its row's sum
#pragma unroll
    for (int k = 0; k < N; k++) RR_DPP_ADD_ROWS(v[k], 0x142, 0xa); // row_bcast:15 into rows 1 and 3
#pragma unroll
    for (int k = 0; k < N; k++) RR_DPP_ADD_ROWS(v[k], 0x143, 0xc); // row_bcast:31 into rows 2 and 3
}
// The same for one 64-bit value (the halves move separately, the add carries): 24 instructions instead of 6, for the rare wide depth.
RR_DEV unsigned long long wave_sum64(unsigned long long v) {
#define RR_SUM64_STEP(ctrl, rows, bc)                                                                                      \
    v += ((unsigned long long)(uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)(v >> 32), ctrl, rows, 0xf, bc) << 32) | \
         (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)v, ctrl, rows, 0xf, bc);
    RR_SUM64_STEP(0xB1, 0xf, true) RR_SUM64_STEP(0x4E, 0xf, true) RR_SUM64_STEP(0x141, 0xf, true) RR_SUM64_STEP(0x140, 0xf, true)
    RR_SUM64_STEP(0x142, 0xa, false) RR_SUM64_STEP(0x143, 0xc, false)
#undef RR_SUM64_STEP
    return v;
}
// |w[k]| bounds of the 32-bit wave sum: fits25 admits -2^25 <= w < 2^25 (fits25i's test), so 64 terms sum within
// [-64 * 2^25, 64 * (2^25 - 1)] = [-2^31, 2^31 - 64]: an int holds the total exactly (tests/test_gpu_wave_sums.py adds 64 of each end).
template <int N> RR_DEV bool fits25(const int (&w)[N]) {
    uint32_t m = 0u;
#pragma unroll
    for (int k = 0; k < N; k++) m |= (uint32_t)(w[k] + (1 << 25));
    return (m >> 26) == 0u;
}
// The totals side by side: lane k < N takes channel k's total from lane 63 (a readlane and a select each), so that the N adds of a
// packet leave as ONE atomic instruction with N lanes on N planes instead of N instructions with one lane each (the next packet's
// first load waits for every one of them: vector memory operations are counted in order).  The other lanes hold 0.
template <int N> RR_DEV int totals_to_lanes(const int (&w)[N]) {
    const int lane = (int)(threadIdx.x & 63u);
    int t = 0;
#pragma unroll
    for (int k = 0; k < N; k++) { const int total = __builtin_amdgcn_readlane(w[k], 63); if (lane == k) t = total; }
    return t;
}
// The entries.  A lane without a pixel may hold anything in its values (the *_runs forms discard its run): the wave sums need zeros
// there, written in place before the bound is tested, so that the *_runs forms' own bound ballot is the same expression.  A wave of
// one pixel with a term beyond 2^25 (rare: a saturating highlight) keeps the segmented 64-bit scan.
RR_DEV void accum_merged(const DAccum& acc, uint32_t pix, int r, int g, int b) {
    uint32_t p0 = 0u;
    const int one = wave_one_pixel(pix, 0xffffffffu, &p0);
    if (one == 0) return;
    if (pix == 0xffffffffu) r = g = b = 0;
    if (one == 1 && __ballot(!fits25i(r, g, b)) == 0ull) {
        int w[3] = {r, g, b};
        wave_sum32<3>(w);
        const int t = totals_to_lanes<3>(w);
        const uint32_t lane = threadIdx.x & 63u; // channel `lane`; a zero total adds nothing, as in the *_runs forms
        if (lane < 3u && t) atomicAdd((unsigned long long*)acc.rgb + lane * acc.n + p0, (unsigned long long)(long long)t);
    } else accum_merged_runs(acc, pix, r, g, b);
}
RR_DEV void accum_aux_merged(const DAccum& acc, uint32_t pix, int nx, int ny, int nz, int depth) {
    uint32_t p0 = 0u;
    const int one = wave_one_pixel(pix, 0xffffffffu, &p0);
    if (one == 0) return;
    if (pix == 0xffffffffu) nx = ny = nz = depth = 0;
    if (one == 1 && __ballot(!fits25i(nx, ny, nz) || !fits25i(depth, 0, 0)) == 0ull) {
        int w[4] = {nx, ny, nz, depth};
        wave_sum32<4>(w);
        const int t = totals_to_lanes<4>(w);
        const uint32_t lane = threadIdx.x & 63u;
        long long* plane = lane < 3u ? acc.normal : acc.depth; // (either may be absent)
        const uint32_t ch = lane < 3u ? lane : 0u;
        if (lane < 4u && t && plane) atomicAdd((unsigned long long*)plane + ch * acc.n + p0, (unsigned long long)(long long)t);
    } else accum_aux_merged_runs(acc, pix, nx, ny, nz, depth);
}
RR_DEV void accum_depth_wide_merged(const DAccum& acc, uint32_t pix, long long depth) {
    uint32_t p0 = 0u;
    const int one = wave_one_pixel(pix, 0xffffffffu, &p0);
    if (one == 0) return;
    if (one == 1) { // (a depth term is clamped to 1e9 * 2^16 < 2^46: 64 of them are far inside 64 bits)
        const unsigned long long t = wave_sum64(pix != 0xffffffffu ? (unsigned long long)depth : 0ull);
        if ((threadIdx.x & 63u) == 63u && acc.depth && t) atomicAdd((unsigned long long*)acc.depth + p0, t);
    } else accum_depth_wide_merged_runs(acc, pix, depth);
}
// A shaded hit's colour sums and its root's aux sums together (k_shade: sum_pix and aux_pix are the hit's own pixel, where set): one
// test, one bound ballot and seven sums where the wave's colour lanes and aux lanes name one pixel, the two entries above otherwise.
RR_DEV void accum_hit_merged(const DAccum& acc, uint32_t sum_pix, int r, int g, int b, uint32_t aux_pix, int nx, int ny, int nz, int depth) {
    uint32_t p0 = 0u;
    const int one = wave_one_pixel(sum_pix, aux_pix, &p0);
    if (sum_pix == 0xffffffffu) r = g = b = 0;
    if (aux_pix == 0xffffffffu) nx = ny = nz = depth = 0;
    int w[7] = {r, g, b, nx, ny, nz, depth};
    if (one == 1 && __ballot(!fits25(w)) == 0ull) {
        wave_sum32<7>(w);
        const int t = totals_to_lanes<7>(w);
        const uint32_t lane = threadIdx.x & 63u;
        long long* plane = lane < 3u ? acc.rgb : (lane < 6u ? acc.normal : acc.depth); // (normal or depth may be absent)
        const uint32_t ch = lane < 3u ? lane : (lane < 6u ? lane - 3u : 0u);
        if (lane < 7u && t && plane) atomicAdd((unsigned long long*)plane + ch * acc.n + p0, (unsigned long long)(long long)t);
    } else {
        accum_merged(acc, sum_pix, r, g, b);
        accum_aux_merged(acc, aux_pix, nx, ny, nz, depth);
    }
}

// ---------------------------------------------------------------------------
// resolving a slot: the sums as the f32 means the reference holds (src/raytracing.rs:406-426), before any clamp (k_resolve, k_resolve_rays).
// `nf`: the slot's acc.flags word; `n`: the number of samples as a float
// ---------------------------------------------------------------------------
RR_DEV float from_fix(long long sum) { return (float)((double)sum * (1.0 / 16777216.0)); } // RR_FIX_SCALE
// (the *_sum forms take the slot's integer sums themselves: k_resolve_pixel_parts resolves sums it formed across lanes)
RR_DEV float resolve_color_sum(long long fix, uint32_t nf, int k, float n) { // channel k
    float sum = from_fix(fix);
    // what the reference's f32 sum would hold if a sample was not finite: NaN (also +inf + -inf) or +-inf
    const bool pinf = (nf >> (3 + k)) & 1u, ninf = (nf >> (6 + k)) & 1u;
    if (((nf >> k) & 1u) || (pinf && ninf)) sum = __builtin_nanf("");
    else if (pinf) sum = __builtin_inff();
    else if (ninf) sum = -__builtin_inff();
    return sum / n;
}
RR_DEV float resolve_color(const DAccum& acc, uint32_t p, uint32_t nf, int k, float n) { // channel k
    return resolve_color_sum(acc.rgb[(unsigned long long)k * acc.n + p], nf, k, n);
}
RR_DEV f3 resolve_normal_sum(long long fx, long long fy, long long fz, uint32_t nf, float n) {
    f3 nn = mk3(from_fix(fx) / n, from_fix(fy) / n, from_fix(fz) / n);
    if (nf & (RR_NF_NORMAL_NAN * 7u)) { // a NaN sample normal poisons its component, and through the norm all three
        if (nf & RR_NF_NORMAL_NAN) nn.x = __builtin_nanf("");
        if (nf & (RR_NF_NORMAL_NAN << 1)) nn.y = __builtin_nanf("");
        if (nf & (RR_NF_NORMAL_NAN << 2)) nn.z = __builtin_nanf("");
    }
    return normalize3(nn); // 0/0 = NaN where every ray missed, as in the reference (:426)
}
RR_DEV f3 resolve_normal(const DAccum& acc, uint32_t p, uint32_t nf, float n) {
    return resolve_normal_sum(acc.normal[p], acc.normal[acc.n + p], acc.normal[2ull * acc.n + p], nf, n);
}
RR_DEV float resolve_depth_sum(long long fix, uint32_t nf, float n) {
    return (nf & RR_NF_DEPTH_NAN) ? __builtin_nanf("") : (float)((double)fix * (1.0 / 65536.0)) / n; // RR_DEPTH_SCALE
}
RR_DEV float resolve_depth(const DAccum& acc, uint32_t p, uint32_t nf, float n) { return resolve_depth_sum(acc.depth[p], nf, n); }

// An rr_radiance as the device moves it: two float4 = (colour rgb, depth), (normal xyz, bits(object id)); record o of `out` is its pair.
struct Record { float4 color_depth, normal_id; };
RR_DEV Record load_record(const float4* __restrict__ in, unsigned long long i) { return Record{in[2ull * i], in[2ull * i + 1]}; }
RR_DEV void store_record(float4* __restrict__ out, unsigned long long o, const Record& r) { out[2ull * o] = r.color_depth; out[2ull * o + 1] = r.normal_id; }
// the seven integer sums of slot p (colour r g b, normal x y z, depth), and their record over n samples: what k_resolve computes BEFORE
// its clamp.  The kernels that form a pixel's sums across lanes or slots resolve them through the same function, so a pixel has the bytes
// one slot would have given it (integer adds commute).
enum { RECORD_SUMS = 7 };
RR_DEV void load_slot_sums(const DAccum& acc, uint32_t p, long long (&w)[RECORD_SUMS]) {
#pragma unroll
    for (int k = 0; k < 3; k++) { w[k] = acc.rgb[(unsigned long long)k * acc.n + p]; w[3 + k] = acc.normal[(unsigned long long)k * acc.n + p]; }
    w[6] = acc.depth[p];
}
RR_DEV Record resolve_record_sums(const long long (&w)[RECORD_SUMS], uint32_t nf, uint32_t id, float n) {
    float c[3];
#pragma unroll
    for (int k = 0; k < 3; k++) c[k] = resolve_color_sum(w[k], nf, k, n);
    const f3 nn = resolve_normal_sum(w[3], w[4], w[5], nf, n);
    return Record{make_float4(c[0], c[1], c[2], resolve_depth_sum(w[6], nf, n)), make_float4(nn.x, nn.y, nn.z, __uint_as_float(id))};
}
RR_DEV Record resolve_record(const DAccum& acc, uint32_t p, float n) {
    long long w[RECORD_SUMS];
    load_slot_sums(acc, p, w);
    return resolve_record_sums(w, acc.flags[p], acc.object_id[p], n);
}

#undef RR_DPP_SHR
#undef RR_DPP_ADD
#undef RR_DPP_ADD_ROWS
#undef RR_DPP_SHL
#undef RR_DPP_SHR64
#undef RR_SEG_STEP
#undef RR_SEG_STEP32
