// rr_accumulate.h — layer 5 of the device code: the per-pixel fixed-point accumulators that stand for the reference's f32 sums
// over samples (src/raytracing.rs:400-417).  Integer adds commute, so the frame does not depend on the order of anything.
//
// Offers: to_fix, fix_add, nonfinite_flags, accum_merged, accum_aux_merged, accum_depth_wide_merged (the last three must be
// called by all 64 lanes of a wave); from_fix, resolve_color, resolve_normal, resolve_depth (and their *_sum forms).  wave_merge_runs /
// wave_merge_runs32 / fits25i are this layer's own, and so are its DPP macros (RR_DPP_*, RR_SEG_STEP, RR_SEG_STEP32),
// un-defined at the end.
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
RR_DEV void fix_add(int& n, float v, float scale, float clampv, long long* plane, uint32_t pix) {
    const float x = v * scale;
    if (rr_abs(x) < 33554432.0f) n += __float2int_rn(x); // (inside every clamp in use: |v| < 2 at scale 2^24, < 512 at 2^16)
    else { const long long t = to_fix(v, scale, clampv); if (t != 0ll && plane) atomicAdd((unsigned long long*)plane + pix, (unsigned long long)t); }
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
RR_DEV void accum_merged(const DAccum& acc, uint32_t pix, int r, int g, int b) {
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
RR_DEV void accum_aux_merged(const DAccum& acc, uint32_t pix, int nx, int ny, int nz, int depth) {
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
RR_DEV void accum_depth_wide_merged(const DAccum& acc, uint32_t pix, long long depth) {
    unsigned long long v[1] = {(unsigned long long)depth};
    if (wave_merge_runs<1>(pix, v) && acc.depth && v[0]) atomicAdd((unsigned long long*)acc.depth + pix, v[0]);
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

#undef RR_DPP_SHR
#undef RR_DPP_SHL
#undef RR_DPP_SHR64
#undef RR_SEG_STEP
#undef RR_SEG_STEP32
