// rr_denoise.h — the arithmetic of the edge-avoiding a-trous filter that host and device share (rr_denoise_records; the yardstick is
// rustray_amd/denoise.py: atrous_denoise): the luminance, the demodulation rule, the variance seed of a pixel's two halves and its 3x3
// prefilter weights, the flags of a pixel, the weight of one tap and the 25 taps of one pixel in one pass.  Plain host logic, no HIP calls
// and no include of its own: the kernels of rr_kernels.hip (k_denoise_prepare, k_denoise_pass_gather, k_denoise_pass_tile,
// k_denoise_finish) apply these functions per lane, and tests/native/denoise_test.cpp runs the same functions as a host loop.
//
// Every step is exact in binary32 in the order written here (products, sums, one correctly rounded division or square root at a time)
// and must be compiled without contraction (-ffp-contract=off, as the library is): host, device and numpy give the same bits.  There
// are no transcendentals: the weights are rational functions.
#pragma once

#ifndef RR_SETUP_HD // (rr_primary_setup.h, rr_pixel_list.h and rr_adaptive.h define the same)
#if defined(__HIPCC__)
#define RR_SETUP_HD __host__ __device__ inline
#else
#define RR_SETUP_HD inline
#endif
#endif

enum { DN_FIN = 1u, DN_VALID = 2u, DN_ABSENT = 4u }; // flags of a pixel: colour finite; depth and normal finite; (tiles only) no pixel here
#define DN_EPS 9.5367431640625e-07f                // 2^-20
#define DN_ALBEDO_MIN 0.0009765625f                // 2^-10
#define DN_FLT_MAX 3.402823466e+38f

// what a pass reads of one pixel: the working colour and variance, and the packed guide
struct DnTap {
    float c[3], var;
    float n[3], z;
    unsigned int id, flags;
};
// what the call's parameters come to inside a pass
struct DnPass {
    float sigma_depth, sigma_luminance;
    unsigned int normal_power_log2;
    unsigned int halves; // non-zero: the luminance weight is used
    int step;            // 2^i
};

RR_SETUP_HD bool denoise_is_finite(float v) { return __builtin_fabsf(v) <= DN_FLT_MAX; } // false for NaN and both infinities
RR_SETUP_HD float denoise_lum(const float* c) { return (0.2126f * c[0] + 0.7152f * c[1]) + 0.0722f * c[2]; }
// channel k of a colour over the albedo: divided where 2^-10 < a <= FLT_MAX, else left as it is (false for a NaN albedo)
RR_SETUP_HD bool denoise_albedo_used(float a) { return a > DN_ALBEDO_MIN && a <= DN_FLT_MAX; }
RR_SETUP_HD float denoise_demodulate(float c, float a) { return denoise_albedo_used(a) ? c / a : c; }
RR_SETUP_HD float denoise_remodulate(float c, float a) { return denoise_albedo_used(a) ? c * a : c; }

// the flags of a record: colour, depth, normal as rr_radiance holds them
RR_SETUP_HD unsigned int denoise_flags(const float* color, float depth, const float* normal) {
    const bool fin = denoise_is_finite(color[0]) && denoise_is_finite(color[1]) && denoise_is_finite(color[2]);
    const bool valid = denoise_is_finite(depth) && denoise_is_finite(normal[0]) && denoise_is_finite(normal[1]) && denoise_is_finite(normal[2]);
    return (fin ? (unsigned int)DN_FIN : 0u) | (valid ? (unsigned int)DN_VALID : 0u);
}

// The variance seed of a pixel: a, b = the colours of its two halves as the records hold them, albedo = its three albedo floats or NULL.
// Finiteness is judged on the six floats as given; the luminances are those of the demodulated halves.
RR_SETUP_HD float denoise_variance_seed(bool fin, const float* a, const float* b, const float* albedo) {
    if (!fin) return 0.0f;
    for (int k = 0; k < 3; k++)
        if (!denoise_is_finite(a[k]) || !denoise_is_finite(b[k])) return 0.0f;
    float da[3], db[3];
    for (int k = 0; k < 3; k++) {
        da[k] = albedo ? denoise_demodulate(a[k], albedo[k]) : a[k];
        db[k] = albedo ? denoise_demodulate(b[k], albedo[k]) : b[k];
    }
    const float d = (denoise_lum(da) - denoise_lum(db)) * 0.5f;
    return d * d;
}
// the 3x3 prefilter of the seeds: {1/2, 1/4}[|dx|] * {1/2, 1/4}[|dy|]
RR_SETUP_HD float denoise_prefilter_weight(int dx, int dy) { return (dx ? 0.25f : 0.5f) * (dy ? 0.25f : 0.5f); }
// seed(dx, dy, &v): false = no tap there (outside the frame or not DN_FIN); row-major, dy outer
template <class Seed>
RR_SETUP_HD float denoise_prefilter(Seed seed) {
    float sum_v = 0.0f, sum_g = 0.0f;
    for (int dy = -1; dy <= 1; dy++)
        for (int dx = -1; dx <= 1; dx++) {
            float v;
            if (!seed(dx, dy, &v)) continue;
            const float g = denoise_prefilter_weight(dx, dy);
            sum_v += g * v;
            sum_g += g;
        }
    return sum_v / sum_g; // the centre is a tap of every DN_FIN pixel: sum_g >= 1/4
}

// the B3 spline: K = {3/8, 1/4, 1/16}
RR_SETUP_HD float denoise_spline(int d) { const int a = d < 0 ? -d : d; return a == 0 ? 0.375f : a == 1 ? 0.25f : 0.0625f; }

// is q a tap of p at all (both inside the frame; p is DN_FIN)
RR_SETUP_HD bool denoise_tap_taken(const DnTap& p, const DnTap& q) {
    return (q.flags & DN_FIN) && !(q.flags & DN_ABSENT) && q.id == p.id && ((q.flags ^ p.flags) & DN_VALID) == 0u;
}
// the weight of tap q = p + step * (dx, dy) for the pixel p; lum_p = denoise_lum(p.c), sd_p = sqrtf(p.var)
RR_SETUP_HD float denoise_tap_weight(const DnPass& pass, const DnTap& p, float lum_p, float sd_p, const DnTap& q, int dx, int dy) {
    float w = denoise_spline(dx) * denoise_spline(dy);
    if (p.flags & DN_VALID) {
        float cs = (p.n[0] * q.n[0] + p.n[1] * q.n[1]) + p.n[2] * q.n[2];
        cs = cs > 0.0f ? cs : 0.0f;
        for (unsigned int k = 0; k < pass.normal_power_log2; k++) cs = cs * cs;
        w = w * cs;
        if (dx != 0 || dy != 0) {
            const int ax = dx < 0 ? -dx : dx, ay = dy < 0 ? -dy : dy;
            const float t = __builtin_fabsf(p.z - q.z) / ((pass.sigma_depth * __builtin_fabsf(p.z)) * (float)(pass.step * (ax > ay ? ax : ay)) + DN_EPS);
            w = w / (1.0f + t * t);
        }
    }
    if (pass.halves) {
        const float t = __builtin_fabsf(lum_p - denoise_lum(q.c)) / (pass.sigma_luminance * sd_p + DN_EPS);
        w = w / (1.0f + t * t);
    }
    return w;
}

// One pixel of one pass: p is DN_FIN; fetch(dx, dy, &q) gives the tap at p + step * (dx, dy), false = outside the frame (fetch may also
// return false for a tap denoise_tap_taken would refuse).  out_c, *out_var: the pass's output for p.
template <class Fetch>
RR_SETUP_HD void denoise_pixel_pass(const DnPass& pass, const DnTap& p, Fetch fetch, float* out_c, float* out_var) {
    float sum_c[3] = {0.0f, 0.0f, 0.0f}, sum_v = 0.0f, sum_w = 0.0f;
    const float lum_p = denoise_lum(p.c), sd_p = __builtin_sqrtf(p.var);
    for (int dy = -2; dy <= 2; dy++)
        for (int dx = -2; dx <= 2; dx++) {
            DnTap q;
            if (!fetch(dx, dy, &q)) continue;
            if (!denoise_tap_taken(p, q)) continue;
            const float w = denoise_tap_weight(pass, p, lum_p, sd_p, q, dx, dy);
            for (int k = 0; k < 3; k++) sum_c[k] += w * q.c[k];
            sum_v += (w * w) * q.var;
            sum_w += w;
        }
    // a weightless pixel keeps its colour and variance for this pass: sum_w is 0 when the centre's own cs is (a zero normal, a short one
    // at a high power), inf or NaN when a dot product of huge normals overflows; false for NaN
    const bool ok = sum_w > 0.0f && sum_w <= DN_FLT_MAX;
    for (int k = 0; k < 3; k++) out_c[k] = ok ? sum_c[k] / sum_w : p.c[k];
    *out_var = ok ? sum_v / (sum_w * sum_w) : p.var;
}

// ---- where the passes run (host only): the three forms a pass kernel has, and what a forced choice comes to at a step
enum { DN_FORM_AUTO = 0, DN_FORM_GATHER = 1, DN_FORM_TILE = 2, DN_FORM_LATTICE = 3 };
enum { DN_TILE_W = 32, DN_TILE_H = 8, DN_TILE_MAX_HALO = 8 };
// A tile kernel works on the sub-lattice of period `lattice` (1 = the frame itself): taps lie step / lattice lattice points apart, the
// halo is twice that.  DN_FORM_TILE: lattice 1, for steps whose halo fits (step <= 4); DN_FORM_LATTICE: lattice = step, halo 2.
inline bool denoise_form_available(int form, int step) {
    return form == DN_FORM_GATHER || (form == DN_FORM_TILE && 2 * step <= DN_TILE_MAX_HALO) || (form == DN_FORM_LATTICE && step >= 2);
}
inline unsigned long long denoise_tile_entries(int halo) { return (unsigned long long)(DN_TILE_W + 2 * halo) * (DN_TILE_H + 2 * halo); }
