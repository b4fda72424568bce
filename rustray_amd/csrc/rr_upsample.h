// rr_upsample.h — the arithmetic of the joint-bilateral upsampler that host and device share (rr_upsample_records; the yardstick is
// rustray_amd/upsample.py: upsample_records): where a full-resolution pixel lies in the low frame, the flags of a guide, the weight of
// one of its four taps, the guided sum with its bilinear fallback, and the guide fields of the record that leaves.  Plain host logic, no
// HIP calls; the one include is rr_denoise.h, whose denoise_is_finite, denoise_demodulate / denoise_remodulate, DN_EPS and DN_FLT_MAX
// are used here as they stand.  k_upsample_records (rr_kernels.hip) applies these functions per lane, and tests/native/upsample_test.cpp
// runs the same functions as a host loop.
//
// Every step is exact in binary32 in the order written here (products, sums, one correctly rounded division at a time; floorf is exact)
// and must be compiled without contraction (-ffp-contract=off, as the library is): host, device and numpy give the same bits.  There
// are no transcendentals: the weights are rational functions.
//
// A half colour that is not finite at a taken tap PROPAGATES: only the colour of low[q] decides whether q is a tap (fin_q), and the
// halves are summed with the colour's weights, so wt * inf or wt * NaN (0 * inf included) reaches the half's sum as it is.
#pragma once
#include "rr_denoise.h"

enum { UP_TILE_W = 32, UP_TILE_H = 8 };   // full pixels of a workgroup
// The low-frame patch such a tile reads.  x0 is monotone in x, and over the 31 steps of a tile row u grows by 31 w / W <= 31 (plus a
// few roundings of at most 2^-8 each): floor(u) grows by at most 32, and with the tap to its right a row touches at most 34 columns;
// a tile's 8 rows touch at most 8 + 2 low rows in the same way.
enum { UP_PATCH_W = UP_TILE_W + 2, UP_PATCH_H = UP_TILE_H + 2 };

// The guide fields of a record whose pixel missed, as rr_render_pixels writes them for a pixel all of whose rays missed: depth +0
// (0x00000000), object_id 0, and in each normal float the NaN the device's correctly rounded 0 / 0 gives, 0xffc00000.
#define UP_MISS_NORMAL_BITS 0xffc00000u

// what the sum reads of a surface record: rows 0, 1, 2 and 4 of rr_surface_hit (hit, object_id; distance; normal; base_color[0 .. 2])
struct UpGuide {
    float n[3], z;
    float albedo[3];
    unsigned int id;
    bool hit, valid;   // valid: hit, and distance and the three normal floats are finite
};
// one pixel of the low frame: its colour, with halves the colours of its two halves, its guide
struct UpTap {
    float c[3];
    float h[2][3];
    UpGuide g;
    bool fin;          // the three colour floats of low[q] are finite
};
// the call's parameters as the sum takes them; r = max((float)W / (float)w, (float)H / (float)h), formed once on the host
struct UpCall {
    float sigma_depth, r;
    unsigned int normal_power_log2, use_albedo;
};
struct UpResult {
    float c[3];
    float h[2][3];
    float weight;      // sum_w of the guided sum; 0 where the fallback answered
};

RR_SETUP_HD float upsample_ratio(unsigned int W, unsigned int H, unsigned int w, unsigned int h) {
    const float rx = (float)W / (float)w, ry = (float)H / (float)h;
    return rx > ry ? rx : ry;
}
// full coordinate x of a frame `full` wide in a low frame `low` wide: the left tap x0 (-1 .. low - 1) and the weight fx of the right one
RR_SETUP_HD void upsample_position(int x, unsigned int low, unsigned int full, int* x0, float* fx) {
    const float u = (((float)x + 0.5f) * (float)low) / (float)full - 0.5f;
    *x0 = (int)__builtin_floorf(u);
    *fx = u - (float)*x0;
}
RR_SETUP_HD UpGuide upsample_guide(unsigned int hit, unsigned int object_id, float distance, const float* normal, const float* base_color) {
    UpGuide g;
    g.hit = hit != 0u;
    g.id = object_id;
    g.z = distance;
    for (int k = 0; k < 3; k++) { g.n[k] = normal[k]; g.albedo[k] = base_color[k]; }
    g.valid = g.hit && denoise_is_finite(distance) && denoise_is_finite(normal[0]) && denoise_is_finite(normal[1]) && denoise_is_finite(normal[2]);
    return g;
}
RR_SETUP_HD bool upsample_fin(const float* c) { return denoise_is_finite(c[0]) && denoise_is_finite(c[1]) && denoise_is_finite(c[2]); }
// is q a tap of the guided sum of p (q lies inside the low frame)
RR_SETUP_HD bool upsample_tap_taken(const UpGuide& p, const UpTap& q) {
    if (!q.fin || q.g.hit != p.hit) return false;
    if (p.hit && q.g.id != p.id) return false;
    return q.g.valid == p.valid;
}
// the weight of a taken tap whose bilinear weight is b
RR_SETUP_HD float upsample_tap_weight(const UpCall& call, const UpGuide& p, const UpGuide& q, float b) {
    float wt = b;
    if (p.valid) {
        float cs = (p.n[0] * q.n[0] + p.n[1] * q.n[1]) + p.n[2] * q.n[2];
        cs = cs > 0.0f ? cs : 0.0f;
        for (unsigned int k = 0; k < call.normal_power_log2; k++) cs = cs * cs;
        wt = wt * cs;
        const float t = __builtin_fabsf(p.z - q.z) / ((call.sigma_depth * __builtin_fabsf(p.z)) * call.r + DN_EPS);
        wt = wt / (1.0f + t * t);
    }
    return wt;
}

// One full pixel: (x0, fx), (y0, fy) from upsample_position, p the full guide of the pixel; fetch(qx, qy, &q) gives the low pixel
// (qx, qy), false = outside the low frame.  The four taps are read once and serve the guided sum and, where that is weightless, the
// fallback: the bilinear mean of the taps with a finite colour, no guide and no albedo; three zeros where there is none.
template <bool HALVES, class Fetch>
RR_SETUP_HD void upsample_pixel(const UpCall& call, int x0, float fx, int y0, float fy, const UpGuide& p, Fetch fetch, UpResult* out) {
    UpTap q[4];
    bool inside[4];
    float b[4];
    for (int dy = 0; dy < 2; dy++)
        for (int dx = 0; dx < 2; dx++) {
            const int k = 2 * dy + dx;
            inside[k] = fetch(x0 + dx, y0 + dy, &q[k]);
            b[k] = (dx ? fx : 1.0f - fx) * (dy ? fy : 1.0f - fy);
        }
    float sum_c[3] = {0.0f, 0.0f, 0.0f}, sum_h[2][3] = {{0.0f, 0.0f, 0.0f}, {0.0f, 0.0f, 0.0f}}, sum_w = 0.0f;
    for (int k = 0; k < 4; k++) {
        if (!inside[k] || !upsample_tap_taken(p, q[k])) continue;
        const float wt = upsample_tap_weight(call, p, q[k].g, b[k]);
        const bool demod = call.use_albedo && p.hit; // (a taken tap is hit exactly when p is)
        for (int c = 0; c < 3; c++) {
            sum_c[c] += wt * (demod ? denoise_demodulate(q[k].c[c], q[k].g.albedo[c]) : q[k].c[c]);
            if (HALVES)
                for (int s = 0; s < 2; s++) sum_h[s][c] += wt * (demod ? denoise_demodulate(q[k].h[s][c], q[k].g.albedo[c]) : q[k].h[s][c]);
        }
        sum_w += wt;
    }
    if (sum_w > 0.0f && sum_w <= DN_FLT_MAX) {
        const bool remod = call.use_albedo && p.hit;
        for (int c = 0; c < 3; c++) {
            const float v = sum_c[c] / sum_w;
            out->c[c] = remod ? denoise_remodulate(v, p.albedo[c]) : v;
            for (int s = 0; s < 2; s++) {
                const float hv = HALVES ? sum_h[s][c] / sum_w : 0.0f;
                out->h[s][c] = HALVES && remod ? denoise_remodulate(hv, p.albedo[c]) : hv;
            }
        }
        out->weight = sum_w;
        return;
    }
    float sum_b = 0.0f;
    for (int c = 0; c < 3; c++) sum_c[c] = sum_h[0][c] = sum_h[1][c] = 0.0f;
    for (int k = 0; k < 4; k++) {
        if (!inside[k] || !q[k].fin) continue;
        for (int c = 0; c < 3; c++) {
            sum_c[c] += b[k] * q[k].c[c];
            if (HALVES)
                for (int s = 0; s < 2; s++) sum_h[s][c] += b[k] * q[k].h[s][c];
        }
        sum_b += b[k];
    }
    const bool ok = sum_b > 0.0f && sum_b <= DN_FLT_MAX;
    for (int c = 0; c < 3; c++) {
        out->c[c] = ok ? sum_c[c] / sum_b : 0.0f;
        for (int s = 0; s < 2; s++) out->h[s][c] = HALVES && ok ? sum_h[s][c] / sum_b : 0.0f;
    }
    out->weight = 0.0f;
}

// The guide fields of out[p] and of both halves_out records, as bits: for a hit the full guide's distance, normal and object_id -- a
// frame's record holds the id of the item its last sample hit as that item's id itself, so for a pixel all of whose rays hit the item
// the bits are the guide's; for a miss the bits above.  The result is an input of rr_denoise_records, rr_accumulate_records and
// rr_motion_records at W x H.
RR_SETUP_HD void upsample_guide_fields(const UpGuide& p, unsigned int* depth, unsigned int* normal, unsigned int* id) {
    if (p.hit) {
        __builtin_memcpy(depth, &p.z, 4);
        __builtin_memcpy(normal, p.n, 12);
        *id = p.id;
    } else {
        *depth = 0u;
        normal[0] = normal[1] = normal[2] = UP_MISS_NORMAL_BITS;
        *id = 0u;
    }
}
