// rr_temporal.h — the arithmetic of the temporal reprojection that host and device share (rr_accumulate_records; the yardstick is
// rustray_amd/temporal.py: accumulate_records): the pinhole ray through a pixel's centre and the world point a record's depth puts on it,
// the reprojection into the previous frame, the tap list with its snap, the test of one history tap and the blend of one layer.  Plain
// host logic, no HIP call and no system include: the accumulation kernels (rr_kernels.hip, 7e .. 7e''') apply these functions per lane
// (7e and 7e' through temporal_pixel, rr_history_clamp.h), and tests/native/temporal_pixel_test.cpp runs that step as a host loop.
//
// Every step is exact in binary32 in the order written here (products, sums, one correctly rounded division or square root at a time)
// and must be compiled without contraction (-ffp-contract=off, as the library is): host, device and numpy give the same bits.  There
// are no transcendentals.
#pragma once
#include "rr_denoise.h"    // denoise_is_finite, denoise_flags (DN_FIN, DN_VALID), DN_EPS, DN_TILE_W, DN_TILE_H
#include "rr_pixel_list.h" // pixel_ray (and pixel_centre behind it), temporal_row, temporal_dot

#define TP_MIN_WEIGHT 0.015625f // 2^-6: a pixel whose taken taps weigh less has no history

// what a call comes to for one pixel: the current camera, the previous view and the scalars (a kernel argument: it travels in SGPRs)
struct TpFrame {
    float proj_inv[16], view_inv[16]; // rr_camera's, column-major
    float prev_clip[16];              // rr_accumulate_params::prev_world_to_clip, column-major
    float prev_eye[3];
    float w, h;                       // the frame's size as floats
    float max_history, normal_min, sigma_depth, snap;
    int width, height;
};
// where the history of a pixel is read: one tap at (x0, y0) with weight 1 (n = 1: snapped, tx = ty = 0), or the four bilinear taps
// (x0 + (k & 1), y0 + (k >> 1)), k = 0 .. 3, with weight (k & 1 ? tx : 1 - tx) * (k >> 1 ? ty : 1 - ty)
struct TpTaps {
    int x0, y0, n;
    float tx, ty;
};
// the history of a pixel: the weighted means of its taps and the blend factor
struct TpMix {
    float h[3], ha[3], hb[3]; // of the records and (with halves) of the two half-histories
    float length, a;          // N = min(len + 1, max_history) and 1 / N
};

// world = o + d * depth: o and d are the pinhole ray through the centre of pixel (x, y), d normalised
RR_SETUP_HD void temporal_world(const TpFrame& f, unsigned int x, unsigned int y, float depth, float* world) {
    float o[3], d[3];
    pixel_ray(f.proj_inv, f.view_inv, x | (y << 16), f.w, f.h, o, d);
    for (int r = 0; r < 3; r++) world[r] = o[r] + d[r] * depth;
}

// Where `prev`, a world point of the previous frame, lay on that frame's screen (in pixels: the centre of pixel (i, j) is (i, j)) and the
// depth its record held there.  false: behind the previous eye, not finite, or so far outside that no tap can lie inside the frame.
// A record's depth is the distance from its ray's origin, which lies on the plane one unit ahead of the eye: of the distance
// |prev - prev_eye| the part before that plane is dist / clip.w (clip.w of a perspective projection is the distance ahead of the eye).
RR_SETUP_HD bool temporal_reproject(const TpFrame& f, const float* prev, float* fx, float* fy, float* z_exp) {
    const float cx = temporal_row(f.prev_clip, 0, prev[0], prev[1], prev[2], 1.0f);
    const float cy = temporal_row(f.prev_clip, 1, prev[0], prev[1], prev[2], 1.0f);
    const float cw = temporal_row(f.prev_clip, 3, prev[0], prev[1], prev[2], 1.0f);
    if (!(cw > DN_EPS)) return false;
    *fx = ((cx / cw) * 0.5f + 0.5f) * f.w - 0.5f;
    *fy = (0.5f - (cy / cw) * 0.5f) * f.h - 0.5f;
    if (!denoise_is_finite(*fx) || !denoise_is_finite(*fy)) return false;
    if (!(*fx > -1.0f && *fx < f.w && *fy > -1.0f && *fy < f.h)) return false; // every tap would lie outside the frame
    const float e[3] = {prev[0] - f.prev_eye[0], prev[1] - f.prev_eye[1], prev[2] - f.prev_eye[2]};
    const float dist = __builtin_sqrtf(temporal_dot(e, e));
    *z_exp = dist - dist / cw;
    return true;
}

// the taps of a screen point (-1 < fx < width, -1 < fy < height): one when both coordinates lie within `snap` of a pixel centre
RR_SETUP_HD TpTaps temporal_taps(float fx, float fy, float snap) {
    TpTaps t;
    const float rx = __builtin_rintf(fx), ry = __builtin_rintf(fy);
    if (__builtin_fabsf(fx - rx) <= snap && __builtin_fabsf(fy - ry) <= snap) {
        t.x0 = (int)rx; t.y0 = (int)ry; t.n = 1; t.tx = 0.0f; t.ty = 0.0f;
    } else {
        const float x0 = __builtin_floorf(fx), y0 = __builtin_floorf(fy);
        t.x0 = (int)x0; t.y0 = (int)y0; t.n = 4; t.tx = fx - x0; t.ty = fy - y0;
    }
    return t;
}
RR_SETUP_HD float temporal_tap_weight(const TpTaps& t, int k) { return ((k & 1) ? t.tx : 1.0f - t.tx) * ((k >> 1) ? t.ty : 1.0f - t.ty); }

// the tests of one history tap, in the order its rows are read: the guide row (normal, id), then the colour row (colour, depth)
RR_SETUP_HD bool temporal_guide_ok(const TpFrame& f, unsigned int id_p, const float* n_p, unsigned int id_q, const float* n_q) {
    if (id_q != id_p) return false;
    if (!denoise_is_finite(n_q[0]) || !denoise_is_finite(n_q[1]) || !denoise_is_finite(n_q[2])) return false;
    return temporal_dot(n_p, n_q) >= f.normal_min; // (false for NaN)
}
RR_SETUP_HD bool temporal_colour_ok(const float* c) { return denoise_is_finite(c[0]) && denoise_is_finite(c[1]) && denoise_is_finite(c[2]); }
RR_SETUP_HD bool temporal_depth_ok(const TpFrame& f, float z_exp, float z_q) {
    return denoise_is_finite(z_q) && __builtin_fabsf(z_exp - z_q) <= f.sigma_depth * z_exp + DN_EPS;
}

// the history of a pixel's diffuse part (rr_accumulate_split_records): the means of the same taps under the same weights
struct TpSplitMix {
    float d[3], da[3], db[3]; // of `diffuse` and (with halves) of the two diffuse half-histories
};

// The history of pixel (x, y), whose record has DN_FIN and DN_VALID: its depth, normal and id, and its motion (3 floats, or NULL).
// hist gives the previous frame at pixel index q: length(q); guide(q, n, &id); colour(q, c, &z); with HALVES half(q, h, c); with SPLIT
// diffuse(q, c) and, with HALVES too, diffuse_half(q, h, c), read after the half rows of a tap that is taken: no diffuse value decides
// anything, so taps, weights, m and the answer are those of the build without SPLIT.  d is written with SPLIT only.
// false: the pixel takes the no-history path.
template <bool HALVES, class Hist, bool SPLIT = false>
RR_SETUP_HD bool temporal_history(const TpFrame& f, unsigned int x, unsigned int y, float depth, const float* n_p, unsigned int id_p, const float* motion,
                                  Hist hist, TpMix* m, TpSplitMix* d = nullptr) {
    float prev[3], fx, fy, z_exp;
    temporal_world(f, x, y, depth, prev);
    if (motion)
        for (int k = 0; k < 3; k++) prev[k] = prev[k] + motion[k];
    if (!temporal_reproject(f, prev, &fx, &fy, &z_exp)) return false;
    const TpTaps t = temporal_taps(fx, fy, f.snap);
    float sum_w = 0.0f, sum_l = 0.0f, sum_c[3] = {0.0f, 0.0f, 0.0f}, sum_a[3] = {0.0f, 0.0f, 0.0f}, sum_b[3] = {0.0f, 0.0f, 0.0f};
    float sum_d[3] = {0.0f, 0.0f, 0.0f}, sum_da[3] = {0.0f, 0.0f, 0.0f}, sum_db[3] = {0.0f, 0.0f, 0.0f};
    for (int k = 0; k < 4; k++) {
        if (k >= t.n) break;
        const int qx = t.x0 + (k & 1), qy = t.y0 + (k >> 1);
        if (qx < 0 || qy < 0 || qx >= f.width || qy >= f.height) continue;
        const unsigned long long q = (unsigned long long)qy * (unsigned int)f.width + (unsigned int)qx;
        float n_q[3], c_q[3], a_q[3], b_q[3], z_q;
        unsigned int id_q;
        hist.guide(q, n_q, &id_q);
        if (!temporal_guide_ok(f, id_p, n_p, id_q, n_q)) continue;
        hist.colour(q, c_q, &z_q);
        if (!temporal_colour_ok(c_q) || !temporal_depth_ok(f, z_exp, z_q)) continue;
        const float len_q = hist.length(q);
        if (!(len_q > 0.0f)) continue;
        if (HALVES) {
            hist.half(q, 0, a_q);
            hist.half(q, 1, b_q);
            if (!temporal_colour_ok(a_q) || !temporal_colour_ok(b_q)) continue;
        }
        const float w = temporal_tap_weight(t, k);
        for (int c = 0; c < 3; c++) sum_c[c] += w * c_q[c];
        if (HALVES)
            for (int c = 0; c < 3; c++) { sum_a[c] += w * a_q[c]; sum_b[c] += w * b_q[c]; }
        sum_l += w * len_q;
        sum_w += w;
        if constexpr (SPLIT) {
            float d_q[3], da_q[3], db_q[3];
            hist.diffuse(q, d_q);
            for (int c = 0; c < 3; c++) sum_d[c] += w * d_q[c];
            if (HALVES) {
                hist.diffuse_half(q, 0, da_q);
                hist.diffuse_half(q, 1, db_q);
                for (int c = 0; c < 3; c++) { sum_da[c] += w * da_q[c]; sum_db[c] += w * db_q[c]; }
            }
        }
    }
    if (!(sum_w >= TP_MIN_WEIGHT)) return false;
    for (int c = 0; c < 3; c++) {
        m->h[c] = sum_c[c] / sum_w;
        m->ha[c] = HALVES ? sum_a[c] / sum_w : 0.0f;
        m->hb[c] = HALVES ? sum_b[c] / sum_w : 0.0f;
    }
    const float n1 = sum_l / sum_w + 1.0f;
    m->length = n1 < f.max_history ? n1 : f.max_history; // (a NaN or infinite length becomes max_history)
    m->a = 1.0f / m->length;
    if constexpr (SPLIT)
        for (int c = 0; c < 3; c++) {
            d->d[c] = sum_d[c] / sum_w;
            d->da[c] = HALVES ? sum_da[c] / sum_w : 0.0f;
            d->db[c] = HALVES ? sum_db[c] / sum_w : 0.0f;
        }
    else { (void)d; (void)sum_d; (void)sum_da; (void)sum_db; }
    return true;
}

// one channel of one layer: the history moved towards the current colour by a
RR_SETUP_HD float temporal_blend(float h, float a, float cur) { return h + a * (cur - h); }

// one diffuse layer of a pixel that kept its history (rr_accumulate_split_records): blended where the current triple and the three
// history means are finite, the current bits otherwise.  out may be cur.
RR_SETUP_HD void temporal_blend_diffuse(const float* hd, float a, const float* cur, float* out) {
    const bool ok = temporal_colour_ok(cur) && temporal_colour_ok(hd);
    for (int c = 0; c < 3; c++) out[c] = ok ? temporal_blend(hd[c], a, cur[c]) : cur[c];
}
