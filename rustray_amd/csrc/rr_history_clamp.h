// rr_history_clamp.h — the arithmetic of the neighbourhood clamp that host and device share (rr_accumulate_clamped_records, steps 7 .. 9
// of its text in include/rustray_hip.h; the yardstick is rustray_amd/temporal.py: accumulate_clamped_records): the sums over the window
// of the current frame, the box they make, the clamp of one layer's history mean to it and the shorter length of a pixel whose record
// layer had to be moved.  history_clamp_split is the same for rr_accumulate_clamped_split_records (the yardstick is
// accumulate_clamped_split_records): the colour side as it stands, and a box of the current diffuse layer for the three diffuse means.
// At its end temporal_pixel, THE step of one pixel of the four accumulation calls between its loads and its stores.
// Plain host logic, no HIP call and no system include: accumulate_pixel_body (rr_kernels.hip, kernels 7e and 7e') applies temporal_pixel
// per lane, kernels 7e'' and 7e''' write the same sequence out between their stores, tests/native/temporal_pixel_test.cpp runs it as a
// host loop.
//
// Every step is exact in binary32 in the order written here and must be compiled without contraction, as rr_temporal.h.
#pragma once
#include "rr_temporal.h" // TpMix, DN_EPS and denoise_is_finite behind it

// the window of one pixel: how many colours were taken, their sums and the sums of their squares per channel
struct HcSums {
    int m;
    float s1[3], s2[3];
};
// the box of one pixel per channel, and the half width e = sigma_scale * sd it was made from.  A channel in which s2 / m, mean * mean or e
// is not finite -- an s1 or s2 that overflowed, a square of the mean that did, an e that did -- has no box: lo = -inf, hi = +inf,
// e = +inf, and nothing is moved in it.  (Without the test of the two terms of v a colour above about 1.7e20 would give v = inf - inf,
// sd = 0 and a box that is the point `mean`, to which its neighbours' histories would be pulled.)
struct HcBox {
    float lo[3], hi[3], e[3];
};

// step 7, the sums: colour(dx, dy, c) gives the colour of pixel (x + dx, y + dy) and says whether it is taken (inside the frame, three
// finite floats); the pixel itself is always taken.  dy outside, dx inside, both ascending.
template <class Colour>
RR_SETUP_HD HcSums history_clamp_sums(int r, Colour colour) {
    HcSums s;
    s.m = 0;
    for (int c = 0; c < 3; c++) s.s1[c] = s.s2[c] = 0.0f;
    for (int dy = -r; dy <= r; dy++)
        for (int dx = -r; dx <= r; dx++) {
            float q[3];
            if (!colour(dx, dy, q)) continue;
            s.m += 1;
            for (int c = 0; c < 3; c++) {
                const float sq = q[c] * q[c];
                s.s1[c] += q[c];
                s.s2[c] += sq;
            }
        }
    return s;
}

// step 7, the box
RR_SETUP_HD HcBox history_clamp_box(const HcSums& s, float sigma_scale) {
    HcBox b;
    const float m = (float)s.m;
    for (int c = 0; c < 3; c++) {
        const float mean = s.s1[c] / m;
        const float q = s.s2[c] / m, mm = mean * mean;
        const float v = q - mm;
        const float sd = __builtin_sqrtf(v > 0.0f ? v : 0.0f); // (a NaN gives 0; with q and mm finite none arises)
        const float e = sigma_scale * sd;
        if (denoise_is_finite(q) && denoise_is_finite(mm) && denoise_is_finite(e)) { // (mm finite: so is the mean)
            b.e[c] = e; b.lo[c] = mean - e; b.hi[c] = mean + e;
        } else {
            b.e[c] = __builtin_inff(); b.lo[c] = -__builtin_inff(); b.hi[c] = __builtin_inff();
        }
    }
    return b;
}

// step 8: one layer's history mean held to the box, in place.  true: a channel was moved.  (A NaN is below and above nothing: it stays.)
RR_SETUP_HD bool history_clamp_layer(const HcBox& b, float* h) {
    bool moved = false;
    for (int c = 0; c < 3; c++) {
        if (h[c] < b.lo[c]) { h[c] = b.lo[c]; moved = true; }
        else if (h[c] > b.hi[c]) { h[c] = b.hi[c]; moved = true; }
    }
    return moved;
}

// step 9: the length of a pixel whose record layer went from h to hc != h.  u is 0 in a channel that was not moved; in one that was, e is
// finite and >= 0, so u is >= 0 or +inf, keep lies in [0, 1] and the new length in [1, N].
RR_SETUP_HD void history_clamp_length(const HcBox& b, const float* h, const float* hc, TpMix* m) {
    float u[3];
    for (int c = 0; c < 3; c++) u[c] = (hc[c] < h[c] || hc[c] > h[c]) ? __builtin_fabsf(h[c] - hc[c]) / (b.e[c] + DN_EPS) : 0.0f;
    const float t01 = u[0] > u[1] ? u[0] : u[1];
    const float t = t01 > u[2] ? t01 : u[2];
    const float keep = 1.0f / (1.0f + t);
    m->length = (m->length - 1.0f) * keep + 1.0f;
    m->a = 1.0f / m->length;
}

// steps 7 .. 9 for a pixel that kept its history: m's three means clamped, its length and a shortened where the record layer moved
template <bool HALVES, class Colour>
RR_SETUP_HD void history_clamp(int r, float sigma_scale, Colour colour, TpMix* m) {
    const HcBox b = history_clamp_box(history_clamp_sums(r, colour), sigma_scale);
    const float h[3] = {m->h[0], m->h[1], m->h[2]};
    if (history_clamp_layer(b, m->h)) history_clamp_length(b, h, m->h, m);
    if (HALVES) { history_clamp_layer(b, m->ha); history_clamp_layer(b, m->hb); }
}

// rr_accumulate_clamped_split_records for a pixel that kept its history.  The colour side is history_clamp as it stands: no diffuse value
// takes part in it.  Then the diffuse box, from the window of the current `diffuse` layer: diffuse(dx, dy, c) as colour above, but taken
// on its own three floats, so the pixel itself may fail -- with nothing taken m = 0, s1 / 0.0f is a NaN and the channel has no box.  Both
// diffuse halves are held to this one box.  A layer whose mean is not finite is left alone (it will not be blended: were an infinite mean
// pulled onto a finite bound, it would be); the length is the colour side's.
template <bool HALVES, class Colour, class Diffuse>
RR_SETUP_HD void history_clamp_split(int r, float sigma_scale, Colour colour, Diffuse diffuse, TpMix* m, TpSplitMix* d) {
    history_clamp<HALVES>(r, sigma_scale, colour, m);
    const HcBox b = history_clamp_box(history_clamp_sums(r, diffuse), sigma_scale);
    if (temporal_colour_ok(d->d)) history_clamp_layer(b, d->d);
    if (HALVES) {
        if (temporal_colour_ok(d->da)) history_clamp_layer(b, d->da);
        if (temporal_colour_ok(d->db)) history_clamp_layer(b, d->db);
    }
}

// ---- one pixel of rr_accumulate_records and its three variants, between its loads and its stores
// in: the current record and, with HALVES, the colours of its two halves; with SPLIT the diffuse triple and, with HALVES, those of the two
// halves.  out: every colour blended where the step below says so (the other floats keep their bits), and the length.
struct TpPixel {
    float c[3], depth, n[3];
    unsigned int id;
    float a[3], b[3];
    float d[3], da[3], db[3];
    float length;
};
static_assert(__builtin_offsetof(TpPixel, a) == 32, "c, depth, n and id are the eight words of a record, in its order");
// the window of a call that does not clamp: never read
struct TpNoWindow {
    RR_SETUP_HD bool operator()(int, int, float*) const { return false; }
};

// The step.  hist: the previous frame as temporal_history reads it, not looked at on the first frame (has_history false); motion: the
// pixel's 3 floats, or NULL.
// The four calls differ in SPLIT (the diffuse means ride on the taps and are blended) and CLAMPED (a pixel that kept its history has its
// means held to the box of `colour`, with SPLIT the diffuse means to the box of `diffuse`: windows of radius r as history_clamp_sums
// takes them).  A pixel keeps its history when its record has DN_FIN and DN_VALID and temporal_history finds one; its length is then N,
// else 1 where its colour is finite and 0 where not.  A current half whose colour is not finite keeps its bits (the pixel's own colour is
// finite where anything is blended); a diffuse layer by temporal_blend_diffuse's rule.
template <bool HALVES, bool SPLIT, bool CLAMPED, class Hist, class Colour, class Diffuse>
RR_SETUP_HD void temporal_pixel(const TpFrame& f, unsigned int x, unsigned int y, const float* motion, bool has_history, const Hist& hist, int r, float sigma_scale,
                                Colour colour, Diffuse diffuse, TpPixel* p) {
    const unsigned int flags = denoise_flags(p->c, p->depth, p->n);
    TpMix m;
    TpSplitMix s;
    bool kept = false;
    if (has_history && flags == (unsigned int)(DN_FIN | DN_VALID)) kept = temporal_history<HALVES, Hist, SPLIT>(f, x, y, p->depth, p->n, p->id, motion, hist, &m, &s);
    if (CLAMPED && kept) {
        if constexpr (SPLIT) history_clamp_split<HALVES>(r, sigma_scale, colour, diffuse, &m, &s);
        else history_clamp<HALVES>(r, sigma_scale, colour, &m);
    }
    if (kept)
        for (int k = 0; k < 3; k++) p->c[k] = temporal_blend(m.h[k], m.a, p->c[k]);
    const float length = kept ? m.length : ((flags & DN_FIN) ? 1.0f : 0.0f);
    if (SPLIT && kept) temporal_blend_diffuse(s.d, m.a, p->d, p->d);
    if (HALVES) {
        if (kept && temporal_colour_ok(p->a))
            for (int k = 0; k < 3; k++) p->a[k] = temporal_blend(m.ha[k], m.a, p->a[k]);
        if (kept && temporal_colour_ok(p->b))
            for (int k = 0; k < 3; k++) p->b[k] = temporal_blend(m.hb[k], m.a, p->b[k]);
        if (SPLIT && kept) { temporal_blend_diffuse(s.da, m.a, p->da, p->da); temporal_blend_diffuse(s.db, m.a, p->db, p->db); }
    }
    p->length = length; // (written last: between the branches above, the device compiler merged this store with one of theirs and kept *p in scratch)
}
