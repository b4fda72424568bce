// rr_primary_setup.h — what the derivation of a primary ray (rr_kernels.hip primary_ray) does NOT owe to the ray: the parts
// that are constant for the frame, the sample, the pixel or the launch, evaluated once on the host.  Plain host arithmetic,
// no HIP calls (rr_api_frame.h builds the tables and records; tests/native/primary_setup_test.cpp checks them on the CPU against
// the per-ray formula they replace).  The kernels read the records declared here and evaluate rr_div_* on the device.
//
// Every float below is the IEEE binary32 expression the per-ray code evaluated, in its order, and must be compiled without
// contraction (-ffp-contract=off, as the library is): the ray a kernel builds from the tables is then bit for bit the ray
// it built from (pixel, sample) before.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define RR_SETUP_HD __host__ __device__ inline
#else
#define RR_SETUP_HD inline
#endif
#include "rr_pixel_list.h" // pixel_centre: the centre of one packed pixel, also what k_pixel_slots evaluates per list entry

// ---- exact division by a run-time constant --------------------------------------------------------------------------------
// q = n / d as one multiply-high, a shift and at most one add (Granlund & Montgomery, "Division by invariant integers using
// multiplication", PLDI 1994); the remainder is n - q * d.
struct RrDiv {
    uint32_t d;     // the divisor (>= 1)
    uint32_t mul;   // the low 32 bits of the multiplier
    uint32_t shift; // rr_div_small: the one shift; rr_div_wide: the shift after the add
    uint32_t add;   // rr_div_small: mask of n added to the high product; rr_div_wide: the shift of (n - t), 0 or 1
};

RR_SETUP_HD uint32_t rr_mulhi(uint32_t a, uint32_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __umulhi(a, b);
#else
    return (uint32_t)(((uint64_t)a * b) >> 32);
#endif
}

// Dividends below 2^RR_DIV_SMALL_BITS (packet indices: RR_LEVEL_MAX / 64 < 2^25).
#define RR_DIV_SMALL_BITS 25
// d = 2^k: mul = 0 and the dividend itself is shifted.  Otherwise, with s = floor(log2 d), m = floor(2^(32 + s) / d) + 1 lies in
// (2^31, 2^32) and e = m * d - 2^(32 + s) in (0, d): floor(n * m / 2^(32 + s)) = floor(n / d + n * e / (d * 2^(32 + s))), which is
// floor(n / d) whenever n * e < 2^(32 + s) -- and n < 2^25, e < d < 2^(s + 1) give n * e < 2^(26 + s).
inline RrDiv rr_div_make_small(uint32_t d) {
    if (d == 0) d = 1;
    uint32_t s = 0;
    while ((d >> s) > 1u) s++; // floor(log2 d)
    if ((d & (d - 1u)) == 0u) return RrDiv{d, 0u, s, 0xffffffffu};
    const uint64_t m = ((1ull << (32 + s)) / d) + 1ull;
    return RrDiv{d, (uint32_t)m, s, 0u};
}
RR_SETUP_HD uint32_t rr_div_small(uint32_t n, const RrDiv& dv) { return (rr_mulhi(n, dv.mul) + (n & dv.add)) >> dv.shift; }

// Every 32-bit dividend: the 33-bit multiplier m = 2^32 + mul = floor(2^(32 + s) / d) + 1 with s = ceil(log2 d) has
// e = m * d - 2^(32 + s) in (0, d] and d <= 2^s, so n * e < 2^(32 + s) for every n < 2^32.  t = high(n * mul); the sum n + t may
// carry, so it is formed as t + ((n - t) >> 1) and shifted by s - 1 (add-and-shift).  d = 1 has s = 0: mul = 0, no halving.
inline RrDiv rr_div_make_wide(uint32_t d) {
    if (d <= 1u) return RrDiv{1u, 0u, 0u, 0u};
    uint32_t s = 0;
    while (((uint64_t)1 << s) < d) s++; // ceil(log2 d), 1 .. 32
    const uint64_t hi = ((uint64_t)1 << s) - d; // m - 2^32 = floor(2^32 * (2^s - d) / d) + 1 (2^s - d < d: below 2^32)
    const uint64_t m = ((hi << 32) / d) + 1ull;
    return RrDiv{d, (uint32_t)m, s - 1u, 1u};
}
RR_SETUP_HD uint32_t rr_div_wide(uint32_t n, const RrDiv& dv) {
    const uint32_t t = rr_mulhi(n, dv.mul);
    return (t + ((n - t) >> dv.add)) >> dv.shift;
}

// ---- per-frame record: read by the kernels through the pointer they read the frame constants through -------------------
struct PrimaryFrame {
    const float* slot_c; // (cx, cy) per accumulator slot: primary_slot_centres
    RrDiv per_group;     // packets per sample group = n_region_pixels / (64 / G), for packet indices (rr_div_small)
    RrDiv npix;          // n_region_pixels, for first_pix + i of a batch without sample groups (rr_div_wide)
};

// ---- per-launch constants of the batch [first, first + n) with sample group G (rr_frame_plan.h batch_group) ----------------
struct PrimaryLaunch {
    uint32_t first_sample; // first / npix
    uint32_t first_pix;    // first % npix (0 when G > 1: such a batch holds whole sample slices)
    uint32_t lg_group;     // log2(G); 0 = one sample of 64 pixels per packet
    uint32_t lg_pixels;    // log2(64 / G)
};
inline PrimaryLaunch primary_launch(uint64_t first, uint32_t npix, uint32_t G) {
    uint32_t lg = 0;
    while ((G >> lg) > 1u) lg++;
    return PrimaryLaunch{(uint32_t)(first / npix), (uint32_t)(first % npix), lg, 6u - lg};
}
inline PrimaryFrame primary_frame(const float* slot_c, uint32_t npix, uint32_t G) {
    return PrimaryFrame{slot_c, rr_div_make_small(npix / (64u / (G ? G : 1u))), rr_div_make_wide(npix)};
}

// (accumulator slot, sample) of primary index i of the launch: what primary_ray starts with.
RR_SETUP_HD void primary_index(const PrimaryFrame& pf, const PrimaryLaunch& pl, uint32_t i, uint32_t* pix, uint32_t* sample) {
    if (pl.lg_group == 0u) {
        const uint32_t gi = pl.first_pix + i; // below 2^32: first_pix < npix <= 2^30 and i < 2^31
        const uint32_t q = rr_div_wide(gi, pf.npix);
        *pix = gi - q * pf.npix.d;
        *sample = pl.first_sample + q;
    } else {
        // a 64-ray packet = 64/G neighbouring pixels x G samples of each (the host guarantees whole groups); the samples of
        // one pixel sit in neighbouring lanes, so that their accumulator adds can be merged (accum_merged)
        const uint32_t pkt = i >> 6, lane = i & 63u;
        const uint32_t q = rr_div_small(pkt, pf.per_group);
        *pix = ((pkt - q * pf.per_group.d) << pl.lg_pixels) + (lane >> pl.lg_group);
        *sample = pl.first_sample + (q << pl.lg_group) + (lane & ((1u << pl.lg_group) - 1u));
    }
}

// ---- interleaved parts (rr_render_pixel_parts): K = 2^lg_parts accumulator slots per pixel ----------------------------------
// Slot i * K + h is part h of list entry i and receives the frame samples {s : s mod K == h}.  The batch plan and the index
// arithmetic above see K * n slots of S / K samples each; the k-th sample of a slot is frame sample k * K + (slot mod K), and
// that is the sample everything behind the index means (the row of sample_tr, the generator's key, the object-id rule).
// lg_parts == 0 is the identity: the frame without parts.
RR_SETUP_HD uint32_t primary_part_sample(uint32_t slot, uint32_t k, uint32_t lg_parts) {
    return (k << lg_parts) | (slot & ((1u << lg_parts) - 1u));
}
RR_SETUP_HD void primary_index(const PrimaryFrame& pf, const PrimaryLaunch& pl, uint32_t lg_parts, uint32_t i, uint32_t* pix, uint32_t* sample) {
    primary_index(pf, pl, i, pix, sample);
    *sample = primary_part_sample(*pix, *sample, lg_parts);
}

// ---- per-sample offsets: sample_tr[s] = (x_trans, y_trans) -----------------------------------------------------------------
// What the table depends on besides the sub-sample table itself.
struct PrimarySampleKey {
    uint32_t width, height, cell_size, dof, samples;
    float aperture_size;
};
inline bool same_key(const PrimarySampleKey& a, const PrimarySampleKey& b) {
    return a.width == b.width && a.height == b.height && a.cell_size == b.cell_size && a.dof == b.dof && a.samples == b.samples &&
           a.aperture_size == b.aperture_size;
}
// sample_xy: samples x (x_i, y_i); out: samples x (x_trans, y_trans)
inline void primary_sample_offsets(const uint16_t* sample_xy, const PrimarySampleKey& k, float* out) {
    const float w = (float)k.width, h = (float)k.height;
    const float x_step = 2.0f / w, y_step = 2.0f / h;
    const float inv_cell = 1.0f / (float)k.cell_size;
    for (uint32_t s = 0; s < k.samples; s++) {
        const float x_i = (float)sample_xy[2u * s], y_i = (float)sample_xy[2u * s + 1u];
        float x_trans = x_step * x_i * inv_cell;
        float y_trans = y_step * y_i * inv_cell;
        if (k.dof && k.samples > 1u) { x_trans -= x_step / 2.0f; y_trans -= y_step / 2.0f; }
        if (k.dof) {
            const float aperture_scale = (float)k.width / 800.0f;
            x_trans *= k.aperture_size * aperture_scale;
            y_trans *= k.aperture_size * aperture_scale;
        }
        out[2u * s] = x_trans; out[2u * s + 1u] = y_trans;
    }
}

// ---- per-slot centres: slot_c[j] = (cx, cy) of the pixel slot_xy[j] = x | y << 16 ------------------------------------------
inline void primary_slot_centres(const uint32_t* slot_xy, size_t n, uint32_t width, uint32_t height, float* out) {
    const float w = (float)width, h = (float)height;
    for (size_t j = 0; j < n; j++) pixel_centre(slot_xy[j], w, h, &out[2 * j], &out[2 * j + 1]);
}
