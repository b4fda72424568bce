// rr_adaptive.h — the arithmetic of adaptive sampling that host and device share: the half-buffer error estimate of one pixel
// (rustray_amd/adaptive.py: half_error) and the order in which a frame's pixels enter a refinement list (refine_list: 8x8 blocks
// row-major, row-major inside a block).  Plain host logic, no HIP calls and no include of its own: k_refine_masks and k_refine_scatter
// (rr_kernels.hip) apply these functions per lane, rr_api_adaptive.h sizes its buffers with them, and
// tests/native/adaptive_order_test.cpp checks all of it on the CPU.
//
// half_error is exact in binary32 step by step (a compare, a subtraction whose rounding is the IEEE one, a sign clear, a halving, a
// maximum) and must be compiled without contraction (-ffp-contract=off, as the library is): host, device and numpy give the same bits.
#pragma once

#ifndef RR_SETUP_HD // (rr_primary_setup.h and rr_pixel_list.h define the same)
#if defined(__HIPCC__)
#define RR_SETUP_HD __host__ __device__ inline
#else
#define RR_SETUP_HD inline
#endif
#endif

RR_SETUP_HD bool adaptive_is_finite(float v) { return __builtin_fabsf(v) <= 3.402823466e+38f; } // false for NaN and both infinities
RR_SETUP_HD float adaptive_min1(float v) { return v < 1.0f ? v : 1.0f; }                      // fminf(v, 1) of a finite v

// a, b: the LINEAR colours of the two halves of a pixel (rr_render_pixel_parts at K = 2).  max over channels of |min(a, 1) - min(b, 1)| / 2;
// 0 where any of the six floats is NaN or infinite: more samples cannot cure a non-finite term.
RR_SETUP_HD float half_error(const float* a, const float* b) {
    for (int k = 0; k < 3; k++)
        if (!adaptive_is_finite(a[k]) || !adaptive_is_finite(b[k])) return 0.0f;
    float e = 0.0f;
    for (int k = 0; k < 3; k++) {
        const float d = __builtin_fabsf(adaptive_min1(a[k]) - adaptive_min1(b[k])) * 0.5f;
        e = d > e ? d : e;
    }
    return e;
}

// ---- the block order.  Position j of a width x height frame: block j >> 6 of ceil(width / 8) blocks per row, row-major; inside the
// block row (j >> 3) & 7 and column j & 7.  Blocks at the right and lower border hold positions without a pixel.
RR_SETUP_HD unsigned int refine_blocks_x(unsigned int width) { return (width + 7u) >> 3; }
RR_SETUP_HD unsigned int refine_blocks(unsigned int width, unsigned int height) { return refine_blocks_x(width) * ((height + 7u) >> 3); } // width * height <= 2^29
RR_SETUP_HD unsigned long long refine_positions(unsigned int width, unsigned int height) { return (unsigned long long)refine_blocks(width, height) << 6; }

// the pixel at position j as x | y << 16; false = the position lies outside the frame (*xy is then not written)
RR_SETUP_HD bool refine_position_pixel(unsigned long long j, unsigned int width, unsigned int height, unsigned int* xy) {
    const unsigned int bx_n = refine_blocks_x(width), b = (unsigned int)(j >> 6);
    const unsigned int x = (b % bx_n) * 8u + ((unsigned int)j & 7u), y = (b / bx_n) * 8u + (((unsigned int)j >> 3) & 7u);
    if (x >= width || y >= height) return false;
    *xy = x | (y << 16);
    return true;
}
// its inverse: the position of pixel (x, y) -- the sort key of adaptive.refine_list
RR_SETUP_HD unsigned long long refine_pixel_position(unsigned int x, unsigned int y, unsigned int width) {
    return ((unsigned long long)((y >> 3) * refine_blocks_x(width) + (x >> 3)) << 6) + (y & 7u) * 8u + (x & 7u);
}

// a list of `count` entries, padded with its last one to whole 64-ray packets (an empty list has no pad)
RR_SETUP_HD unsigned int refine_padded(unsigned int count) { return (count + 63u) & ~63u; }
// entries a list of a width x height frame may need: every pixel, padded
RR_SETUP_HD unsigned long long refine_capacity(unsigned int width, unsigned int height) { return ((unsigned long long)width * height + 63ull) & ~63ull; }
