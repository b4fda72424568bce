// rr_pixel_list.h — the caller's pixel list of rr_render_pixels (entry i = x | y << 16): is every entry inside the frame, and where on the
// screen is the centre of one packed pixel.  Plain host logic, no HIP calls and no include of its own: rr_api_frame.h checks a host list
// with it before anything is uploaded, k_pixel_slots (rr_kernels.hip) applies the same two functions per lane to a list on the device,
// and primary_slot_centres (rr_primary_setup.h) forms a region's centres through pixel_centre, so a pixel has ONE centre whichever way
// it became a slot; tests/native/pixel_list_test.cpp checks all of it on the CPU.
//
// pixel_centre is the IEEE binary32 expression of the reference's `render` (src/raytracing.rs:319-331), in its order, and must be
// compiled without contraction (-ffp-contract=off, as the library is): host and device then give the same bits.
#pragma once

#ifndef RR_SETUP_HD // (rr_primary_setup.h defines the same)
#if defined(__HIPCC__)
#define RR_SETUP_HD __host__ __device__ inline
#else
#define RR_SETUP_HD inline
#endif
#endif

#define RR_PIXEL_LIST_OK 0xffffffffu // pixel_list_first_bad: every entry lies inside the frame

RR_SETUP_HD bool pixel_in_frame(unsigned int xy, unsigned int width, unsigned int height) { return (xy & 0xffffu) < width && (xy >> 16) < height; }

// the first index i < n whose entry has x >= width or y >= height, or RR_PIXEL_LIST_OK (n <= 2^30: rr_render_pixels)
inline unsigned int pixel_list_first_bad(const unsigned int* pixel_xy, unsigned int n, unsigned int width, unsigned int height) {
    for (unsigned int i = 0; i < n; i++)
        if (!pixel_in_frame(pixel_xy[i], width, height)) return i;
    return RR_PIXEL_LIST_OK;
}

// (cx, cy): the screen point of the centre of pixel xy = x | y << 16 in a frame of w x h pixels (w, h: the sizes as floats)
RR_SETUP_HD void pixel_centre(unsigned int xy, float w, float h, float* cx, float* cy) {
    const float x_f = (float)(xy & 0xffffu), y_f = (float)(xy >> 16);
    *cx = ((x_f + 0.5f) / w) * 2.0f - 1.0f;
    *cy = 1.0f - ((y_f + 0.5f) / h) * 2.0f;
}
