// The pinhole ray of a pixel centre as a host program: pixel_ray, pixel_of_block_slot and pixel_ray_reach of rustray_amd/csrc/rr_pixel_list.h
// (the functions k_pixel_rays applies per lane and rr_surface_pixels calls before its first launch) and temporal_world of rr_temporal.h,
// which takes its ray from pixel_ray.  tests/test_pixel_rays_host.py compares what this writes with the numpy yardstick, bit for bit.
//
//   pixel_rays_test in.bin out.bin
//   in.bin:  u32 n_cases, then per case: u32 width, height, mode; f32 proj_inv[16], view_inv[16]; mode 2: width * height f32 depths
//     mode 0: every pixel in row-major order: 6 f32 per pixel (origin, direction), then f64 reach[3]
//     mode 1: the first and the last pixel only: 12 f32, then f64 reach[3]
//     mode 2: every pixel: 3 f32 per pixel, temporal_world at the given depth
//     mode 3: f64 reach[3] alone
//   Modes 0 and 2 also walk the frame's slot order: every pixel exactly once, blocks of 8x8 row-major, row-major inside (exit 2 otherwise).
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../rustray_amd/csrc/rr_temporal.h"

static bool read_exact(FILE* f, void* p, size_t bytes) { return bytes == 0 || fread(p, 1, bytes, f) == bytes; }

// the slots of a width x height frame against the plain loops that define the order
static bool slot_order_ok(uint32_t width, uint32_t height) {
    uint32_t j = 0;
    for (uint32_t by = 0; by < height; by += 8)
        for (uint32_t bx = 0; bx < width; bx += 8)
            for (uint32_t y = by; y < by + 8 && y < height; y++)
                for (uint32_t x = bx; x < bx + 8 && x < width; x++, j++)
                    if (pixel_of_block_slot(j, width, height) != (x | (y << 16))) {
                        fprintf(stderr, "slot %u of %ux%u: got %08x, want (%u, %u)\n", j, width, height, pixel_of_block_slot(j, width, height), x, y);
                        return false;
                    }
    return j == width * height;
}

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: pixel_rays_test in.bin out.bin\n"); return 1; }
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!in || !out) { fprintf(stderr, "cannot open the files\n"); return 1; }
    uint32_t n_cases = 0;
    if (!read_exact(in, &n_cases, 4)) return 1;
    for (uint32_t c = 0; c < n_cases; c++) {
        uint32_t head[3];
        float m[32];
        if (!read_exact(in, head, sizeof head) || !read_exact(in, m, sizeof m)) { fprintf(stderr, "case %u: short input\n", c); return 1; }
        const uint32_t width = head[0], height = head[1], mode = head[2];
        if (width == 0 || height == 0 || width > 65535u || height > 65535u || mode > 3u) { fprintf(stderr, "case %u: bad header\n", c); return 1; }
        const float w = (float)width, h = (float)height;
        if ((mode == 0 || mode == 2) && !slot_order_ok(width, height)) return 2;
        if (mode == 0 || mode == 1) {
            std::vector<uint32_t> pixels;
            if (mode == 0)
                for (uint32_t y = 0; y < height; y++)
                    for (uint32_t x = 0; x < width; x++) pixels.push_back(x | (y << 16));
            else { pixels.push_back(0u); pixels.push_back((width - 1u) | ((height - 1u) << 16)); }
            std::vector<float> rays(6 * pixels.size());
            for (size_t i = 0; i < pixels.size(); i++) pixel_ray(m, m + 16, pixels[i], w, h, &rays[6 * i], &rays[6 * i + 3]);
            fwrite(rays.data(), 4, rays.size(), out);
        }
        if (mode == 2) {
            std::vector<float> depth((size_t)width * height), world(3 * (size_t)width * height);
            if (!read_exact(in, depth.data(), 4 * depth.size())) { fprintf(stderr, "case %u: short depths\n", c); return 1; }
            TpFrame f{};
            memcpy(f.proj_inv, m, 64);
            memcpy(f.view_inv, m + 16, 64);
            f.w = w; f.h = h; f.width = (int)width; f.height = (int)height;
            for (uint32_t y = 0; y < height; y++)
                for (uint32_t x = 0; x < width; x++) temporal_world(f, x, y, depth[(size_t)y * width + x], &world[3 * ((size_t)y * width + x)]);
            fwrite(world.data(), 4, world.size(), out);
        } else {
            double reach[3];
            pixel_ray_reach(m, m + 16, width, height, reach);
            fwrite(reach, 8, 3, out);
        }
    }
    fclose(in);
    if (fclose(out) != 0) return 1;
    printf("pixel rays test OK: %u cases\n", n_cases);
    return 0;
}
