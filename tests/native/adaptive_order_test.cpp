// Host-only test of rustray_amd/csrc/rr_adaptive.h, built with g++ -ffp-contract=off -fsanitize=address,undefined by
// tests/test_adaptive_device_host.py: the arithmetic k_refine_masks and k_refine_scatter apply per lane.  The block order -- position ->
// pixel -> position is the identity on the pixels of the frame, and the present positions in ascending order are the pixels sorted by the
// key of adaptive.refine_list (rustray_amd/adaptive.py); half_error on the rows of tests/test_adaptive.py::test_half_error, bit for bit;
// the padded length of a list.
#include "../../rustray_amd/csrc/rr_adaptive.h"

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <utility>
#include <vector>

#define CHECK(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

static long g_pixels = 0, g_absent = 0;

static int test_order(uint32_t w, uint32_t h) {
    const uint32_t bxn = (w + 7) / 8, byn = (h + 7) / 8;
    CHECK(refine_blocks_x(w) == bxn && refine_blocks(w, h) == bxn * byn && refine_positions(w, h) == 64ull * bxn * byn);
    CHECK(refine_capacity(w, h) == (((uint64_t)w * h + 63) / 64) * 64);
    std::vector<uint32_t> in_order;
    std::vector<uint8_t> seen((size_t)w * h, 0);
    for (uint64_t j = 0; j < refine_positions(w, h); j++) {
        uint32_t xy = 0xdeadbeefu;
        if (!refine_position_pixel(j, w, h, &xy)) { CHECK(xy == 0xdeadbeefu); g_absent++; continue; }
        const uint32_t x = xy & 0xffffu, y = xy >> 16;
        CHECK(x < w && y < h && seen[(size_t)y * w + x] == 0);
        seen[(size_t)y * w + x] = 1;
        CHECK(refine_pixel_position(x, y, w) == j);
        CHECK((j >> 6) == (uint64_t)(y / 8) * bxn + x / 8 && ((j >> 3) & 7) == y % 8 && (j & 7) == x % 8);
        in_order.push_back(xy);
        g_pixels++;
    }
    CHECK(in_order.size() == (size_t)w * h);
    // brute force: every pixel, sorted by the Python key ((y >> 3) * ceil(w / 8) + (x >> 3)) * 64 + (y & 7) * 8 + (x & 7)
    std::vector<std::pair<uint64_t, uint32_t>> keyed;
    for (uint32_t y = 0; y < h; y++)
        for (uint32_t x = 0; x < w; x++) keyed.push_back({((uint64_t)(y >> 3) * ((w + 7) >> 3) + (x >> 3)) * 64 + (y & 7) * 8 + (x & 7), x | (y << 16)});
    std::stable_sort(keyed.begin(), keyed.end(), [](const std::pair<uint64_t, uint32_t>& a, const std::pair<uint64_t, uint32_t>& b) { return a.first < b.first; });
    for (size_t i = 0; i < keyed.size(); i++) CHECK(keyed[i].second == in_order[i]);
    return 0;
}

static int test_half_error() {
    const float nan = std::nanf(""), inf = INFINITY;
    const float rows[8][2][3] = {
        {{0.25f, 0.5f, 0.0f}, {0.75f, 0.5f, 0.0f}},
        {{0.0f, 0.0f, 0.0f}, {0.0f, 0.0f, 0.0f}},
        {{3.0f, 0.0f, 0.0f}, {1.5f, 0.0f, 0.0f}},
        {{2.0f, 0.25f, 0.0f}, {0.5f, 0.0f, 0.0f}},
        {{nan, 0.0f, 0.0f}, {0.5f, 0.9f, 0.0f}},
        {{0.0f, inf, 0.0f}, {0.0f, 0.0f, 1.0f}},
        {{0.0f, 0.0f, 0.0f}, {0.0f, 0.0f, -inf}},
        {{-0.5f, 0.0f, 0.0f}, {0.5f, 0.0f, 0.0f}},
    };
    const float want[8] = {0.25f, 0.0f, 0.0f, 0.25f, 0.0f, 0.0f, 0.0f, 0.5f};
    for (int i = 0; i < 8; i++) {
        const float e = half_error(rows[i][0], rows[i][1]), f = half_error(rows[i][1], rows[i][0]);
        CHECK(std::memcmp(&e, &want[i], 4) == 0 && std::memcmp(&f, &want[i], 4) == 0);
    }
    // equal halves of either sign of zero give +0, as numpy's abs does
    const float nz[3] = {-0.0f, -0.0f, -0.0f}, pz[3] = {0.0f, 0.0f, 0.0f};
    const float z = half_error(nz, pz), zero = 0.0f;
    CHECK(std::memcmp(&z, &zero, 4) == 0);
    CHECK(adaptive_is_finite(3.402823466e+38f) && adaptive_is_finite(-3.402823466e+38f) && !adaptive_is_finite(inf) && !adaptive_is_finite(-inf) && !adaptive_is_finite(nan));
    return 0;
}

int main() {
    const uint32_t frames[][2] = {{1, 1}, {7, 9}, {8, 8}, {9, 1}, {20, 12}, {50, 38}, {264, 264}};
    for (const auto& f : frames)
        if (test_order(f[0], f[1])) return 1;
    if (test_half_error()) return 1;
    CHECK(refine_padded(0) == 0 && refine_padded(1) == 64 && refine_padded(63) == 64 && refine_padded(64) == 64 && refine_padded(65) == 128);
    std::printf("adaptive order test OK (%ld pixels, %ld absent positions)\n", g_pixels, g_absent);
    return 0;
}
