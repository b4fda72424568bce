// Host-only test of rustray_amd/csrc/rr_pixel_list.h (built with g++ -ffp-contract=off -fsanitize=address,undefined by
// tests/test_pixel_list.py): the check of a caller's pixel list (the first entry outside the frame) and the centre of one packed pixel,
// as bit patterns, against primary_slot_centres (rr_primary_setup.h) and against the reference's expression restated here.
#include "../../rustray_amd/csrc/rr_pixel_list.h"
#include "../../rustray_amd/csrc/rr_primary_setup.h"

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#define CHECK(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

static uint32_t pack(uint32_t x, uint32_t y) { return x | (y << 16); }
static uint32_t bits(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }

static int test_list_check() {
    // an empty list: nothing to refuse, and the pointer is not read (a one-past-the-end pointer of an empty vector)
    std::vector<uint32_t> none;
    CHECK(pixel_list_first_bad(none.data(), 0, 50, 38) == RR_PIXEL_LIST_OK);
    CHECK(pixel_list_first_bad(nullptr, 0, 50, 38) == RR_PIXEL_LIST_OK);
    // every pixel of the frame, the last column and the last row included
    std::vector<uint32_t> all;
    for (uint32_t y = 0; y < 38; y++) for (uint32_t x = 0; x < 50; x++) all.push_back(pack(x, y));
    CHECK(pixel_list_first_bad(all.data(), (unsigned)all.size(), 50, 38) == RR_PIXEL_LIST_OK);
    const uint32_t corner[1] = {pack(49, 37)}; // x == W - 1, y == H - 1
    CHECK(pixel_list_first_bad(corner, 1, 50, 38) == RR_PIXEL_LIST_OK);
    CHECK(pixel_in_frame(pack(49, 37), 50, 38) && !pixel_in_frame(pack(50, 37), 50, 38) && !pixel_in_frame(pack(49, 38), 50, 38));
    // the last entry bad: x == W, then y == H
    std::vector<uint32_t> l = all;
    l.push_back(pack(50, 0));
    CHECK(pixel_list_first_bad(l.data(), (unsigned)l.size(), 50, 38) == l.size() - 1);
    l.back() = pack(0, 38);
    CHECK(pixel_list_first_bad(l.data(), (unsigned)l.size(), 50, 38) == l.size() - 1);
    CHECK(pixel_list_first_bad(l.data(), (unsigned)l.size() - 1, 50, 38) == RR_PIXEL_LIST_OK); // (the length is honoured)
    // the first of several bad entries
    l = all;
    l[1700] = pack(65535, 0); l[70] = pack(50, 3); l[71] = pack(3, 38); l[900] = pack(60, 60);
    CHECK(pixel_list_first_bad(l.data(), (unsigned)l.size(), 50, 38) == 70);
    l[70] = pack(49, 3);
    CHECK(pixel_list_first_bad(l.data(), (unsigned)l.size(), 50, 38) == 71);
    l[0] = 0xffffffffu;
    CHECK(pixel_list_first_bad(l.data(), (unsigned)l.size(), 50, 38) == 0);
    // the largest frame: every 16-bit coordinate but 65535 is inside
    const uint32_t big[4] = {pack(65534, 65534), pack(0, 65534), pack(65535, 0), pack(0, 65535)};
    CHECK(pixel_list_first_bad(big, 2, 65535, 65535) == RR_PIXEL_LIST_OK);
    CHECK(pixel_list_first_bad(big, 4, 65535, 65535) == 2);
    CHECK(pixel_list_first_bad(big + 3, 1, 65535, 65535) == 0);
    // a frame of one pixel
    CHECK(pixel_list_first_bad(big + 1, 1, 1, 1) == 0 && pixel_in_frame(0u, 1, 1));
    return 0;
}

// every pixel of a w x h frame: pixel_centre = primary_slot_centres = the reference's expression (src/raytracing.rs:319-331), bit for bit
static int test_centres(uint32_t w, uint32_t h) {
    std::vector<uint32_t> xy;
    for (uint32_t y = 0; y < h; y++) for (uint32_t x = 0; x < w; x++) xy.push_back(pack(x, y));
    std::vector<float> table(2 * xy.size());
    primary_slot_centres(xy.data(), xy.size(), w, h, table.data());
    const float wf = (float)w, hf = (float)h;
    for (size_t j = 0; j < xy.size(); j++) {
        float cx, cy;
        pixel_centre(xy[j], wf, hf, &cx, &cy);
        const float x_f = (float)(xy[j] & 0xffffu), y_f = (float)(xy[j] >> 16);
        const float rx = ((x_f + 0.5f) / wf) * 2.0f - 1.0f;
        const float ry = 1.0f - ((y_f + 0.5f) / hf) * 2.0f;
        CHECK(bits(cx) == bits(table[2 * j]) && bits(cy) == bits(table[2 * j + 1]));
        CHECK(bits(cx) == bits(rx) && bits(cy) == bits(ry));
        CHECK(cx > -1.0f && cx < 1.0f && cy > -1.0f && cy < 1.0f);
    }
    return 0;
}

int main() {
    if (test_list_check()) return 1;
    if (test_centres(50, 38) || test_centres(1, 1) || test_centres(65535, 3)) return 1;
    std::printf("pixel list test OK\n");
    return 0;
}
