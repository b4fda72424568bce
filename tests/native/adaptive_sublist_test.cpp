// Host-only test of the list arithmetic of rustray_amd/csrc/rr_adaptive.h, built with g++ -ffp-contract=off
// -fsanitize=address,undefined by tests/test_adaptive_levels_host.py: what k_refine_masks and k_refine_scatter apply per lane, over both
// entry sources.  The three launches are replayed on the CPU, wave by wave and lane by lane, through the shared functions -- the masks, an
// exclusive scan of their popcounts, the scatter and the pad -- into a buffer with guard words, and the result is compared with a brute
// force.  ListSource: a filter of the list: order kept, entries at `count` and beyond never taken, padded with the last entry to a
// multiple of 64, nothing written behind.  FrameSource: the flagged pixels of a frame sorted by refine_pixel_position, padded the same way.
#include "../../rustray_amd/csrc/rr_adaptive.h"

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#define CHECK(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

static const uint32_t GUARD = 0x5a5a5a5au;
static long g_lists = 0, g_taken = 0, g_frames = 0, g_partial_last = 0;

static uint32_t rng(uint32_t* state) { *state = *state * 1664525u + 1013904223u; return *state >> 8; }

// a part record is two of these; the colour is the first one's x y z (the device's float4)
struct F4 { float x, y, z, w; };
static float& channel(F4& v, uint32_t k) { return k == 0u ? v.x : k == 1u ? v.y : v.z; }
// the two part records of entry i: both halves 0.25 everywhere, then on request an error of 0.5 in channel i % 3
static void fill_parts(std::vector<F4>& parts, size_t i, bool take) {
    for (int r = 0; r < 4; r++) parts[4 * i + r] = F4{0.25f, 0.25f, 0.25f, 0.25f};
    if (take) { channel(parts[4 * i], (uint32_t)(i % 3u)) = 1.0f; channel(parts[4 * i + 2], (uint32_t)(i % 3u)) = 0.0f; }
}

// The three launches of a list over `src`, lane by lane: out (guard words, `cap` of them may be written) gets the list, *total_out its
// length, error[index] half_error of every entry (written once each; `error` has a NaN where nothing was written).  *last_wave: the wave
// that wrote the pad (not written for an empty list).
template <class Source>
static int compact_model(const Source& src, const std::vector<F4>& parts, float threshold, uint32_t cap, std::vector<uint32_t>& out, uint32_t* total_out,
                         std::vector<float>& error, uint32_t* last_wave) {
    const uint32_t nw = src.waves();
    std::vector<unsigned long long> masks(nw, 0ull);
    std::vector<uint32_t> offsets(nw, 0u);
    for (uint32_t w = 0; w < nw; w++)
        for (uint32_t lane = 0; lane < 64u; lane++) {
            uint32_t i = 0xdeadbeefu, word = 0xdeadbeefu;
            if (!src.entry(w, lane, &i, &word)) { CHECK(i == 0xdeadbeefu && word == 0xdeadbeefu); continue; }
            CHECK(i < error.size() && error[i] != error[i]); // inside the parts, and no entry belongs to two lanes
            error[i] = half_error_of_parts(parts.data(), i);
            if (error[i] > threshold) masks[w] |= 1ull << lane;
        }
    uint32_t total = 0;
    for (uint32_t w = 0; w < nw; w++) { offsets[w] = total; total += (uint32_t)__builtin_popcountll(masks[w]); }
    uint32_t last_waves = 0;
    for (uint32_t w = 0; w < nw; w++) {
        if (masks[w] == 0ull) continue;
        uint32_t words[64];
        for (uint32_t lane = 0; lane < 64u; lane++) {
            uint32_t i = 0;
            words[lane] = 0u;
            const bool present = src.entry(w, lane, &i, &words[lane]);
            if (!((masks[w] >> lane) & 1ull)) continue;
            CHECK(present); // a set bit is a lane with an entry
            const uint32_t at = offsets[w] + refine_mask_rank(masks[w], lane);
            CHECK(at < cap && out[at] == GUARD); // inside the buffer, and no word is written twice
            out[at] = words[lane];
        }
        if (!sublist_wave_is_last(masks[w], offsets[w], total)) continue;
        last_waves++;
        *last_wave = w;
        const uint32_t ll = sublist_last_lane(masks[w]);
        CHECK(ll < 64u && ((masks[w] >> ll) & 1ull) && (ll == 63u || (masks[w] >> (ll + 1u)) == 0ull));
        for (uint32_t lane = 0; lane < 64u; lane++) {
            uint32_t at = 0xdeadbeefu;
            if (!sublist_pad_word(total, lane, &at)) { CHECK(at == 0xdeadbeefu); continue; }
            CHECK(at == total + lane && at < refine_padded(total) && at < cap && out[at] == GUARD);
            out[at] = words[ll];
        }
    }
    CHECK(last_waves == (total ? 1u : 0u));
    *total_out = total;
    return 0;
}

// `pattern`: 0 = nothing taken, 1 = everything, 2 = every third entry, 3 = random, 4 = only the last entry, 5 = only the first
static int test_sublist(uint32_t count, int pattern, float threshold) {
    uint32_t state = count * 7919u + (uint32_t)pattern;
    const uint32_t own_pad = 64u; // the caller's list carries a pad of its own, with halves far above the threshold: it is never taken
    std::vector<uint32_t> list(count + own_pad);
    std::vector<F4> parts((size_t)(count + own_pad) * 4); // two records of two F4 per entry
    for (uint32_t i = 0; i < count + own_pad; i++) {
        list[i] = (rng(&state) & 0xffffu) | (rng(&state) << 16);
        if (i > 0 && rng(&state) % 5u == 0u) list[i] = list[i - 1]; // duplicates are entries like any other
        bool take = pattern == 1 || (pattern == 2 && i % 3u == 0u) || (pattern == 3 && (rng(&state) & 1u)) || (pattern == 4 && i + 1 == count) || (pattern == 5 && i == 0);
        if (i >= count) take = true;
        fill_parts(parts, i, take);                                                       // error 0.5
        if (!take && rng(&state) % 7u == 0u) parts[4 * (size_t)i].y = std::nanf("");      // a NaN half: error 0, not taken
        else if (!take && rng(&state) % 7u == 0u) parts[4 * (size_t)i].z = 0.25f + 2.0f * threshold; // error == threshold exactly: not taken
    }
    // brute force
    std::vector<uint32_t> want;
    for (uint32_t i = 0; i < count; i++) {
        const float a[3] = {parts[4 * (size_t)i].x, parts[4 * (size_t)i].y, parts[4 * (size_t)i].z};
        const float b[3] = {parts[4 * (size_t)i + 2].x, parts[4 * (size_t)i + 2].y, parts[4 * (size_t)i + 2].z};
        CHECK(half_error_of_parts(parts.data(), i) == half_error(a, b));
        if (half_error(a, b) > threshold) want.push_back(list[i]);
    }
    const uint32_t taken = (uint32_t)want.size();
    while (want.size() % 64u) want.push_back(want[taken - 1]);
    // the source: lane l of wave w holds entry 64 w + l, its index is the entry and its word the list's
    const ListSource src{list.data(), count};
    const uint32_t nw = src.waves();
    CHECK(nw == sublist_waves(count) && nw == (count + 63u) / 64u);
    for (uint32_t w = 0; w < nw; w++)
        for (uint32_t lane = 0; lane < 64u; lane++) {
            uint32_t i = 0xdeadbeefu, j = 0xdeadbeefu, word = 0xdeadbeefu;
            if (!sublist_lane_entry(w, lane, count, &i)) {
                CHECK(i == 0xdeadbeefu && w * 64u + lane >= count && !src.entry(w, lane, &j, &word) && j == 0xdeadbeefu && word == 0xdeadbeefu);
                continue;
            }
            CHECK(i == w * 64u + lane && i < count && src.entry(w, lane, &j, &word) && j == i && word == list[i]);
        }
    // the three launches
    std::vector<uint32_t> out(refine_padded(count) + 64u, GUARD);
    std::vector<float> error(count, std::nanf(""));
    uint32_t total = 0, last_wave = 0;
    if (compact_model(src, parts, threshold, refine_padded(count), out, &total, error, &last_wave)) return 1;
    CHECK(total == taken);
    for (uint32_t i = 0; i < count; i++) CHECK(error[i] == error[i]); // every entry before `count` has its error
    CHECK(refine_padded(taken) == want.size() && refine_padded(taken) <= refine_padded(count));
    for (size_t i = 0; i < out.size(); i++) CHECK(out[i] == (i < want.size() ? want[i] : GUARD));
    g_lists++;
    g_taken += taken;
    return 0;
}

// The list of a width x height frame: `pattern` 1 = every pixel flagged, 3 = random, 4 = only the frame's last pixel (the last taken
// entry then lies in the last block, which is partial wherever the frame is no multiple of 8)
static int test_frame(uint32_t width, uint32_t height, int pattern, float threshold) {
    uint32_t state = width * 7919u + height * 104729u + (uint32_t)pattern;
    const uint32_t n = width * height;
    std::vector<F4> parts((size_t)n * 4); // the frame's part records: pixel (x, y)'s two at (y * width + x) * 2
    std::vector<std::pair<unsigned long long, uint32_t>> keyed; // (position in the block order, x | y << 16) of every flagged pixel
    std::vector<char> flagged(n, 0);
    for (uint32_t y = 0; y < height; y++)
        for (uint32_t x = 0; x < width; x++) {
            const uint32_t xy = x | (y << 16), o = frame_index(xy, width);
            CHECK(o == y * width + x);
            const bool take = pattern == 1 || (pattern == 3 && (rng(&state) & 1u)) || (pattern == 4 && o + 1 == n);
            fill_parts(parts, o, take);
            flagged[o] = take ? 1 : 0;
            if (take) keyed.push_back({refine_pixel_position(x, y, width), xy});
        }
    // brute force: the flagged pixels sorted by refine_pixel_position, padded with the last one to a multiple of 64
    std::sort(keyed.begin(), keyed.end());
    std::vector<uint32_t> want;
    for (const auto& k : keyed) want.push_back(k.second);
    const uint32_t taken = (uint32_t)want.size();
    while (want.size() % 64u) want.push_back(want[taken - 1]);
    // the source: wave w is block w, lane l its position l; the index is the pixel's place in the frame and the word the pixel
    const FrameSource src{width, height};
    CHECK(src.waves() == refine_blocks(width, height));
    uint32_t present = 0;
    for (uint32_t w = 0; w < src.waves(); w++)
        for (uint32_t lane = 0; lane < 64u; lane++) {
            uint32_t i = 0xdeadbeefu, word = 0xdeadbeefu, xy = 0xdeadbeefu;
            if (!refine_position_pixel(((unsigned long long)w << 6) | lane, width, height, &xy)) {
                CHECK(!src.entry(w, lane, &i, &word) && i == 0xdeadbeefu && word == 0xdeadbeefu);
                continue;
            }
            CHECK(src.entry(w, lane, &i, &word) && word == xy && i == (xy >> 16) * width + (xy & 0xffffu) && i < n);
            CHECK(refine_pixel_position(xy & 0xffffu, xy >> 16, width) == (((unsigned long long)w << 6) | lane));
            present++;
        }
    CHECK(present == n);
    // the three launches
    const uint32_t cap = (uint32_t)refine_capacity(width, height);
    std::vector<uint32_t> out(cap + 64u, GUARD);
    std::vector<float> error(n, std::nanf(""));
    uint32_t total = 0, last_wave = 0;
    if (compact_model(src, parts, threshold, cap, out, &total, error, &last_wave)) return 1;
    CHECK(total == taken);
    for (uint32_t o = 0; o < n; o++) CHECK(error[o] == (flagged[o] ? 0.5f : 0.0f)); // every pixel has its error, written once
    CHECK(refine_padded(taken) == want.size() && want.size() <= cap);
    for (size_t i = 0; i < out.size(); i++) CHECK(out[i] == (i < want.size() ? want[i] : GUARD)); // nothing behind the padded length
    if (taken) { // was the last taken entry in a block with positions outside the frame?
        uint32_t in_block = 0, i = 0, word = 0;
        for (uint32_t lane = 0; lane < 64u; lane++) in_block += src.entry(last_wave, lane, &i, &word) ? 1u : 0u;
        if (in_block < 64u) g_partial_last++;
    }
    g_frames++;
    g_taken += taken;
    return 0;
}

int main() {
    const uint32_t counts[] = {0, 1, 63, 64, 65, 4097};
    for (uint32_t count : counts)
        for (int pattern = 0; pattern < 6; pattern++)
            if (test_sublist(count, pattern, 0.125f)) return 1;
    const uint32_t frames[][2] = {{1, 1}, {9, 1}, {8, 8}, {20, 12}, {50, 38}};
    const int frame_patterns[] = {3, 1, 4, 0};
    for (const auto& f : frames)
        for (int pattern : frame_patterns)
            if (test_frame(f[0], f[1], pattern, 0.125f)) return 1;
    CHECK(g_frames == 20 && g_partial_last >= 8); // (every frame but 8x8 ends in a partial block: all-set and last-pixel patterns at least)
    // the rank is the number of set bits below the lane, for every lane of a few masks
    const unsigned long long masks[] = {0ull, 1ull, 1ull << 63, ~0ull, 0xaaaaaaaaaaaaaaaaull, 0x00000001ffffffffull, 0x8000000080000001ull};
    for (unsigned long long m : masks)
        for (uint32_t lane = 0; lane < 64u; lane++) {
            uint32_t below = 0;
            for (uint32_t b = 0; b < lane; b++) below += (uint32_t)((m >> b) & 1ull);
            CHECK(refine_mask_rank(m, lane) == below);
        }
    CHECK(sublist_waves(0) == 0 && sublist_waves(1) == 1 && sublist_waves(64) == 1 && sublist_waves(65) == 2 && sublist_waves(1u << 29) == (1u << 23));
    CHECK(!sublist_wave_is_last(0ull, 0u, 0u) && sublist_wave_is_last(3ull, 5u, 7u) && !sublist_wave_is_last(3ull, 5u, 8u));
    std::printf("adaptive sublist test OK (%ld lists, %ld frames, %ld entries taken)\n", g_lists, g_frames, g_taken);
    return 0;
}
