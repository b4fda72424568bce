// Host-only test of the list-of-a-list arithmetic of rustray_amd/csrc/rr_adaptive.h, built with g++ -ffp-contract=off
// -fsanitize=address,undefined by tests/test_adaptive_levels_host.py: what k_sublist_masks and k_sublist_scatter apply per lane.  The three
// launches are replayed on the CPU, wave by wave and lane by lane, through the shared functions -- the masks, an exclusive scan of their
// popcounts, the scatter and the pad -- into a buffer with guard words, and the result is compared with a brute-force filter of the
// list: order kept, entries at `count` and beyond never taken, padded with the last entry to a multiple of 64, nothing written behind.
#include "../../rustray_amd/csrc/rr_adaptive.h"

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#define CHECK(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

static const uint32_t GUARD = 0x5a5a5a5au;
static long g_lists = 0, g_taken = 0;

static uint32_t rng(uint32_t* state) { *state = *state * 1664525u + 1013904223u; return *state >> 8; }

// `pattern`: 0 = nothing taken, 1 = everything, 2 = every third entry, 3 = random, 4 = only the last entry, 5 = only the first
static int test_sublist(uint32_t count, int pattern, float threshold) {
    uint32_t state = count * 7919u + (uint32_t)pattern;
    const uint32_t own_pad = 64u; // the caller's list carries a pad of its own, with halves far above the threshold: it is never taken
    std::vector<uint32_t> list(count + own_pad);
    std::vector<float> parts((size_t)(count + own_pad) * 16); // two records of 8 floats per entry; the colour is the first three of each
    for (uint32_t i = 0; i < count + own_pad; i++) {
        list[i] = (rng(&state) & 0xffffu) | (rng(&state) << 16);
        if (i > 0 && rng(&state) % 5u == 0u) list[i] = list[i - 1]; // duplicates are entries like any other
        bool take = pattern == 1 || (pattern == 2 && i % 3u == 0u) || (pattern == 3 && (rng(&state) & 1u)) || (pattern == 4 && i + 1 == count) || (pattern == 5 && i == 0);
        if (i >= count) take = true;
        float* a = &parts[(size_t)i * 16];
        float* b = a + 8;
        for (int k = 0; k < 8; k++) { a[k] = 0.25f; b[k] = 0.25f; }
        if (take) { a[i % 3u] = 1.0f; b[i % 3u] = 0.0f; }                        // error 0.5
        else if (rng(&state) % 7u == 0u) a[1] = std::nanf("");                     // a NaN half: error 0, not taken
        else if (rng(&state) % 7u == 0u) { a[2] = 0.25f + 2.0f * threshold; }      // error == threshold exactly: not taken
    }
    // brute force
    std::vector<uint32_t> want;
    for (uint32_t i = 0; i < count; i++)
        if (half_error(&parts[(size_t)i * 16], &parts[(size_t)i * 16 + 8]) > threshold) want.push_back(list[i]);
    const uint32_t taken = (uint32_t)want.size();
    while (want.size() % 64u) want.push_back(want[taken - 1]);
    // the three launches
    const uint32_t nw = sublist_waves(count);
    CHECK(nw == (count + 63u) / 64u);
    std::vector<unsigned long long> masks(nw, 0ull);
    std::vector<uint32_t> offsets(nw, 0u);
    for (uint32_t w = 0; w < nw; w++)
        for (uint32_t lane = 0; lane < 64u; lane++) {
            uint32_t i = 0xdeadbeefu;
            if (!sublist_lane_entry(w, lane, count, &i)) { CHECK(i == 0xdeadbeefu && w * 64u + lane >= count); continue; }
            CHECK(i == w * 64u + lane && i < count);
            if (half_error(&parts[(size_t)i * 16], &parts[(size_t)i * 16 + 8]) > threshold) masks[w] |= 1ull << lane;
        }
    uint32_t total = 0;
    for (uint32_t w = 0; w < nw; w++) { offsets[w] = total; total += (uint32_t)__builtin_popcountll(masks[w]); }
    CHECK(total == taken);
    std::vector<uint32_t> out(refine_padded(count) + 64u, GUARD);
    uint32_t last_waves = 0;
    for (uint32_t w = 0; w < nw; w++) {
        if (masks[w] == 0ull) continue;
        for (uint32_t lane = 0; lane < 64u; lane++) {
            uint32_t i = 0;
            if (!((masks[w] >> lane) & 1ull)) continue;
            CHECK(sublist_lane_entry(w, lane, count, &i));
            const uint32_t at = offsets[w] + refine_mask_rank(masks[w], lane);
            CHECK(at < refine_padded(count) && out[at] == GUARD); // inside the buffer, and no word is written twice
            out[at] = list[i];
        }
        if (!sublist_wave_is_last(masks[w], offsets[w], total)) continue;
        last_waves++;
        const uint32_t ll = sublist_last_lane(masks[w]);
        CHECK(ll < 64u && ((masks[w] >> ll) & 1ull) && (ll == 63u || (masks[w] >> (ll + 1u)) == 0ull));
        for (uint32_t lane = 0; lane < 64u; lane++) {
            uint32_t at = 0xdeadbeefu;
            if (!sublist_pad_word(total, lane, &at)) { CHECK(at == 0xdeadbeefu); continue; }
            CHECK(at == total + lane && at < refine_padded(total) && out[at] == GUARD);
            out[at] = list[w * 64u + ll];
        }
    }
    CHECK(last_waves == (taken ? 1u : 0u));
    CHECK(refine_padded(taken) == want.size() && refine_padded(taken) <= refine_padded(count));
    for (size_t i = 0; i < out.size(); i++) CHECK(out[i] == (i < want.size() ? want[i] : GUARD));
    g_lists++;
    g_taken += taken;
    return 0;
}

int main() {
    const uint32_t counts[] = {0, 1, 63, 64, 65, 4097};
    for (uint32_t count : counts)
        for (int pattern = 0; pattern < 6; pattern++)
            if (test_sublist(count, pattern, 0.125f)) return 1;
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
    std::printf("adaptive sublist test OK (%ld lists, %ld entries taken)\n", g_lists, g_taken);
    return 0;
}
