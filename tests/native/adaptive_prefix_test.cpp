// Host-only test of the resident-accumulator arithmetic of rustray_amd/csrc/rr_adaptive.h, built with g++ -ffp-contract=off
// -fsanitize=address,undefined by tests/test_adaptive_prefix_host.py: what k_prefix_masks and k_prefix_compact apply per lane.  A set of
// accumulators is laid out in a byte buffer with guard words through the shared offset functions, every word of every entry tagged with
// (entry, half, plane); a compaction is replayed on the CPU, wave by wave and lane by lane, into a second set and a second list, both with
// guards, and compared with a plain loop: the survivors in their order, two slots each, every plane, the flags, the pad as copies of the
// last survivor up to a multiple of 64, nothing written twice and nothing written behind.  Last: the ladder rule of the calls that refine
// level by level (ladder_fault), every fault at every position.
#include "../../rustray_amd/csrc/rr_adaptive.h"

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#define CHECK(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

static const uint8_t GUARD = 0x5a;
static long g_sets = 0, g_moved = 0;

static uint64_t tag64(uint32_t entry, uint32_t half, uint32_t plane) { return ((uint64_t)entry << 16) | ((uint64_t)half << 8) | plane | 0x7700000000000000ull; }
static uint32_t tag32(uint32_t entry, uint32_t half, uint32_t what) { return (entry << 4) | (half << 2) | what | 0x80000000u; }

// a set as bytes: 64 B of guard in front and behind
struct Set {
    unsigned long long n;
    std::vector<uint8_t> bytes;
    explicit Set(unsigned long long n_) : n(n_), bytes((size_t)prefix_set_bytes(n_) + 128u, GUARD) {}
    uint8_t* base() { return bytes.data() + 64; }
    uint64_t* word(uint32_t plane, unsigned long long slot) { return (uint64_t*)(base() + prefix_plane_offset(plane, n)) + slot; }
    uint32_t* id(unsigned long long slot) { return (uint32_t*)(base() + prefix_id_offset(n)) + slot; }
    uint32_t* flags(unsigned long long slot) { return (uint32_t*)(base() + prefix_flags_offset(n)) + slot; }
    bool guards_intact() const {
        for (size_t i = 0; i < 64; i++) if (bytes[i] != GUARD || bytes[bytes.size() - 1 - i] != GUARD) return false;
        return true;
    }
};

// the layout: planes, ids and flags tile the set's 64 n bytes without a gap or an overlap, each plane on a 16-byte boundary
static int test_layout(uint32_t entries) {
    const unsigned long long n = prefix_set_slots(entries);
    CHECK(n == 2ull * refine_padded(entries) && n % 128ull == 0ull);
    CHECK(prefix_set_bytes(n) == 64ull * n);
    unsigned long long at = 0;
    for (uint32_t k = 0; k < (uint32_t)PREFIX_PLANES; k++) { CHECK(prefix_plane_offset(k, n) == at && at % 16ull == 0ull); at += 8ull * n; }
    CHECK(prefix_id_offset(n) == at && at % 16ull == 0ull); at += 4ull * n;
    CHECK(prefix_flags_offset(n) == at && at % 16ull == 0ull); at += 4ull * n;
    CHECK(at == prefix_set_bytes(n));
    for (uint32_t i = 0; i < entries; i += (entries > 200u ? 97u : 1u)) CHECK(prefix_entry_slot(i) == 2ull * i && prefix_entry_slot(i) + 1ull < n);
    return 0;
}

// `pattern`: 0 = nothing taken, 1 = everything, 2 = every third entry, 3 = random, 4 = only lane 0 of every wave, 5 = only lane 63 of
// every wave (where the list has one), 6 = only the last entry, 7 = only the first
static int test_compaction(uint32_t count, int pattern) {
    uint32_t state = count * 7919u + (uint32_t)pattern;
    auto rng = [&state]() { state = state * 1664525u + 1013904223u; return state >> 8; };
    const uint32_t nw = sublist_waves(count);
    Set src(prefix_set_slots(count));
    std::vector<uint32_t> list(refine_padded(count));
    for (uint32_t i = 0; i < (uint32_t)list.size(); i++) {
        list[i] = i < count ? ((rng() & 0xffffu) | (rng() << 16)) : list[count - 1];
        for (uint32_t h = 0; h < 2u; h++) { // (the source's own pad holds sums too: they are never looked at)
            for (uint32_t k = 0; k < (uint32_t)PREFIX_PLANES; k++) *src.word(k, prefix_entry_slot(i) + h) = tag64(i, h, k);
            *src.id(prefix_entry_slot(i) + h) = tag32(i, h, 1u);
            *src.flags(prefix_entry_slot(i) + h) = tag32(i, h, 2u);
        }
    }
    std::vector<unsigned long long> masks(nw, 0ull);
    std::vector<uint32_t> offsets(nw, 0u), want;
    for (uint32_t i = 0; i < count; i++) {
        const bool take = pattern == 1 || (pattern == 2 && i % 3u == 0u) || (pattern == 3 && (rng() & 1u)) || (pattern == 4 && i % 64u == 0u) ||
                          (pattern == 5 && i % 64u == 63u) || (pattern == 6 && i + 1u == count) || (pattern == 7 && i == 0u);
        if (!take) continue;
        masks[i >> 6] |= 1ull << (i & 63u);
        want.push_back(i);
    }
    uint32_t total = 0;
    for (uint32_t w = 0; w < nw; w++) { offsets[w] = total; total += (uint32_t)__builtin_popcountll(masks[w]); }
    const uint32_t taken = (uint32_t)want.size();
    CHECK(total == taken);
    while (want.size() % 64u) want.push_back(want[taken - 1]); // the plain loop's pad: the last survivor again
    // the compaction, lane by lane
    Set dst(prefix_set_slots(taken));
    std::vector<uint32_t> list_out(refine_padded(taken) + 64u, 0x5a5a5a5au);
    std::vector<uint8_t> written(refine_padded(taken), 0);
    auto move = [&](uint32_t i, uint32_t j) {
        list_out[j] = list[i];
        for (uint32_t h = 0; h < 2u; h++) {
            for (uint32_t k = 0; k < (uint32_t)PREFIX_PLANES; k++) *dst.word(k, prefix_entry_slot(j) + h) = *src.word(k, prefix_entry_slot(i) + h);
            *dst.id(prefix_entry_slot(j) + h) = 0u; // the ids are not carried
            *dst.flags(prefix_entry_slot(j) + h) = *src.flags(prefix_entry_slot(i) + h);
        }
    };
    uint32_t last_waves = 0;
    for (uint32_t w = 0; w < nw; w++) {
        if (masks[w] == 0ull) continue;
        for (uint32_t lane = 0; lane < 64u; lane++) {
            uint32_t j = 0xdeadbeefu, i = 0;
            if (!prefix_survivor_entry(masks[w], offsets[w], lane, &j)) { CHECK(j == 0xdeadbeefu && !((masks[w] >> lane) & 1ull)); continue; }
            CHECK(sublist_lane_entry(w, lane, count, &i));
            CHECK(j < refine_padded(taken) && !written[j] && prefix_entry_slot(j) + 1ull < dst.n);
            written[j] = 1;
            move(i, j);
        }
        if (!sublist_wave_is_last(masks[w], offsets[w], total)) continue;
        last_waves++;
        for (uint32_t lane = 0; lane < 64u; lane++) {
            uint32_t i = 0xdeadbeefu, j = 0xdeadbeefu;
            if (!prefix_pad_entry(w, masks[w], total, lane, &i, &j)) { CHECK(j == 0xdeadbeefu && total + lane >= refine_padded(total)); continue; }
            CHECK(i < count && ((masks[w] >> (i & 63u)) & 1ull) && (i >> 6) == w && i == want[taken - 1]);
            CHECK(j == total + lane && j < refine_padded(taken) && !written[j] && prefix_entry_slot(j) + 1ull < dst.n);
            written[j] = 1;
            move(i, j);
        }
    }
    CHECK(last_waves == (taken ? 1u : 0u));
    CHECK(src.guards_intact() && dst.guards_intact());
    for (size_t j = 0; j < list_out.size(); j++) CHECK(list_out[j] == (j < want.size() ? list[want[j]] : 0x5a5a5a5au));
    for (uint32_t j = 0; j < (uint32_t)want.size(); j++) {
        CHECK(written[j]);
        for (uint32_t h = 0; h < 2u; h++) {
            for (uint32_t k = 0; k < (uint32_t)PREFIX_PLANES; k++) CHECK(*dst.word(k, 2ull * j + h) == tag64(want[j], h, k));
            CHECK(*dst.id(2ull * j + h) == 0u && *dst.flags(2ull * j + h) == tag32(want[j], h, 2u));
        }
    }
    g_sets++;
    g_moved += (long)want.size();
    return 0;
}

// the ladder rule: 2 .. 8 counts, each even and at least 2, strictly increasing; the first fault and its entry.  The ladders live in
// vectors of exactly n_levels entries, so a read behind the ladder is the sanitizer's to find.
static int test_ladders() {
    const unsigned short good[9] = {2, 4, 6, 8, 10, 12, 14, 16, 18};
    const unsigned int UNSET = 0xdeadbeefu;
    for (unsigned int n : {0u, 1u, 2u, 8u, 9u}) {
        const std::vector<unsigned short> v(good, good + n);
        unsigned int at = UNSET;
        const LadderFault f = ladder_fault(v.data(), n, 8u, &at);
        CHECK(f == ((n == 2u || n == 8u) ? LADDER_OK : LADDER_LEVELS));
        if (f == LADDER_LEVELS) CHECK(at == UNSET);
        at = UNSET;
        CHECK(ladder_fault(nullptr, n, 8u, &at) == ((n == 2u || n == 8u) ? LADDER_NULL : LADDER_LEVELS) && at == UNSET); // the count is judged first
    }
    for (unsigned int n : {2u, 3u, 8u})
        for (unsigned int k = 0; k < n; k++) {
            unsigned int at = UNSET;
            std::vector<unsigned short> v(good, good + n);
            v[k] = (unsigned short)(good[k] + 1u); // an odd entry (above its neighbour below: the fault is the entry's own)
            CHECK(ladder_fault(v.data(), n, 8u, &at) == LADDER_ENTRY && at == k);
            v[k] = 0; // an entry of 0: below 2 before it is "not above" anything
            CHECK(ladder_fault(v.data(), n, 8u, &at) == LADDER_ENTRY && at == k);
            v[k] = 1;
            CHECK(ladder_fault(v.data(), n, 8u, &at) == LADDER_ENTRY && at == k);
            if (k == 0) continue;
            v[k] = good[k - 1]; // equal neighbours
            CHECK(ladder_fault(v.data(), n, 8u, &at) == LADDER_ORDER && at == k);
            v[k] = (unsigned short)(good[k - 1] - 2u); // decreasing (2 -> 0 is an entry fault, covered above)
            CHECK(ladder_fault(v.data(), n, 8u, &at) == (v[k] ? LADDER_ORDER : LADDER_ENTRY) && at == k);
        }
    // the first fault wins: an odd entry at 1 before equal neighbours at 3; a valid ladder of 8 with large steps
    const unsigned short two_faults[4] = {6, 15, 30, 30}, wide[8] = {2, 6, 14, 30, 62, 126, 254, 65534};
    unsigned int at = UNSET;
    CHECK(ladder_fault(two_faults, 4u, 8u, &at) == LADDER_ENTRY && at == 1u);
    CHECK(ladder_fault(wide, 8u, 8u, &at) == LADDER_OK);
    CHECK(ladder_fault(wide, 8u, 7u, &at) == LADDER_LEVELS); // (the limit is the caller's)
    return 0;
}

int main() {
    if (test_ladders()) return 1;
    const uint32_t counts[] = {1, 63, 64, 65, 4097};
    for (uint32_t count : counts) {
        if (test_layout(count)) return 1;
        for (int pattern = 0; pattern < 8; pattern++)
            if (test_compaction(count, pattern)) return 1;
    }
    // single masks: empty, full, bit 0 alone, bit 63 alone -- where every lane's entry goes, and the pad behind a full wave
    const unsigned long long masks[] = {0ull, ~0ull, 1ull, 1ull << 63};
    for (unsigned long long m : masks)
        for (uint32_t lane = 0; lane < 64u; lane++) {
            uint32_t j = 0xdeadbeefu, below = 0;
            for (uint32_t b = 0; b < lane; b++) below += (uint32_t)((m >> b) & 1ull);
            const bool got = prefix_survivor_entry(m, 100u, lane, &j);
            CHECK(got == (((m >> lane) & 1ull) != 0ull) && j == (got ? 100u + below : 0xdeadbeefu));
        }
    uint32_t i = 0, j = 0;
    CHECK(!prefix_pad_entry(0u, ~0ull, 64u, 0u, &i, &j));                                // 64 taken: no pad
    CHECK(prefix_pad_entry(3u, 1ull << 63, 65u, 62u, &i, &j) && i == 3u * 64u + 63u && j == 127u);
    CHECK(!prefix_pad_entry(3u, 1ull << 63, 65u, 63u, &i, &j));                           // 63 pad entries behind 65
    CHECK(prefix_pad_entry(0u, 1ull, 1u, 0u, &i, &j) && i == 0u && j == 1u);
    CHECK(prefix_set_slots(0) == 0ull && prefix_set_slots(1) == 128ull && prefix_set_slots(64) == 128ull && prefix_set_slots(65) == 256ull);
    std::printf("adaptive prefix test OK (%ld sets, %ld entries moved)\n", g_sets, g_moved);
    return 0;
}
