// Host-only test of the (slot, sample) mapping of rr_render_pixel_parts (rustray_amd/csrc/rr_primary_setup.h: primary_part_sample and the
// primary_index that takes lg_parts), built with g++ -fsanitize=address,undefined by tests/test_pixel_parts.py.  A call with K parts runs
// as n * K accumulator slots of S / K samples each under the frame's own batch plan (rr_frame_plan.h); over all primary indices of all
// batches every pair (slot, frame sample) with sample = slot (mod K) must occur exactly once and no other pair at all, whatever sample
// group the plan chose and wherever a batch starts.  With one part the new function is the old one.
#include "../../rustray_amd/csrc/rr_frame_plan.h"
#include "../../rustray_amd/csrc/rr_primary_setup.h"

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <vector>

#define CHECK(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

static long g_batches = 0, g_grouped = 0, g_mid = 0, g_indices = 0;

// the batches [first, first + B) of `plan` over n_slots slots, as run_batches cuts them
static int check_cover(uint32_t n_slots, uint32_t S, uint32_t lg_parts, const FramePlan& plan, uint64_t B) {
    const uint32_t K = 1u << lg_parts, per_slot = S / K;
    CHECK(plan.total_primary == (uint64_t)n_slots * per_slot);
    const PrimaryFrame pf = primary_frame(nullptr, n_slots, plan.G);
    std::vector<uint8_t> seen((size_t)n_slots * S, 0);
    for (uint64_t first = 0; first < plan.total_primary; first += B) {
        const uint32_t n = (uint32_t)std::min<uint64_t>(B, plan.total_primary - first);
        const uint32_t G = batch_group(plan, n_slots, first, n);
        const PrimaryLaunch at = primary_launch(first, n_slots, G);
        g_batches++; g_grouped += G > 1; g_mid += first % n_slots != 0;
        for (uint32_t i = 0; i < n; i++) {
            uint32_t slot = 0xffffffffu, s = 0xffffffffu, slot1, k;
            primary_index(pf, at, lg_parts, i, &slot, &s);
            primary_index(pf, at, i, &slot1, &k); // the plan's own view: the k-th sample of the slot
            CHECK(slot == slot1 && slot < n_slots && k < per_slot && s < S);
            CHECK((s & (K - 1u)) == (slot & (K - 1u)) && (s >> lg_parts) == k);
            CHECK(s == primary_part_sample(slot, k, lg_parts));
            CHECK(seen[(size_t)slot * S + s] == 0);
            seen[(size_t)slot * S + s] = 1;
            g_indices++;
        }
    }
    for (uint32_t slot = 0; slot < n_slots; slot++)
        for (uint32_t s = 0; s < S; s++) CHECK(seen[(size_t)slot * S + s] == (((s ^ slot) & (K - 1u)) == 0u ? 1 : 0));
    return 0;
}

static int test_mapping() {
    const uint32_t lgs[] = {1, 2, 6}, ns[] = {1, 3, 32, 33}, per_slots[] = {1, 2, 3, 4, 8, 64}, groups[] = {0, 1, 2, 4, 8, 16, 32, 64};
    for (uint32_t lg : lgs) for (uint32_t n : ns) for (uint32_t m : per_slots) {
        const uint32_t K = 1u << lg, S = K * m, n_slots = n * K;
        for (uint32_t forced : groups) for (int small_budget = 0; small_budget < 2; small_budget++) {
            // a budget that holds the call in one batch, and one that cuts it into batches of one whole group (at least 4096 rays)
            const uint64_t small = 128ull * n_slots * (forced ? forced : 64u);
            const FramePlan plan = plan_frame(FramePlanInputs{n_slots, m, 4, small_budget ? small : 1ull << 34, forced, 0, 2, 1, 0});
            // every group the plan can choose: a power of two that divides S / K, with whole packets of 64 / G slots
            CHECK(plan.G >= 1 && plan.G <= 64 && (plan.G & (plan.G - 1)) == 0 && m % plan.G == 0);
            CHECK(plan.G == 1 || n_slots % (64 / plan.G) == 0);
            if (forced >= 2) CHECK((plan.G == forced) == (m % forced == 0 && n_slots % (64 / forced) == 0));
            if (check_cover(n_slots, S, lg, plan, plan.B)) return 1;
        }
        // batches that start in the middle of a sample slice (G = 1 is then the only form)
        const FramePlan whole = plan_frame(FramePlanInputs{n_slots, m, 4, 1ull << 34, 1, 0, 2, 1, 0});
        const uint64_t odd = std::max<uint64_t>(1, whole.total_primary / 3) + 7;
        if (check_cover(n_slots, S, lg, whole, odd)) return 1;
    }
    CHECK(g_grouped > 0 && g_mid > 0 && g_batches > g_grouped);
    return 0;
}

// one part: what the functions returned before parts existed
static int test_one_part() {
    const uint32_t npixs[] = {1, 3, 64, 1900}, sampless[] = {1, 6, 64};
    for (uint32_t npix : npixs) for (uint32_t samples : sampless) for (uint32_t forced : {0u, 1u, 2u, 64u}) {
        const FramePlan plan = plan_frame(FramePlanInputs{npix, samples, 4, 1ull << 34, forced, 0, 2, 1, 0});
        const PrimaryFrame pf = primary_frame(nullptr, npix, plan.G);
        const PrimaryLaunch at = primary_launch(0, npix, batch_group(plan, npix, 0, plan.B));
        for (uint32_t i = 0; i < (uint32_t)plan.B; i++) {
            uint32_t a, b, c, d;
            primary_index(pf, at, i, &a, &b);
            primary_index(pf, at, 0u, i, &c, &d);
            CHECK(a == c && b == d && primary_part_sample(a, b, 0u) == b);
        }
    }
    CHECK(sizeof(PrimaryLaunch) == 16 && sizeof(PrimaryFrame) == sizeof(const float*) + 2 * sizeof(RrDiv));
    return 0;
}

int main() {
    if (test_mapping() || test_one_part()) return 1;
    std::printf("pixel parts test OK (%ld batches, %ld grouped, %ld mid-slice, %ld indices)\n", g_batches, g_grouped, g_mid, g_indices);
    return 0;
}
