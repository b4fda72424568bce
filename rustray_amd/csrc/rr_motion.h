// rr_motion.h — the arithmetic of the per-pixel motion of moved items that host and device share (rr_motion_records; the yardstick is
// rustray_amd/temporal.py: motion_records), and the host-only builder of the call's table.  Plain logic, no HIP call: k_motion_records
// (rr_kernels.hip) applies motion_pixel per lane, and tests/native/motion_test.cpp runs the same functions as a host loop.
//
// Every step is exact in binary32 in the order written here and must be compiled without contraction (-ffp-contract=off, as the library
// is): host, device and numpy give the same bits.  There are no transcendentals.  `row` and `dot` are rr_temporal.h's.
#pragma once
#include "rr_temporal.h" // TpFrame, temporal_world, denoise_is_finite

#include <algorithm>
#include <cstdio>
#include <utility>
#include <vector>

// One moved item: its object id, rows 0 .. 2 of its trans_inv as the handle holds it (the frame the records were traced with) and rows
// 0 .. 2 of its trans in the frame the history was rendered from; row r is the four floats at 4 r.  112 bytes, sorted by id as unsigned.
struct MoEntry {
    unsigned int id, _pad[3];
    float inv[12], prev[12];
};
static_assert(sizeof(MoEntry) == 112, "the table of rr_motion_records is 112 bytes per entry");

// a row of MoEntry times (x, y, z, 1): temporal_row of the column-major matrix the row was taken from
RR_SETUP_HD float motion_row(const float* a, float x, float y, float z) { return ((a[0] * x + a[1] * y) + a[2] * z) + a[3] * 1.0f; }

// the entry of `id` among n entries sorted by id, or -1
RR_SETUP_HD int motion_find(const MoEntry* table, unsigned int n, unsigned int id) {
    unsigned int lo = 0, hi = n;
    while (lo < hi) {
        const unsigned int mid = lo + ((hi - lo) >> 1);
        if (table[mid].id < id) lo = mid + 1; else hi = mid;
    }
    return (lo < n && table[lo].id == id) ? (int)lo : -1;
}

// where the point `world` of an item lay one step ago, minus where it lies now; all three 0 if one of them is not finite
RR_SETUP_HD void motion_of_entry(const float* inv, const float* prev, const float* world, float* m) {
    float local[3];
    for (int r = 0; r < 3; r++) local[r] = motion_row(inv + 4 * r, world[0], world[1], world[2]);
    for (int r = 0; r < 3; r++) m[r] = motion_row(prev + 4 * r, local[0], local[1], local[2]) - world[r];
    if (!denoise_is_finite(m[0]) || !denoise_is_finite(m[1]) || !denoise_is_finite(m[2])) m[0] = m[1] = m[2] = 0.0f;
}

// valid_p of rr_denoise_records: depth and the three floats of the normal are finite (a miss has a NaN normal)
RR_SETUP_HD bool motion_valid(float depth, const float* n) {
    return denoise_is_finite(depth) && denoise_is_finite(n[0]) && denoise_is_finite(n[1]) && denoise_is_finite(n[2]);
}

// One pixel: world = the point its depth puts on its ray (whatever the record holds), m = its motion.
RR_SETUP_HD void motion_pixel(const TpFrame& f, unsigned int x, unsigned int y, float depth, const float* n_p, unsigned int id_p, const MoEntry* table,
                              unsigned int n_moved, float* world, float* m) {
    temporal_world(f, x, y, depth, world);
    m[0] = m[1] = m[2] = 0.0f;
    if (!motion_valid(depth, n_p)) return;
    const int e = motion_find(table, n_moved, id_p);
    if (e >= 0) motion_of_entry(table[e].inv, table[e].prev, world, m);
}

// ---- host only: the table of one call --------------------------------------------------------------------------------------------
// item_of(i, inv12, &id) gives rows 0 .. 2 of trans_inv and the object id of item i < n_items; item_index[k] < n_items names moved item
// k and prev_trans + 16 k is its previous trans, column-major.  *out: one entry per listed item, sorted by id as unsigned.
// false with a message in msg: an index out of range, a prev_trans that is not finite, or two listed items with one id.
template <class ItemOf>
inline bool motion_build_table(ItemOf item_of, unsigned int n_items, const unsigned int* item_index, const float* prev_trans, unsigned int n_moved,
                               std::vector<MoEntry>* out, char* msg, size_t msg_len) {
    out->clear();
    std::vector<std::pair<unsigned int, unsigned int>> order(n_moved); // (id, entry)
    for (unsigned int k = 0; k < n_moved; k++) {
        if (item_index[k] >= n_items) {
            snprintf(msg, msg_len, "item_index[%u] = %u, the scene has %u items", k, item_index[k], n_items);
            return false;
        }
        for (int c = 0; c < 16; c++)
            if (!denoise_is_finite(prev_trans[16 * (size_t)k + c])) {
                snprintf(msg, msg_len, "prev_trans of entry %u is not finite (float %d)", k, c);
                return false;
            }
        float inv[12];
        item_of(item_index[k], inv, &order[k].first);
        order[k].second = k;
    }
    std::sort(order.begin(), order.end());
    for (unsigned int k = 1; k < n_moved; k++)
        if (order[k].first == order[k - 1].first) {
            snprintf(msg, msg_len, "entries %u and %u (items %u and %u) have the same object id %u: a record holds no item index, the id is the key",
                     order[k - 1].second, order[k].second, item_index[order[k - 1].second], item_index[order[k].second], order[k].first);
            return false;
        }
    out->resize(n_moved);
    for (unsigned int k = 0; k < n_moved; k++) {
        MoEntry& e = (*out)[k];
        const unsigned int src = order[k].second;
        e._pad[0] = e._pad[1] = e._pad[2] = 0u;
        item_of(item_index[src], e.inv, &e.id);
        const float* p = prev_trans + 16 * (size_t)src;
        for (int r = 0; r < 3; r++)
            for (int c = 0; c < 4; c++) e.prev[4 * r + c] = p[4 * c + r];
    }
    return true;
}
