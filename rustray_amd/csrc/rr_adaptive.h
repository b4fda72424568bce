// rr_adaptive.h — the arithmetic of adaptive sampling that host and device share: the half-buffer error estimate of one pixel
// (rustray_amd/adaptive.py: half_error), the order in which a frame's pixels enter a refinement list (refine_list: 8x8 blocks
// row-major, row-major inside a block), and where the entries of a list go in the list made from it (refine_sublist).  Plain host
// logic, no HIP calls and no include of its own: k_refine_masks and k_refine_scatter (rr_kernels.hip), one body each over the two entry
// sources below, apply these functions per lane, rr_api_adaptive.h and rr_api_levels.h size their buffers with them, and
// tests/native/adaptive_order_test.cpp and adaptive_sublist_test.cpp check all of it on the CPU.  Last: where the accumulators of a
// list's entries lie and where a compaction moves them (rr_render_adaptive_prefix: k_prefix_masks, k_prefix_compact, rr_api_prefix.h;
// tests/native/adaptive_prefix_test.cpp).
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
// of entry i's two part records (rr_render_pixel_parts at K = 2).  V4: four floats x y z w, 16 bytes (the device's float4); a record is
// two of them and its colour the first one's x y z, so the halves of entry i are parts[4 i] and parts[4 i + 2]: two whole 16-byte loads.
template <class V4> RR_SETUP_HD float half_error_of_parts(const V4* parts, unsigned long long i) {
    const V4 a = parts[4ull * i], b = parts[4ull * i + 2];
    const float ca[3] = {a.x, a.y, a.z}, cb[3] = {b.x, b.y, b.z};
    return half_error(ca, cb);
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
// where the frame keeps what belongs to pixel xy = x | y << 16: y * width + x (< 2^30: every frame's slots fit the accumulators)
RR_SETUP_HD unsigned int frame_index(unsigned int xy, unsigned int width) { return (xy >> 16) * width + (xy & 0xffffu); }
// its inverse: the position of pixel (x, y) -- the sort key of adaptive.refine_list
RR_SETUP_HD unsigned long long refine_pixel_position(unsigned int x, unsigned int y, unsigned int width) {
    return ((unsigned long long)((y >> 3) * refine_blocks_x(width) + (x >> 3)) << 6) + (y & 7u) * 8u + (x & 7u);
}

// a list of `count` entries, padded with its last one to whole 64-ray packets (an empty list has no pad)
RR_SETUP_HD unsigned int refine_padded(unsigned int count) { return (count + 63u) & ~63u; }
// entries a list of a width x height frame may need: every pixel, padded
RR_SETUP_HD unsigned long long refine_capacity(unsigned int width, unsigned int height) { return ((unsigned long long)width * height + 63ull) & ~63ull; }

// ---- the list of a list (adaptive.refine_sublist): entries 64 w .. 64 w + 63 of a list of `count` entries are wave w's, lane l holding
// entry 64 w + l; the entries with error > threshold keep their order.  A wave's 64-bit mask has bit l set where lane l's entry is taken.
RR_SETUP_HD unsigned int sublist_waves(unsigned int count) { return (count + 63u) >> 6; } // count <= 2^29
// the entry of lane `lane` of wave `wave`; false = the lane lies behind the list (the caller's own pad is never looked at)
RR_SETUP_HD bool sublist_lane_entry(unsigned int wave, unsigned int lane, unsigned int count, unsigned int* entry) {
    const unsigned int i = (wave << 6) | lane;
    if (i >= count) return false;
    *entry = i;
    return true;
}
// set bits of `mask` below bit `lane`: the place of a taken entry among its wave's (on the device: the two mbcnt instructions)
RR_SETUP_HD unsigned int refine_mask_rank(unsigned long long mask, unsigned int lane) {
#if defined(__HIP_DEVICE_COMPILE__)
    (void)lane; // (the hardware counts below the executing lane, which is `lane`)
    return __builtin_amdgcn_mbcnt_hi((unsigned int)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned int)mask, 0u));
#else
    return (unsigned int)__builtin_popcountll(mask & ((1ull << lane) - 1ull));
#endif
}
// the wave whose taken entries end the output (offset: taken entries of the waves before it; total: all taken) writes the pad
RR_SETUP_HD bool sublist_wave_is_last(unsigned long long mask, unsigned int offset, unsigned int total) {
    return mask != 0ull && offset + (unsigned int)__builtin_popcountll(mask) == total;
}
// the lane of that wave whose entry is the output's last one
RR_SETUP_HD unsigned int sublist_last_lane(unsigned long long mask) { return 63u - (unsigned int)__builtin_clzll(mask); } // mask != 0
// lane `lane` of that wave writes one word of the pad at *at; false = the pad ends before this lane (fewer than 64 words: one per lane)
RR_SETUP_HD bool sublist_pad_word(unsigned int total, unsigned int lane, unsigned int* at) {
    if (total + lane >= refine_padded(total)) return false;
    *at = total + lane;
    return true;
}

// ---- the entry source of a compaction: what differs between the list of a frame and the list of a list.  waves(): the 64-lane groups
// of the source; entry(wave, lane, &index, &word): false = the lane has no entry (nothing is then written); else *index is where the
// entry's two part records and its error lie, and *word what it contributes to the output list.  A third source is a third such struct.
// On wave64 one wave is one 8x8 block of the frame: lane l is the block's pixel l, the ballot of the lanes' flags is the block's
// 64-bit refine mask, and the blocks row-major ARE the list's order.
struct FrameSource {
    unsigned int width, height;
    RR_SETUP_HD unsigned int waves() const { return refine_blocks(width, height); }
    RR_SETUP_HD bool entry(unsigned int wave, unsigned int lane, unsigned int* index, unsigned int* word) const {
        if (!refine_position_pixel(((unsigned long long)wave << 6) | lane, width, height, word)) return false;
        *index = frame_index(*word, width);
        return true;
    }
};
// 64 consecutive entries of a list per wave; the entries' coordinates are not interpreted: there is no frame here
struct ListSource {
    const unsigned int* list;
    unsigned int count;
    RR_SETUP_HD unsigned int waves() const { return sublist_waves(count); }
    RR_SETUP_HD bool entry(unsigned int wave, unsigned int lane, unsigned int* index, unsigned int* word) const {
        if (!sublist_lane_entry(wave, lane, count, index)) return false;
        *word = list[*index];
        return true;
    }
};

// ---- resident accumulators (rr_render_adaptive_prefix): the pixels of a list keep their integer sums from level to level.  A SET holds
// the two halves of every entry of a padded list in list order: entry i owns slots 2 i (samples s with s mod 2 == 0) and 2 i + 1, which
// are the slots rr_render_pixel_parts gives it at K = 2.  With n slots a set is seven planes of n 8-byte words (colour r g b, normal
// x y z, depth), then n 4-byte object ids, then n 4-byte flag words: 64 n bytes, and with n a multiple of 128 every plane starts on a
// 16-byte boundary, so the two slots of an entry are one 16-byte access per plane (8 bytes for ids and flags).
RR_SETUP_HD unsigned long long prefix_set_slots(unsigned int entries) { return 2ull * refine_padded(entries); } // n of the set of a list of `entries`
RR_SETUP_HD unsigned long long prefix_set_bytes(unsigned long long n) { return 64ull * n; }
enum { PREFIX_PLANES = 7 }; // 8-byte planes of a set
RR_SETUP_HD unsigned long long prefix_plane_offset(unsigned int plane, unsigned long long n) { return 8ull * plane * n; } // bytes; plane < PREFIX_PLANES
RR_SETUP_HD unsigned long long prefix_id_offset(unsigned long long n) { return 56ull * n; }
RR_SETUP_HD unsigned long long prefix_flags_offset(unsigned long long n) { return 60ull * n; }
// the first of the two slots of entry i (the other one follows it)
RR_SETUP_HD unsigned long long prefix_entry_slot(unsigned int entry) { return 2ull * entry; }
// Compaction of a set into the set of the list made from its list (sublist_* above give the wave, the lane's entry and the last wave):
// the entry of lane `lane` of a wave with `mask`, `offset` taken entries before the wave; false = the lane's entry is not taken
RR_SETUP_HD bool prefix_survivor_entry(unsigned long long mask, unsigned int offset, unsigned int lane, unsigned int* entry_out) {
    if (!((mask >> lane) & 1ull)) return false;
    *entry_out = offset + refine_mask_rank(mask, lane);
    return true;
}
// The last wave's pad: lane `lane` copies the source entry *src (the wave's last taken one) to entry *dst of the new list and set;
// false = the pad ends before this lane.  A pad entry is a duplicate like any other: traced, accumulated and never looked at.
RR_SETUP_HD bool prefix_pad_entry(unsigned int wave, unsigned long long mask, unsigned int total, unsigned int lane, unsigned int* src, unsigned int* dst) {
    if (!sublist_pad_word(total, lane, dst)) return false;
    *src = (wave << 6) | sublist_last_lane(mask);
    return true;
}

// ---- the ladder of a call that refines level by level (rr_render_adaptive_levels: level_samples; rr_render_adaptive_prefix:
// prefix_samples), host only: 2 .. max_levels counts, every one even and at least 2 (the two halves of a pixel must be equal), strictly
// increasing.  The first fault in the order the calls report them, and in *at the entry it was found at (LADDER_ENTRY, LADDER_ORDER:
// entry *at is not above entry *at - 1); nothing of `ladder` is read where n_levels is refused.
enum LadderFault { LADDER_OK, LADDER_LEVELS, LADDER_NULL, LADDER_ENTRY, LADDER_ORDER };
inline LadderFault ladder_fault(const unsigned short* ladder, unsigned int n_levels, unsigned int max_levels, unsigned int* at) {
    if (n_levels < 2u || n_levels > max_levels) return LADDER_LEVELS;
    if (!ladder) return LADDER_NULL;
    for (unsigned int l = 0; l < n_levels; l++) {
        *at = l;
        if (ladder[l] < 2u || (ladder[l] & 1u)) return LADDER_ENTRY;
        if (l && ladder[l] <= ladder[l - 1]) return LADDER_ORDER;
    }
    return LADDER_OK;
}
