// rr_walk.h — layer 2 of the device code: the BVH4 node step and the walks of ONE mesh's tree, per lane (blas_closest, blas_any)
// and for a packet whose 64 lanes share one control flow (blas_closest_packet).  Stands for TriMesh::cast_local_ray_and_get_normal
// (reference src/shape/mesh.rs:67) over parry's Qbvh; the box tests here are conservative filters, the hits are rr_primitives.h's.
//
// Offers: rr_global; Slab4, make_slab, make_slab4; TriBest, blas_closest<SCALAR_LEAVES>, blas_any, blas_closest_packet;
// the instrumentation hooks RR_UTIL / RR_UTIL_KIND (empty unless -DRR_EXP_UTIL; g_util is read by rr_api_probe.h: rr_exp_util);
// and, for the top-level walks of rr_trace.h, the step itself as macros: RR_NODE4_STEP, RR_NODE4_STEP_PLAIN, RR_NODE4_STEP_ANY
// with STK and RR_SENTINEL.  A step macro expands where it is USED, so everything it is made of (RR_NODE4_FORM, RR_NODE4_ROWS_*,
// RR_NODE4_TESTS, RR_NODE4_SINGLE_HIT, RR_NODE4_DESCEND_*, RR_ROW, RR_CHILD, RR_CSWAP, RR_UTIL_UNI, RR_UTIL_ONE, RR_UTIL_NODE_SLOT)
// has to stay defined for that one user: rr_trace.h un-defines the whole step, these included, at its own end.
// What only the walks in this file expand (RR_TRI_*, RR_LEAF_CLOSEST, RR_LEAF_ANY, RR_PK_*, RR_SCSWAP) is un-defined at the end of this file.
// Needs: rr_primitives.h; RR_PEND_NUM / RR_PEND_DEN from the knob block of rr_kernels.hip; an `int* s_stack` (LDS,
// RR_STACK_DEPTH * RR_BLOCK words) in scope wherever a step or STK is expanded.
#pragma once
#include "rr_primitives.h"

// ---------------------------------------------------------------------------
// BVH4 traversal (DNode4, rr_device.h).  Per-lane stack in LDS, lane-interleaved (conflict free), terminated by a
// sentinel entry instead of a depth test.
// ---------------------------------------------------------------------------
// A scene pointer is a GLOBAL pointer.  The trace kernels get the scene view as kernel arguments and the compiler knows;
// k_shade reads it from a device record (DShadeConst), where a pointer loaded from memory is generic and every access
// through it becomes a flat_load (aperture check, counted against both vmcnt and lgkmcnt).  The integer round trip gives
// the optimiser the address space back.
template <class T> RR_DEV const T* rr_global(const T* p) { return (const T*)(const __attribute__((address_space(1))) T*)(uintptr_t)p; }
#define STK(sp) s_stack[(sp) * RR_BLOCK + threadIdx.x]
#define RR_SENTINEL ((int)0x80000000) // bottom of every stack; root of an empty tree

// Developer instrumentation (-DRR_EXP_UTIL): active lanes per executed step, by kind.  Never in the shipped build.
#ifdef RR_EXP_UTIL
__device__ unsigned long long g_util[64];
__shared__ uint32_t s_util_kind; // 0: closest-hit level 1, 1: closest-hit deeper levels, 2: shadow rays (set by the kernels)
#define RR_UTIL(slot) { const unsigned long long m_ = __ballot(1); if ((int)(threadIdx.x & 63u) == __ffsll((long long)m_) - 1) { \
        atomicAdd(&g_util[10 * s_util_kind + 2 * (slot)], (unsigned long long)__popcll(m_)); atomicAdd(&g_util[10 * s_util_kind + 2 * (slot) + 1], 1ull); } }
#define RR_UTIL_KIND(k) { s_util_kind = (k); __syncthreads(); }
#define RR_UTIL_NODE_SLOT (((const void*)nodes4_ptr_ == (const void*)sc.tnodes4 || (const void*)nodes4_ptr_ == (const void*)sc.tnodes4c) ? 0 : 2)
// steps whose address is the same in every active lane (g_util[30 + ...]: [0] same address, [1] same address and same key2)
#define RR_UTIL_UNI(slot, addr, key2) { const unsigned long long m_ = __ballot(1); const int l_ = __ffsll((long long)m_) - 1;                \
        const uint32_t a_ = (uint32_t)(addr), k_ = (uint32_t)(key2); const uint32_t ua_ = __shfl(a_, l_), uk_ = __shfl(k_, l_);               \
        const bool u1_ = __ballot(a_ == ua_) == m_; const bool u2_ = u1_ && __ballot(k_ == uk_) == m_;                                       \
        if ((int)(threadIdx.x & 63u) == l_) { if (u1_) atomicAdd(&g_util[30 + 10 * s_util_kind + 2 * (slot)], 1ull);                         \
                                              if (u2_) atomicAdd(&g_util[30 + 10 * s_util_kind + 2 * (slot) + 1], 1ull); } }
// node steps in which no lane has more than one (g_util[60]) / two (61) children hit, of all node steps (62)
#define RR_UTIL_ONE { const int nh_ = (int)h0 + (int)h1 + (int)h2 + (int)h3; const unsigned long long m_ = __ballot(1); const bool one_ = __ballot(nh_ > 1) == 0ull; const bool two_ = __ballot(nh_ > 2) == 0ull; \
        if ((int)(threadIdx.x & 63u) == __ffsll((long long)m_) - 1) { if (one_) atomicAdd(&g_util[60], 1ull); if (two_) atomicAdd(&g_util[61], 1ull); atomicAdd(&g_util[62], 1ull); } }
#else
#define RR_UTIL(slot)
#define RR_UTIL_KIND(k)
#define RR_UTIL_UNI(slot, addr, key2)
#define RR_UTIL_ONE
#endif

// The traversal's own box test is NOT part of the parity contract (only the exact primitive tests decide
// hits), so its reciprocal is the hardware approximation.  The subtraction stays in front of the multiply:
// the fused form plane * inv - o * inv cancels catastrophically when the origin sits within the shadow bias
// of a box plane (measured as missed hits on scenes/spheres_room).
struct SlabRay { f3 o, inv; };
RR_DEV SlabRay make_slab(f3 o, f3 d) {
    SlabRay r; r.o = o;
    r.inv = mk3(__builtin_amdgcn_rcpf(d.x), __builtin_amdgcn_rcpf(d.y), __builtin_amdgcn_rcpf(d.z));
    return r;
}

// One BVH4 inner-node step: four slab tests, a five-exchange sorting network on (entry, child), the three
// farther children written far-to-near with the stack pointer advanced past the ones that were hit (a missed
// child sorts last and its slot is overwritten), and the nearest taken directly.  Single branch.
#define RR_CSWAP(ka, ca, kb, cb) { const bool s_ = kb < ka; const float tk_ = s_ ? ka : kb; const int tc_ = s_ ? ca : cb; \
                                   ka = s_ ? kb : ka; ca = s_ ? cb : ca; kb = tk_; cb = tc_; }
// Per-walk constants of the 4-wide step: the ray in slab form, and for every axis which of the node's two plane
// rows is the near one for this ray's direction sign (row index 0/1), so that the step loads "near" and "far" rows
// directly instead of ordering the two plane distances of every child with a min and a max.
typedef float v2f __attribute__((ext_vector_type(2)));
// Rows are addressed as (uniform node array) + 32-bit byte offset, so the loads take the scalar-base form and the
// step needs one 32-bit add per row instead of 64-bit address arithmetic: off = (tree base + node) * 128 + row * 16.
struct Slab4 {
    f3 o, inv; uint32_t nx, fx, ny, fy, nz, fz, cc;
    // wave-uniform copies: `uni` when every lane that starts this walk has the same tree and the same direction signs, so
    // that a step whose node is the same in all of its lanes can fetch the rows ONCE through the scalar cache (u*: the same
    // row offsets in scalar registers)
    bool uni; uint32_t unx, ufx, uny, ufy, unz, ufz, ucc;
};
RR_DEV Slab4 make_slab4(const SlabRay& r, uint32_t node_base) {
    Slab4 s; s.o = r.o; s.inv = r.inv;
    const uint32_t sx = __float_as_uint(r.inv.x) >> 31, sy = __float_as_uint(r.inv.y) >> 31, sz = __float_as_uint(r.inv.z) >> 31;
    const uint32_t b = node_base << 7;
    s.nx = b + (sx << 4); s.fx = b + ((1u - sx) << 4);
    s.ny = b + ((2u + sy) << 4); s.fy = b + ((3u - sy) << 4);
    s.nz = b + ((4u + sz) << 4); s.fz = b + ((5u - sz) << 4);
    s.cc = b + (6u << 4);
    const uint32_t key = b | (sx << 4) | (sy << 5) | (sz << 6); // b is a multiple of 128
    const uint32_t ukey = (uint32_t)__builtin_amdgcn_readfirstlane((int)key);
    s.uni = __ballot(key != ukey) == 0ull;
    const uint32_t ub = ukey & ~127u, ux = (ukey >> 4) & 1u, uy = (ukey >> 5) & 1u, uz = (ukey >> 6) & 1u;
    s.unx = ub + (ux << 4); s.ufx = ub + ((1u - ux) << 4);
    s.uny = ub + ((2u + uy) << 4); s.ufy = ub + ((3u - uy) << 4);
    s.unz = ub + ((4u + uz) << 4); s.ufz = ub + ((5u - uz) << 4);
    s.ucc = ub + (6u << 4);
    return s;
}
RR_DEV DTriX tri_at(const DTriX* tris, uint32_t byte_off) { return *(const DTriX*)((const char*)tris + byte_off); }
RR_DEV float4 node_row(const DNode4* nodes, uint32_t byte_off) { return *(const float4*)((const char*)nodes + byte_off); }
// the same row at a wave-uniform offset, through the constant address space: one s_load_dwordx4 for the wave, the row
// arrives in scalar registers and feeds the packed subtracts directly.  (A vector load costs the L1 pipeline a quad of
// lanes per cycle whether or not the 64 addresses are equal: 16 cycles per row, and the walks are bound by exactly that.)
RR_DEV float4 node_row_uniform(const DNode4* nodes, uint32_t byte_off) {
    const rr_f4v v = *(const __attribute__((address_space(4))) rr_f4v*)((const __attribute__((address_space(4))) char*)(uintptr_t)nodes + byte_off);
    return make_float4(v.x, v.y, v.z, v.w);
}
// (row - o) * inv for the four children of one plane row, as two packed pairs
#define RR_ROW(row, oc, ic, lo_, hi_) const v2f lo_ = (v2f{row.x, row.y} - v2f{oc, oc}) * v2f{ic, ic}; \
                                      const v2f hi_ = (v2f{row.z, row.w} - v2f{oc, oc}) * v2f{ic, ic};
// conservative hit test of one child from its three near and three far plane distances (4e-6 of relative slack on either side)
#define RR_CHILD(k_, h_, nx, ny, nz, fx, fy, fz)                                                               \
    float k_; bool h_;                                                                                         \
    {                                                                                                          \
        const float tn_ = fmaxf(fmaxf(nx, ny), fmaxf(nz, 0.0f));                                               \
        const float tf_ = fminf(fminf(fx, fy), fminf(fz, RR_FLT_MAX));                                         \
        const float tc_ = tn_ * 0.999996f;                                                                     \
        h_ = tc_ <= tf_ * 1.000004f && tc_ <= bound_;                                                          \
        k_ = h_ ? tn_ : inf_;                                                                                  \
    }
#define RR_NODE4_ROWS_VECTOR(nodes4, s4)                                                                        \
        const uint32_t no_ = (uint32_t)cur << 7;                                                               \
        const float4 rnx = node_row(nodes4, no_ + (s4).nx), rfx = node_row(nodes4, no_ + (s4).fx);             \
        const float4 rny = node_row(nodes4, no_ + (s4).ny), rfy = node_row(nodes4, no_ + (s4).fy);             \
        const float4 rnz = node_row(nodes4, no_ + (s4).nz), rfz = node_row(nodes4, no_ + (s4).fz);             \
        const float4 cc = node_row(nodes4, no_ + (s4).cc);
#define RR_NODE4_ROWS_UNIFORM(nodes4, s4)                                                                       \
        const uint32_t no_ = (uint32_t)ucur_ << 7;                                                             \
        const float4 rnx = node_row_uniform(nodes4, no_ + (s4).unx), rfx = node_row_uniform(nodes4, no_ + (s4).ufx); \
        const float4 rny = node_row_uniform(nodes4, no_ + (s4).uny), rfy = node_row_uniform(nodes4, no_ + (s4).ufy); \
        const float4 rnz = node_row_uniform(nodes4, no_ + (s4).unz), rfz = node_row_uniform(nodes4, no_ + (s4).ufz); \
        const float4 cc = node_row_uniform(nodes4, no_ + (s4).ucc);
#define RR_NODE4_TESTS(s4, bound)                                                                              \
        const float bound_ = (bound);                                                                          \
        const float inf_ = __builtin_inff();                                                                   \
        RR_ROW(rnx, (s4).o.x, (s4).inv.x, nx01, nx23) RR_ROW(rfx, (s4).o.x, (s4).inv.x, fx01, fx23)            \
        RR_ROW(rny, (s4).o.y, (s4).inv.y, ny01, ny23) RR_ROW(rfy, (s4).o.y, (s4).inv.y, fy01, fy23)            \
        RR_ROW(rnz, (s4).o.z, (s4).inv.z, nz01, nz23) RR_ROW(rfz, (s4).o.z, (s4).inv.z, fz01, fz23)            \
        RR_CHILD(k0, h0, nx01.x, ny01.x, nz01.x, fx01.x, fy01.x, fz01.x)                                       \
        RR_CHILD(k1, h1, nx01.y, ny01.y, nz01.y, fx01.y, fy01.y, fz01.y)                                       \
        RR_CHILD(k2, h2, nx23.x, ny23.x, nz23.x, fx23.x, fy23.x, fz23.x)                                       \
        RR_CHILD(k3, h3, nx23.y, ny23.y, nz23.y, fx23.y, fy23.y, fz23.y) RR_UTIL_ONE
// Two thirds of the node steps of the contract frame have at most ONE child hit in every lane (9.6 % have more than two):
// then nothing is ordered and nothing is pushed.  The test is scalar (the hit flags are lane masks).  Closest-hit walks
// only (-1 % sponza_syn, -3 % lotus_syn): the shadow kernel, at its register limit, loses 3 % to it.
#define RR_NODE4_SINGLE_HIT                                                                                    \
        const bool multi_ = (h0 && (h1 || h2 || h3)) || (h1 && (h2 || h3)) || (h2 && h3);                      \
        if (__ballot(multi_) == 0ull) {                                                                        \
            const int c_ = __float_as_int(h0 ? cc.x : (h1 ? cc.y : (h2 ? cc.z : cc.w)));                       \
            if (h0 || h1 || h2 || h3) cur = c_;                                                                \
            else { sp--; cur = STK(sp); }                                                                      \
        } else
#define RR_NODE4_DESCEND_SORTED_PLAIN                                                                          \
        {                                                                                                      \
        int c0 = __float_as_int(cc.x), c1 = __float_as_int(cc.y), c2 = __float_as_int(cc.z), c3 = __float_as_int(cc.w); \
        RR_CSWAP(k0, c0, k1, c1) RR_CSWAP(k2, c2, k3, c3) RR_CSWAP(k0, c0, k2, c2) RR_CSWAP(k1, c1, k3, c3) RR_CSWAP(k1, c1, k2, c2) \
        STK(sp) = c3; sp += (k3 < inf_) ? 1 : 0;                                                               \
        STK(sp) = c2; sp += (k2 < inf_) ? 1 : 0;                                                               \
        STK(sp) = c1; sp += (k1 < inf_) ? 1 : 0;                                                               \
        if (k0 < inf_) cur = c0;                                                                               \
        else { sp--; cur = STK(sp); }                                                                          \
        }
#define RR_NODE4_DESCEND_SORTED RR_NODE4_SINGLE_HIT RR_NODE4_DESCEND_SORTED_PLAIN
#define RR_NODE4_DESCEND_ANY                                                                                   \
        (void)k0; (void)k1; (void)k2; (void)k3;                                                                \
        STK(sp) = __float_as_int(cc.w); sp += h3 ? 1 : 0;                                                      \
        STK(sp) = __float_as_int(cc.z); sp += h2 ? 1 : 0;                                                      \
        STK(sp) = __float_as_int(cc.y); sp += h1 ? 1 : 0;                                                      \
        if (h0) cur = __float_as_int(cc.x);                                                                    \
        else { sp--; cur = STK(sp); }
// A step whose node is the same in all of its lanes (on a walk that is `uni`) takes the scalar form of the loads.
#define RR_NODE4_FORM(nodes4, s4, bound, DESCEND)                                                              \
    {                                                                                                          \
        const void* nodes4_ptr_ = (nodes4); (void)nodes4_ptr_;                                                 \
        RR_UTIL(RR_UTIL_NODE_SLOT) RR_UTIL_UNI(RR_UTIL_NODE_SLOT, cur, ((s4).nx & 16u) | ((s4).ny & 16u) << 1 | ((s4).nz & 16u) << 2 | ((s4).cc << 3)) \
        const int ucur_ = __builtin_amdgcn_readfirstlane(cur);                                                 \
        if ((s4).uni && __ballot(cur != ucur_) == 0ull) { RR_NODE4_ROWS_UNIFORM(nodes4, s4) RR_NODE4_TESTS(s4, bound) DESCEND } \
        else { RR_NODE4_ROWS_VECTOR(nodes4, s4) RR_NODE4_TESTS(s4, bound) DESCEND }                            \
    }
#define RR_NODE4_STEP(nodes4, s4, bound) RR_NODE4_FORM(nodes4, s4, bound, RR_NODE4_DESCEND_SORTED)
#define RR_NODE4_STEP_PLAIN(nodes4, s4, bound) RR_NODE4_FORM(nodes4, s4, bound, RR_NODE4_DESCEND_SORTED_PLAIN)
// The same step for walks that only ask whether anything is hit (shadow queries inside one mesh): the order in which
// the children are visited does not matter, so the hit children are pushed in slot order and the sort is skipped.
#define RR_NODE4_STEP_ANY(nodes4, s4, bound) RR_NODE4_FORM(nodes4, s4, bound, RR_NODE4_DESCEND_ANY)

// Nearest triangle of one mesh (TriMesh::cast_local_ray_and_get_normal,
// reference src/shape/mesh.rs:67).  Ties at bit-equal toi go to the lowest
// ORIGINAL face index.  `gbound`: hits beyond it cannot win upstream.
// Returns slot (leaf-order triangle index) and side.
struct TriBest { float t; uint32_t slot; uint32_t face; uint32_t side; bool found; };

// Postponed leaves: a lane that reaches a leaf parks it and keeps walking; the wave tests parked
// leaves together once RR_PEND_NUM/RR_PEND_DEN of its unfinished lanes hold one, or nobody can walk on.  The
// order in which triangles are tested is free: the winner is the minimum over (toi, face) and the walk only ever
// prunes with a bound no smaller than the current best.  (Measured before: node steps ran with ~27 of 64 lanes,
// triangle tests with 7-15.)

#define RR_TRI_CLOSEST(tr, slot_)                                                                               \
            {                                                                                                  \
                float t; uint32_t side;                                                                        \
                if (ray_triangle(mk3(tr.t0.x, tr.t0.y, tr.t0.z), mk3(tr.t1.x, tr.t1.y, tr.t1.z),               \
                                 mk3(tr.t1.w, tr.t2.x, tr.t2.y), ray, &t, &side)) {                            \
                    const uint32_t face = __float_as_uint(tr.t0.w);                                            \
                    /* (best starts at (FLT_MAX, face 0xffffffff): the first hit always wins without asking best.found) */ \
                    if (t < best.t || (t == best.t && face < best.face)) {                                     \
                        best.found = true; best.t = t; best.slot = (slot_); best.face = face; best.side = side; \
                    }                                                                                          \
                }                                                                                              \
            }
// A leaf that is the same in every lane of a walk that shares its tree (three quarters of the triangle tests of level 1)
// is fetched through the scalar cache, TWO triangles per wait: the tests of a leaf are a chain of load -> test -> load.
#define RR_TRI_FETCH(t_, o_) t_.t0 = node_row_uniform((const DNode4*)sc.trix, o_); t_.t1 = node_row_uniform((const DNode4*)sc.trix, (o_) + 16u); t_.t2 = node_row_uniform((const DNode4*)sc.trix, (o_) + 32u);
#define RR_LEAF_CLOSEST(leaf)                                                                                  \
    {                                                                                                          \
        const int uleaf_ = __builtin_amdgcn_readfirstlane(leaf);                                               \
        const uint32_t utri_ = (uint32_t)__builtin_amdgcn_readfirstlane((int)tri_base_);                       \
        /* (the triangle base is compared too: meshes small enough to be ONE leaf add no nodes and share a node base) */ \
        if (SCALAR_LEAVES && sr.uni && __ballot((leaf) != uleaf_ || tri_base_ != utri_) == 0ull) {                              \
            const uint32_t ucode = (uint32_t)~uleaf_;                                                          \
            const uint32_t ufirst = RR_LEAF_FIRST(ucode), ucount = RR_LEAF_COUNT(ucode);                       \
            const uint32_t ubase = utri_ + ufirst;                                                             \
            for (uint32_t i = 0; i < ucount; i += 2u) {                                                        \
                RR_UTIL(3)                                                                                     \
                const bool two_ = i + 1u < ucount;                                                             \
                const uint32_t o0 = (ubase + i) * 48u, o1 = (ubase + i + (two_ ? 1u : 0u)) * 48u;              \
                DTriX ta, tb;                                                                                  \
                RR_TRI_FETCH(ta, o0) RR_TRI_FETCH(tb, o1)                                                      \
                RR_TRI_CLOSEST(ta, ufirst + i)                                                                 \
                if (two_) RR_TRI_CLOSEST(tb, ufirst + i + 1u)                                                  \
            }                                                                                                  \
        } else {                                                                                               \
            const uint32_t code = (uint32_t)~(leaf);                                                           \
            const uint32_t first = RR_LEAF_FIRST(code), count = RR_LEAF_COUNT(code);                           \
            for (uint32_t i = 0; i < count; i++) {                                                             \
                RR_UTIL(3) RR_UTIL_UNI(3, tri_base_ + first + i, 0)                                            \
                const DTriX tr = tri_at(sc.trix, (tri_base_ + first + i) * 48u);                               \
                RR_TRI_CLOSEST(tr, first + i)                                                                  \
            }                                                                                                  \
        }                                                                                                      \
    }
#define RR_LEAF_ANY(leaf)                                                                                      \
    {                                                                                                          \
        const uint32_t code = (uint32_t)~(leaf);                                                               \
        const uint32_t first = RR_LEAF_FIRST(code), count = RR_LEAF_COUNT(code);                               \
        for (uint32_t i = 0; i < count; i++) {                                                                 \
            RR_UTIL(3) RR_UTIL_UNI(3, tri_base_ + first + i, 0)                                                \
            const DTriX tr = tri_at(sc.trix, (tri_base_ + first + i) * 48u);                                   \
            float t; uint32_t side;                                                                            \
            if (ray_triangle(mk3(tr.t0.x, tr.t0.y, tr.t0.z), mk3(tr.t1.x, tr.t1.y, tr.t1.z),                   \
                             mk3(tr.t1.w, tr.t2.x, tr.t2.y), ray, &t, &side)) {                                \
                any = true;                                                                                    \
                if (t <= limit) within = true;                                                                 \
            }                                                                                                  \
        }                                                                                                      \
    }

// SCALAR_LEAVES: the closest-hit kernels' form (see RR_LEAF_CLOSEST); the shadow kernel, at its register limit, keeps the plain loop.
// Item (here and below): ItemRec, the register copy of the walks of rr_trace.h, or DItem itself (its rare passes over all items).
template <bool SCALAR_LEAVES, class Item>
RR_DEV void blas_closest(const DSceneView& sc, const Item& it, const LRay& ray, float gbound,
                         int* s_stack, int sp_base, TriBest* out) {
    TriBest best; best.found = false; best.t = RR_FLT_MAX; best.slot = 0; best.face = 0xffffffffu; best.side = 0u;
    const Slab4 sr = make_slab4(make_slab(ray.o, ray.d), it.node_base4);
    const DNode4* nodes = sc.nodes4; // uniform; the tree's base is folded into the node offsets of the Slab4
    const uint32_t tri_base_ = it.tri_base; // triangles, like node rows, are addressed as uniform base + 32-bit offset
    int sp = sp_base;
    STK(sp) = RR_SENTINEL; sp++;
    int cur = it.root4;
    RR_UTIL(4)
    int pend = 0; // parked leaf (leaf codes are negative), 0 = none
    for (;;) {
        if (cur >= 0) {
            RR_NODE4_STEP(nodes, sr, fminf(gbound, best.t))
        } else if (pend == 0 && cur != RR_SENTINEL) {
            pend = cur; sp--; cur = STK(sp);
        }
        const unsigned long long can_walk = __ballot(cur >= 0 || (pend == 0 && cur != RR_SENTINEL));
        const unsigned long long parked = __ballot(pend != 0);
        if ((can_walk | parked) == 0ull) break; // every lane of this walk is done
        const unsigned long long alive = __ballot(cur != RR_SENTINEL || pend != 0);
        if (can_walk == 0ull || __popcll(parked) * RR_PEND_DEN >= __popcll(alive) * RR_PEND_NUM) {
            if (pend != 0) { RR_LEAF_CLOSEST(pend) pend = 0; }
        }
    }
    *out = best;
}

// Shadow query of one mesh: is there ANY hit, and is there one with toi <= limit?
// Stops at the first hit within the limit.
template <class Item>
RR_DEV void blas_any(const DSceneView& sc, const Item& it, const LRay& ray, float limit,
                     int* s_stack, int sp_base, bool* found_any, bool* found_within) {
    bool any = false, within = false;
    const Slab4 sr = make_slab4(make_slab(ray.o, ray.d), it.node_base4);
    const DNode4* nodes = sc.nodes4; // uniform; the tree's base is folded into the node offsets of the Slab4
    const uint32_t tri_base_ = it.tri_base; // triangles, like node rows, are addressed as uniform base + 32-bit offset
    int sp = sp_base;
    STK(sp) = RR_SENTINEL; sp++;
    int cur = it.root4;
    RR_UTIL(4)
    // until some hit is known every box matters; afterwards only boxes that can still hold a hit within the limit
    int pend = 0;
    for (;;) {
        if (cur >= 0) {
            RR_NODE4_STEP_ANY(nodes, sr, any ? limit : RR_FLT_MAX)
        } else if (pend == 0 && cur != RR_SENTINEL) {
            pend = cur; sp--; cur = STK(sp);
        }
        const unsigned long long can_walk = __ballot(cur >= 0 || (pend == 0 && cur != RR_SENTINEL));
        const unsigned long long parked = __ballot(pend != 0);
        if ((can_walk | parked) == 0ull) break;
        const unsigned long long alive = __ballot(cur != RR_SENTINEL || pend != 0);
        if (can_walk == 0ull || __popcll(parked) * RR_PEND_DEN >= __popcll(alive) * RR_PEND_NUM) {
            if (pend != 0) {
                RR_LEAF_ANY(pend)
                pend = 0;
                if (within) cur = RR_SENTINEL; // decided: this lane stops walking
            }
        }
    }
    *found_any = any; *found_within = within;
}

// ---------------------------------------------------------------------------
// The per-mesh walk of a PACKET: all 64 lanes walk ONE mesh with ONE wave-uniform control flow (trace_closest_packet /
// trace_shadow_packet visit a candidate item with every lane together).  A node step costs its instructions per WAVE, not per
// lane, and in a packet of 64 samples of one pixel three quarters of the per-lane steps had the same node in every lane anyway:
// here the node index, the stack (one LDS word per entry, the wave's own column) and the order in which children are tried are
// scalar; each lane still tests the four child boxes with ITS ray and its own bound, and tests a leaf's triangles only if ITS
// box test of that leaf passed -- so a lane's set of tested triangles is what its own walk would test, up to nodes that a bound
// (its best hit so far) prunes, which never changes a result: the frame is the same bit for bit.  What goes away per step is the
// per-lane bookkeeping: the five-exchange sorting network, three LDS pushes with their addresses, the parked-leaf ballots.
// Leaves are tested when their parent is visited (under the lanes' hit flags of that step); only inner nodes are stacked, in
// the order of the FIRST hitting lane's entry distances (any order is correct; near-first prunes best).
// (A bound prunes by the ORDER in which hits are found, and the order here follows the first hitting lane.  That never matters for
// a triangle hit that lies inside its leaf's box; the per-lane walks have the same dependence on their wave through the moment at
// which parked leaves are tested.  Where a reported toi lies in front of the leaf's box -- rounding noise for origins >~ 1e4 mesh
// sizes away, DESIGN.md D12 -- neither form promises the reference's pick.)
// `in`: this lane takes part (its exact test of the item's box passed).  Must be called by all 64 lanes.
// ---------------------------------------------------------------------------
#define RR_PK_STK(sp_) s_stack[(sp_) * RR_BLOCK + wave_col_]
// the triangles of a wave-uniform leaf for the lanes with `hit_`, two per wait through the scalar cache
#define RR_PK_LEAF(code_, hit_, TEST)                                                                          \
    {                                                                                                          \
        const uint32_t ucode = (uint32_t)~(code_);                                                             \
        const uint32_t ufirst = RR_LEAF_FIRST(ucode), ucount = RR_LEAF_COUNT(ucode);                           \
        const uint32_t ubase = utri_ + ufirst;                                                                 \
        for (uint32_t i = 0; i < ucount; i += 2u) {                                                            \
            const bool two_ = i + 1u < ucount;                                                                 \
            const uint32_t o0 = (ubase + i) * 48u, o1 = (ubase + i + (two_ ? 1u : 0u)) * 48u;                  \
            DTriX ta, tb;                                                                                      \
            RR_TRI_FETCH(ta, o0) RR_TRI_FETCH(tb, o1)                                                          \
            if (hit_) { TEST(ta, ufirst + i) if (two_) TEST(tb, ufirst + i + 1u) }                             \
        }                                                                                                      \
    }
// the child test of RR_CHILD with ONE compare (entry <= min(exit, bound): the same predicate; a lane mask less to combine on the
// scalar unit, which the packet walk leans on) and the raw entry distance as the key (only hit children's keys are read)
#define RR_PK_CHILD(k_, h_, nx, ny, nz, fx, fy, fz)                                                            \
        {                                                                                                      \
            const float tn_ = fmaxf(fmaxf(nx, ny), fmaxf(nz, 0.0f));                                           \
            const float tf_ = fminf(fminf(fx, fy), fminf(fz, RR_FLT_MAX));                                     \
            h_ = tn_ * 0.999996f <= fminf(tf_ * 1.000004f, bound_);                                            \
            k_ = tn_;                                                                                          \
        }
// one uniform node: tests (by the lanes that are `in`), leaves, and the choice of the next node.  BOUND: the lane's pruning bound;
// TEST: the triangle macro
#define RR_PK_NODE(BOUND, TEST)                                                                                \
    {                                                                                                          \
        const int ucur_ = cur;                                                                                 \
        RR_NODE4_ROWS_UNIFORM(nodes, sr)                                                                       \
        bool h0 = false, h1 = false, h2 = false, h3 = false;                                                   \
        float k0 = 0.0f, k1 = 0.0f, k2 = 0.0f, k3 = 0.0f;                                                      \
        if (in) {                                                                                              \
            const float bound_ = (BOUND);                                                                      \
            RR_ROW(rnx, sr.o.x, sr.inv.x, nx01, nx23) RR_ROW(rfx, sr.o.x, sr.inv.x, fx01, fx23)                \
            RR_ROW(rny, sr.o.y, sr.inv.y, ny01, ny23) RR_ROW(rfy, sr.o.y, sr.inv.y, fy01, fy23)                \
            RR_ROW(rnz, sr.o.z, sr.inv.z, nz01, nz23) RR_ROW(rfz, sr.o.z, sr.inv.z, fz01, fz23)                \
            RR_PK_CHILD(k0, h0, nx01.x, ny01.x, nz01.x, fx01.x, fy01.x, fz01.x)                                \
            RR_PK_CHILD(k1, h1, nx01.y, ny01.y, nz01.y, fx01.y, fy01.y, fz01.y)                                \
            RR_PK_CHILD(k2, h2, nx23.x, ny23.x, nz23.x, fx23.x, fy23.x, fz23.x)                                \
            RR_PK_CHILD(k3, h3, nx23.y, ny23.y, nz23.y, fx23.y, fy23.y, fz23.y)                                \
        }                                                                                                      \
        const int c0 = __float_as_int(cc.x), c1 = __float_as_int(cc.y), c2 = __float_as_int(cc.z), c3 = __float_as_int(cc.w); \
        const unsigned long long m0 = __ballot(h0), m1 = __ballot(h1), m2 = __ballot(h2), m3 = __ballot(h3);   \
        /* leaves of this node: tested now, by the lanes that hit them */                                      \
        if (m0 != 0ull && c0 < 0) RR_PK_LEAF(c0, h0, TEST)                                                     \
        if (m1 != 0ull && c1 < 0) RR_PK_LEAF(c1, h1, TEST)                                                     \
        if (m2 != 0ull && c2 < 0) RR_PK_LEAF(c2, h2, TEST)                                                     \
        if (m3 != 0ull && c3 < 0) RR_PK_LEAF(c3, h3, TEST)                                                     \
        /* inner children that some lane hits: none or one (most steps) needs no order; otherwise they are keyed by the entry distance */ \
        /* of the first lane that hits them (non-negative floats order as integers) and sorted in scalar registers */ \
        const bool i0 = m0 != 0ull && c0 >= 0, i1 = m1 != 0ull && c1 >= 0, i2 = m2 != 0ull && c2 >= 0, i3 = m3 != 0ull && c3 >= 0; \
        const int n_in = (int)i0 + (int)i1 + (int)i2 + (int)i3;                                                \
        if (n_in == 1) cur = i0 ? c0 : (i1 ? c1 : (i2 ? c2 : c3));                                             \
        else if (n_in > 1) {                                                                                   \
            uint32_t q0 = 0xffffffffu, q1 = 0xffffffffu, q2 = 0xffffffffu, q3 = 0xffffffffu;                   \
            if (i0) q0 = (uint32_t)__builtin_amdgcn_readlane(__float_as_int(k0), __ffsll((long long)m0) - 1);  \
            if (i1) q1 = (uint32_t)__builtin_amdgcn_readlane(__float_as_int(k1), __ffsll((long long)m1) - 1);  \
            if (i2) q2 = (uint32_t)__builtin_amdgcn_readlane(__float_as_int(k2), __ffsll((long long)m2) - 1);  \
            if (i3) q3 = (uint32_t)__builtin_amdgcn_readlane(__float_as_int(k3), __ffsll((long long)m3) - 1);  \
            int e0 = c0, e1 = c1, e2 = c2, e3 = c3;                                                            \
            RR_SCSWAP(q0, e0, q1, e1) RR_SCSWAP(q2, e2, q3, e3) RR_SCSWAP(q0, e0, q2, e2) RR_SCSWAP(q1, e1, q3, e3) RR_SCSWAP(q1, e1, q2, e2) \
            if (q3 != 0xffffffffu) { if (lane_ == 0u) RR_PK_STK(sp) = e3; sp++; }                               \
            if (q2 != 0xffffffffu) { if (lane_ == 0u) RR_PK_STK(sp) = e2; sp++; }                               \
            if (lane_ == 0u) RR_PK_STK(sp) = e1;                                                               \
            sp++;                                                                                              \
            cur = e0;                                                                                          \
        }                                                                                                      \
        else if (sp > sp_base) { sp--; __builtin_amdgcn_wave_barrier(); cur = __builtin_amdgcn_readfirstlane(RR_PK_STK(sp)); } \
        else cur = RR_SENTINEL;                                                                                \
    }
#define RR_SCSWAP(ka, ca, kb, cb) { const bool s_ = kb < ka; const uint32_t tk_ = s_ ? ka : kb; const int tc_ = s_ ? ca : cb; \
                                    ka = s_ ? kb : ka; ca = s_ ? cb : ca; kb = tk_; cb = tc_; }

// returns false (nothing done) when the lanes do not share their direction signs in the mesh's space: the caller walks per lane
template <class Item>
RR_DEV bool blas_closest_packet(const DSceneView& sc, const Item& it, const LRay& ray, bool in, float gbound,
                                int* s_stack, int sp_base, TriBest* out) {
    const Slab4 sr = make_slab4(make_slab(ray.o, ray.d), it.node_base4);
    if (!sr.uni) return false;
    TriBest best; best.found = false; best.t = RR_FLT_MAX; best.slot = 0; best.face = 0xffffffffu; best.side = 0u;
    const DNode4* nodes = sc.nodes4; // uniform; the tree's base is folded into the node offsets of the Slab4
    const uint32_t utri_ = (uint32_t)__builtin_amdgcn_readfirstlane((int)it.tri_base);
    const uint32_t wave_col_ = threadIdx.x & ~(RR_WAVE - 1u), lane_ = threadIdx.x & (RR_WAVE - 1u);
    int sp = sp_base;
    int cur = __builtin_amdgcn_readfirstlane(it.root4);
    if (cur < 0 && cur != RR_SENTINEL) { RR_PK_LEAF(cur, in, RR_TRI_CLOSEST) cur = RR_SENTINEL; } // a mesh of one leaf
    while (cur >= 0) RR_PK_NODE(fminf(gbound, best.t), RR_TRI_CLOSEST)
    *out = best;
    return true;
}

#undef RR_TRI_CLOSEST
#undef RR_TRI_FETCH
#undef RR_LEAF_CLOSEST
#undef RR_LEAF_ANY
#undef RR_PK_STK
#undef RR_PK_LEAF
#undef RR_PK_CHILD
#undef RR_PK_NODE
#undef RR_SCSWAP
