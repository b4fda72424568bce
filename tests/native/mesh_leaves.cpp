// Leaf membership of a per-mesh tree (tests/test_aimed_rays.py): reads "n" and n lines "lo.x lo.y lo.z hi.x hi.y hi.z" (the triangles'
// boxes, as build_mesh_trees of rr_scene_build.h forms them) from stdin, builds and collapses the tree as append_mesh_records does
// (rr::build_bvh with RR_MAX_LEAF_TRIS, rr::collapse_bvh4 greedy, RR_BLAS_MAX_DEPTH levels) and prints one line per leaf of the BVH4:
// "leaf <parent node or -1> <count> <original face ids ...>", then "nodes <n>".
#include "../../rustray_amd/csrc/rr_bvh.h"

#include <cstdio>
#include <cstring>

static const int32_t SENTINEL = (int32_t)0x80000000;

static void walk(const std::vector<DNode4>& n4, const rr::BvhResult& r, int32_t code, int32_t parent) {
    if (code == SENTINEL) return;
    if (code < 0) {
        const uint32_t c = (uint32_t)~code, first = RR_LEAF_FIRST(c), count = RR_LEAF_COUNT(c);
        std::printf("leaf %d %u", parent, count);
        for (uint32_t i = 0; i < count; i++) std::printf(" %u", r.order[first + i]);
        std::printf("\n");
        return;
    }
    for (int k = 0; k < 4; k++) {
        const float v[4] = {n4[code].q[6].x, n4[code].q[6].y, n4[code].q[6].z, n4[code].q[6].w};
        int32_t c; std::memcpy(&c, &v[k], 4);
        walk(n4, r, c, code);
    }
}

int main() {
    unsigned n = 0;
    if (std::scanf("%u", &n) != 1) return 2;
    std::vector<float> lo(3 * (size_t)n), hi(3 * (size_t)n);
    for (unsigned i = 0; i < n; i++)
        if (std::scanf("%f %f %f %f %f %f", &lo[3 * i], &lo[3 * i + 1], &lo[3 * i + 2], &hi[3 * i], &hi[3 * i + 1], &hi[3 * i + 2]) != 6) return 2;
    rr::BvhResult r;
    if (!rr::build_bvh(lo.data(), hi.data(), n, RR_MAX_LEAF_TRIS, RR_BLAS_MAX_DEPTH, &r)) return 3;
    std::vector<DNode4> n4; int pending = 0;
    const int32_t root4 = rr::collapse_bvh4(r, RR_BLAS_MAX_DEPTH, true, &n4, &pending);
    walk(n4, r, root4, -1);
    std::printf("nodes %zu\n", n4.size());
    return 0;
}
