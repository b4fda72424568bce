// query_pointer_test.cpp — rustray_amd/csrc/rr_query_pointers.h on the CPU (tests/test_query_pointers.py builds it with
// -fsanitize=address,undefined): the whole decision table of query_pointer_ok -- every memory kind x own / other device x peer
// access enabled or not -- against the rule written out here a second time, plus the cases the device-buffer ray queries
// (rr_trace_rays_device, rr_trace_shadow_rays_device, rr_shade_rays_device) rely on by name.
#include "../../rustray_amd/csrc/rr_query_pointers.h"

#include <cstdio>
#include <cstring>

static int failures = 0;
#define CHECK(cond)                                                            \
    do {                                                                       \
        if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); failures++; } \
    } while (0)

// the rule, stated independently: host-visible-everywhere kinds pass, device memory passes on its own device or over an enabled
// peer link, everything else -- memory the runtime never saw, arrays, kinds this library does not know -- does not
static bool expected(int kind, int owner, int scene, bool peer) {
    if (kind == RR_QMEM_HOST || kind == RR_QMEM_MANAGED) return true;
    if (kind == RR_QMEM_DEVICE) return owner >= 0 && scene >= 0 && (owner == scene || peer);
    return false;
}

int main() {
    // the whole table, with kinds beyond the enum on both sides
    int n = 0, n_ok = 0;
    for (int kind = -2; kind <= RR_QMEM_KINDS + 2; kind++)
        for (int owner = -1; owner < 9; owner++)
            for (int scene = -1; scene < 9; scene++)
                for (int peer = 0; peer < 2; peer++) {
                    const bool got = query_pointer_ok((QueryMemKind)kind, owner, scene, peer != 0);
                    CHECK(got == expected(kind, owner, scene, peer != 0));
                    n++; n_ok += got ? 1 : 0;
                }
    CHECK(n == 10 * 10 * 10 * 2 && n_ok > 0 && n_ok < n);
    // by name: what must never reach a launch ...
    CHECK(!query_pointer_ok(RR_QMEM_UNREGISTERED, -1, 0, false));   // a numpy array, malloc
    CHECK(!query_pointer_ok(RR_QMEM_UNREGISTERED, 0, 0, true));     // ... whatever else the attributes claim
    CHECK(!query_pointer_ok(RR_QMEM_DEVICE, 1, 0, false));          // another device's memory, no peer access
    CHECK(!query_pointer_ok(RR_QMEM_DEVICE, 0, 1, false));
    CHECK(!query_pointer_ok(RR_QMEM_DEVICE, -1, 0, true));          // device memory without an owner
    CHECK(!query_pointer_ok(RR_QMEM_ARRAY, 0, 0, true));            // not a linear buffer
    // ... and what may
    CHECK(query_pointer_ok(RR_QMEM_DEVICE, 0, 0, false));           // the scene's own device, peer state irrelevant
    CHECK(query_pointer_ok(RR_QMEM_DEVICE, 3, 3, false));
    CHECK(query_pointer_ok(RR_QMEM_DEVICE, 1, 0, true));            // another device's memory over an enabled link
    CHECK(query_pointer_ok(RR_QMEM_HOST, -1, 0, false));            // pinned host memory: mapped into every device
    CHECK(query_pointer_ok(RR_QMEM_HOST, 5, 2, false));
    CHECK(query_pointer_ok(RR_QMEM_MANAGED, 1, 0, false));
    // peer access is directional state of (scene device -> owner): the function takes it as given and never widens it
    for (int kind = 0; kind < RR_QMEM_KINDS; kind++)
        if (kind != RR_QMEM_DEVICE)
            CHECK(query_pointer_ok((QueryMemKind)kind, 1, 0, true) == query_pointer_ok((QueryMemKind)kind, 1, 0, false));
    // every kind has a name for the message, distinct from the others
    for (int a = 0; a < RR_QMEM_KINDS; a++) {
        CHECK(query_mem_kind_name((QueryMemKind)a) && std::strlen(query_mem_kind_name((QueryMemKind)a)) > 0);
        for (int b = a + 1; b <= RR_QMEM_KINDS; b++) CHECK(std::strcmp(query_mem_kind_name((QueryMemKind)a), query_mem_kind_name((QueryMemKind)b)) != 0);
    }
    if (failures) { std::printf("%d check(s) failed\n", failures); return 1; }
    std::printf("query pointer test OK (%d combinations, %d accepted)\n", n, n_ok);
    return 0;
}
