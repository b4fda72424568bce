// Host-only test of the size of DSceneView::flat_normals (rr_scene_build.h: flat_normals_bytes): three float4 per entry -- normal,
// tangent, bitangent --, two entries per instanced triangle, an empty table still one float4; and no 32-bit wrap at the entry limit.
// build: g++ -std=c++17 -O1 -g -Wall -Wno-unused-function -ffp-contract=off -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include tests/native/flat_table_size_test.cpp rustray_amd/csrc/rr_bvh.cpp -pthread
#include <cstdarg>
#include <cstdio>

#include "../../rustray_amd/csrc/rr_scene_build.h"

static int fail(int code, const char* fmt, ...) noexcept { // (what rr_scene_build.h expects of whoever includes it)
    va_list ap;
    va_start(ap, fmt);
    std::vfprintf(stderr, fmt, ap);
    va_end(ap);
    std::fputc('\n', stderr);
    return code;
}

static int failures = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); failures++; } } while (0)

int main() {
    static_assert(RR_FLAT_ENTRY_F4 == 3u, "normal, tangent, bitangent");
    CHECK(sizeof(float4) == 16);
    CHECK(flat_normals_bytes(0) == 16);                                   // an empty table still gets a buffer
    CHECK(flat_normals_bytes(1) == 48 && flat_normals_bytes(2) == 96);     // 96 B per instanced triangle (both signs)
    CHECK(flat_normals_bytes(2ull * 559376ull) == 96ull * 559376ull);
    CHECK(flat_normals_bytes(0xffffffffull) == 48ull * 0xffffffffull);    // the entry limit of build_item_records: beyond 2^32 bytes, no wrap
    CHECK(flat_normals_bytes(1ull << 32) == 48ull << 32);
    // the last float4 of the last entry lies inside the buffer for every count
    for (uint64_t n : {1ull, 2ull, 3ull, 16384ull, 16385ull, 0x7fffffffull, 0xffffffffull})
        CHECK((n - 1) * RR_FLAT_ENTRY_F4 * 16 + 2 * 16 + 16 <= flat_normals_bytes(n));
    std::printf("flat table sizes: %d failures\n", failures);
    return failures ? 1 : 0;
}
