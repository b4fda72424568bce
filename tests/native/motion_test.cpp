// motion_test.cpp — rr_motion_records as a plain host program over rustray_amd/csrc/rr_motion.h: the table builder of the call, then the
// functions the kernel applies per lane as a host loop.  tests/test_motion_host.py compares the output with rustray_amd/temporal.py bit
// for bit.  Built with -ffp-contract=off, once plain and once with -fsanitize=address,undefined.
//
// usage: motion_test IN OUT
// IN : 4 words -- width, height, n_items, n_moved -- then projection_inverse[16], view_inverse[16] (column-major floats), n_items words of
//      object ids, n_items * 16 floats of trans_inv (column-major), n_moved words of item indices, n_moved * 16 floats of prev_trans
//      (column-major), width*height records of 8 floats.
// OUT: n_moved * 28 words of the table, width*height*3 floats of motion, width*height*3 floats of world.
// A list the builder refuses: exit status 3 and "refused: <message>" on stdout, no OUT.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../rustray_amd/csrc/rr_motion.h"

static bool read_all(FILE* f, void* p, size_t bytes) { return bytes == 0 || fread(p, 1, bytes, f) == bytes; }

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: motion_test IN OUT\n"); return 2; }
    FILE* fi = fopen(argv[1], "rb");
    if (!fi) { perror(argv[1]); return 2; }
    uint32_t head[4];
    float cam[32];
    if (!read_all(fi, head, sizeof head) || !read_all(fi, cam, sizeof cam)) { fprintf(stderr, "short header\n"); return 2; }
    const int W = (int)head[0], H = (int)head[1];
    const uint32_t n_items = head[2], n_moved = head[3];
    if (W <= 0 || H <= 0 || W > 4096 || H > 4096 || n_items > 65536 || n_moved > 65536) { fprintf(stderr, "bad header\n"); return 2; }
    const size_t N = (size_t)W * H;
    std::vector<uint32_t> ids(n_items), item_index(n_moved);
    std::vector<float> inv(16 * (size_t)n_items), prev(16 * (size_t)n_moved), records(8 * N);
    if (!read_all(fi, ids.data(), 4 * ids.size()) || !read_all(fi, inv.data(), 4 * inv.size()) || !read_all(fi, item_index.data(), 4 * item_index.size()) ||
        !read_all(fi, prev.data(), 4 * prev.size()) || !read_all(fi, records.data(), 4 * records.size())) { fprintf(stderr, "short input\n"); return 2; }
    fclose(fi);

    std::vector<MoEntry> table;
    char msg[256];
    const bool ok = motion_build_table([&](unsigned int i, float* rows, unsigned int* id) {
        for (int r = 0; r < 3; r++)
            for (int c = 0; c < 4; c++) rows[4 * r + c] = inv[16 * (size_t)i + 4 * c + r];
        *id = ids[i];
    }, n_items, item_index.data(), prev.data(), n_moved, &table, msg, sizeof msg);
    if (!ok) { printf("refused: %s\n", msg); return 3; }

    TpFrame f{};
    memcpy(f.proj_inv, cam, 64);
    memcpy(f.view_inv, cam + 16, 64);
    f.w = (float)W; f.h = (float)H; f.width = W; f.height = H;
    std::vector<float> motion(3 * N), world(3 * N);
    for (int y = 0; y < H; y++)
        for (int x = 0; x < W; x++) {
            const size_t o = (size_t)y * W + x;
            const float* r = records.data() + 8 * o;
            unsigned int id;
            memcpy(&id, r + 7, 4);
            motion_pixel(f, (unsigned int)x, (unsigned int)y, r[3], r + 4, id, table.data(), n_moved, world.data() + 3 * o, motion.data() + 3 * o);
        }

    FILE* fo = fopen(argv[2], "wb");
    if (!fo) { perror(argv[2]); return 2; }
    if (n_moved && fwrite(table.data(), sizeof(MoEntry), n_moved, fo) != n_moved) { fprintf(stderr, "short write\n"); return 2; }
    if (fwrite(motion.data(), 4, motion.size(), fo) != motion.size() || fwrite(world.data(), 4, world.size(), fo) != world.size()) { fprintf(stderr, "short write\n"); return 2; }
    fclose(fo);
    printf("motion test OK\n");
    return 0;
}
