// denoise_test.cpp — the a-trous filter of rr_denoise_records as a plain host loop over rustray_amd/csrc/rr_denoise.h, the functions the
// kernels apply per lane.  Reads a raw frame, filters it, writes the result; tests/test_denoise_host.py compares the output with
// rustray_amd/denoise.py bit for bit.  Built with -ffp-contract=off -fsanitize=address,undefined.
//
// usage: denoise_test IN OUT
// IN : 8 words -- width, height, has_halves, has_albedo, iterations, normal_power_log2, sigma_depth (float), sigma_luminance (float) --
//      then width*height records of 8 floats, then (has_halves) width*height*2 records, then (has_albedo) width*height*3 floats.
// OUT: width*height records of 8 floats, then width*height floats of variance.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../rustray_amd/csrc/rr_denoise.h"

static bool read_all(FILE* f, void* p, size_t bytes) { return bytes == 0 || fread(p, 1, bytes, f) == bytes; }

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: denoise_test IN OUT\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    uint32_t head[8];
    if (!read_all(f, head, sizeof head)) { fprintf(stderr, "short header\n"); return 2; }
    const int W = (int)head[0], H = (int)head[1];
    const bool has_halves = head[2] != 0, has_albedo = head[3] != 0;
    const uint32_t iterations = head[4];
    DnPass pass{};
    pass.normal_power_log2 = head[5];
    memcpy(&pass.sigma_depth, &head[6], 4);
    memcpy(&pass.sigma_luminance, &head[7], 4);
    pass.halves = has_halves ? 1u : 0u;
    if (W <= 0 || H <= 0 || W > 4096 || H > 4096 || iterations == 0 || iterations > 6) { fprintf(stderr, "bad header\n"); return 2; }
    const size_t N = (size_t)W * H;
    std::vector<float> records(8 * N), halves(has_halves ? 16 * N : 0), albedo(has_albedo ? 3 * N : 0);
    if (!read_all(f, records.data(), 4 * records.size()) || !read_all(f, halves.data(), 4 * halves.size()) || !read_all(f, albedo.data(), 4 * albedo.size())) {
        fprintf(stderr, "short input\n");
        return 2;
    }
    fclose(f);

    // ---- prepare: flags, guide, demodulated colour, variance seeds and their prefilter
    std::vector<DnTap> cur(N), next(N);
    std::vector<float> seed(N, 0.0f);
    for (size_t o = 0; o < N; o++) {
        const float* r = &records[8 * o];
        DnTap& t = cur[o];
        t.flags = denoise_flags(r, r[3], r + 4);
        for (int k = 0; k < 3; k++) {
            t.c[k] = (t.flags & DN_FIN) && has_albedo ? denoise_demodulate(r[k], albedo[3 * o + k]) : r[k];
            t.n[k] = r[4 + k];
        }
        t.z = r[3];
        memcpy(&t.id, &r[7], 4);
        t.var = 0.0f;
        if (has_halves) seed[o] = denoise_variance_seed((t.flags & DN_FIN) != 0, &halves[16 * o], &halves[16 * o + 8], has_albedo ? &albedo[3 * o] : nullptr);
    }
    if (has_halves)
        for (int y = 0; y < H; y++)
            for (int x = 0; x < W; x++) {
                DnTap& t = cur[(size_t)y * W + x];
                if (!(t.flags & DN_FIN)) continue;
                t.var = denoise_prefilter([&](int dx, int dy, float* v) {
                    const int qx = x + dx, qy = y + dy;
                    if (qx < 0 || qy < 0 || qx >= W || qy >= H || !(cur[(size_t)qy * W + qx].flags & DN_FIN)) return false;
                    *v = seed[(size_t)qy * W + qx];
                    return true;
                });
            }

    // ---- the passes
    for (uint32_t i = 0; i < iterations; i++) {
        pass.step = 1 << i;
        for (int y = 0; y < H; y++)
            for (int x = 0; x < W; x++) {
                const size_t o = (size_t)y * W + x;
                next[o] = cur[o];
                if (!(cur[o].flags & DN_FIN)) continue;
                denoise_pixel_pass(pass, cur[o], [&](int dx, int dy, DnTap* q) {
                    const int qx = x + dx * pass.step, qy = y + dy * pass.step;
                    if (qx < 0 || qy < 0 || qx >= W || qy >= H) return false;
                    *q = cur[(size_t)qy * W + qx];
                    return true;
                }, next[o].c, &next[o].var);
            }
        cur.swap(next);
    }

    // ---- finish
    std::vector<float> out(records), variance(N);
    for (size_t o = 0; o < N; o++) {
        if (cur[o].flags & DN_FIN)
            for (int k = 0; k < 3; k++) out[8 * o + k] = has_albedo ? denoise_remodulate(cur[o].c[k], albedo[3 * o + k]) : cur[o].c[k];
        variance[o] = cur[o].var;
    }
    f = fopen(argv[2], "wb");
    if (!f) { perror(argv[2]); return 2; }
    if (fwrite(out.data(), 4, out.size(), f) != out.size() || fwrite(variance.data(), 4, variance.size(), f) != variance.size()) { fprintf(stderr, "short write\n"); return 2; }
    fclose(f);
    printf("denoise test OK\n");
    return 0;
}
