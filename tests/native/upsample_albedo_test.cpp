// upsample_albedo_test.cpp — the joint-bilateral upsampler of rr_upsample_albedo_records as a plain host loop over
// rustray_amd/csrc/rr_upsample.h, the functions the kernel applies per lane, with the guides loaded the way the kernel's planes build
// loads them: rows 0, 1 and 2 of the surface record, and the albedo from the caller's plane where there is one (three floats at a stride
// of 12 bytes, from a buffer of exactly that size), from row 4 where there is none.  Reads a low frame, the two guides and the planes,
// raises the frame, writes the result; tests/test_upsample_planes_host.py compares the output with rustray_amd/upsample.py bit for bit.
// Built with -ffp-contract=off -fsanitize=address,undefined.
//
// usage: upsample_albedo_test IN OUT
// IN : 10 words -- low_width, low_height, width, height, has_halves, normal_power_log2, use_albedo, sigma_depth (float), has_albedo_low,
//      has_albedo -- then low_width*low_height records of 8 floats, then (has_halves) twice as many, then low_width*low_height surface
//      records of 32 words, then width*height surface records, then (has_albedo_low) low_width*low_height*3 floats, then (has_albedo)
//      width*height*3 floats.
// OUT: width*height records of 8 floats, then (has_halves) width*height*2 records, then width*height floats of weight.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../rustray_amd/csrc/rr_upsample.h"

static bool read_all(FILE* f, void* p, size_t bytes) { return bytes == 0 || fread(p, 1, bytes, f) == bytes; }

// rows 0, 1 and 2 of surface record o, and the albedo in use: pixel o of `plane`, or row 4 where the call has no plane
static UpGuide guide_of(const std::vector<uint32_t>& g, size_t o, const float* plane) {
    const uint32_t* r = &g[32 * o];
    float distance, normal[3], base[3];
    memcpy(&distance, r + 7, 4);
    memcpy(normal, r + 8, 12);
    if (plane) {
        for (int k = 0; k < 3; k++) base[k] = plane[3 * o + k];
    } else {
        memcpy(base, r + 16, 12);
    }
    return upsample_guide(r[0], r[2], distance, normal, base);
}

template <bool HALVES>
static void run(int w, int h, int W, int H, const UpCall& call, const std::vector<float>& low, const std::vector<float>& halves, const std::vector<uint32_t>& guide_low,
                const std::vector<uint32_t>& guide, const float* albedo_low, const float* albedo, std::vector<float>& out, std::vector<float>& halves_out, std::vector<float>& weight) {
    for (int y = 0; y < H; y++)
        for (int x = 0; x < W; x++) {
            const size_t o = (size_t)y * W + x;
            const UpGuide p = guide_of(guide, o, albedo);
            int x0, y0;
            float fx, fy;
            upsample_position(x, (unsigned)w, (unsigned)W, &x0, &fx);
            upsample_position(y, (unsigned)h, (unsigned)H, &y0, &fy);
            UpResult res;
            upsample_pixel<HALVES>(call, x0, fx, y0, fy, p, [&](int qx, int qy, UpTap* q) {
                if (qx < 0 || qy < 0 || qx >= w || qy >= h) return false;
                const size_t oq = (size_t)qy * w + qx;
                for (int k = 0; k < 3; k++) {
                    q->c[k] = low[8 * oq + k];
                    for (int s = 0; s < 2; s++) q->h[s][k] = HALVES ? halves[16 * oq + 8 * s + k] : 0.0f;
                }
                q->fin = upsample_fin(q->c);
                q->g = guide_of(guide_low, oq, albedo_low);
                return true;
            }, &res);
            unsigned int words[5]; // depth, normal, id
            upsample_guide_fields(p, &words[0], &words[1], &words[4]);
            memcpy(&out[8 * o], res.c, 12);
            memcpy(&out[8 * o + 3], words, 20);
            if (HALVES)
                for (int s = 0; s < 2; s++) {
                    memcpy(&halves_out[16 * o + 8 * s], res.h[s], 12);
                    memcpy(&halves_out[16 * o + 8 * s + 3], words, 20);
                }
            weight[o] = res.weight;
        }
}

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: upsample_albedo_test IN OUT\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    uint32_t head[10];
    if (!read_all(f, head, sizeof head)) { fprintf(stderr, "short header\n"); return 2; }
    const int w = (int)head[0], h = (int)head[1], W = (int)head[2], H = (int)head[3];
    const bool has_halves = head[4] != 0;
    UpCall call{};
    call.normal_power_log2 = head[5];
    call.use_albedo = head[6];
    memcpy(&call.sigma_depth, &head[7], 4);
    if (w <= 0 || h <= 0 || w > W || h > H || W > 4096 || H > 4096 || call.normal_power_log2 > 7) { fprintf(stderr, "bad header\n"); return 2; }
    call.r = upsample_ratio((unsigned)W, (unsigned)H, (unsigned)w, (unsigned)h);
    const size_t nl = (size_t)w * h, N = (size_t)W * H;
    std::vector<float> low(8 * nl), halves(has_halves ? 16 * nl : 0);
    std::vector<uint32_t> guide_low(32 * nl), guide(32 * N);
    std::vector<float> plane_low(head[8] ? 3 * nl : 0), plane(head[9] ? 3 * N : 0);
    if (!read_all(f, low.data(), 4 * low.size()) || !read_all(f, halves.data(), 4 * halves.size()) || !read_all(f, guide_low.data(), 4 * guide_low.size()) ||
        !read_all(f, guide.data(), 4 * guide.size()) || !read_all(f, plane_low.data(), 4 * plane_low.size()) || !read_all(f, plane.data(), 4 * plane.size())) {
        fprintf(stderr, "short input\n");
        return 2;
    }
    fclose(f);
    std::vector<float> out(8 * N), halves_out(has_halves ? 16 * N : 0), weight(N);
    // (with use_albedo off the planes are not read: the entry points drop them before the launch)
    const float* albedo_low = head[8] && call.use_albedo ? plane_low.data() : nullptr;
    const float* albedo = head[9] && call.use_albedo ? plane.data() : nullptr;
    if (has_halves) run<true>(w, h, W, H, call, low, halves, guide_low, guide, albedo_low, albedo, out, halves_out, weight);
    else run<false>(w, h, W, H, call, low, halves, guide_low, guide, albedo_low, albedo, out, halves_out, weight);
    f = fopen(argv[2], "wb");
    if (!f) { perror(argv[2]); return 2; }
    const auto write_all = [&](const std::vector<float>& v) { return v.empty() || fwrite(v.data(), 4, v.size(), f) == v.size(); };
    if (!write_all(out) || !write_all(halves_out) || !write_all(weight)) {
        fprintf(stderr, "short write\n");
        return 2;
    }
    fclose(f);
    printf("upsample albedo test OK\n");
    return 0;
}
