// temporal_pixel_test.cpp — rr_accumulate_records, rr_accumulate_split_records, rr_accumulate_clamped_records and
// rr_accumulate_clamped_split_records as a plain host loop over rustray_amd/csrc/rr_history_clamp.h: temporal_pixel, THE step the kernels
// apply per lane (flags, temporal_history, the clamp, the blends, the length).  Reads a raw frame and its history, accumulates, writes the
// result; tests/test_temporal_host.py, test_temporal_split_host.py, test_temporal_clamp_host.py and test_temporal_clamp_split_host.py
// compare the output with rustray_amd/temporal.py bit for bit (tests/temporal_host_loop.py builds and feeds it).  Built with
// -ffp-contract=off -fsanitize=address,undefined.
//
// usage: temporal_pixel_test IN OUT
// IN : 7 words -- width, height, has_halves, has_history, has_motion, split, radius (0: no clamp) -- then 56 floats --
//      projection_inverse[16], view_inverse[16], prev_world_to_clip[16] (all column-major), prev_eye[3], max_history, normal_min,
//      sigma_depth, snap, sigma_scale -- then, n = width*height: 8n floats of records, (has_halves) 16n of halves, (split) 3n of diffuse,
//      (split and has_halves) 6n of diffuse halves, (has_history) 8n of history, (has_history and has_halves) 16n of its halves,
//      (has_history and split) 3n of its diffuse, (has_history, has_halves and split) 6n of its diffuse halves, (has_history) n of length,
//      (has_motion) 3n of motion.
// OUT: 8n floats of records, n of length, (has_halves) 16n of halves, (split) 3n of diffuse, (split and has_halves) 6n of diffuse halves,
//      (radius) 3n of lo and 3n of hi of the colour box (of every pixel whose colour is finite; 0 elsewhere), (radius and split) 3n of lo
//      and 3n of hi of the diffuse box (of every pixel).
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../rustray_amd/csrc/rr_history_clamp.h"

static bool read_all(FILE* f, void* p, size_t bytes) { return bytes == 0 || fread(p, 1, bytes, f) == bytes; }

struct HostHistory {
    const float* history;
    const float* history_halves;
    const float* history_length;
    const float* history_diffuse;
    const float* history_dif_halves;
    float length(unsigned long long q) const { return history_length[q]; }
    void guide(unsigned long long q, float* n, unsigned int* id) const {
        memcpy(n, history + 8 * q + 4, 12);
        memcpy(id, history + 8 * q + 7, 4);
    }
    void colour(unsigned long long q, float* c, float* z) const {
        memcpy(c, history + 8 * q, 12);
        *z = history[8 * q + 3];
    }
    void half(unsigned long long q, int h, float* c) const { memcpy(c, history_halves + 16 * q + 8 * h, 12); }
    void diffuse(unsigned long long q, float* c) const { memcpy(c, history_diffuse + 3 * q, 12); }
    void diffuse_half(unsigned long long q, int h, float* c) const { memcpy(c, history_dif_halves + 3 * (2 * q + h), 12); }
};

struct Layers {
    const float* records; const float* halves; const float* diffuse; const float* dif_halves;
    float* out; float* halves_out; float* diffuse_out; float* dif_halves_out; float* length_out;
    float* lo; float* hi; float* dlo; float* dhi;
};

template <bool HALVES, bool SPLIT, bool CLAMPED>
static void run(const TpFrame& f, int radius, float sigma_scale, const Layers& io, bool has_history, const HostHistory& hist, const float* motion) {
    for (int y = 0; y < f.height; y++)
        for (int x = 0; x < f.width; x++) {
            const size_t o = (size_t)y * f.width + x;
            // the windows of the current frame around (x, y): inside the frame, three finite floats of the layer itself
            auto window = [&](int dx, int dy, float* c) {
                const int qx = x + dx, qy = y + dy;
                if (qx < 0 || qy < 0 || qx >= f.width || qy >= f.height) return false;
                memcpy(c, io.records + 8 * ((size_t)qy * f.width + qx), 12);
                return temporal_colour_ok(c);
            };
            auto diffuse_window = [&](int dx, int dy, float* c) {
                const int qx = x + dx, qy = y + dy;
                if (qx < 0 || qy < 0 || qx >= f.width || qy >= f.height) return false;
                memcpy(c, io.diffuse + 3 * ((size_t)qy * f.width + qx), 12);
                return temporal_colour_ok(c);
            };
            TpPixel p;
            memcpy(&p, io.records + 8 * o, 32); // c, depth, n and the id's bits: the record's eight words
            if (HALVES) { memcpy(p.a, io.halves + 16 * o, 12); memcpy(p.b, io.halves + 16 * o + 8, 12); }
            if (SPLIT) memcpy(p.d, io.diffuse + 3 * o, 12);
            if (SPLIT && HALVES) { memcpy(p.da, io.dif_halves + 6 * o, 12); memcpy(p.db, io.dif_halves + 6 * o + 3, 12); }
            if (CLAMPED) { // (the boxes as outputs of their own, for the yardstick's `box` and `diffuse_box`)
                if (temporal_colour_ok(p.c)) {
                    const HcBox b = history_clamp_box(history_clamp_sums(radius, window), sigma_scale);
                    memcpy(io.lo + 3 * o, b.lo, 12);
                    memcpy(io.hi + 3 * o, b.hi, 12);
                }
                if (SPLIT) {
                    const HcBox bd = history_clamp_box(history_clamp_sums(radius, diffuse_window), sigma_scale);
                    memcpy(io.dlo + 3 * o, bd.lo, 12);
                    memcpy(io.dhi + 3 * o, bd.hi, 12);
                }
            }
            temporal_pixel<HALVES, SPLIT, CLAMPED>(f, (unsigned int)x, (unsigned int)y, motion ? motion + 3 * o : nullptr, has_history, hist, radius, sigma_scale, window,
                                                   diffuse_window, &p);
            memcpy(io.out + 8 * o, io.records + 8 * o, 32);
            memcpy(io.out + 8 * o, p.c, 12);
            io.length_out[o] = p.length;
            if (HALVES) {
                memcpy(io.halves_out + 16 * o, io.halves + 16 * o, 64);
                memcpy(io.halves_out + 16 * o, p.a, 12);
                memcpy(io.halves_out + 16 * o + 8, p.b, 12);
            }
            if (SPLIT) memcpy(io.diffuse_out + 3 * o, p.d, 12);
            if (SPLIT && HALVES) { memcpy(io.dif_halves_out + 6 * o, p.da, 12); memcpy(io.dif_halves_out + 6 * o + 3, p.db, 12); }
        }
}

template <bool HALVES, bool SPLIT>
static void run_clamped_or_not(const TpFrame& f, int radius, float sigma_scale, const Layers& io, bool has_history, const HostHistory& hist, const float* motion) {
    if (radius) run<HALVES, SPLIT, true>(f, radius, sigma_scale, io, has_history, hist, motion);
    else run<HALVES, SPLIT, false>(f, radius, sigma_scale, io, has_history, hist, motion);
}

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: temporal_pixel_test IN OUT\n"); return 2; }
    FILE* fi = fopen(argv[1], "rb");
    if (!fi) { perror(argv[1]); return 2; }
    uint32_t head[7];
    float par[56];
    if (!read_all(fi, head, sizeof head) || !read_all(fi, par, sizeof par)) { fprintf(stderr, "short header\n"); return 2; }
    const int W = (int)head[0], H = (int)head[1], radius = (int)head[6];
    const bool has_halves = head[2] != 0, has_history = head[3] != 0, has_motion = head[4] != 0, split = head[5] != 0;
    if (W <= 0 || H <= 0 || W > 4096 || H > 4096 || radius < 0 || radius > 2) { fprintf(stderr, "bad header\n"); return 2; }
    TpFrame f{};
    memcpy(f.proj_inv, par, 64);
    memcpy(f.view_inv, par + 16, 64);
    memcpy(f.prev_clip, par + 32, 64);
    memcpy(f.prev_eye, par + 48, 12);
    f.max_history = par[51]; f.normal_min = par[52]; f.sigma_depth = par[53]; f.snap = par[54];
    const float sigma_scale = par[55];
    f.w = (float)W; f.h = (float)H; f.width = W; f.height = H;
    const size_t N = (size_t)W * H, S = split ? N : 0, B = radius ? N : 0;
    const bool hh = has_history && has_halves;
    std::vector<float> records(8 * N), halves(has_halves ? 16 * N : 0), diffuse(3 * S), dif_halves(has_halves ? 6 * S : 0), history(has_history ? 8 * N : 0),
        history_halves(hh ? 16 * N : 0), history_diffuse(has_history ? 3 * S : 0), history_dif_halves(hh ? 6 * S : 0), history_length(has_history ? N : 0),
        motion(has_motion ? 3 * N : 0);
    for (std::vector<float>* v : {&records, &halves, &diffuse, &dif_halves, &history, &history_halves, &history_diffuse, &history_dif_halves, &history_length, &motion})
        if (!read_all(fi, v->data(), 4 * v->size())) { fprintf(stderr, "short input\n"); return 2; }
    fclose(fi);

    std::vector<float> out(8 * N), halves_out(has_halves ? 16 * N : 0), diffuse_out(3 * S), dif_halves_out(has_halves ? 6 * S : 0), length_out(N), lo(3 * B), hi(3 * B),
        dlo(split ? 3 * B : 0), dhi(split ? 3 * B : 0);
    const HostHistory hist{history.data(), history_halves.data(), history_length.data(), history_diffuse.data(), history_dif_halves.data()};
    const Layers io{records.data(), halves.data(), diffuse.data(), dif_halves.data(), out.data(), halves_out.data(), diffuse_out.data(), dif_halves_out.data(),
                    length_out.data(), lo.data(), hi.data(), dlo.data(), dhi.data()};
    const float* mv = has_motion ? motion.data() : nullptr;
    if (has_halves && split) run_clamped_or_not<true, true>(f, radius, sigma_scale, io, has_history, hist, mv);
    else if (has_halves) run_clamped_or_not<true, false>(f, radius, sigma_scale, io, has_history, hist, mv);
    else if (split) run_clamped_or_not<false, true>(f, radius, sigma_scale, io, has_history, hist, mv);
    else run_clamped_or_not<false, false>(f, radius, sigma_scale, io, has_history, hist, mv);

    FILE* fo = fopen(argv[2], "wb");
    if (!fo) { perror(argv[2]); return 2; }
    for (std::vector<float>* v : {&out, &length_out, &halves_out, &diffuse_out, &dif_halves_out, &lo, &hi, &dlo, &dhi})
        if (v->size() && fwrite(v->data(), 4, v->size(), fo) != v->size()) { fprintf(stderr, "short write\n"); return 2; }
    fclose(fo);
    printf("temporal pixel test OK\n");
    return 0;
}
