// temporal_test.cpp — the temporal reprojection of rr_accumulate_records as a plain host loop over rustray_amd/csrc/rr_temporal.h, the
// functions the kernel applies per lane.  Reads a raw frame and its history, accumulates, writes the result; tests/test_temporal_host.py
// compares the output with rustray_amd/temporal.py bit for bit.  Built with -ffp-contract=off -fsanitize=address,undefined.
//
// usage: temporal_test IN OUT
// IN : 5 words -- width, height, has_halves, has_history, has_motion -- then 55 floats -- projection_inverse[16], view_inverse[16],
//      prev_world_to_clip[16] (all column-major), prev_eye[3], max_history, normal_min, sigma_depth, snap -- then width*height records of
//      8 floats, (has_halves) width*height*2 records, (has_history) width*height records, (has_history and has_halves) width*height*2 records, (has_history) width*height floats, (has_motion) width*height*3 floats.
// OUT: width*height records, width*height floats of length, (has_halves) width*height*2 records.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../rustray_amd/csrc/rr_temporal.h"

static bool read_all(FILE* f, void* p, size_t bytes) { return bytes == 0 || fread(p, 1, bytes, f) == bytes; }

struct HostHistory {
    const float* history;
    const float* history_halves;
    const float* history_length;
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
};

template <bool HALVES>
static void run(const TpFrame& f, const float* records, const float* halves, const HostHistory* hist, const float* motion, float* out, float* halves_out,
                float* length_out) {
    for (int y = 0; y < f.height; y++)
        for (int x = 0; x < f.width; x++) {
            const size_t o = (size_t)y * f.width + x;
            const float* r = records + 8 * o;
            const unsigned int flags = denoise_flags(r, r[3], r + 4);
            unsigned int id;
            memcpy(&id, r + 7, 4);
            TpMix m;
            bool kept = false;
            if (hist && flags == (unsigned int)(DN_FIN | DN_VALID))
                kept = temporal_history<HALVES>(f, (unsigned int)x, (unsigned int)y, r[3], r + 4, id, motion ? motion + 3 * o : nullptr, *hist, &m);
            memcpy(out + 8 * o, r, 32);
            if (kept)
                for (int k = 0; k < 3; k++) out[8 * o + k] = temporal_blend(m.h[k], m.a, r[k]);
            length_out[o] = kept ? m.length : ((flags & DN_FIN) ? 1.0f : 0.0f);
            if (HALVES)
                for (int h = 0; h < 2; h++) {
                    const float* c = halves + 16 * o + 8 * h;
                    float* d = halves_out + 16 * o + 8 * h;
                    memcpy(d, c, 32);
                    if (kept && temporal_colour_ok(c))
                        for (int k = 0; k < 3; k++) d[k] = temporal_blend(h ? m.hb[k] : m.ha[k], m.a, c[k]);
                }
        }
}

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: temporal_test IN OUT\n"); return 2; }
    FILE* fi = fopen(argv[1], "rb");
    if (!fi) { perror(argv[1]); return 2; }
    uint32_t head[5];
    float par[55];
    if (!read_all(fi, head, sizeof head) || !read_all(fi, par, sizeof par)) { fprintf(stderr, "short header\n"); return 2; }
    const int W = (int)head[0], H = (int)head[1];
    const bool has_halves = head[2] != 0, has_history = head[3] != 0, has_motion = head[4] != 0;
    if (W <= 0 || H <= 0 || W > 4096 || H > 4096) { fprintf(stderr, "bad header\n"); return 2; }
    TpFrame f{};
    memcpy(f.proj_inv, par, 64);
    memcpy(f.view_inv, par + 16, 64);
    memcpy(f.prev_clip, par + 32, 64);
    memcpy(f.prev_eye, par + 48, 12);
    f.max_history = par[51]; f.normal_min = par[52]; f.sigma_depth = par[53]; f.snap = par[54];
    f.w = (float)W; f.h = (float)H; f.width = W; f.height = H;
    const size_t N = (size_t)W * H;
    std::vector<float> records(8 * N), halves(has_halves ? 16 * N : 0), history(has_history ? 8 * N : 0), history_halves(has_history && has_halves ? 16 * N : 0),
        history_length(has_history ? N : 0), motion(has_motion ? 3 * N : 0);
    for (std::vector<float>* v : {&records, &halves, &history, &history_halves, &history_length, &motion})
        if (!read_all(fi, v->data(), 4 * v->size())) { fprintf(stderr, "short input\n"); return 2; }
    fclose(fi);

    std::vector<float> out(8 * N), halves_out(has_halves ? 16 * N : 0), length_out(N);
    const HostHistory hist{history.data(), history_halves.data(), history_length.data()};
    if (has_halves) run<true>(f, records.data(), halves.data(), has_history ? &hist : nullptr, has_motion ? motion.data() : nullptr, out.data(), halves_out.data(), length_out.data());
    else run<false>(f, records.data(), nullptr, has_history ? &hist : nullptr, has_motion ? motion.data() : nullptr, out.data(), nullptr, length_out.data());

    FILE* fo = fopen(argv[2], "wb");
    if (!fo) { perror(argv[2]); return 2; }
    for (std::vector<float>* v : {&out, &length_out, &halves_out})
        if (v->size() && fwrite(v->data(), 4, v->size(), fo) != v->size()) { fprintf(stderr, "short write\n"); return 2; }
    fclose(fo);
    printf("temporal test OK\n");
    return 0;
}
