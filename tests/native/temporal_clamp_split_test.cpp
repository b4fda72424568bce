// temporal_clamp_split_test.cpp — rr_accumulate_clamped_split_records as a plain host loop over rustray_amd/csrc/rr_history_clamp.h and
// rr_temporal.h, the functions the kernel applies per lane: temporal_history with the diffuse means as temporal_split_test.cpp calls it,
// then history_clamp_split (the two windows, the two boxes, the clamps and the length rule), then the blends.  Reads a raw split frame and
// its history, accumulates, writes the result; tests/test_temporal_clamp_split_host.py compares the output with
// rustray_amd/temporal.py: accumulate_clamped_split_records bit for bit.  Built with -ffp-contract=off -fsanitize=address,undefined.
//
// usage: temporal_clamp_split_test IN OUT
// IN : 6 words -- width, height, has_halves, has_history, has_motion, radius -- then 56 floats -- projection_inverse[16],
//      view_inverse[16], prev_world_to_clip[16] (all column-major), prev_eye[3], max_history, normal_min, sigma_depth, snap, sigma_scale --
//      then, n = width*height: 8n floats of records, (has_halves) 16n of halves, 3n of diffuse, (has_halves) 6n of diffuse halves,
//      (has_history) 8n of history, (has_history and has_halves) 16n of its halves, (has_history) 3n of its diffuse, (has_history and
//      has_halves) 6n of its diffuse halves, (has_history) n of length, (has_motion) 3n of motion.
// OUT: 8n floats of records, n of length, (has_halves) 16n of halves, 3n of diffuse, (has_halves) 6n of diffuse halves, then 3n of lo and
//      3n of hi of the colour box (of every pixel whose colour is finite; 0 elsewhere), then 3n of lo and 3n of hi of the diffuse box (of
//      every pixel).
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

template <bool HALVES>
static void run(const TpFrame& f, int radius, float sigma_scale, const Layers& io, const HostHistory* hist, const float* motion) {
    for (int y = 0; y < f.height; y++)
        for (int x = 0; x < f.width; x++) {
            const size_t o = (size_t)y * f.width + x;
            const float* r = io.records + 8 * o;
            const unsigned int flags = denoise_flags(r, r[3], r + 4);
            unsigned int id;
            memcpy(&id, r + 7, 4);
            // the two windows of the current frame around (x, y): inside the frame, three finite floats of the layer itself
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
            if (flags & DN_FIN) { // (the boxes as outputs of their own, for the yardstick's `box` and `diffuse_box`)
                const HcBox b = history_clamp_box(history_clamp_sums(radius, window), sigma_scale);
                memcpy(io.lo + 3 * o, b.lo, 12);
                memcpy(io.hi + 3 * o, b.hi, 12);
            }
            const HcBox bd = history_clamp_box(history_clamp_sums(radius, diffuse_window), sigma_scale);
            memcpy(io.dlo + 3 * o, bd.lo, 12);
            memcpy(io.dhi + 3 * o, bd.hi, 12);
            TpMix m;
            TpSplitMix s;
            bool kept = false;
            if (hist && flags == (unsigned int)(DN_FIN | DN_VALID))
                kept = temporal_history<HALVES, HostHistory, true>(f, (unsigned int)x, (unsigned int)y, r[3], r + 4, id, motion ? motion + 3 * o : nullptr, *hist, &m, &s);
            if (kept) history_clamp_split<HALVES>(radius, sigma_scale, window, diffuse_window, &m, &s);
            memcpy(io.out + 8 * o, r, 32);
            if (kept)
                for (int k = 0; k < 3; k++) io.out[8 * o + k] = temporal_blend(m.h[k], m.a, r[k]);
            io.length_out[o] = kept ? m.length : ((flags & DN_FIN) ? 1.0f : 0.0f);
            memcpy(io.diffuse_out + 3 * o, io.diffuse + 3 * o, 12);
            if (kept) temporal_blend_diffuse(s.d, m.a, io.diffuse + 3 * o, io.diffuse_out + 3 * o);
            if (HALVES)
                for (int h = 0; h < 2; h++) {
                    const float* c = io.halves + 16 * o + 8 * h;
                    float* d = io.halves_out + 16 * o + 8 * h;
                    memcpy(d, c, 32);
                    if (kept && temporal_colour_ok(c))
                        for (int k = 0; k < 3; k++) d[k] = temporal_blend(h ? m.hb[k] : m.ha[k], m.a, c[k]);
                    const float* cd = io.dif_halves + 3 * (2 * o + h);
                    float* dd = io.dif_halves_out + 3 * (2 * o + h);
                    memcpy(dd, cd, 12);
                    if (kept) temporal_blend_diffuse(h ? s.db : s.da, m.a, cd, dd);
                }
        }
}

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: temporal_clamp_split_test IN OUT\n"); return 2; }
    FILE* fi = fopen(argv[1], "rb");
    if (!fi) { perror(argv[1]); return 2; }
    uint32_t head[6];
    float par[56];
    if (!read_all(fi, head, sizeof head) || !read_all(fi, par, sizeof par)) { fprintf(stderr, "short header\n"); return 2; }
    const int W = (int)head[0], H = (int)head[1], radius = (int)head[5];
    const bool has_halves = head[2] != 0, has_history = head[3] != 0, has_motion = head[4] != 0;
    if (W <= 0 || H <= 0 || W > 4096 || H > 4096 || radius < 1 || radius > 2) { fprintf(stderr, "bad header\n"); return 2; }
    TpFrame f{};
    memcpy(f.proj_inv, par, 64);
    memcpy(f.view_inv, par + 16, 64);
    memcpy(f.prev_clip, par + 32, 64);
    memcpy(f.prev_eye, par + 48, 12);
    f.max_history = par[51]; f.normal_min = par[52]; f.sigma_depth = par[53]; f.snap = par[54];
    const float sigma_scale = par[55];
    f.w = (float)W; f.h = (float)H; f.width = W; f.height = H;
    const size_t N = (size_t)W * H;
    const bool hh = has_history && has_halves;
    std::vector<float> records(8 * N), halves(has_halves ? 16 * N : 0), diffuse(3 * N), dif_halves(has_halves ? 6 * N : 0), history(has_history ? 8 * N : 0),
        history_halves(hh ? 16 * N : 0), history_diffuse(has_history ? 3 * N : 0), history_dif_halves(hh ? 6 * N : 0), history_length(has_history ? N : 0),
        motion(has_motion ? 3 * N : 0);
    for (std::vector<float>* v : {&records, &halves, &diffuse, &dif_halves, &history, &history_halves, &history_diffuse, &history_dif_halves, &history_length, &motion})
        if (!read_all(fi, v->data(), 4 * v->size())) { fprintf(stderr, "short input\n"); return 2; }
    fclose(fi);

    std::vector<float> out(8 * N), halves_out(has_halves ? 16 * N : 0), diffuse_out(3 * N), dif_halves_out(has_halves ? 6 * N : 0), length_out(N), lo(3 * N), hi(3 * N),
        dlo(3 * N), dhi(3 * N);
    const HostHistory hist{history.data(), history_halves.data(), history_length.data(), history_diffuse.data(), history_dif_halves.data()};
    const Layers io{records.data(), halves.data(), diffuse.data(), dif_halves.data(), out.data(), halves_out.data(), diffuse_out.data(), dif_halves_out.data(),
                    length_out.data(), lo.data(), hi.data(), dlo.data(), dhi.data()};
    if (has_halves) run<true>(f, radius, sigma_scale, io, has_history ? &hist : nullptr, has_motion ? motion.data() : nullptr);
    else run<false>(f, radius, sigma_scale, io, has_history ? &hist : nullptr, has_motion ? motion.data() : nullptr);

    FILE* fo = fopen(argv[2], "wb");
    if (!fo) { perror(argv[2]); return 2; }
    for (std::vector<float>* v : {&out, &length_out, &halves_out, &diffuse_out, &dif_halves_out, &lo, &hi, &dlo, &dhi})
        if (v->size() && fwrite(v->data(), 4, v->size(), fo) != v->size()) { fprintf(stderr, "short write\n"); return 2; }
    fclose(fo);
    printf("temporal clamp split test OK\n");
    return 0;
}
