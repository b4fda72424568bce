// rr_api_probe.h — test and developer probes of the device arithmetic; no scene handle is involved.
// Offers: rr_math_probe; rr_exp_util (developer builds with -DRR_EXP_UTIL only).
// Needs:  rr_api_base.h (fail, HIP_TRY, DevBuf, RR_GUARD_END), rr_math.h, rr_scene_build.h (tri_shading_constants), the kernel k_math_probe.

// ---------------------------------------------------------------------------
// device arithmetic probe (tests/test_device_math.py): runs rr_math.h functions on the GPU
// ---------------------------------------------------------------------------
extern "C" int rr_math_probe(int op, const float* a, const float* b, const float* c, int n, float* out0, float* out1, float* out2,
                             uint64_t seed, int device) try {
    if (n <= 0 || !a || !out0) return fail(RR_ERR_INVALID_ARGUMENT, "bad arguments");
    if (op == 11) { // the HOST build of the per-triangle shading constants (tri_shading_constants): a, b, c hold n / 3 triangles' vertices, xyz interleaved
        for (int t = 0; t + 2 < n; t += 3) {
            float ng[3], area;
            tri_shading_constants(a + t, b + t, c + t, ng, &area);
            for (int k = 0; k < 3; k++) { out0[t + k] = ng[k]; if (out1) out1[t + k] = area; }
        }
        return RR_OK;
    }
    if (op == 6) { // the HOST build of rr_cos, as make_dmaterial uses it for DMaterial::cos_*: out0[i] = rr_cos(a[i] * pi); needs no device
        for (int i = 0; i < n; i++) out0[i] = rr_cos(a[i] * RR_PI_F);
        return RR_OK;
    }
    if (op == 14) { // the HOST build of philox4x32_10: the layout of op 12 (k_math_probe), words as bit patterns; needs no device
        if (!b || !c || !out1) return fail(RR_ERR_INVALID_ARGUMENT, "bad arguments");
        const int m = n / 2;
        for (int i = 0; i < m; i++) {
            uint32_t r0, r1;
            philox4x32_10(f_bits(a[i]), f_bits(b[i]), f_bits(c[i]), f_bits(a[m + i]), (uint32_t)seed, (uint32_t)(seed >> 32), &r0, &r1);
            out0[i] = bits_f(r0); out1[i] = bits_f(r1);
        }
        return RR_OK;
    }
    // op 13, the wave merges of rr_accumulate.h (tests/test_gpu_wave_sums.py): one workgroup works, so the layout has a fixed size, and the
    // low word of the seed picks the entry (k_math_probe)
    if (op == 13 && (n != 9 * 256 || (seed & 0xffffffffull) > 3ull)) return fail(RR_ERR_INVALID_ARGUMENT, "op 13 takes n = 2304 and an entry 0 .. 3");
    HIP_TRY(hipSetDevice(device));
    DevBuf in[3], o[3];
    const float* src[3] = {a, b, c};
    float* dst[3] = {out0, out1, out2};
    for (int k = 0; k < 3; k++) {
        HIP_TRY(in[k].reserve((size_t)n * 4)); HIP_TRY(o[k].reserve((size_t)n * 4));
        if (src[k]) HIP_TRY(hipMemcpy(in[k].p, src[k], (size_t)n * 4, hipMemcpyHostToDevice));
        else HIP_TRY(hipMemset(in[k].p, 0, (size_t)n * 4));
        HIP_TRY(hipMemset(o[k].p, 0, (size_t)n * 4));
    }
    hipLaunchKernelGGL(k_math_probe, dim3((n + 255) / 256), dim3(256), 0, nullptr, op, in[0].as<float>(), in[1].as<float>(), in[2].as<float>(), n,
                       o[0].as<float>(), o[1].as<float>(), o[2].as<float>(), (uint32_t)seed, (uint32_t)(seed >> 32));
    HIP_TRY(hipDeviceSynchronize());
    for (int k = 0; k < 3; k++) {
        if (dst[k]) HIP_TRY(hipMemcpy(dst[k], o[k].p, (size_t)n * 4, hipMemcpyDeviceToHost));
        in[k].release(); o[k].release();
    }
    return RR_OK;
} RR_GUARD_END("rr_math_probe")

#ifdef RR_EXP_UTIL
extern "C" int rr_exp_util(unsigned long long* out64, int reset) {
    if (out64 && hipMemcpyFromSymbol(out64, HIP_SYMBOL(g_util), sizeof(g_util)) != hipSuccess) return RR_ERR_DEVICE;
    if (reset) { unsigned long long z[64] = {0}; if (hipMemcpyToSymbol(HIP_SYMBOL(g_util), z, sizeof(z)) != hipSuccess) return RR_ERR_DEVICE; }
    return RR_OK;
}
#endif
