#!/usr/bin/env python3
"""Developer probe: what rr_upsample_records_device costs next to a copy of the bytes it moves, and what a frame traced at half the size
each way and raised costs next to the full-size frame.

One process, one handle.  Per size W x H <- W/2 x H/2 the inputs (a low frame in two halves and both G-buffers, made by the library on
the scene) stay on the device; the arms ALTERNATE round by round, every figure is device time between two HIP events around CALLS
back-to-back calls on one stream, divided by CALLS; WARMUP rounds, then the median of ROUNDS timed rounds with their range.
  (a) rr_upsample_records_device with halves and weight_out      (b) the same without halves
  (c), (d) a device-to-device copy (torch's copy kernel) of as many bytes as (a) and (b) read and write, timed in the same rounds.
           Bytes: per low pixel 32 (colour record) [+ 64 halves] + 128 (guide); per full pixel 128 (guide) + 32 [+ 64] + 4 (weight).
           The kernel needs 16 + [32 +] 64 B of a low pixel and 64 B of a full guide record, but the rows of a 128-byte record share
           its cache line, so whole records are what the memory system moves.
Then the whole frame at the last size, one call each per round:
  (e) render_upsampled_torch(scale=2) with the filter behind it     (f) render_denoised_torch at full size with the centre albedo
and the share of hole pixels (weight 0 on a surface) of the upsampled frame.  Scene `sponza_syn` is the benchmark's stand-in.
--albedo: rr_upsample_albedo_records_device beside the call above, in the same rounds:
  (a) as above                                                   (a1) the same with the low albedo plane   (a2) with both planes
  (c) the copy of (a)'s bytes; the planes add 12 B per low pixel and per full pixel to the bytes counted for (a1) and (a2)
and the whole frame at the last size:
  (e), (f) as above   (e1) render_upsampled_torch(scale=2, albedo="mean") + filter   (e2) the same with full_albedo_samples = samples
  (e3) (e1) with low_denoise_params at the filter's defaults and no filter at full size.

usage: upsample_time.py [scene [samples]] [--albedo] [--out FILE]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

WARMUP, ROUNDS, CALLS = 2, 9, 20
SIZES = ((640, 360), (1280, 720), (1920, 1080))


def _median(runs):
    runs = sorted(runs)
    return runs[len(runs) // 2], runs[0], runs[-1]


def main(argv):
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    out_path = None
    if "--out" in argv:
        i = argv.index("--out")
        out_path = argv[i + 1]
        del argv[i:i + 2]
    measure(argv, emit)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "a") as fh:
            fh.write("\n".join(lines) + "\n")


def measure(argv, emit):
    import torch
    from rustray_amd import capi, renderer, synthetic
    from rustray_amd.denoise import DenoiseParams
    from rustray_amd.flat import make_config
    from tests.helpers import camera_for, load_scene
    with_planes = "--albedo" in argv
    argv = [a for a in argv if a != "--albedo"]
    scene = argv[1] if len(argv) > 1 else "sponza_syn"
    samples = int(argv[2]) if len(argv) > 2 else 4
    if capi.device_count() < 1:
        raise SystemExit("upsample_time.py needs a GPU: no HIP device visible")
    fs = synthetic.sponza_syn() if scene == "sponza_syn" else load_scene(scene)
    cfg = make_config(samples=samples, monte_carlo=True, seed=1, max_recursion=4)
    prm = capi.upsample_default_params()

    def timed(fn, calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / calls

    with capi.DeviceScene(fs, 0) as ds:
        stream = torch.cuda.current_stream().cuda_stream
        emit(f"rr_upsample_records_device, {scene}, {samples} samples in two halves; device ms per call, median of {ROUNDS} rounds of {CALLS} calls [min .. max]")
        for W, H in SIZES:
            cam = camera_for(fs, W, H).c_struct()
            low_cam, w, h = renderer._low_camera(cam, 2)
            n, nl = W * H, w * h
            base = renderer.render_pixel_parts_torch(ds, low_cam, cfg, None, 2)
            g_low = renderer.surface_pixels_torch(ds, low_cam, None, albedo=False)["records"]
            g_full = renderer.surface_pixels_torch(ds, cam, None, albedo=False)["records"]
            out = torch.empty((n, 8), dtype=torch.float32, device="cuda")
            hout = torch.empty((n, 2, 8), dtype=torch.float32, device="cuda")
            wt = torch.empty((n,), dtype=torch.float32, device="cuda")
            bytes_a = nl * (32 + 64 + 128) + n * (128 + 32 + 64 + 4)
            bytes_b = nl * (32 + 128) + n * (128 + 32 + 4)
            src_a, dst_a = torch.empty(bytes_a // 2, dtype=torch.uint8, device="cuda"), torch.empty(bytes_a // 2, dtype=torch.uint8, device="cuda")
            src_b, dst_b = torch.empty(bytes_b // 2, dtype=torch.uint8, device="cuda"), torch.empty(bytes_b // 2, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            low, hv = base["records"], base["part_records"]
            if with_planes:
                a_low = renderer.albedo_pixels_torch(ds, low_cam, cfg, None)
                a_full = renderer.albedo_pixels_torch(ds, cam, cfg, None)
                torch.cuda.synchronize()
            planes_call = lambda al, af: ds.upsample_device(w, h, W, H, low.data_ptr(), hv.data_ptr(), g_low.data_ptr(), g_full.data_ptr(), out.data_ptr(),
                                                            hout.data_ptr(), None, wt.data_ptr(), prm, stream, albedo_low=al, albedo=af)
            arms = {
                "a": lambda: ds.upsample_device(w, h, W, H, low.data_ptr(), hv.data_ptr(), g_low.data_ptr(), g_full.data_ptr(), out.data_ptr(), hout.data_ptr(), None,
                                                wt.data_ptr(), prm, stream),
                "b": lambda: ds.upsample_device(w, h, W, H, low.data_ptr(), None, g_low.data_ptr(), g_full.data_ptr(), out.data_ptr(), None, None, wt.data_ptr(), prm, stream),
                "c": lambda: dst_a.copy_(src_a),      # (a copy reads and writes each of its bytes: half of the call's bytes each way)
                "d": lambda: dst_b.copy_(src_b),
            }
            if with_planes:
                arms["a1"] = lambda: planes_call(a_low.data_ptr(), None)
                arms["a2"] = lambda: planes_call(a_low.data_ptr(), a_full.data_ptr())
            runs = {k: [] for k in arms}
            for r in range(WARMUP + ROUNDS):
                for k, fn in arms.items():
                    t = timed(fn, CALLS)
                    if r >= WARMUP:
                        runs[k].append(t)
            torch.cuda.synchronize()
            med = {k: _median(v) for k, v in runs.items()}
            emit(f"  {W}x{H} <- {w}x{h}:")
            for k, name, nbytes in (("a", "(a) with halves and weight", bytes_a), ("c", "(c) copy of (a)'s bytes", bytes_a), ("b", "(b) without halves", bytes_b),
                                    ("d", "(d) copy of (b)'s bytes", bytes_b)):
                m, lo, hi = med[k]
                emit(f"    {name}: {m * 1e3:.1f} us [{lo * 1e3:.1f} .. {hi * 1e3:.1f}], {nbytes / 1e6:.1f} MB, {nbytes / m / 1e9:.2f} TB/s")
            emit(f"    (a) / (c) = {med['a'][0] / med['c'][0]:.2f}, (b) / (d) = {med['b'][0] / med['d'][0]:.2f}")
            if with_planes:
                for k, name, nbytes in (("a1", "(a1) (a) with the low albedo plane", bytes_a + 12 * nl), ("a2", "(a2) (a) with both albedo planes", bytes_a + 12 * (nl + n))):
                    m, lo, hi = med[k]
                    emit(f"    {name}: {m * 1e3:.1f} us [{lo * 1e3:.1f} .. {hi * 1e3:.1f}], {nbytes / 1e6:.1f} MB, {nbytes / m / 1e9:.2f} TB/s")
                emit(f"    (a1) / (a) = {med['a1'][0] / med['a'][0]:.3f}, (a2) / (a) = {med['a2'][0] / med['a'][0]:.3f}, (a2) / (c) = {med['a2'][0] / med['c'][0]:.2f}")
        # ---- the whole frame at the last size
        dprm = DenoiseParams()
        arms = {"e": lambda: renderer.render_upsampled_torch(ds, cam, cfg, scale=2, denoise_params=dprm),
                "f": lambda: renderer.render_denoised_torch(ds, cam, cfg, dprm, albedo=True)}
        if with_planes:
            arms["e1"] = lambda: renderer.render_upsampled_torch(ds, cam, cfg, scale=2, denoise_params=dprm, albedo="mean")
            arms["e2"] = lambda: renderer.render_upsampled_torch(ds, cam, cfg, scale=2, denoise_params=dprm, albedo="mean", full_albedo_samples=samples)
            arms["e3"] = lambda: renderer.render_upsampled_torch(ds, cam, cfg, scale=2, albedo="mean", low_denoise_params=dprm)
        runs = {k: [] for k in arms}
        for r in range(WARMUP + ROUNDS):
            for k, fn in arms.items():
                t = timed(fn, 1)
                if r >= WARMUP:
                    runs[k].append(t)
        res = renderer.render_upsampled_torch(ds, cam, cfg, scale=2)
        holes = int(((res["weight"] == 0) & (g_full.view(torch.int32)[:, 0] != 0)).sum())
        torch.cuda.synchronize()
    e, f = _median(runs["e"]), _median(runs["f"])
    emit(f"the whole frame, {scene} {W}x{H}, {samples} samples in two halves, the filter at its defaults; ms per frame between device events, median of {ROUNDS} [min .. max]")
    emit(f"  (e) render_upsampled_torch(scale=2) + filter: {e[0]:.3f} ms [{e[1]:.3f} .. {e[2]:.3f}]")
    emit(f"  (f) render_denoised_torch at full size, centre albedo: {f[0]:.3f} ms [{f[1]:.3f} .. {f[2]:.3f}]")
    for k, name in (("e1", '(e1) (e) with albedo="mean"'), ("e2", f"(e2) (e1) with full_albedo_samples = {samples}"),
                    ("e3", "(e3) (e1) with the low frame filtered and no filter at full size")) if with_planes else ():
        m = _median(runs[k])
        emit(f"  {name}: {m[0]:.3f} ms [{m[1]:.3f} .. {m[2]:.3f}], / (e) = {m[0] / e[0]:.3f}, / (f) = {m[0] / f[0]:.3f}")
    emit(f"  (e) / (f) = {e[0] / f[0]:.3f}; hole pixels (weight 0 on a surface): {holes} of {W * H} = {holes / (W * H):.4%}")


if __name__ == "__main__":
    main(list(sys.argv))
