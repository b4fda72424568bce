#!/usr/bin/env python3
"""Developer probe: what a frame traced at half the size each way and raised by the G-buffer looks like next to what the same rays buy
at full resolution.

Per scene, at W x H with S samples per low pixel (S a multiple of 8): the reference is the full-resolution frame at 16 S samples
(rr_render_pixels, another seed).  Four arms, each the mean squared error of the linear colour, clamped to [0, 1] as the frame's bytes
are, against that reference over the whole frame:
  guided     rr_upsample_records of the W/2 x H/2 frame at S samples (render_upsampled, scale 2, default parameters, albedo on)
  no albedo  the guided arm with use_albedo off: the guide in the weights only, colour summed as it is
  bilinear   upsample.bilinear_records of the same low frame: the same rays without the guide
  equal rays the full-resolution frame at S / 4 samples: the same number of primary rays, spent per displayed pixel
and the share of hole pixels (weight 0 on a surface) of the guided arm, which a caller may trace at full resolution.
Four more arms with albedo planes (rr_upsample_albedo_records), the same scenes, seeds and reference in the same run:
  (e) mean low       the guided arm with albedo="mean": the low frame demodulated by rr_albedo_pixels on the small camera
  (f) mean both      (e) plus full_albedo_samples = S: remodulated by rr_albedo_pixels at full size with S samples
  (g) low filtered   (e) plus low_denoise_params at the filter's defaults: the low frame filtered before it is raised
  (h) equal rays, filtered   render_denoised(albedo="mean") at full size with S / 4 samples: the opponent of (g)

usage: upsample_quality.py [width height samples] [--out FILE] [scene ...]   (default: 640 360 8, sponza_syn monkey)"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(argv):
    from rustray_amd import capi, synthetic
    from rustray_amd.denoise import DenoiseParams
    from rustray_amd.flat import make_config
    from rustray_amd.renderer import Raytracing, _low_camera, _pack_records
    from rustray_amd.upsample import UpsampleParams, bilinear_records
    from tests.helpers import camera_for, load_scene
    out_path = None
    if "--out" in argv:
        i = argv.index("--out")
        out_path = argv[i + 1]
        del argv[i:i + 2]
    args = argv[1:]
    W, H, S = 640, 360, 8
    if len(args) >= 3 and all(a.isdigit() for a in args[:3]):
        W, H, S = (int(a) for a in args[:3])
        args = args[3:]
    scenes = args or ["sponza_syn", "monkey"]
    if S % 8:
        raise SystemExit("samples must be a multiple of 8: the equal-ray arm runs at samples / 4 in two halves")
    if capi.device_count() < 1:
        raise SystemExit("upsample_quality.py needs a GPU: no HIP device visible")
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    mse = lambda c, ref: float(np.mean((np.clip(np.nan_to_num(c.astype(np.float64)), 0, 1) - ref) ** 2))
    emit(f"upsampling quality, {W}x{H} <- half the size each way, {S} samples per low pixel; MSE of min(colour, 1) against the full frame at {16 * S} samples")
    for scene in scenes:
        fs = synthetic.sponza_syn() if scene == "sponza_syn" else load_scene(scene)
        rt = Raytracing(fs, camera_for(fs, W, H), 0)
        try:
            cam = rt.camera.c_struct()
            rt.config = make_config(samples=16 * S, monte_carlo=True, seed=9, max_recursion=4)
            ref = np.clip(np.nan_to_num(rt.render_pixels()["color"].astype(np.float64)), 0, 1)
            rt.config = make_config(samples=S, monte_carlo=True, seed=1, max_recursion=4)
            guided = rt.render_upsampled(scale=2)
            unmodulated = rt.render_upsampled(scale=2, params=UpsampleParams(use_albedo=False))
            low_cam, w, h = _low_camera(cam, 2)
            low = _pack_records(rt.device_scene.render_pixel_parts(low_cam, rt.config, n_parts=2))
            guide = rt.surface_pixels()
            plain = bilinear_records(low, None, guide, w, h, W, H)
            mean_low = rt.render_upsampled(scale=2, albedo="mean")
            mean_both = rt.render_upsampled(scale=2, albedo="mean", full_albedo_samples=S)
            low_filtered = rt.render_upsampled(scale=2, albedo="mean", low_denoise_params=DenoiseParams())
            rt.config = make_config(samples=S // 4, monte_carlo=True, seed=1, max_recursion=4)
            equal = rt.render_pixels()
            equal_filtered = rt.render_denoised(albedo="mean")
            holes = int(((guided["weight"] == 0) & (guide["hit"] != 0)).sum())
            emit(f"  {scene}: guided {mse(guided['color'], ref):.4e}, no albedo {mse(unmodulated['color'], ref):.4e}, bilinear {mse(plain['records'][:, 0:3], ref):.4e}, equal rays ({S // 4} samples at full size) "
                 f"{mse(equal['color'], ref):.4e}; holes {holes} of {W * H} = {holes / (W * H):.3%}")
            emit(f"  {scene}, albedo planes: (e) mean low {mse(mean_low['color'], ref):.4e}, (f) mean both ({S} samples at full size) {mse(mean_both['color'], ref):.4e}, "
                 f"(g) mean low, low frame filtered {mse(low_filtered['color'], ref):.4e}, (h) equal rays ({S // 4} samples at full size), filtered, mean albedo "
                 f"{mse(equal_filtered['color'], ref):.4e}")
        finally:
            rt.close()
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "a") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main(list(sys.argv))
