#!/usr/bin/env python3
"""Developer probe: what rr_denoise_records_device costs, launch by launch, and which form of the pass kernel each step should run in.

One frame (spheres_room, 1280 x 720, 8 samples in two halves by default) is rendered on one handle, on the device, and stays there;
the filter then runs on it with halves, 5 iterations, in one process.  Every figure is device time between two HIP events around CALLS
back-to-back calls on one stream, divided by CALLS; the arms ALTERNATE round by round (a drift of the clocks or of the machine's load
meets all of them alike), WARMUP rounds and then the median of ROUNDS timed rounds with their range.

  whole call        5 iterations, every pass in its shipped form
  k iterations      k = 1 .. 5, shipped forms: T(k) - T(k - 1) is pass k - 1 (step 2^(k-1)); T(1) is prepare + pass 0 + finish + bytes
  pass i as form f  iterations = i + 1 with pass i forced to gather / tile / lattice (the passes before it shipped): minus T(i) it is
                    that pass in that form -- the A/B of the forms, per step
next to two yardsticks: the compulsory traffic of a pass (working colour, guide and flags read once: 16 + 16 + 8 B, 16 B written per
pixel) at the HBM rate the machine reaches with a float4 copy (6.29 TB/s), and the device time of the frame being filtered (the two
halves at 8 samples per pixel) on the same handle.

With --sweep (no GPU): the four defaults on the CPU quality frame of tests/denoise_cases.py through the numpy yardstick -- RMSE against
the truth for a grid around rr_denoise_default_params.

With --albedo: what the albedo guide costs next to the filter and the frame, same protocol (one process, one handle, arms alternating,
device events around CALLS back-to-back calls, WARMUP rounds, the median of ROUNDS):
  (a) rr_surface_pixels_device, albedo only      (b) the same with records
  (c) the path it replaces: host-made pixel-centre rays already resident on the device + rr_surface_rays_device + a torch gather of base_color
  (d) rr_denoise_records_device (5 iterations, halves, that albedo)      (e) the 4-sample rr_render_pixel_parts_device frame, and the 8-sample one
  (f) rr_albedo_pixels_device, the frame's mean albedo, at 4 and at 8 samples: a strict subset of (e)'s level-1 work at the same count
  (g) rr_render_pixel_split_device at 4 and at 8 samples: (e)'s frame plus the direct diffuse sum; the bar is (g) < 2 x (e), rendering twice
  (h) rr_denoise_split_records_device (5 iterations, halves, that albedo): (d)'s launches twice between two streaming kernels
next to the compulsory traffic of (a) per pixel (the walk's records: 16 + 16 + 8 B written and read, 16 B of hit written and read, the
4 B slot map written and read, 12 B of albedo written) at the float4-copy rate.  Scene `sponza_syn` is the benchmark's stand-in.

usage: denoise_time.py [scene [width height samples]] [--out FILE] [--sweep | --albedo]"""
import itertools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

WARMUP, ROUNDS, CALLS = 2, 9, 20
HBM_BYTES_PER_S = 6.29e12        # float4 copy, measured
PASS_BYTES_PER_PIXEL = 16 + 16 + 8 + 16
FORM_NAMES = {1: "gather", 2: "tile", 3: "lattice"}


def _median(runs):
    runs = sorted(runs)
    return runs[len(runs) // 2], runs[0], runs[-1]


def sweep(emit):
    from rustray_amd.denoise import DenoiseParams, atrous_denoise
    from tests.denoise_cases import quality_frame
    truth, records, halves = quality_frame()
    rmse = lambda rec: float(np.sqrt(np.mean((rec[:, 0:3].astype(np.float64) - truth) ** 2)))
    emit(f"sweep of the defaults, 64x48 quality frame (halves = truth + N(0, 0.1)): raw RMSE {rmse(records):.4f}")
    rows = []
    for it, power, sd, sl in itertools.product((3, 4, 5, 6), (3, 5, 7), (0.02, 0.05, 0.2), (1.0, 2.0, 4.0, 8.0)):
        prm = DenoiseParams(iterations=it, normal_power_log2=power, sigma_depth=sd, sigma_luminance=sl)
        rows.append((rmse(atrous_denoise(records, halves, None, 64, 48, prm)["records"]), it, power, sd, sl))
    rows.sort()
    default = [r for r in rows if r[1:] == (5, 5, 0.05, 4.0)][0]
    emit(f"  defaults (5 iterations, power 5, sigma_depth 0.05, sigma_luminance 4): RMSE {default[0]:.4f}, rank {rows.index(default) + 1} of {len(rows)}")
    for r in rows[:8]:
        emit(f"  RMSE {r[0]:.4f}  iterations {r[1]}  power {r[2]}  sigma_depth {r[3]}  sigma_luminance {r[4]}")
    emit(f"  worst: RMSE {rows[-1][0]:.4f}  iterations {rows[-1][1]}  power {rows[-1][2]}  sigma_depth {rows[-1][3]}  sigma_luminance {rows[-1][4]}")


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
    if "--sweep" in argv:
        sweep(emit)
    elif "--albedo" in argv:
        argv.remove("--albedo")
        measure_albedo(argv, emit)
    else:
        measure(argv, emit)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "a") as fh:
            fh.write("\n".join(lines) + "\n")


def measure(argv, emit):
    import torch
    from rustray_amd import capi, renderer
    from rustray_amd.denoise import DenoiseParams
    from rustray_amd.flat import make_config
    from tests.helpers import camera_for, load_scene
    scene = argv[1] if len(argv) > 1 else "spheres_room"
    w, h, samples = (int(argv[2]), int(argv[3]), int(argv[4])) if len(argv) > 4 else (1280, 720, 8)
    if capi.device_count() < 1:
        raise SystemExit("denoise_time.py needs a GPU: no HIP device visible")
    fs = load_scene(scene)
    cam = camera_for(fs, w, h).c_struct()
    cfg = make_config(samples=samples, monte_carlo=True, seed=1, max_recursion=4)
    n = w * h
    with capi.DeviceScene(fs, 0) as ds:
        def timed(fn, calls):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(calls):
                fn()
            b.record()
            b.synchronize()
            return a.elapsed_time(b) / calls

        frame = renderer.render_pixel_parts_torch(ds, cam, cfg, None, 2)
        torch.cuda.synchronize()
        rec, halves = frame["records"], frame["part_records"]
        out = torch.empty_like(rec)
        rgba = torch.empty((n, 4), dtype=torch.uint8, device="cuda")
        stream = torch.cuda.current_stream().cuda_stream

        def call(iterations, forms=None):
            prm = capi.denoise_params(DenoiseParams(iterations=iterations))

            def run():
                capi.denoise_forms(forms)
                ds.denoise_records_device(w, h, rec.data_ptr(), halves.data_ptr(), None, out.data_ptr(), rgba.data_ptr(), None, prm, stream)
            return run

        arms = {("auto", k): call(k) for k in range(1, 6)}
        for i in range(5):
            for f in (1, 2, 3):
                if (f == 2 and 2 * (1 << i) > 8) or (f == 3 and i == 0):
                    continue
                arms[("pass", i, f)] = call(i + 1, [0] * i + [f])
        runs = {k: [] for k in arms}
        frame_runs = []
        try:
            for r in range(WARMUP + ROUNDS):
                for k, fn in arms.items():
                    t = timed(fn, CALLS)
                    if r >= WARMUP:
                        runs[k].append(t)
                t = timed(lambda: renderer.render_pixel_parts_torch(ds, cam, cfg, None, 2), 1)
                if r >= WARMUP:
                    frame_runs.append(t)
        finally:
            capi.denoise_forms(None)
        torch.cuda.synchronize()

    med = {k: _median(v) for k, v in runs.items()}
    floor_ms = n * PASS_BYTES_PER_PIXEL / HBM_BYTES_PER_S * 1e3
    emit(f"rr_denoise_records_device, {scene} {w}x{h}, {samples} samples in two halves, with halves, rgba8_out; device ms per call, median of {ROUNDS} rounds of {CALLS} calls [min .. max]")
    emit(f"  the frame being filtered (rr_render_pixel_parts_device, n_parts = 2): {_median(frame_runs)[0]:.3f} ms [{_median(frame_runs)[1]:.3f} .. {_median(frame_runs)[2]:.3f}]")
    emit(f"  compulsory traffic of one pass: {PASS_BYTES_PER_PIXEL} B per pixel = {n * PASS_BYTES_PER_PIXEL / 1e6:.1f} MB, {floor_ms * 1e3:.1f} us at {HBM_BYTES_PER_S / 1e12:.2f} TB/s")
    m, lo, hi = med[("auto", 5)]
    emit(f"  whole call, 5 iterations, shipped forms: {m:.4f} ms [{lo:.4f} .. {hi:.4f}]")
    m1 = med[("auto", 1)][0]
    emit(f"  1 iteration (prepare + pass 0 + finish + bytes): {m1:.4f} ms")
    for k in range(2, 6):
        d = med[("auto", k)][0] - med[("auto", k - 1)][0]
        emit(f"  pass {k - 1} (step {1 << (k - 1)}), shipped form, T({k}) - T({k - 1}): {d * 1e3:.1f} us = {floor_ms / d:.2f} of the traffic floor's rate")
    emit("  the forms per pass (pass 0: the whole 1-iteration call; later passes: minus the shipped call of the passes before):")
    for i in range(5):
        base = med[("auto", i)][0] if i else 0.0
        row = []
        for f in (1, 2, 3):
            if ("pass", i, f) in med:
                m, lo, hi = med[("pass", i, f)]
                row.append(f"{FORM_NAMES[f]} {(m - base) * 1e3:.1f} us [{(lo - base) * 1e3:.1f} .. {(hi - base) * 1e3:.1f}]")
        emit(f"    pass {i} (step {1 << i}): " + ", ".join(row))


ALBEDO_BYTES_PER_PIXEL = 2 * (16 + 16 + 8) + 2 * 16 + 2 * 4 + 12


def measure_albedo(argv, emit):
    import torch
    from rustray_amd import capi, renderer, synthetic
    from rustray_amd.denoise import DenoiseParams
    from rustray_amd.flat import make_config
    from rustray_amd.pixel_rays import pixel_rays
    from tests.helpers import camera_for, load_scene
    scene = argv[1] if len(argv) > 1 else "spheres_room"
    w, h = (int(argv[2]), int(argv[3])) if len(argv) > 3 else (1280, 720)
    if capi.device_count() < 1:
        raise SystemExit("denoise_time.py needs a GPU: no HIP device visible")
    fs = synthetic.sponza_syn() if scene == "sponza_syn" else load_scene(scene)
    cam = camera_for(fs, w, h).c_struct()
    cfg = make_config(samples=4, monte_carlo=True, seed=1, max_recursion=4)
    n = w * h
    with capi.DeviceScene(fs, 0) as ds:
        def timed(fn, calls):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(calls):
                fn()
            b.record()
            b.synchronize()
            return a.elapsed_time(b) / calls

        stream = torch.cuda.current_stream().cuda_stream
        o, d = (torch.from_numpy(a).cuda() for a in pixel_rays(cam))
        frame = renderer.render_pixel_parts_torch(ds, cam, cfg, None, 2)
        rec, halves = frame["records"], frame["part_records"]
        albedo = torch.empty((n, 3), dtype=torch.float32, device="cuda")
        mean = torch.empty((n, 3), dtype=torch.float32, device="cuda")
        cfg8 = make_config(samples=8, monte_carlo=True, seed=1, max_recursion=4)
        surf = torch.empty((n, 32), dtype=torch.float32, device="cuda")
        out = torch.empty_like(rec)
        split = renderer.render_pixel_split_torch(ds, cam, cfg, None, True)
        dif, dif_h = split["diffuse"], split["diffuse_halves"]
        prm = capi.denoise_params(DenoiseParams(iterations=5))
        torch.cuda.synchronize()

        def replaced():
            ds.surface_rays_device(o.data_ptr(), d.data_ptr(), n, 1, surf.data_ptr(), stream)
            return surf[:, 16:19].contiguous()

        arms = {
            "a": lambda: ds.surface_pixels_device(cam, None, n, None, albedo.data_ptr(), stream),
            "b": lambda: ds.surface_pixels_device(cam, None, n, surf.data_ptr(), albedo.data_ptr(), stream),
            "c": replaced,
            "d": lambda: ds.denoise_records_device(w, h, rec.data_ptr(), halves.data_ptr(), albedo.data_ptr(), out.data_ptr(), None, None, prm, stream),
            "e": lambda: renderer.render_pixel_parts_torch(ds, cam, cfg, None, 2),
            "e8": lambda: renderer.render_pixel_parts_torch(ds, cam, cfg8, None, 2),
            "f4": lambda: ds.albedo_pixels_device(cam, cfg, None, n, mean.data_ptr(), stream),
            "f8": lambda: ds.albedo_pixels_device(cam, cfg8, None, n, mean.data_ptr(), stream),
            "g4": lambda: renderer.render_pixel_split_torch(ds, cam, cfg, None, True),
            "g8": lambda: renderer.render_pixel_split_torch(ds, cam, cfg8, None, True),
            "h": lambda: ds.denoise_split_device(w, h, rec.data_ptr(), halves.data_ptr(), dif.data_ptr(), dif_h.data_ptr(), albedo.data_ptr(), out.data_ptr(), None, prm, stream),
        }
        runs = {k: [] for k in arms}
        for r in range(WARMUP + ROUNDS):
            for k, fn in arms.items():
                t = timed(fn, 1 if k in ("e", "e8", "g4", "g8") else CALLS)
                if r >= WARMUP:
                    runs[k].append(t)
        torch.cuda.synchronize()
        same = bool(torch.equal(replaced().view(torch.int32), albedo.view(torch.int32)))
    med = {k: _median(v) for k, v in runs.items()}
    floor_ms = n * ALBEDO_BYTES_PER_PIXEL / HBM_BYTES_PER_S * 1e3
    names = {"a": "(a) rr_surface_pixels_device, albedo only", "b": "(b) rr_surface_pixels_device, records and albedo",
             "c": "(c) resident rays + rr_surface_rays_device + torch gather of base_color", "d": "(d) rr_denoise_records_device, 5 iterations, halves, albedo",
             "e": "(e) rr_render_pixel_parts_device, 4 samples in two halves", "e8": "(e) the same at 8 samples",
             "f4": "(f) rr_albedo_pixels_device, the frame's mean albedo, 4 samples", "f8": "(f) the same at 8 samples",
             "g4": "(g) rr_render_pixel_split_device, 4 samples in two halves", "g8": "(g) the same at 8 samples",
             "h": "(h) rr_denoise_split_records_device, 5 iterations, halves, albedo"}
    emit(f"the albedo guide, {scene} {w}x{h}; device ms per call, median of {ROUNDS} rounds of {CALLS} calls (e, g: 1 call) [min .. max]; (c)'s albedo equals (a)'s bit for bit: {same}")
    for k in ("a", "b", "c", "d", "e", "e8", "f4", "f8", "g4", "g8", "h"):
        m, lo, hi = med[k]
        emit(f"  {names[k]}: {m:.4f} ms [{lo:.4f} .. {hi:.4f}]")
    for f, e, s in (("f4", "e", 4), ("f8", "e8", 8)):
        below = med[f][2] < med[e][1]   # outside the two arms' ranges
        emit(f"  (f) / (e) at {s} samples = {med[f][0] / med[e][0]:.3f}; (f)'s largest below (e)'s smallest: {below}; (f) / (a) = {med[f][0] / med['a'][0]:.2f}")
    for g, e, s in (("g4", "e", 4), ("g8", "e8", 8)):   # what a caller can do without the call: render the frame twice
        below = med[g][2] < 2.0 * med[e][1]
        emit(f"  (g) / (e) at {s} samples = {med[g][0] / med[e][0]:.3f}; (g)'s largest below twice (e)'s smallest: {below}")
    emit(f"  (h) / (d) = {med['h'][0] / med['d'][0]:.3f}")
    a, c = med["a"], med["c"]
    emit(f"  (a) / (c) = {a[0] / c[0]:.3f}; (c)'s own spread {c[1]:.4f} .. {c[2]:.4f}; (a) / (d) = {a[0] / med['d'][0]:.3f}; (a) / (e) = {a[0] / med['e'][0]:.3f}")
    emit(f"  compulsory traffic of (a): {ALBEDO_BYTES_PER_PIXEL} B per pixel = {n * ALBEDO_BYTES_PER_PIXEL / 1e6:.1f} MB, {floor_ms * 1e3:.1f} us at {HBM_BYTES_PER_S / 1e12:.2f} TB/s: "
         f"(a) reaches {floor_ms / a[0]:.3f} of that rate (the walk between the two streaming kernels reads the scene, not the frame)")


if __name__ == "__main__":
    main(list(sys.argv))
