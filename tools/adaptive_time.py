#!/usr/bin/env python3
"""Developer probe: what the host loop of adaptive sampling costs next to the fused call.  One frame (sponza_syn 1280 x 720, monte_carlo,
16 -> 128 samples by default) on one handle, in one process.  The threshold is chosen once, from the base frame's half_error, so that
about a fifth of the frame is refined.  Two arms, wall time around the call, WARMUP frames each and then the median of FRAMES timed
frames with their spread:
  host loop  Raytracing.render_adaptive: rr_render_pixel_parts, half_error and refine_list in numpy, rr_render_pixels, a numpy scatter
  fused      Raytracing.render_adaptive_on_device: rr_render_adaptive
Then, with kernel_timing, the device time of the three launches that make the list (rr_frame_stats::ms_binning after a fused call), their
share of the fused call's device time and the bandwidth they achieved over the 64 B read and 4 + 4 B written per pixel and list entry.

With --levels the probe compares refinement level by level with the two-level call instead.  Three arms, ALTERNATING frame by frame in
the one process (a drift of the clocks or of the machine's load meets all of them alike), WARMUP rounds and then FRAMES timed rounds:
  two-level     Raytracing.render_adaptive_on_device(first level, last level): rr_render_adaptive
  levels        Raytracing.render_adaptive_levels_on_device(levels): rr_render_adaptive_levels
  levels, host  Raytracing.render_adaptive_levels(levels): rr_render_pixel_parts per level, half_error, refine_list and refine_sublist in numpy
Per arm: wall ms (median and range), primary_rays, the pixels of each level and the pixels left above the threshold at their final
count; then, with kernel_timing and again alternating, the device ms of the passes and of the list launches of the two fused arms.

With --prefix the ladder is taken as PREFIXES of one frame of its top count, and refinement that keeps its samples is compared with the
two calls above.  Three arms, alternating in the same way:
  two-level     Raytracing.render_adaptive_on_device(first, last): rr_render_adaptive
  levels        Raytracing.render_adaptive_levels_on_device(ladder): rr_render_adaptive_levels, every level a frame of its own
  prefix        Raytracing.render_adaptive_prefix_on_device(ladder): rr_render_adaptive_prefix, every level the samples a pixel lacks
Per arm the same figures.  The arms estimate on different samples, so their lists differ: compare rays and time at the pixels left.

usage: adaptive_time.py [scene [width height base_samples max_samples]] [--levels S0,S1,...] [--prefix P0,P1,...] [--threshold T] [--limit SECONDS]"""
import os
import signal
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench
from rustray_amd import adaptive
from rustray_amd.flat import rr_config
from rustray_amd.renderer import Raytracing

WARMUP, FRAMES, FRACTION = 3, 9, 0.2


def _option(argv, name, default, convert):
    if name not in argv:
        return default
    i = argv.index(name)
    value = convert(argv[i + 1])
    del argv[i:i + 2]
    return value


def _median(runs):
    runs = sorted(runs)
    return runs[len(runs) // 2], runs[0], runs[-1]


def levels_arms(rt, ds, scene, w, h, levels, threshold):
    """The --levels comparison: the two-level call, the level-by-level call and its host loop, alternating."""
    n, base, top = w * h, levels[0], levels[-1]
    arms = {"two-level": lambda: rt.render_adaptive_on_device(base, top, threshold),
            "levels": lambda: rt.render_adaptive_levels_on_device(levels, threshold),
            "levels, host": lambda: rt.render_adaptive_levels(levels, threshold)}
    print(f"{scene} {w}x{h}, levels {list(levels)} against {base} -> {top}, threshold {threshold:.6g}; {WARMUP} warm-up rounds, median of {FRAMES} (range), the arms alternating")
    keep, wall, rays = {}, {tag: [] for tag in arms}, {}
    for r in range(WARMUP + FRAMES):
        for tag, call in arms.items():
            t0 = time.perf_counter(); keep[tag] = call(); ms = (time.perf_counter() - t0) * 1e3
            if r >= WARMUP:
                wall[tag].append(ms)
            if tag != "levels, host":
                rays[tag] = ds.stats()["primary_rays"]
    lv = keep["levels"]
    padded = [n] + [(c + 63) // 64 * 64 for c in lv["level_pixels"][1:]]
    rays["levels, host"] = sum(p * s for p, s in zip(keep["levels, host"]["padded"], levels))
    assert rays["levels"] == sum(p * s for p, s in zip(padded, levels)), (rays["levels"], padded)
    same = all(np.array_equal(np.ascontiguousarray(lv[k]).view(np.uint32), np.ascontiguousarray(keep["levels, host"][k]).view(np.uint32))
               for k in ("color", "depth", "normal", "object_id", "samples", "error")) and lv["level_pixels"] == keep["levels, host"]["level_pixels"]
    two_residual = rt.render_adaptive_levels_on_device((base, top), threshold)      # the two-level frame with the error of its refined pixels at `top`
    left = {"two-level": int((two_residual["error"] > np.float32(threshold)).sum()), "levels": int((lv["error"] > np.float32(threshold)).sum())}
    left["levels, host"] = int((keep["levels, host"]["error"] > np.float32(threshold)).sum())
    pixels = {"two-level": [n, int(keep["two-level"]["n_refined"])], "levels": lv["level_pixels"], "levels, host": keep["levels, host"]["level_pixels"]}
    med = {}
    for tag in arms:
        med[tag], lo, hi = _median(wall[tag])
        print(f"{tag:13s} wall {med[tag]:8.3f} ms ({lo:8.3f} .. {hi:8.3f})  primary_rays {rays[tag]:>11d}  level_pixels {pixels[tag]}  left above the threshold {left[tag]}")
    print(f"the fused levels call and its host loop agree bit for bit: {same}")
    print(f"levels / two-level: rays {rays['levels'] / rays['two-level']:.3f}, wall {med['levels'] / med['two-level']:.3f};  levels, host / levels: wall {med['levels, host'] / med['levels']:.3f}")
    ds.set_profiling(True)
    dev = {tag: ([], []) for tag in ("two-level", "levels")}
    for r in range(WARMUP + FRAMES):
        for tag in dev:
            arms[tag]()
            st = ds.stats()
            if r >= WARMUP:
                dev[tag][0].append(st["ms_total"]); dev[tag][1].append(st["ms_binning"])
    for tag, (passes, lists) in dev.items():
        (p, plo, phi), (l, llo, lhi) = _median(passes), _median(lists)
        print(f"{tag:13s} kernel_timing: passes {p:8.3f} ms ({plo:.3f} .. {phi:.3f}), list launches {l * 1e3:7.1f} us ({llo * 1e3:.1f} .. {lhi * 1e3:.1f})")
    # where the device time goes: the passes of both arms one by one, as separate library calls on the lists the fused call made
    cam = rt.camera.c_struct()
    lists = []
    xy, count = adaptive.refine_list(adaptive.half_error(ds.render_pixel_parts(cam, _with(rt.config, base), None, n_parts=2)["parts"]["color"]), threshold, w, h)
    for s in levels[1:]:
        if not count:
            break
        lists.append((s, xy, count))
        fine = ds.render_pixel_parts(cam, _with(rt.config, s), xy, n_parts=2)
        xy, count = adaptive.refine_sublist(adaptive.half_error(fine["parts"]["color"]), threshold, xy, count)
    passes = [(f"whole frame, {base} samples, 2 parts", lambda: ds.render_pixel_parts(cam, _with(rt.config, base), None, n_parts=2), n, base)]
    passes += [(f"list of {c}, {s} samples, 2 parts", (lambda s=s, l=l: ds.render_pixel_parts(cam, _with(rt.config, s), l, n_parts=2)), len(l), s) for s, l, c in lists]
    if lists:
        s, l, c = top, lists[0][1], lists[0][2]
        passes.append((f"list of {c}, {s} samples, whole (the two-level call's fine pass)", lambda: ds.render_pixels(cam, _with(rt.config, s), l), len(l), s))
    for tag, call, slots, s in passes:
        ms, launches = [], 0
        for r in range(2 + 5):
            call()
            st = ds.stats()
            launches = st["launches_trace_closest"] + st["launches_trace_shadow"] + st["launches_shade"]
            if r >= 2:
                ms.append(st["ms_total"])
        m, lo, hi = _median(ms)
        print(f"pass: {tag:62s} {m:7.3f} ms ({lo:.3f} .. {hi:.3f})  {slots * s / 1e6:7.2f} M primary rays, {slots * s / m / 1e6:6.2f} G/s, {st['batches']} batches, {launches} walk and shade launches")
    ds.set_profiling(False)


def prefix_arms(rt, ds, scene, w, h, ladder, threshold):
    """The --prefix comparison: the two-level call, the level-by-level call and the call that keeps its samples, alternating."""
    n, base, top = w * h, ladder[0], ladder[-1]
    rt.config = _with(rt.config, top)        # the frame every prefix is taken from (the other two arms ignore config.samples)
    arms = {"two-level": lambda: rt.render_adaptive_on_device(base, top, threshold),
            "levels": lambda: rt.render_adaptive_levels_on_device(ladder, threshold),
            "prefix": lambda: rt.render_adaptive_prefix_on_device(ladder, threshold)}
    print(f"{scene} {w}x{h}, ladder {list(ladder)}, threshold {threshold:.6g}; {WARMUP} warm-up rounds, median of {FRAMES} (range), the arms alternating")
    keep, wall, rays = {}, {tag: [] for tag in arms}, {}
    for r in range(WARMUP + FRAMES):
        for tag, call in arms.items():
            t0 = time.perf_counter(); keep[tag] = call(); ms = (time.perf_counter() - t0) * 1e3
            if r >= WARMUP:
                wall[tag].append(ms)
            rays[tag] = ds.stats()["primary_rays"]
    px = keep["prefix"]
    padded = [n] + [(c + 63) // 64 * 64 for c in px["level_pixels"][1:]]
    assert rays["prefix"] == n * base + sum(p * (ladder[l] - ladder[l - 1]) for l, p in enumerate(padded) if l), (rays["prefix"], padded)
    scratch = sum(p * s for p, s in zip(padded, ladder))
    two_residual = rt.render_adaptive_levels_on_device((base, top), threshold)      # the two-level frame with the error of its refined pixels at `top`
    left = {"two-level": int((two_residual["error"] > np.float32(threshold)).sum())}
    pixels = {"two-level": [n, int(keep["two-level"]["n_refined"])]}
    for tag in ("levels", "prefix"):
        left[tag] = int((keep[tag]["error"] > np.float32(threshold)).sum()); pixels[tag] = keep[tag]["level_pixels"]
    med = {}
    for tag in arms:
        med[tag], lo, hi = _median(wall[tag])
        print(f"{tag:13s} wall {med[tag]:8.3f} ms ({lo:8.3f} .. {hi:8.3f})  primary_rays {rays[tag]:>11d}  level_pixels {pixels[tag]}  left above the threshold {left[tag]}")
    print(f"prefix: its own lists rendered from scratch would cost {scratch} primary rays ({rays['prefix'] / scratch:.3f} kept)")
    print(f"prefix / levels: rays {rays['prefix'] / rays['levels']:.3f}, wall {med['prefix'] / med['levels']:.3f};  prefix / two-level: rays {rays['prefix'] / rays['two-level']:.3f}, "
          f"wall {med['prefix'] / med['two-level']:.3f}")
    ds.set_profiling(True)
    dev = {tag: ([], []) for tag in arms}
    for r in range(WARMUP + FRAMES):
        for tag in dev:
            arms[tag]()
            st = ds.stats()
            if r >= WARMUP:
                dev[tag][0].append(st["ms_total"]); dev[tag][1].append(st["ms_binning"])
    for tag, (passes, lists) in dev.items():
        (p, plo, phi), (l, llo, lhi) = _median(passes), _median(lists)
        print(f"{tag:13s} kernel_timing: passes {p:8.3f} ms ({plo:.3f} .. {phi:.3f}), list launches {l * 1e3:7.1f} us ({llo * 1e3:.1f} .. {lhi * 1e3:.1f})")
    ds.set_profiling(False)


def _with(config, samples):
    c = rr_config.from_buffer_copy(config)
    c.samples = samples
    return c


def main():
    argv = list(sys.argv[1:])
    limit = _option(argv, "--limit", 300, int)
    levels = _option(argv, "--levels", None, lambda t: tuple(int(v) for v in t.split(",")))
    prefix = _option(argv, "--prefix", None, lambda t: tuple(int(v) for v in t.split(",")))
    fixed_threshold = _option(argv, "--threshold", None, float)
    signal.alarm(limit)      # the probe's own time limit: SIGALRM ends the process
    scene = argv[0] if argv else "sponza_syn"
    w, h, base, top = (int(a) for a in argv[1:5]) if len(argv) > 4 else (1280, 720, 16, 128)
    if levels or prefix:
        base, top = (levels or prefix)[0], (levels or prefix)[-1]
    fs, camera, cfg = bench.build_workload(scene, w, h, base, 1)
    rt = Raytracing(fs, camera, 0)
    try:
        rt.config = cfg
        ds = rt.device_scene
        first = ds.render_pixel_parts(camera.c_struct(), cfg, None, n_parts=2)
        err = adaptive.half_error(first["parts"]["color"])
        threshold = fixed_threshold if fixed_threshold is not None else float(np.quantile(err, 1.0 - FRACTION))
        if prefix:
            prefix_arms(rt, ds, scene, w, h, prefix, threshold)
            return
        if levels:
            levels_arms(rt, ds, scene, w, h, levels, threshold)
            return
        arms = {"host loop": lambda: rt.render_adaptive(base, top, threshold), "fused": lambda: rt.render_adaptive_on_device(base, top, threshold)}
        keep, median = {}, {}
        print(f"{scene} {w}x{h}, {base} -> {top} samples, threshold {threshold:.6g} (the {1.0 - FRACTION:.2f} quantile of the base frame's half_error)")
        for tag, call in arms.items():
            for _ in range(WARMUP):
                keep[tag] = call()
            runs = []
            for _ in range(FRAMES):
                t0 = time.perf_counter(); call(); runs.append((time.perf_counter() - t0) * 1e3)
            runs.sort()
            median[tag] = runs[FRAMES // 2]
            print(f"{tag:10s} wall {median[tag]:8.3f} ms median of {FRAMES} ({runs[0]:8.3f} .. {runs[-1]:8.3f}, spread {runs[-1] - runs[0]:6.3f}), {WARMUP} warm-up frames")
        a, b = keep["host loop"], keep["fused"]
        same = all(np.array_equal(np.ascontiguousarray(a[k]).view(np.uint32), np.ascontiguousarray(b[k]).view(np.uint32)) for k in ("color", "depth", "normal", "object_id", "samples", "error"))
        n, count = w * h, int(b["n_refined"])
        print(f"refined {count} of {n} pixels ({count / n:.3f}); the two arms agree bit for bit: {same}")
        print(f"host loop / fused = {median['host loop'] / median['fused']:.3f}")
        ds.set_profiling(True)
        lists, totals = [], []
        for _ in range(WARMUP + FRAMES):
            rt.render_adaptive_on_device(base, top, threshold)
            st = ds.stats()
            lists.append(st["ms_binning"]); totals.append(st["ms_total"])
        lists, totals = sorted(lists[WARMUP:]), sorted(totals[WARMUP:])
        ms_list, ms_total = lists[FRAMES // 2], totals[FRAMES // 2]
        moved = 64 * n + 4 * n + 4 * ((count + 63) // 64 * 64)
        print(f"list kernels (masks, scan, scatter; kernel_timing) {ms_list * 1e3:8.1f} us median ({lists[0] * 1e3:.1f} .. {lists[-1] * 1e3:.1f}), "
              f"{ms_list / (ms_total + ms_list):.4f} of the fused call's device time ({ms_total:.3f} ms in its two passes + the list); {moved / 1e6:.2f} MB moved: "
              f"{moved / (ms_list * 1e-3) / 1e9:.0f} GB/s")
    finally:
        rt.device_scene.close()


if __name__ == "__main__":
    main()
