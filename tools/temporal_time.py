#!/usr/bin/env python3
"""Developer probe: what rr_accumulate_records_device costs, next to rr_denoise_records_device on the same frame and handle.

Two frames (spheres_room, 1280 x 720, 4 samples in two halves by default, two seeds) are rendered on one handle, on the device, and stay
there; the first is accumulated once and is the history of the calls that are timed.  Every figure is device time between two HIP events
around CALLS back-to-back calls on one stream, divided by CALLS; the arms ALTERNATE round by round (a drift of the clocks or of the
machine's load meets all of them alike), WARMUP rounds and then the median of ROUNDS timed rounds with their range.

  with halves       records, halves and their histories: three layers
  without halves    records and their history alone
  static / moved    the previous view is the camera's own (every pixel snaps to itself: one tap) or yawed by 1.3 pixels (four taps)
  first frame       no history: a copy with lengths
next to the compulsory traffic of a call (with halves per pixel 96 B of records read, 96 + 4 B of history gathered, 96 + 4 B written) at
the HBM rate the machine reaches with a float4 copy (6.29 TB/s), and rr_denoise_records_device (5 iterations, with halves) in the same
rounds.

--motion: rr_motion_records_device in the same rounds, on the same records -- every item of the scene listed as moved (each one's
previous transform shifted by 0.05), or one item, with and without world_out -- next to ITS compulsory traffic: 32 B of records read
and 12 B of motion written per pixel, 12 more with world_out.  The yardstick is the static-view accumulation with halves of the same run.

--split: rr_accumulate_split_records_device in the same rounds, with halves, static view and 1.3-pixel yaw, on a frame and a history of
rr_render_pixel_split_device -- next to ITS compulsory traffic: per pixel 36 B of diffuse layers read, 36 B gathered and 36 B written
beside the 296 B of the record call, 404 B in the static case.  The yardstick is the alternative a caller has without the call: two
rr_accumulate_records_device calls of the same run and view.

--clamp: rr_accumulate_clamped_records_device in the same rounds, with halves, static view and 1.3-pixel yaw, at radius 1 and 2 (sigma_scale
1).  The call moves the HBM bytes of a record call -- the window is read from LDS, the halo costs about a third more colour rows, which
hit in cache --, so the yardstick is the record call of the same run and view.

--clamp-split: rr_accumulate_clamped_split_records_device in the same rounds (this turns --split and --clamp on), with halves, static view
and 1.3-pixel yaw, at radius 1 and 2 (sigma_scale 1), on the split frame and history.  The call moves the split call's HBM bytes; the
two windows are read from LDS.  The bar is what a caller would pay for both effects apart: the sum of the split call and the clamped
call of the same run, view and radius.

usage: temporal_time.py [scene [width height samples]] [--motion] [--split] [--clamp] [--clamp-split] [--out FILE]"""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

WARMUP, ROUNDS, CALLS = 2, 7, 20
HBM_BYTES_PER_S = 6.29e12        # float4 copy, measured
BYTES_PER_PIXEL = {True: 96 + 100 + 100, False: 32 + 36 + 36}


def _median(runs):
    runs = sorted(runs)
    return runs[len(runs) // 2], runs[0], runs[-1]


def main(argv):
    import torch
    from rustray_amd import capi, renderer
    from rustray_amd.camera import Camera
    from rustray_amd.flat import make_config
    from rustray_amd.temporal import AccumulateParams, previous_view
    from tests.helpers import camera_for, load_scene
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    out_path = None
    if "--out" in argv:
        i = argv.index("--out")
        out_path = argv[i + 1]
        del argv[i:i + 2]
    with_motion = "--motion" in argv
    if with_motion:
        argv.remove("--motion")
    with_clamp_split = "--clamp-split" in argv
    if with_clamp_split:
        argv.remove("--clamp-split")
        argv += [f for f in ("--split", "--clamp") if f not in argv]
    with_split = "--split" in argv
    if with_split:
        argv.remove("--split")
    with_clamp = "--clamp" in argv
    if with_clamp:
        argv.remove("--clamp")
    scene = argv[1] if len(argv) > 1 else "spheres_room"
    w, h, samples = (int(argv[2]), int(argv[3]), int(argv[4])) if len(argv) > 4 else (1280, 720, 4)
    if capi.device_count() < 1:
        raise SystemExit("temporal_time.py needs a GPU: no HIP device visible")
    fs = load_scene(scene)
    camera = camera_for(fs, w, h)
    st = camera.state()
    a = 1.3 * 2.0 * math.tan(camera.fov / 2.0) / h
    d = np.asarray(st["dir"], np.float64)
    st["dir"] = [d[0] * math.cos(a) - d[2] * math.sin(a), d[1], d[0] * math.sin(a) + d[2] * math.cos(a)]
    views = {"static": previous_view(camera), "moved": previous_view(Camera.from_state(st))}
    cam = camera.c_struct()
    n = w * h
    with capi.DeviceScene(fs, 0) as ds:
        def timed(fn, calls):
            ea, eb = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            ea.record()
            for _ in range(calls):
                fn()
            eb.record()
            eb.synchronize()
            return ea.elapsed_time(eb) / calls

        frames = [renderer.render_pixel_parts_torch(ds, cam, make_config(samples=samples, monte_carlo=True, seed=s, max_recursion=4), None, 2) for s in (1, 2)]
        hist = renderer.accumulate_torch(ds, cam, frames[0]["records"], frames[0]["part_records"])
        torch.cuda.synchronize()
        rec, halves = frames[1]["records"], frames[1]["part_records"]
        out, out_h = torch.empty_like(rec), torch.empty_like(halves)
        length = torch.empty((n,), dtype=torch.float32, device="cuda")
        rgba = torch.empty((n, 4), dtype=torch.uint8, device="cuda")
        stream = torch.cuda.current_stream().cuda_stream

        def call(use_halves, view, first=False):
            prm = capi.accumulate_params(AccumulateParams(prev_world_to_clip=views[view][0], prev_eye=views[view][1]))
            p = lambda t, on=True: t.data_ptr() if on else None
            return lambda: ds.accumulate_records_device(cam, rec.data_ptr(), p(halves, use_halves), p(hist["records"], not first), p(hist["halves"], use_halves and not first),
                                                        p(hist["length"], not first), None, out.data_ptr(), p(out_h, use_halves), length.data_ptr(), None, prm, stream)

        dprm = capi.denoise_default_params()
        arms = {(hv, view): call(hv, view) for hv in (True, False) for view in ("static", "moved")}
        arms[(True, "first frame")] = call(True, "static", first=True)
        arms["denoise"] = lambda: ds.denoise_records_device(w, h, rec.data_ptr(), halves.data_ptr(), None, out.data_ptr(), rgba.data_ptr(), None, dprm, stream)
        if with_motion:
            from tests.helpers import item_transforms
            prev_trans = item_transforms(fs, dx=0.05)[0]
            motion, world = torch.empty((n, 3), dtype=torch.float32, device="cuda"), torch.empty((n, 3), dtype=torch.float32, device="cuda")
            index = np.arange(len(fs.items), dtype=np.uint32)

            def motion_call(k, with_world):
                return lambda: ds.motion_records_device(cam, index[:k], prev_trans[:k], rec.data_ptr(), motion.data_ptr(), world.data_ptr() if with_world else None, stream)
            for k in (len(fs.items), 1):
                for with_world in (False, True):
                    arms[("motion", k, with_world)] = motion_call(k, with_world)
        if with_split:
            cfgs = [make_config(samples=samples, monte_carlo=True, seed=s, max_recursion=4) for s in (1, 2)]
            sf = [renderer.render_pixel_split_torch(ds, cam, c, None, True) for c in cfgs]
            sh = renderer.accumulate_split_torch(ds, cam, sf[0]["records"], sf[0]["part_records"], sf[0]["diffuse"], sf[0]["diffuse_halves"])
            torch.cuda.synchronize()
            s_out = {k: torch.empty_like(sh[k]) for k in ("records", "halves", "diffuse", "diffuse_halves", "length")}

            def split_call(view):
                prm = capi.accumulate_params(AccumulateParams(prev_world_to_clip=views[view][0], prev_eye=views[view][1]))
                cur = [sf[1][k].data_ptr() for k in ("records", "part_records", "diffuse", "diffuse_halves")]
                old = [sh[k].data_ptr() for k in ("records", "halves", "diffuse", "diffuse_halves", "length")]
                new = [s_out[k].data_ptr() for k in ("records", "halves", "diffuse", "diffuse_halves", "length")]
                return lambda: ds.accumulate_split_device(cam, *cur, *old, None, *new, None, prm, stream)
            for view in ("static", "moved"):
                arms[("split", view)] = split_call(view)
        if with_clamp:
            from rustray_amd.temporal import HistoryClampParams
            c_out, c_out_h = torch.empty_like(rec), torch.empty_like(halves)

            def clamp_call(view, radius):
                prm = capi.accumulate_params(AccumulateParams(prev_world_to_clip=views[view][0], prev_eye=views[view][1]))
                clamp = capi.history_clamp_params(HistoryClampParams(radius, 1.0))
                return lambda: ds.accumulate_clamped_device(cam, rec.data_ptr(), halves.data_ptr(), hist["records"].data_ptr(), hist["halves"].data_ptr(),
                                                            hist["length"].data_ptr(), None, c_out.data_ptr(), c_out_h.data_ptr(), length.data_ptr(), None, prm, clamp, stream)
            for view in ("static", "moved"):
                for radius in (1, 2):
                    arms[("clamp", view, radius)] = clamp_call(view, radius)
        if with_clamp_split:
            cs_out = {k: torch.empty_like(sh[k]) for k in ("records", "halves", "diffuse", "diffuse_halves", "length")}

            def clamp_split_call(view, radius):
                prm = capi.accumulate_params(AccumulateParams(prev_world_to_clip=views[view][0], prev_eye=views[view][1]))
                clamp = capi.history_clamp_params(HistoryClampParams(radius, 1.0))
                cur = [sf[1][k].data_ptr() for k in ("records", "part_records", "diffuse", "diffuse_halves")]
                old = [sh[k].data_ptr() for k in ("records", "halves", "diffuse", "diffuse_halves", "length")]
                new = [cs_out[k].data_ptr() for k in ("records", "halves", "diffuse", "diffuse_halves", "length")]
                return lambda: ds.accumulate_clamped_split_device(cam, *cur, *old, None, *new, None, prm, clamp, stream)
            for view in ("static", "moved"):
                for radius in (1, 2):
                    arms[("clamp_split", view, radius)] = clamp_split_call(view, radius)
        runs = {k: [] for k in arms}
        for r in range(WARMUP + ROUNDS):
            for k, fn in arms.items():
                t = timed(fn, CALLS)
                if r >= WARMUP:
                    runs[k].append(t)
        kept = {}
        for view in ("static", "moved"):
            arms[(True, view)]()
            torch.cuda.synchronize()
            kept[view] = float((length > 1).float().mean().item())

    emit(f"rr_accumulate_records_device, {scene} {w}x{h}, {samples} samples in two halves; device ms per call, median of {ROUNDS} rounds of {CALLS} calls [min .. max]")
    for k, v in runs.items():
        m, lo, hi = _median(v)
        if k == "denoise":
            emit(f"  rr_denoise_records_device, 5 iterations, with halves, rgba8_out, same rounds: {m:.4f} ms [{lo:.4f} .. {hi:.4f}]")
            continue
        if k[0] == "split":
            per_pixel = BYTES_PER_PIXEL[True] + 108
            floor_ms = n * per_pixel / HBM_BYTES_PER_S * 1e3
            bm, blo, bhi = _median(runs[(True, k[1])])
            apart = "outside" if hi < 2 * blo else "NOT outside"
            emit(f"  rr_accumulate_split_records_device, with halves, {k[1]}: {m:.4f} ms [{lo:.4f} .. {hi:.4f}] = {floor_ms / m:.2f} of the rate of its compulsory "
                 f"traffic ({per_pixel} B per pixel, {floor_ms * 1e3:.1f} us), {m / bm:.2f} x rr_accumulate_records_device with halves, {k[1]}; the bar, two "
                 f"such calls: {2 * bm:.4f} ms [{2 * blo:.4f} .. {2 * bhi:.4f}], {'met' if m < 2 * bm else 'MISSED'}, {apart} the arms' ranges")
            continue
        if k[0] == "clamp":
            per_pixel = BYTES_PER_PIXEL[True]
            floor_ms = n * per_pixel / HBM_BYTES_PER_S * 1e3
            bm, blo, bhi = _median(runs[(True, k[1])])
            emit(f"  rr_accumulate_clamped_records_device, with halves, {k[1]}, radius {k[2]}: {m:.4f} ms [{lo:.4f} .. {hi:.4f}] = {floor_ms / m:.2f} of the rate of its "
                 f"compulsory traffic ({per_pixel} B per pixel, {floor_ms * 1e3:.1f} us), {m / bm:.2f} x rr_accumulate_records_device with halves, {k[1]} "
                 f"({bm:.4f} ms [{blo:.4f} .. {bhi:.4f}])")
            continue
        if k[0] == "clamp_split":
            per_pixel = BYTES_PER_PIXEL[True] + 108
            floor_ms = n * per_pixel / HBM_BYTES_PER_S * 1e3
            (sm, slo, shi), (cm, clo, chi) = _median(runs[("split", k[1])]), _median(runs[("clamp", k[1], k[2])])
            apart = "outside" if hi < slo + clo else "NOT outside"
            emit(f"  rr_accumulate_clamped_split_records_device, with halves, {k[1]}, radius {k[2]}: {m:.4f} ms [{lo:.4f} .. {hi:.4f}] = {floor_ms / m:.2f} of the rate "
                 f"of its compulsory traffic ({per_pixel} B per pixel, {floor_ms * 1e3:.1f} us), {m / sm:.2f} x the split call, {m / cm:.2f} x the clamped call; the "
                 f"bar, the sum of the two: {sm + cm:.4f} ms [{slo + clo:.4f} .. {shi + chi:.4f}], {'met' if m < sm + cm else 'MISSED'}, {apart} the arms' ranges")
            continue
        if k[0] == "motion":
            per_pixel = 44 + (12 if k[2] else 0)
            floor_ms = n * per_pixel / HBM_BYTES_PER_S * 1e3
            base = _median(runs[(True, "static")])[0]
            emit(f"  rr_motion_records_device, {k[1]} of {len(fs.items)} items moved, {'with' if k[2] else 'without'} world_out: {m:.4f} ms [{lo:.4f} .. {hi:.4f}] = {floor_ms / m:.2f} of the "
                 f"rate of its compulsory traffic ({per_pixel} B per pixel, {floor_ms * 1e3:.1f} us), {m / base:.2f} x the static accumulation with halves")
            continue
        hv, view = k
        per_pixel = BYTES_PER_PIXEL[hv] - (100 if view == "first frame" else 0)      # (no history is read)
        floor_ms = n * per_pixel / HBM_BYTES_PER_S * 1e3
        share = f", {kept[view]:.3f} of the pixels kept history" if view in kept and hv else ""
        emit(f"  {'with' if hv else 'without'} halves, {view}: {m:.4f} ms [{lo:.4f} .. {hi:.4f}] = {floor_ms / m:.2f} of the rate of its compulsory traffic "
             f"({per_pixel} B per pixel, {floor_ms * 1e3:.1f} us at {HBM_BYTES_PER_S / 1e12:.2f} TB/s){share}")
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "a") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main(list(sys.argv))
