#!/usr/bin/env python3
"""Developer probe: the measurements behind rr_history_clamp_default_params.

The protocol is tests/test_gpu_temporal_clamp.py: light_edit_run -- spheres_room at 50x38, a static camera, eight frames of 4 samples, the
lights edited before frame 5, RMSE of the accumulated records over the surface pixels against 512-sample truth under the lights of that
frame -- for radius 1, 2 x sigma_scale 0.5, 1, 1.5, 2, 3 and the unclamped arm, over the seed sets 100.., 200.., 300..; the same frames
without the edit (the static cost at frame 8 and the spread of the unclamped arm between the seed sets); and a LONG static run of
LONG_FRAMES frames, past max_history = 32, where the unclamped arm keeps converging and a clamp that holds the length down cannot.

--split: the split arm instead: the same protocol through Raytracing.render_temporal_split (unclamped),
Raytracing.render_temporal_split_clamped for the same radius x sigma_scale grid and, beside them, Raytracing.render_temporal(clamp=True);
summed RMSE over the eight frames with the edit, the static cost at frame 8, and for the split arms the RMSE of the rest, accumulated
colour - accumulated diffuse against the 512-sample colour - diffuse, alone: what clamping colour and diffuse independently does to it.

usage: temporal_clamp_quality.py [--split] [--out FILE]"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

LONG_FRAMES = 40
LONG_AT = (8, 16, 24, 32, 40)


def split_edit_run(seed0, arms, edit=True):
    """light_edit_run of tests/test_gpu_temporal_clamp.py for the split pipelines: one arm per entry of `arms`, ("split", None) for
    render_temporal_split, ("split", clamp) for render_temporal_split_clamped, ("plain", clamp) for render_temporal(clamp=clamp).
    -> dict(truth_old, truth_new: dict(colour, rest) (n, 3) float64 at 512 samples, surface (n,) bool, frames: per arm a list of eight
    dict(accumulated (n, 3), rest (n, 3) or None, length (n,)))."""
    import torch
    from rustray_amd.renderer import Raytracing, TemporalState, _pack_records
    from tests.helpers import camera_for
    from tests.test_gpu_pixel_parts import _cfg
    from tests.test_gpu_shade_rays import _scene
    from tests.test_gpu_temporal_clamp import EDIT_AT, FRAMES, H3, W3, _edited
    fs = _scene("spheres_room")
    rt = Raytracing(fs, camera_for(fs, W3, H3), 0)

    def truth():
        rt.config = _cfg("plain", samples=512)
        base = rt.render_pixel_split()
        colour = _pack_records(base)[:, 0:3].astype(np.float64)
        rt.config = _cfg("plain", samples=4)
        return dict(colour=colour, rest=colour - base["diffuse"].astype(np.float64))
    try:
        truth_old = truth_new = truth()
        states = [TemporalState() for _ in arms]
        frames = [[] for _ in arms]
        for k in range(FRAMES):
            if edit and k == EDIT_AT:
                assert rt.apply_scene(_edited(_scene("spheres_room"))) == ["update_lights"]
                truth_new = truth()
            for ai, ((kind, clamp), state) in enumerate(zip(arms, states)):
                if kind == "plain":
                    got = rt.render_temporal(state, samples=4, seed=seed0 + k, clamp=clamp)
                elif clamp is None:
                    got = rt.render_temporal_split(state, samples=4, seed=seed0 + k)
                else:
                    got = rt.render_temporal_split_clamped(state, samples=4, seed=seed0 + k, clamp=clamp)
                torch.cuda.synchronize()
                acc = got["accumulated"].cpu().numpy()[:, 0:3].astype(np.float64)
                rest = acc - got["accumulated_diffuse"].cpu().numpy().astype(np.float64) if kind == "split" else None
                frames[ai].append(dict(accumulated=acc, rest=rest, length=got["length"].cpu().numpy()))
                if k == 0 and ai == 0:
                    rec = got["noisy"].cpu().numpy()
                    surface = np.isfinite(rec[:, 0:3]).all(-1) & np.isfinite(rec[:, 3]) & np.isfinite(rec[:, 4:7]).all(-1)
        return dict(truth_old=truth_old, truth_new=truth_new, surface=surface, frames=frames)
    finally:
        rt.device_scene.close()


def split_main(emit):
    from rustray_amd.temporal import HistoryClampParams
    from tests.test_gpu_temporal_clamp import EDIT_AT, FRAMES
    pairs = [(r, k) for r in (1, 2) for k in (0.5, 1.0, 1.5, 2.0, 3.0)]
    arms = [("split", None)] + [("split", HistoryClampParams(r, k)) for r, k in pairs] + [("plain", True)]
    names = ["split unclamped"] + [f"split r={r} k={k}" for r, k in pairs] + ["plain clamp=True"]
    seeds = (100, 200, 300)
    err = lambda a, b, surf: float(np.sqrt(((a[surf] - b[surf]) ** 2).mean()))
    emit("light edit before frame 5, the split pipelines: spheres_room 50x38, static camera, 8 frames of 4 samples; RMSE of the accumulated records over "
         "surface pixels against 512-sample truth (old lights frames 1-4, new lights frames 5-8); rest = colour - diffuse")
    total, rest_total, static8, static8_rest = (np.zeros((len(arms), len(seeds))) for _ in range(4))
    for si, s0 in enumerate(seeds):
        run = split_edit_run(s0, arms)
        surf = run["surface"]
        for ai, name in enumerate(names):
            fr = run["frames"][ai]
            truth = lambda k: run["truth_new"] if k >= EDIT_AT else run["truth_old"]
            r = [err(fr[k]["accumulated"], truth(k)["colour"], surf) for k in range(FRAMES)]
            total[ai, si] = sum(r)
            line = f"seeds {s0}.. {name:18s} rmse " + " ".join(f"{x:.5f}" for x in r) + f" | sum {sum(r):.5f}"
            if fr[0]["rest"] is not None:
                q = [err(fr[k]["rest"], truth(k)["rest"], surf) for k in range(FRAMES)]
                rest_total[ai, si] = sum(q)
                line += " | rest rmse " + " ".join(f"{x:.5f}" for x in q) + f" | sum {sum(q):.5f}"
            emit(line + " | mean length " + " ".join(f"{float(fr[k]['length'][surf].mean()):.2f}" for k in range(FRAMES)))
        still = split_edit_run(s0, arms, edit=False)
        for ai in range(len(arms)):
            static8[ai, si] = err(still["frames"][ai][-1]["accumulated"], still["truth_old"]["colour"], surf)
            if arms[ai][0] == "split":
                static8_rest[ai, si] = err(still["frames"][ai][-1]["rest"], still["truth_old"]["rest"], surf)
        emit(f"seeds {s0}.. static view, frame 8 rmse: " + "; ".join(f"{n} {static8[ai, si]:.5f}" for ai, n in enumerate(names)))
        emit(f"seeds {s0}.. static view, frame 8 rmse of the rest: " + "; ".join(f"{n} {static8_rest[ai, si]:.5f}" for ai, n in enumerate(names) if arms[ai][0] == "split"))
    emit("summed RMSE over the eight frames, mean of the three seed sets [min .. max]; the rest alone; static frame 8:")
    for ai, name in enumerate(names):
        rest = f"rest {rest_total[ai].mean():.5f} [{rest_total[ai].min():.5f} .. {rest_total[ai].max():.5f}]" if arms[ai][0] == "split" else "rest -"
        emit(f"  {name:18s} {total[ai].mean():.5f} [{total[ai].min():.5f} .. {total[ai].max():.5f}]   {rest}   static frame 8: {static8[ai].mean():.5f} "
             f"[{static8[ai].min():.5f} .. {static8[ai].max():.5f}], largest excess over split unclamped {float((static8[ai] - static8[0]).max()):.5f}"
             + (f"; of the rest {static8_rest[ai].mean():.5f} [{static8_rest[ai].min():.5f} .. {static8_rest[ai].max():.5f}]" if arms[ai][0] == "split" else ""))
    spread = float(static8[0].max() - static8[0].min())
    emit(f"split unclamped static frame 8: largest difference between the seed sets {spread:.6f}; 3 x = {3 * spread:.6f}")
    emit(f"smallest summed RMSE of the split arms: {names[int(np.argmin(total[1:-1].mean(1))) + 1]}")


def main(argv):
    import torch  # noqa: F401  (before the library, as tools/temporal_time.py: torch brings its own HIP runtime)
    from rustray_amd import capi
    from rustray_amd.temporal import HistoryClampParams
    from tests.test_gpu_temporal_clamp import EDIT_AT, FRAMES, light_edit_run, rmse
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    out_path = argv[argv.index("--out") + 1] if "--out" in argv else None
    if capi.device_count() < 1:
        raise SystemExit("temporal_clamp_quality.py needs a GPU: no HIP device visible")
    if "--split" in argv:
        split_main(emit)
        if out_path:
            os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
            with open(out_path, "w") as fh:
                fh.write("\n".join(lines) + "\n")
        return
    pairs = [(r, k) for r in (1, 2) for k in (0.5, 1.0, 1.5, 2.0, 3.0)]
    arms = [None] + [HistoryClampParams(r, k) for r, k in pairs]
    names = ["unclamped"] + [f"r={r} k={k}" for r, k in pairs]
    seeds = (100, 200, 300)
    emit("light edit before frame 5: spheres_room 50x38, static camera, 8 frames of 4 samples; RMSE of the accumulated records over surface pixels "
         "against 512-sample truth (old lights frames 1-4, new lights frames 5-8)")
    total, static8 = np.zeros((len(arms), len(seeds))), np.zeros((len(arms), len(seeds)))
    for si, s0 in enumerate(seeds):
        run = light_edit_run(s0, arms)
        surf = run["surface"]
        for ai, name in enumerate(names):
            r = [rmse(run["frames"][ai][k], run["truth_new"] if k >= EDIT_AT else run["truth_old"], surf) for k in range(FRAMES)]
            ln = [float(run["frames"][ai][k]["length"][surf].mean()) for k in range(FRAMES)]
            total[ai, si] = sum(r)
            emit(f"seeds {s0}.. {name:12s} rmse " + " ".join(f"{x:.5f}" for x in r) + f" | sum {sum(r):.5f} | mean length " + " ".join(f"{x:.2f}" for x in ln))
        still = light_edit_run(s0, arms, edit=False)
        for ai in range(len(arms)):
            static8[ai, si] = rmse(still["frames"][ai][-1], still["truth_old"], surf)
        emit(f"seeds {s0}.. static view, frame 8 rmse: " + "; ".join(f"{n} {static8[ai, si]:.5f}" for ai, n in enumerate(names)))
    emit("summed RMSE over the eight frames, mean of the three seed sets [min .. max]:")
    for ai, name in enumerate(names):
        emit(f"  {name:12s} {total[ai].mean():.5f} [{total[ai].min():.5f} .. {total[ai].max():.5f}]   static frame 8: {static8[ai].mean():.5f} "
             f"[{static8[ai].min():.5f} .. {static8[ai].max():.5f}], largest excess over unclamped {float((static8[ai] - static8[0]).max()):.5f}")
    spread = float(static8[0].max() - static8[0].min())
    emit(f"unclamped static frame 8: largest difference between the seed sets {spread:.6f}; 3 x = {3 * spread:.6f}")
    emit(f"smallest summed RMSE: {names[int(np.argmin(total[1:].mean(1))) + 1]}")

    long_arms = [None, True] + [HistoryClampParams(1, k) for k in (1.0, 2.0, 3.0)]
    long_names = ["unclamped", "defaults"] + [f"r=1 k={k}" for k in (1.0, 2.0, 3.0)]
    emit(f"long static view: the same scene and camera, {LONG_FRAMES} frames of 4 samples, no edit; RMSE against 512-sample truth / mean length over "
         f"surface pixels at frames {', '.join(map(str, LONG_AT))}")
    for s0 in seeds:
        run = light_edit_run(s0, long_arms, edit=False, frames=LONG_FRAMES)
        surf = run["surface"]
        for ai, name in enumerate(long_names):
            emit(f"seeds {s0}.. {name:10s} " + "  ".join(f"{rmse(run['frames'][ai][k - 1], run['truth_old'], surf):.5f} / {float(run['frames'][ai][k - 1]['length'][surf].mean()):5.2f}"
                                                       for k in LONG_AT))
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main(list(sys.argv))
