#!/usr/bin/env python3
"""Developer probe: the measurements behind rr_history_clamp_default_params.

The protocol is tests/test_gpu_temporal_clamp.py: light_edit_run -- spheres_room at 50x38, a static camera, eight frames of 4 samples, the
lights edited before frame 5, RMSE of the accumulated records over the surface pixels against 512-sample truth under the lights of that
frame -- for radius 1, 2 x sigma_scale 0.5, 1, 1.5, 2, 3 and the unclamped arm, over the seed sets 100.., 200.., 300..; the same frames
without the edit (the static cost at frame 8 and the spread of the unclamped arm between the seed sets); and a LONG static run of
LONG_FRAMES frames, past max_history = 32, where the unclamped arm keeps converging and a clamp that holds the length down cannot.

usage: temporal_clamp_quality.py [--out FILE]"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

LONG_FRAMES = 40
LONG_AT = (8, 16, 24, 32, 40)


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
