"""tests/native/temporal_pixel_test.cpp for the four host test modules of the accumulation calls: the build line, the input encoding
and the output's layers.  The program is the host loop over rustray_amd/csrc/rr_history_clamp.h: temporal_pixel, the step the kernels
apply per lane, under AddressSanitizer + UBSan, run as its own process."""
import os
import struct
import subprocess

import numpy as np

from tests.denoise_cases import F
from tests.helpers import ROOT

SOURCE = os.path.join(ROOT, "tests", "native", "temporal_pixel_test.cpp")


def build(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("temporal_pixel") / "temporal_pixel_test")
    cmd = ["g++", "-std=c++17", "-O2", "-g", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-o", exe, SOURCE]
    subprocess.check_call(cmd)
    return exe


def run(exe, tmp_path, cam, prm, clamp, split, arrays):
    """arrays: records, halves, [diffuse, diffuse_halves,] history, history_halves, [history_diffuse, history_diffuse_halves,] history_length,
    motion -- the bracketed ones with `split` only; None where the call has none.  clamp: HistoryClampParams or None.
    -> the layers the program wrote: records, length, halves; with split diffuse, diffuse_halves; with clamp lo, hi; with both dlo, dhi."""
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    c = cam.c_struct()
    W, H = int(c.width), int(c.height)
    halves, history, motion = arrays[1], arrays[4 if split else 2], arrays[-1]
    assert len(arrays) == (10 if split else 6)
    with open(src, "wb") as fh:
        fh.write(struct.pack("<7I", W, H, halves is not None, history is not None, motion is not None, bool(split), clamp.radius if clamp else 0))
        fh.write(np.array(c.projection_inverse[:], F).tobytes() + np.array(c.view_inverse[:], F).tobytes())
        fh.write(np.asarray(prm.prev_world_to_clip, F).T.reshape(16).tobytes() + np.asarray(prm.prev_eye, F).tobytes())
        fh.write(struct.pack("<5f", prm.max_history, prm.normal_min, prm.sigma_depth, prm.snap, clamp.sigma_scale if clamp else 0.0))
        for a in arrays:
            if a is not None:
                fh.write(np.ascontiguousarray(a, F).tobytes())
    out = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "temporal pixel test OK" in out.stdout, out.stdout + out.stderr
    raw = np.fromfile(dst, F)
    n = W * H
    hv = halves is not None
    sizes = [("records", 8 * n), ("length", n), ("halves", 16 * n if hv else 0)]
    if split:
        sizes += [("diffuse", 3 * n), ("diffuse_halves", 6 * n if hv else 0)]
    if clamp:
        sizes += [("lo", 3 * n), ("hi", 3 * n)] + ([("dlo", 3 * n), ("dhi", 3 * n)] if split else [])
    assert raw.size == sum(size for _, size in sizes)
    shape = dict(records=(n, 8), length=(n,), halves=(n, 2, 8), diffuse=(n, 3), diffuse_halves=(n, 2, 3), lo=(n, 3), hi=(n, 3), dlo=(n, 3), dhi=(n, 3))
    got, at = {}, 0
    for key, size in sizes:
        got[key] = raw[at:at + size].reshape(shape[key]) if size else None
        at += size
    return got
