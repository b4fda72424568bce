"""Adaptive sampling on the host, from the two interleaved halves of a pixel's samples (rr_render_pixel_parts with n_parts = 2): where is
the frame still noisy, and which pixels deserve more samples.  Pure numpy: no GPU, no library call.

The half-buffer estimate: A and B are the means over the even and the odd samples of a pixel, two independent estimates of the same
integral from S / 2 samples each.  Their mean is the pixel, and |A - B| / 2 estimates the error of that mean; it costs no extra ray."""
from __future__ import annotations

import numpy as np


def half_error(parts_color) -> np.ndarray:
    """parts_color (n, 2, 3): the LINEAR colours of the two halves -> (n,) float32, per pixel max over channels of
    |min(A, 1) - min(B, 1)| / 2.  The clamp is the frame's own (what lies above 1 shows as 1 in both halves).  A pixel with a non-finite
    channel in either half gets error 0: more samples cannot cure a non-finite term."""
    p = np.asarray(parts_color, np.float32)
    if p.ndim != 3 or p.shape[1] != 2 or p.shape[2] != 3:
        raise ValueError(f"parts_color of shape {p.shape}: (n, 2, 3), the two halves of rr_render_pixel_parts with n_parts = 2")
    finite = np.isfinite(p).all(axis=(1, 2))
    q = np.minimum(np.where(finite[:, None, None], p, np.float32(0)), np.float32(1))
    err = (np.abs(q[:, 0, :] - q[:, 1, :]) * np.float32(0.5)).max(axis=1) if len(p) else np.zeros(0, np.float32)
    return np.where(finite, err, np.float32(0)).astype(np.float32)


def refine_list(error, threshold: float, width: int, height: int):
    """error: (width * height,) in row-major order (or (height, width)) -> (pixel list, count): the pixels with error > threshold, packed
    x | y << 16 as rr_render_pixels takes them, ordered as the library orders a whole frame -- 8x8 blocks row-major, row-major inside a
    block -- so that screen neighbours are list neighbours.  The list is padded to a multiple of 64 entries by repeating its last one
    (the call keeps its sample group; duplicates are allowed and give equal records); `count` is the number of entries before the pad."""
    e = np.asarray(error).reshape(int(height), int(width))
    ys, xs = np.nonzero(e > threshold)   # (NaN > threshold is False)
    key = ((ys >> 3) * ((int(width) + 7) >> 3) + (xs >> 3)) * 64 + (ys & 7) * 8 + (xs & 7)
    order = np.argsort(key, kind="stable")
    xy = (xs[order].astype(np.uint32) | (ys[order].astype(np.uint32) << np.uint32(16))).astype(np.uint32)
    count = int(len(xy))
    if count % 64:
        xy = np.concatenate([xy, np.full(64 - count % 64, xy[-1], np.uint32)])
    return np.ascontiguousarray(xy, np.uint32), count


def refine_sublist(error, threshold: float, list_xy, count: int):
    """The list of a list: error (>= count,) the error of entry i of `list_xy` (packed x | y << 16) -> (pixel list, count): the entries
    among the first `count` with error > threshold, in the order they had -- a sub-sequence of a block-ordered list is block-ordered --
    padded to a multiple of 64 entries by repeating its last one, as refine_list pads; an empty result has no pad.  What lies at
    `count` and beyond, the list's own pad, is never taken; duplicates are entries like any other; the coordinates are not interpreted.
    An entry whose error equals the threshold is not taken."""
    count = int(count)
    xy = np.asarray(list_xy, np.uint32).reshape(-1)
    e = np.asarray(error).reshape(-1)
    if count < 0 or count > len(xy) or count > len(e):
        raise ValueError(f"count {count} with {len(xy)} entries and {len(e)} errors")
    out = xy[:count][e[:count].astype(np.float32) > np.float32(threshold)]   # (NaN > threshold is False; the threshold as the library takes it, in binary32)
    taken = int(len(out))
    if taken % 64:
        out = np.concatenate([out, np.full(64 - taken % 64, out[-1], np.uint32)])
    return np.ascontiguousarray(out, np.uint32), taken
