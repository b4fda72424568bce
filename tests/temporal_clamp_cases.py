"""Hand-made frames and histories for the tests of rr_accumulate_clamped_records (tests/test_temporal_clamp_host.py,
tests/test_gpu_temporal_clamp.py): the inputs only, made once per size and never changed by a test."""
import functools

import numpy as np

from rustray_amd.temporal import AccumulateParams
from tests.denoise_cases import F
from tests.temporal_cases import _freeze, static_view, temporal_frame

KEYS = ("records", "halves", "history", "history_halves", "history_length", "motion")


def clamp_frame(W: int, H: int):
    """temporal_cases.temporal_frame(W, H) as it stands: colours in patches with NaN and inf among them, so windows with fewer than
    (2r + 1)^2 taken pixels, under a history of other colours -- at sigma_scale 1 about half of the kept pixels leave their box."""
    return temporal_frame(W, H)


@functools.lru_cache(maxsize=None)
def clamp_frame_odd(W: int, H: int):
    """temporal_frame(W, H) with current colours that strain the box: a flat patch of up to 7x7 pixels right of the middle (sd = 0 inside it: the box
    is a point and e = 0), about 1 % of the pixels with one channel at 1e30 (its square and the square of every window mean that holds it
    overflow: s2 / m = inf and mean * mean = inf, v = inf - inf), about 1 % with one channel at 5e19 (its square overflows, the square of a
    window's mean does not: s2 / m = inf, v = inf) and about 0.5 % of the pixels, each with its right neighbour, at 3e38 in all channels
    (their sum overflows: s1 = inf, the mean is infinite).  By the header's rule every such channel of every window that holds one of
    them has no box.  Halves, history, lengths, motion and the views are temporal_frame's."""
    case = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in temporal_frame(W, H).items()}
    rng = np.random.default_rng(31)
    n = W * H
    col = case["records"].reshape(H, W, 8)
    y0, x0 = max(0, H // 2 - 3), min(W // 2 + 2, max(0, W - 7))          # (near the middle, where pixels keep their history)
    col[y0:y0 + 7, x0:x0 + 7, 0:3] = np.array([0.25, 0.5, 0.75], F)
    flat = case["records"]
    y, x = np.arange(n) // W, np.arange(n) % W
    finite = np.isfinite(flat[:, 0:3]).all(-1) & ~((y >= y0 - 2) & (y < y0 + 9) & (x >= x0 - 2) & (x < x0 + 9))      # (the huge colours stay two pixels clear of the flat patch)
    at = np.flatnonzero((rng.random(n) < 0.01) & finite)
    flat[at, rng.integers(0, 3, len(at))] = F(1e30)
    at = np.flatnonzero((rng.random(n) < 0.01) & finite)
    flat[at, rng.integers(0, 3, len(at))] = F(5e19)
    pair = np.flatnonzero((rng.random(n) < 0.005) & finite & (np.arange(n) % W < W - 1))
    for p in pair:
        if finite[p + 1]:
            flat[p, 0:3] = flat[p + 1, 0:3] = F(3e38)
    return _freeze(case)


@functools.lru_cache(maxsize=None)
def own_colour_frame(W: int, H: int):
    """A frame whose history holds the current frame's own colours, under the camera's own view, and whose halves hold the colour of their
    record: every kept pixel snaps to itself, so the history mean of every layer is the pixel's current colour, a member of its window.
    -> (case dict, AccumulateParams of the static view).  History depth, normal and id are the current record's, so nearly every valid
    pixel keeps its history."""
    base = temporal_frame(W, H)
    case = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in base.items()}
    case["halves"][:, :, 0:3] = base["records"][:, None, 0:3]
    case["history"] = base["records"].copy()
    case["history_halves"] = case["halves"].copy()
    case["motion"] = np.zeros_like(base["motion"])
    m, eye = static_view(base["cam"])
    case["prev_world_to_clip"], case["prev_eye"] = m, eye
    return _freeze(case), AccumulateParams(prev_world_to_clip=m, prev_eye=eye)


KINDS = {"clean": clamp_frame, "odd": clamp_frame_odd}


def inputs(case, use_halves: bool, use_motion: bool, first: bool):
    """the six array arguments of accumulate_clamped_records, in its order"""
    hist = lambda k, on=True: case[k] if on and not first else None
    return (case["records"], case["halves"] if use_halves else None, hist("history"), hist("history_halves", use_halves), hist("history_length"),
            case["motion"] if use_motion else None)
