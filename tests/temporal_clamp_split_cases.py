"""Hand-made split frames and histories for the tests of rr_accumulate_clamped_split_records (tests/test_temporal_clamp_split_host.py,
tests/test_gpu_temporal_clamp_split.py, tests/test_gpu_temporal_clamp_split_cpp.py): the inputs only, made once per size and never changed
by a test."""
import functools

import numpy as np

from tests.denoise_cases import F
from tests.temporal_cases import _freeze
from tests.temporal_clamp_cases import clamp_frame_odd, own_colour_frame
from tests.temporal_split_cases import _fractions, split_frame, split_frame_odd

KEYS = ("records", "halves", "diffuse", "diffuse_halves", "history", "history_halves", "history_diffuse", "history_diffuse_halves", "history_length", "motion")


def clamp_split_frame(W: int, H: int):
    """temporal_split_cases.split_frame(W, H) as it stands: the colours of temporal_frame in patches with NaN and inf among them, diffuse =
    colour * u with u per pixel and layer in [0.1, 0.9], under a history of other colours and other fractions -- at sigma_scale 1 the
    record layer and the diffuse layer each leave their box in a good part of the kept pixels, and not in the same ones."""
    return split_frame(W, H)


@functools.lru_cache(maxsize=None)
def clamp_split_frame_odd(W: int, H: int):
    """clamp_frame_odd(W, H)'s colours (the flat patch, the 1e30 and 5e19 channels, the 3e38 pairs) with diffuse = colour * u in the pixels it
    changed (split_frame's own u), so a flat patch of colours is not flat in diffuse and the huge colours are huge diffuse values, some of
    which overflow when squared and some of which do not; everywhere else split_frame_odd(W, H)'s diffuse layers with their spoiled
    triples (NaN or inf in one channel or in all three where the colour is finite), current and history.  Halves, history, lengths,
    motion and the views are temporal_frame's."""
    base, clean, odd = clamp_frame_odd(W, H), split_frame(W, H), split_frame_odd(W, H)
    n = W * H
    case = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in odd.items()}
    case["records"] = base["records"].copy()
    changed = (base["records"][:, 0:3].view(np.uint32) != clean["records"][:, 0:3].view(np.uint32)).any(-1)
    u = _fractions(np.random.default_rng(23), n)          # (split_frame's first draw: the fractions of its current layers)
    with np.errstate(all="ignore"):
        case["diffuse"][changed] = (base["records"][changed, 0:3] * u[changed, 0:1]).astype(F)
    return _freeze(case)


@functools.lru_cache(maxsize=None)
def own_colour_split_frame(W: int, H: int):
    """temporal_clamp_cases.own_colour_frame(W, H) with its diffuse layers: diffuse = colour * u, u per pixel in [0.1, 0.9]; both diffuse
    halves hold the pixel's diffuse; the history is the frame itself in every layer.  Every kept pixel snaps to itself, so the history
    mean of every layer, colour or diffuse, is a member of the window its box is made from.  -> (case dict, AccumulateParams)."""
    base, prm = own_colour_frame(W, H)
    case = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in base.items()}
    u = _fractions(np.random.default_rng(37), W * H)
    with np.errstate(all="ignore"):
        case["diffuse"] = (base["records"][:, 0:3] * u[:, 0:1]).astype(F)
    case["diffuse_halves"] = np.ascontiguousarray(np.repeat(case["diffuse"][:, None, :], 2, axis=1))
    case["history_diffuse"] = case["diffuse"].copy()
    case["history_diffuse_halves"] = case["diffuse_halves"].copy()
    return _freeze(case), prm


KINDS = {"clean": clamp_split_frame, "odd": clamp_split_frame_odd}


def inputs(case, use_halves: bool, use_motion: bool, first: bool):
    """the ten array arguments of accumulate_clamped_split_records, in its order (KEYS)"""
    cur = lambda k, on=True: case[k] if on else None
    hist = lambda k, on=True: case[k] if on and not first else None
    return (case["records"], cur("halves", use_halves), case["diffuse"], cur("diffuse_halves", use_halves), hist("history"), hist("history_halves", use_halves),
            hist("history_diffuse"), hist("history_diffuse_halves", use_halves), hist("history_length"), case["motion"] if use_motion else None)


def colour_inputs(args):
    """of inputs(...): the six array arguments of accumulate_clamped_records, in its order"""
    a = dict(zip(KEYS, args))
    return tuple(a[k] for k in ("records", "halves", "history", "history_halves", "history_length", "motion"))
