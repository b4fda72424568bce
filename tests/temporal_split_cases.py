"""Hand-made split frames and histories for the tests of rr_accumulate_split_records (tests/test_temporal_split_host.py,
tests/test_gpu_temporal_split.py): the inputs only, made once per size and never changed by a test."""
import functools

import numpy as np

from tests.denoise_cases import F
from tests.temporal_cases import _freeze, static_frames, temporal_frame

ODD_SEED = 1          # (chosen on the CPU: test_the_odd_case_has_what_it_promises holds for it at 33x9, 37x19 and 130x70)


def _fractions(rng, n):
    """u per pixel, layer (diffuse, half 0, half 1) and channel-free, in [0.1, 0.9]"""
    return (F(0.1) + rng.random((n, 3)).astype(F) * F(0.8)).astype(F)


@functools.lru_cache(maxsize=None)
def split_frame(W: int, H: int):
    """temporal_cases.temporal_frame(W, H) plus its diffuse layers: current and history diffuse are colour * u with u per pixel and layer
    in [0.1, 0.9], so a diffuse triple is finite exactly when its colour triple is; the diffuse halves likewise from the halves.
    -> temporal_frame's dict and diffuse (n, 3), diffuse_halves (n, 2, 3), history_diffuse, history_diffuse_halves."""
    case = dict(temporal_frame(W, H))
    n = W * H
    rng = np.random.default_rng(23)
    u, v = _fractions(rng, n), _fractions(rng, n)
    with np.errstate(all="ignore"):
        case["diffuse"] = (case["records"][:, 0:3] * u[:, 0:1]).astype(F)
        case["diffuse_halves"] = np.ascontiguousarray(case["halves"][:, :, 0:3] * u[:, 1:3, None]).astype(F)
        case["history_diffuse"] = (case["history"][:, 0:3] * v[:, 0:1]).astype(F)
        case["history_diffuse_halves"] = np.ascontiguousarray(case["history_halves"][:, :, 0:3] * v[:, 1:3, None]).astype(F)
    return _freeze(case)


@functools.lru_cache(maxsize=None)
def split_frame_odd(W: int, H: int):
    """split_frame(W, H) with finiteness broken on purpose: about 3 % of the history diffuse triples of every layer are NaN or inf (one
    channel, or all three) where the history colour is finite, and about 2 % of the current diffuse triples where the current colour is:
    input rr_render_pixel_split never produces, for the rule that such a layer keeps its current bits while the length goes on."""
    case = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in split_frame(W, H).items()}
    n = W * H
    rng = np.random.default_rng(ODD_SEED)
    bad = np.array([np.nan, np.inf, -np.inf], F)

    def spoil(layer, colour, share):
        at = np.flatnonzero((rng.random(n) < share) & np.isfinite(colour).all(-1))
        layer[at, rng.integers(0, 3, len(at))] = bad[rng.integers(0, 3, len(at))]
        whole = at[rng.random(len(at)) < 0.25]
        layer[whole] = np.nan

    spoil(case["history_diffuse"], case["history"][:, 0:3], 0.03)
    spoil(case["diffuse"], case["records"][:, 0:3], 0.02)
    for h in (0, 1):
        spoil(case["history_diffuse_halves"][:, h], case["history_halves"][:, h, 0:3], 0.03)
        spoil(case["diffuse_halves"][:, h], case["halves"][:, h, 0:3], 0.02)
    return _freeze(case)


@functools.lru_cache(maxsize=None)
def static_split_frames(W: int, H: int, count: int):
    """temporal_cases.static_frames(W, H, count) with diffuse = colour * u, u per frame, pixel and layer in [0.1, 0.9].
    -> (cam, params, records (count, n, 8), halves (count, n, 2, 8), diffuse (count, n, 3), diffuse_halves (count, n, 2, 3))."""
    cam, prm, records, halves = static_frames(W, H, count)
    rng = np.random.default_rng(29)
    n = W * H
    u = np.stack([_fractions(rng, n) for _ in range(count)])
    diffuse = (records[:, :, 0:3] * u[:, :, 0:1]).astype(F)
    diffuse_halves = np.ascontiguousarray(halves[:, :, :, 0:3] * u[:, :, 1:3, None]).astype(F)
    diffuse.setflags(write=False)
    diffuse_halves.setflags(write=False)
    return cam, prm, records, halves, diffuse, diffuse_halves
