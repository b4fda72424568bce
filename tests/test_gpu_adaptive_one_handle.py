"""The pixel queries and the fused adaptive calls interleaved on ONE handle.  The host forms of the list calls share one staging path and
the fused calls another, all of them in the same buffers of the handle; the lists share one scratch carve, one pinned word for their
lengths and two list buffers; the statistics of every fused call go through one pass-sum helper.  Here each call runs between calls of the
other families, and then again on a frame smaller than the buffers the handle holds by then: every result must be, bit for bit in every
field, what the same call gives as the first call of a fresh handle, and so must the primary rays the handle reports after it.
spheres_room, 50 x 38, the "plain" config, ladder 6, 14, 30, ADAPTIVE_THRESHOLD: the setting of tests/test_gpu_adaptive_levels.py."""
import numpy as np
import pytest

from tests.helpers import camera_for
from tests.test_gpu_adaptive_levels import LEVELS
from tests.test_gpu_pixel_parts import ADAPTIVE_THRESHOLD, H, N, W, _bits, _cfg
from tests.test_gpu_shade_rays import _scene

pytestmark = pytest.mark.gpu

SMALL_W, SMALL_H = 21, 13      # partial 8x8 blocks in both directions, fewer pixels than any buffer the calls before it left behind


def _steps(fs):
    """(name, call) in the order they run on the one handle; every call takes the handle and returns its result dict."""
    cam, small = camera_for(fs, W, H).c_struct(), camera_for(fs, SMALL_W, SMALL_H).c_struct()
    any_samples, whole = _cfg("plain", samples=1), _cfg("plain", samples=LEVELS[-1])   # (the levels calls ignore config->samples; a prefix ladder ends at it)
    idx = (np.arange(65, dtype=np.uint32) * np.uint32(29)) % np.uint32(N)               # 65 pixels: one more than a packet, in no screen order
    list65 = (idx % np.uint32(W)) | ((idx // np.uint32(W)) << np.uint32(16))
    one = np.array([7 | (31 << 16)], np.uint32)

    def fused(c, tag):
        return [
            (f"adaptive_prefix{tag}", lambda ds: ds.render_adaptive_prefix(c, whole, LEVELS, ADAPTIVE_THRESHOLD, rgba8=True)),
            (f"adaptive_levels{tag}", lambda ds: ds.render_adaptive_levels(c, any_samples, LEVELS, ADAPTIVE_THRESHOLD, rgba8=True)),
            (f"adaptive{tag}", lambda ds: ds.render_adaptive(c, any_samples, LEVELS[0], LEVELS[-1], ADAPTIVE_THRESHOLD, rgba8=True)),
        ]
    prefix, levels, two = fused(cam, "")
    return [
        prefix,
        ("pixels_65", lambda ds: ds.render_pixels(cam, _cfg("plain"), list65, rgba8=True)),
        levels,
        ("pixel_prefix_halves", lambda ds: ds.render_pixel_prefix(cam, whole, None, samples_used=LEVELS[1], halves=True, rgba8=True)),
        two,
        ("pixel_parts_1", lambda ds: ds.render_pixel_parts(cam, _cfg("plain"), one, n_parts=2)),
        ("adaptive_prefix_again", prefix[1]),
    ] + fused(small, "_small")


def _same(got, want, what):
    assert type(got) is type(want), what
    if isinstance(want, dict):
        assert list(got) == list(want), what
        for k in want:
            _same(got[k], want[k], f"{what}.{k}")
    elif isinstance(want, np.ndarray):
        assert got.shape == want.shape and got.dtype == want.dtype, what
        assert np.array_equal(_bits(got), _bits(want)), f"{what} differs in {int((_bits(got) != _bits(want)).sum())} words"
    else:
        assert got == want, (what, got, want)


def test_interleaved_calls_on_one_handle_equal_fresh_handles(hip):
    fs = _scene("spheres_room")
    steps = _steps(fs)
    want = {}
    for name, call in steps:                       # each call as the first call of a handle of its own
        with hip.DeviceScene(fs, 0) as fresh:
            want[name] = (call(fresh), fresh.stats()["primary_rays"])
    for name in ("adaptive_prefix", "adaptive_levels"):      # the lists shrink and none is empty: every level's pass, list and scatter ran
        n0, n1, n2 = want[name][0]["level_pixels"]
        print(name, "level_pixels", [n0, n1, n2], "small", want[name + "_small"][0]["level_pixels"])
        assert N == n0 > n1 > n2 > 0, (name, n0, n1, n2)
        assert want[name + "_small"][0]["level_pixels"][0] == SMALL_W * SMALL_H
    assert 0 < want["adaptive"][0]["n_refined"] < N
    assert want["adaptive_prefix"][0]["rgba"].any() and want["pixels_65"][0]["rgba"].shape == (65, 4)
    with hip.DeviceScene(fs, 0) as ds:
        for name, call in steps:
            got = call(ds)
            _same(got, want[name][0], name)
            assert ds.stats()["primary_rays"] == want[name][1], name
