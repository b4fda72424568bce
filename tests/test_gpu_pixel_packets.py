"""Level-1 packets of ONE pixel against packets of 64 pixels (run with -m gpu on an MI355X).

With rr_tuning::sample_group 64 a level-1 packet is 64 samples of one pixel: its accumulator adds leave through the plain wave sums of
rr_accumulate.h (one atomic per channel).  With sample_group 1 a packet is one sample of 64 pixels: every add takes the segmented scan,
as it does on all deeper levels.  Integer adds commute, so the two groupings must give the same frame to the bit -- rgba, normal, depth
and object id, and the same ray counts -- at 64 and 128 samples (one and two packets per pixel) and at 4 samples (sixteen pixels per
packet: the control).  Both frames are also held to the oracle's float64 means, so that two equal wrong frames cannot pass.

Scenes, at 32 x 16: lights_scene padded to 17 items (packet form: fixed shadow slots, k_trace_shadow<true>; a third of the frame misses
everything), lights_scene itself (7 items: the dense shadow queue), its lights eight times as bright (colour terms beyond 2: the 64-bit
colour path), spheres_room 200 times larger (root hits beyond 512 units: the wide depth terms), and rr_render_pixel_split on the first."""
import numpy as np
import pytest

from rustray_amd.flat import make_config
from tests.helpers import assert_frames_identical, camera_for, load_scene
from tests.packet_pad import in_packet_range, pad_inert
from tests.test_gpu_corners import _scaled_world
from tests.test_gpu_packet_walk import lights_scene
from tests.test_gpu_parity import assert_parity

pytestmark = pytest.mark.gpu
W, H = 32, 16
COUNTS = ("primary_rays", "secondary_rays", "shaded_hits", "shadow_rays")
SCENES = ("fixed_slots", "dense_queue", "bright", "far")
SAMPLES = (64, 128, 4)


def _scene(name):
    if name == "far":
        return _scaled_world(load_scene("spheres_room"), 200.0)
    fs = lights_scene()
    if name == "bright":
        for l in fs.lights:
            l.intensity = float(l.intensity) * 8.0
    if name != "dense_queue":
        fs = pad_inert(fs, 17, "scattered", seed=17)
    assert in_packet_range(len(fs.items)) == (name in ("fixed_slots", "bright"))
    return fs


def _cfg(samples):
    return make_config(samples=samples, monte_carlo=True, seed=5, max_recursion=3)


def _render(hip, fs, cam, cfg, group):
    with hip.DeviceScene(fs, 0) as ds:
        ds.set_tuning(sample_group=group)
        out = ds.render(cam, cfg)
        st = ds.stats()
    return out, [st[k] for k in COUNTS]


@pytest.mark.parametrize("samples", SAMPLES)
@pytest.mark.parametrize("name", SCENES)
def test_one_pixel_packets_give_the_frame_of_64_pixel_packets(hip, oracle, name, samples):
    fs = _scene(name)
    cam, cfg = camera_for(fs, W, H).c_struct(), _cfg(samples)
    one, n_one = _render(hip, fs, cam, cfg, 64)
    many, n_many = _render(hip, fs, cam, cfg, 1)
    what = f"{name}, {samples} samples"
    assert_frames_identical(one, many, what)
    assert n_one == n_many and n_one[0] == W * H * samples and n_one[3] > 0, (what, n_one, n_many)
    ref = oracle.render(fs.c_struct(), cam, cfg, want_means=True, n_threads=16)
    assert_parity(one, ref, what + ", sample_group 64")
    assert_parity(many, ref, what + ", sample_group 1")
    # the frame holds what the case is about
    ids = one["object_id"]
    if name in ("fixed_slots", "dense_queue"):
        assert (ids == 0).sum() >= W * H // 8 and (ids != 0).sum() >= W * H // 2, what       # pixels that miss everything, and hits
    if name == "bright":
        wide = ref["max_abs_rgb"] > 2.0
        assert wide.sum() >= 50 and (ref["max_abs_rgb"] > 32768.0).sum() == 0, (what, int(wide.sum()))
    if name == "far":
        assert float(np.nanmin(np.where(ids != 0, one["depth"], np.inf))) > 512.0, what      # every root hit is a wide depth term


@pytest.mark.parametrize("samples", SAMPLES)
def test_pixel_split_under_both_groupings(hip, samples):
    """rr_render_pixel_split (the SPLIT builds of the level-1 kernels: the diffuse planes beside the colour planes) on the first scene."""
    fs = _scene("fixed_slots")
    cam, cfg = camera_for(fs, W, H).c_struct(), _cfg(samples)
    got = {}
    for group in (64, 1):
        with hip.DeviceScene(fs, 0) as ds:
            ds.set_tuning(sample_group=group)
            got[group] = ds.render_pixel_split(cam, cfg)

    def same(a, b, path):
        for k in a:
            if isinstance(a[k], dict):
                same(a[k], b[k], path + k + ".")
            elif isinstance(a[k], np.ndarray):
                x, y = np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k])
                if x.dtype == np.float32:
                    x, y = x.view(np.uint32), y.view(np.uint32)
                assert x.shape == y.shape and np.array_equal(x, y), f"{path}{k} differs in {int((x != y).sum())} words at {samples} samples"
    same(got[64], got[1], "")
    assert got[64]["diffuse"].any() and got[64]["color"].shape == (W * H, 3)
