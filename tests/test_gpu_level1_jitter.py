"""Level-1 jitter on the generator's 64-bit products (philox4x32_10, rr_math.h): small frames against the oracle with
tests/test_gpu_parity.py's comparison.  The scene (tests/tangent_scenes.py) has a point and a directional light, shadow_softness 0.01
on every material and roughness on one; its quads stand against nothing, so packets at their silhouettes have lanes that missed, the
first lane among them.  24 x 16 at 64 and 128 samples: every packet is one pixel's.  5 x 3 at 16 samples: four pixels per packet and a
last packet of 48 lanes."""
import numpy as np
import pytest

from rustray_amd.flat import make_config
from tests import tangent_scenes
from tests.helpers import camera_for
from tests.test_gpu_parity import assert_parity

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("w,h,spp", [(24, 16, 64), (24, 16, 128), (5, 3, 16)])
def test_level1_jitter_matches_oracle(hip, oracle, w, h, spp):
    fs = tangent_scenes.scene()
    cam = camera_for(fs, w, h).c_struct()
    cfg = make_config(samples=spp, monte_carlo=True, seed=29, max_recursion=3)
    with hip.DeviceScene(fs, 0) as ds:
        out = ds.render(cam, cfg)
        st = ds.stats()
    ref = oracle.render(fs.c_struct(), cam, cfg, want_means=True, n_threads=16, want_counters=True)
    assert_parity(out, ref, f"{w}x{h} spp {spp}")
    c = ref["counters"]
    assert st["primary_rays"] == c["rays_primary"] == w * h * spp and st["shaded_hits"] == c["shaded_hits"]
    assert 0 < st["shaded_hits"] < st["primary_rays"] and st["shadow_rays"] > st["shaded_hits"]   # misses, and both lights cast shadow rays
    if spp >= 64:   # a silhouette: pixels some of whose samples missed (the mean depth's hit count is not all or nothing)
        hits = np.count_nonzero(ref["object_id"])
        assert 0 < hits < w * h
