"""Records rr_surface_rays of tests/tangent_scenes.py's scene (its 24 x 16 primary rays) as the library answered BEFORE the tangent
frames moved into DSceneView::flat_normals: tests/golden/tangent_frames_surface.npz, the judge of
tests/test_gpu_tangent_frames.py::test_surface_query_returns_the_recorded_bits.  Needs a GPU and the library of that revision
(RUSTRAY_HIP_LIB).  usage: python -m tests.golden.make_tangent_frames <out.npz>"""
import sys

import numpy as np


def query(hip, oracle):
    from rustray_amd.flat import make_config
    from tests import tangent_scenes
    from tests.helpers import camera_for
    from tests.test_gpu_shade_rays import primaries
    from tests.test_gpu_surface_rays import _f32_normalised
    fs = tangent_scenes.scene()
    cam = camera_for(fs, 24, 16).c_struct()
    cfg = make_config(samples=1, monte_carlo=False, seed=3, max_recursion=0, fog_density=0.0)
    table, _ = oracle.sample_table(1)
    o, d = primaries(oracle, cam, cfg, table)
    with hip.DeviceScene(fs, 0) as ds:
        return ds.surface_rays(o, _f32_normalised(d), 1)


if __name__ == "__main__":
    from oracle import binding
    from rustray_amd import capi
    got = query(capi, binding)
    np.savez_compressed(sys.argv[1], records=np.ascontiguousarray(got).view(np.uint32).reshape(len(got), -1))
    print("hits", int((got["hit"] == 1).sum()), "items", sorted(set(got["item_index"][got["hit"] == 1].tolist())))
