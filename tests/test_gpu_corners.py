"""Adversarial scenes for order-dependent and rarely taken paths of the reference's trace loop, GPU vs oracle."""
import numpy as np
import pytest

from rustray_amd.flat import make_config
from tests.corner_scenes import (INSIDE_SPHERES, alpha_occluder_scene, deep_mesh_scene, equal_toi_scene, inside_spheres_scene,
                                 projective_scene, zero_light_term_scene)
from tests.helpers import assert_in_band, camera_for, compare_frames, load_scene
from tests.test_gpu_parity import assert_parity

pytestmark = pytest.mark.gpu


def _check(hip, oracle, fs, w=96, h=96, **cfg):
    cam = camera_for(fs, w, h).c_struct()
    c = make_config(**({"samples": 2, "monte_carlo": True, "seed": 3} | cfg))
    with hip.DeviceScene(fs, 0) as ds:
        out = ds.render(cam, c)
    ref = oracle.render(fs.c_struct(), cam, c, want_means=True, n_threads=8)
    assert_parity(out, ref)
    return out, ref


def test_equal_toi_goes_to_the_smaller_bbox_distance_then_index(hip, oracle):
    """Two items share ONE mesh (bit-equal toi).  The stable sort by bbox distance + strict `<` of the reference
    (src/raytracing.rs:466-476) gives the hit to the item with the smaller bbox distance, index breaking ties."""
    fs = equal_toi_scene()
    out, _ = _check(hip, oracle, fs)
    assert set(np.unique(out["object_id"])) == {0, 3}                       # same key: the lower index wins
    fs = equal_toi_scene(thick=True)                                        # a thicker declared box is entered earlier
    out, _ = _check(hip, oracle, fs)
    assert set(np.unique(out["object_id"])) == {0, 6}


def test_alpha_textured_occluder_and_short_uv_lists(hip, oracle):
    """Occluder alpha maps (src/raytracing.rs:894-913: receiver's alpha, receiver's get_uv, occluder's face id) and
    Mesh::get_uv's bounds test for faces without uv indices (src/shape/mesh.rs:116-120)."""
    for nearest in (False, True):
        fs = alpha_occluder_scene(nearest)
        _check(hip, oracle, fs, samples=3)


def test_camera_inside_solid_and_hollow_spheres(hip, oracle):
    """Ball::cast_local_ray from inside: a solid ball answers toi = 0, a non-solid one its far side."""
    for alpha, cull in INSIDE_SPHERES:
        fs = inside_spheres_scene(alpha, cull)
        _check(hip, oracle, fs, samples=2)


def test_projective_inverse_and_non_uniform_scale(hip, oracle):
    """get_inverse_ray divides the transformed origin by w (Point3::from_homogeneous, src/shape/mod.rs:757-760): a w row
    other than (0,0,0,1) must be honoured; normals use `trans`, not its inverse transpose (Appendix A 13)."""
    fs = projective_scene()
    _check(hip, oracle, fs, samples=2)


def test_deep_mesh_tree_keeps_within_the_traversal_stack(hip, oracle):
    """A geometric progression of nested triangles makes SAH peel one primitive per level, so the per-mesh tree reaches
    the builder's depth limit; the 4-wide collapse must then stay binary where the LDS stack budget is tight
    (rustray_amd/csrc/rr_bvh.cpp) and every triangle must remain reachable."""
    fs = deep_mesh_scene()
    out, _ = _check(hip, oracle, fs, w=128, h=128)
    assert (out["object_id"] == 2).sum() > 1000


@pytest.mark.parametrize("name", ["fuzz_alpha", "fuzz_234", "fuzz_568", "fuzz_6601"])
def test_non_finite_samples_reach_the_pixel_as_in_the_reference(hip, oracle, name):
    """Scenes reduced from tools/fuzz_parity.py mismatches (tests/golden/fuzz_*.npz).  The reference's f32 sums carry a
    NaN sample to the pixel (NaN.min(1.0) = 1.0 -> 255, src/raytracing.rs:406-417): fixed-point sums cannot, so k_shade /
    k_trace_shadow flag the pixel and k_resolve reproduces the value.
      fuzz_alpha: a sphere with flipped normals shadowed by a mesh with an alpha map.  The light term is exactly 0, but the
                  map is sampled at the RECEIVER's uv of the occluder's hit point (:905): acos(> 1) = NaN, 0 * NaN = NaN;
      fuzz_234:   a reflectivity map sampled at a NaN uv at a sphere's pole, no light: color * (1 - NaN) with color = 0;
      fuzz_568:   several such items, semi-transparent and invisible ones, refraction index below 1;
      fuzz_6601:  a normal map gives a sphere a NaN normal, the SHADOW ray starts at NaN: in the reference every candidate
                  sphere then reports Some(NaN), `in_light = toi > len` is false, and the occluder's alpha map sampled at a
                  NaN uv under the bilinear filter makes the attenuation NaN (rr_trace.h: trace_shadow_nonfinite)."""
    from rustray_amd.flat import FlatScene
    import os
    from tests.helpers import GOLDEN
    fs = FlatScene.load(os.path.join(GOLDEN, name + ".npz"))
    w, h = fs.meta["wh"]
    cam = camera_for(fs, w, h).c_struct()
    cfg = make_config(**fs.meta["kw"])
    with hip.DeviceScene(fs, 0) as ds:
        out = ds.render(cam, cfg)
    ref = oracle.render(fs.c_struct(), cam, cfg, want_means=True, n_threads=8)
    res = compare_frames(out, ref)
    assert res["n_rgb_over"] == 0 and res["n_id_diff"] == 0 and res["nan_mismatch"] == 0, res
    assert_in_band(res, name)
    assert int((ref["rgba"][..., :3] == 255).all(axis=-1).sum()) >= 1   # the white pixels are there


def test_zero_light_term_still_reaches_the_pixel_through_a_nan_uv_and_only_then(hip, oracle):
    """A light term that is exactly zero (light behind the receiver, no specular colour) is NaN in the reference when the occluder
    has an alpha map and the RECEIVER's get_uv of the occluder's hit point is not finite (src/raytracing.rs:898-912: 0 * NaN): the pixel
    turns white.  Receivers whose uv can be non-finite: every sphere, and a mesh with a zero-area face (0 / 0 area weights,
    src/shape/mesh.rs:127-143) -- the occluder's face id picks the receiver's face.  For every other receiver the zero term stays zero,
    and the device does not trace its shadow ray at all (D7): same frame, fewer shadow rays than the reference traces."""
    white = {}
    for degenerate in (True, False):
        fs = zero_light_term_scene(degenerate)
        cam = camera_for(fs, 96, 96).c_struct()
        cfg = make_config(samples=2, monte_carlo=False, seed=3)
        with hip.DeviceScene(fs, 0) as ds:
            out = ds.render(cam, cfg)
            st = ds.stats()
        ref = oracle.render(fs.c_struct(), cam, cfg, want_means=True, n_threads=8, want_counters=True)
        assert_parity(out, ref)
        white[degenerate] = int((out["rgba"][..., :3] == 255).all(axis=-1).sum())
        if degenerate:
            assert st["shadow_rays"] > 0                                   # traced although every term is zero: the NaN has to be found
        else:
            assert st["shadow_rays"] == 0 and ref["counters"]["rays_shadow"] > 0   # (D7) nothing to find: not traced
    assert white[True] > 50 and white[False] == 0, white


def _scaled_world(fs, S):
    """The same scene with the world S times larger (item transforms, lights, camera): hit distances scale by S, colours stay
    (point-light falloff is I / (4 pi d): the intensity scales with S)."""
    import copy
    from rustray_amd.scene import inverse_affine
    out = copy.deepcopy(fs)
    sc = np.diag([S, S, S, 1.0]).astype(np.float32)
    for it in out.items:
        it.trans = (sc @ np.asarray(it.trans, np.float32)).astype(np.float32)
        it.trans_inv = inverse_affine(it.trans)
    for l in out.lights:
        l.pos = tuple(float(v) * S for v in l.pos)
        if l.light_type != 0:
            l.intensity = float(l.intensity) * S
    cam = dict(out.meta["camera"])
    cam["eye_pos"] = [float(v) * S for v in cam["eye_pos"]]
    cam["clipping_far"] = float(cam.get("clipping_far", 100.0)) * S
    out.meta = dict(out.meta); out.meta["camera"] = cam
    return out


def test_depth_of_far_hits_is_merged_per_pixel(hip, oracle):
    """a root hit farther than 512 units does not fit the 32-bit lane sum of the depth accumulator (depth * 2^16 >= 2^25)
    and was added as one unmerged 64-bit atomic per lane -- 64 lanes of a level-1 packet to one word.  Such terms are now merged per
    pixel in 64 bits (accum_depth_wide_merged).  spheres_room scaled 200 x (hit distances 600 .. 4000 units) against the oracle, and
    timed against the unscaled scene: the far form must not cost more than a fraction of the frame."""
    near = load_scene("spheres_room")
    far = _scaled_world(near, 200.0)
    cfg = make_config(samples=64, monte_carlo=True, seed=6, max_recursion=2)
    cam_f = camera_for(far, 160, 96).c_struct()
    with hip.DeviceScene(far, 0) as ds:
        out = ds.render(cam_f, cfg)
        assert float(np.nanmax(out["depth"])) > 512.0
        ds.set_profiling(True)
        ds.render(cam_f, cfg); t_far = ds.stats()["ms_shade"]
    ref = oracle.render(far.c_struct(), cam_f, make_config(samples=64, monte_carlo=True, seed=6, max_recursion=2), want_means=True, n_threads=8)
    res = compare_frames(out, ref)
    assert res["n_rgb_over"] == 0 and res["n_id_diff"] == 0 and res["max_depth_rel"] < 1e-4, res
    assert_in_band(res, "far")
    with hip.DeviceScene(near, 0) as ds:
        ds.set_profiling(True)
        cam_n = camera_for(near, 160, 96).c_struct()
        ds.render(cam_n, cfg); ds.render(cam_n, cfg); t_near = ds.stats()["ms_shade"]
    assert t_far < 1.5 * t_near + 0.2, (t_far, t_near)
