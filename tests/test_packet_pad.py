"""The decoys of tests/packet_pad.py are inert under the reference's semantics: the oracle (all-items form) renders a padded scene
bit for bit like the unpadded one, with the same ray and hit counts.  So where tests/test_gpu_packet_walk.py finds the device's
frame of a padded scene differ from its frame of the unpadded one, the device is wrong."""
import os

import numpy as np
import pytest

from rustray_amd.flat import FlatScene, make_config
from tests.corner_scenes import builders
from tests.helpers import GOLDEN, assert_frames_identical, camera_for, load_scene
from tests.packet_pad import MODES, in_packet_range, pad_inert

COUNTS = ("rays_primary", "rays_secondary", "rays_shadow", "shaded_hits")


def _bases():
    from tests.test_gpu_random import _random_scene
    b = {"spheres_room": lambda: load_scene("spheres_room"), "kbert_room": lambda: load_scene("kbert_room"),
         "random_1003": lambda: _random_scene(1003),
         "fuzz_568": lambda: FlatScene.load(os.path.join(GOLDEN, "fuzz_568.npz")),
         "fuzz_far_2514": lambda: FlatScene.load(os.path.join(GOLDEN, "fuzz_far_2514.npz"))}
    c = builders()
    for k in ("equal_toi", "alpha_occluder", "projective", "blocker", "zero_term_degenerate"):
        b[k] = c[k]
    return b


@pytest.mark.parametrize("base", sorted(_bases()))
def test_decoys_are_inert_in_the_oracle(oracle, base):
    fs = _bases()[base]()
    assert len(fs.items) <= 14
    cam = camera_for(fs, 40, 32).c_struct()
    cfg = make_config(samples=2, monte_carlo=True, seed=7, max_recursion=4)
    ref = oracle.render(fs.c_struct(), cam, cfg, n_threads=8, want_counters=True, brute_force=True)
    for mode in MODES:
        for n in (17, 65, 513):
            p = pad_inert(fs, n, mode, seed=n)
            assert len(p.items) == n and in_packet_range(n) == (n <= 512)
            assert [it.id for it in p.items[:len(fs.items)]] == [it.id for it in fs.items]
            assert len({it.id for it in p.items}) == n                      # decoys take ids the scene does not use
            got = oracle.render(p.c_struct(), cam, cfg, n_threads=8, want_counters=True, brute_force=True)
            assert_frames_identical(got, ref, f"{base} {mode} {n}")
            assert [got["counters"][k] for k in COUNTS] == [ref["counters"][k] for k in COUNTS], (base, mode, n)


def test_switch_decoys_set_the_scene_wide_switches():
    """The three switch items are what the device keys its scene-wide paths on (rr_scene_build.h: general_w from a non-affine inverse,
    any_alpha_occluder from an alpha map, RR_VIEW_NAN_BALLS from a ball whose arithmetic can overflow)."""
    fs = pad_inert(load_scene("spheres"), 17, "switches")
    new = fs.items[8:]
    assert any(not (np.asarray(it.trans_inv)[3] == (0, 0, 0, 1)).all() for it in new)
    assert any(fs.materials[it.material].texture[4] >= 0 for it in new)
    assert any(it.kind == 0 and it.radius >= 1e12 for it in new)
    assert not any(it.visible for it in new)
