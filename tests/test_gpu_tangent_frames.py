"""The tangent frames of flat-shaded, normal-mapped hits come from DSceneView::flat_normals (filled by k_world_normals with the function
the per-hit path uses): frames against the oracle with tests/test_gpu_parity.py's comparison, every writer of the table -- scene
creation, rr_scene_update_transforms, rr_scene_set_items (kept and derived runs), and a normal map attached by a material edit --
against a freshly created scene bit for bit, and rr_surface_rays against the bits recorded before the table carried the frames."""
import os

import numpy as np
import pytest

from rustray_amd.flat import make_config
from tests import tangent_scenes
from tests.helpers import GOLDEN, assert_frames_identical, camera_for
from tests.test_gpu_parity import assert_parity

pytestmark = pytest.mark.gpu

W, H, SPP = 24, 16, 64


def _cfg():
    return make_config(samples=SPP, monte_carlo=True, seed=17, max_recursion=3)


def _fresh(hip, **kw):
    fs = tangent_scenes.scene(**kw)
    with hip.DeviceScene(fs, 0) as ds:
        return ds.render(camera_for(fs, W, H).c_struct(), _cfg())


def test_frame_matches_oracle(hip, oracle):
    fs = tangent_scenes.scene()
    cam = camera_for(fs, W, H).c_struct()
    with hip.DeviceScene(fs, 0) as ds:
        out = ds.render(cam, _cfg())
    ref = oracle.render(fs.c_struct(), cam, _cfg(), want_means=True, n_threads=16)
    assert_parity(out, ref, "tangent frames")
    ids = set(np.unique(out["object_id"]).tolist())
    assert {it.id for it in fs.items} <= ids, ids   # every case is in the picture


def test_every_writer_of_the_table_equals_a_fresh_scene(hip):
    base = tangent_scenes.scene()
    cam = camera_for(base, W, H).c_struct()
    with hip.DeviceScene(base, 0) as ds:
        first = ds.render(cam, _cfg())
        turned = tangent_scenes.scene(turn=True)
        ds.update_transforms(np.stack([it.trans for it in turned.items]), np.stack([it.trans_inv for it in turned.items]))
        a = ds.render(cam, _cfg())
        edited = tangent_scenes.scene(turn=True, edit_items=True)
        ds.set_items(edited.items, edited.materials)
        b = ds.render(cam, _cfg())
        attached = tangent_scenes.scene(turn=True, edit_items=True, attach=True)
        ds.update_materials(attached.materials)
        c = ds.render(cam, _cfg())
    assert_frames_identical(first, _fresh(hip), "created twice")
    assert_frames_identical(a, _fresh(hip, turn=True), "rr_scene_update_transforms")
    assert_frames_identical(b, _fresh(hip, turn=True, edit_items=True), "rr_scene_set_items")
    assert_frames_identical(c, _fresh(hip, turn=True, edit_items=True, attach=True), "normal map attached")
    for x, y in ((first, a), (a, b), (b, c)):   # and every edit shows
        assert not np.array_equal(x["rgba"], y["rgba"])


def test_surface_query_returns_the_recorded_bits(hip, oracle):
    """shading_normal, and every other word of the 24 x 16 primary rays' records, as recorded from the revision that derived every
    frame per hit (tests/golden/make_tangent_frames.py)."""
    from tests.golden.make_tangent_frames import query
    got = query(hip, oracle)
    want = np.load(os.path.join(GOLDEN, "tangent_frames_surface.npz"))["records"]
    words = np.ascontiguousarray(got).view(np.uint32).reshape(len(got), -1)
    assert words.shape == want.shape
    assert np.array_equal(words, want), f"{int((words != want).any(axis=1).sum())} records differ"
    hit = got["hit"] == 1
    mapped = hit & (np.abs(got["shading_normal"] - got["normal"]).max(axis=1) > 0)
    assert int(mapped.sum()) >= 40 and len(set(got["item_index"][mapped].tolist())) >= 7   # the normal-mapped cases are among the hits
