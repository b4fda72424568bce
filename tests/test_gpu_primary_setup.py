"""The level-1 kernels build a primary ray from tables the host sets up per frame (rustray_amd/csrc/rr_primary_setup.h: the pixel
centres per accumulator slot, the offsets per sample, the constants of the index arithmetic).  On the GPU: every way a frame can
be cut into packets and batches gives the same arrays, a region that does not start at the origin gives the frame's own pixels,
depth of field and rr_pick still agree with the oracle (run with -m gpu on an MI355X).  The arithmetic itself is checked bit for
bit on the CPU (tests/test_primary_setup.py)."""
import numpy as np
import pytest

from rustray_amd.flat import make_config
from tests.helpers import assert_frames_identical, camera_for, load_scene
from tests.test_gpu_parity import assert_parity

pytestmark = pytest.mark.gpu

W, H = 64, 48                   # 3072 slots: a multiple of 32, so packets of 2 samples x 32 pixels are a plan too
PER_PRIMARY = 16 + 2 * 56       # bytes of queue budget per primary ray of a batch (rr_frame_plan.h plan_frame)


def _render(ds, cam, cfg, **tuning):
    ds.set_tuning(**{"sample_group": 0, "queue_budget_bytes": 0, **tuning})   # 0 = automatic
    out = ds.render(cam, cfg)
    return out, ds.stats()


@pytest.mark.parametrize("spp", [64, 128])
def test_sample_groups_give_the_same_frame(hip, spp):
    """Packets of one sample of 64 pixels, of 2 samples of 32 pixels and of 64 samples of one pixel: the same rays in another order."""
    fs = load_scene("monkey_room")
    cam = camera_for(fs, W, H).c_struct()
    cfg = make_config(samples=spp, monte_carlo=True, seed=17)
    with hip.DeviceScene(fs, 0) as ds:
        ref, st0 = _render(ds, cam, cfg, sample_group=1)
        for group in (2, 0):
            out, st = _render(ds, cam, cfg, sample_group=group)
            assert_frames_identical(out, ref, f"sample_group {group}")
            for k in ("primary_rays", "secondary_rays", "shadow_rays", "shaded_hits"):
                assert st[k] == st0[k], k
    assert st0["primary_rays"] == W * H * spp and (ref["rgba"][..., :3] != 0).any()


def test_three_samples_have_one_plan(hip, oracle):
    """3 spp at 70x50: no sample group divides the samples, every setting is one sample of 64 pixels per packet (3500 slots, 55
    packets per slice, the last one short)."""
    fs = load_scene("monkey_room")
    cam = camera_for(fs, 70, 50).c_struct()
    cfg = make_config(samples=3, monte_carlo=True, seed=18)
    with hip.DeviceScene(fs, 0) as ds:
        ref, _ = _render(ds, cam, cfg, sample_group=1)
        for group in (2, 0):
            out, _ = _render(ds, cam, cfg, sample_group=group)
            assert_frames_identical(out, ref, f"sample_group {group}")
    assert_parity(ref, oracle.render(fs.c_struct(), cam, cfg, want_means=True, n_threads=16), "3 spp")


@pytest.mark.parametrize("spp,group,budget_rays,batches", [
    (256, 0, W * H * 64, 4),    # automatic: 64 samples of a pixel per packet, one group of 64 sample slices per batch
    (64, 2, W * H * 2, 32),     # 2 samples x 32 pixels, one group of 2 slices per batch
    (6, 1, 1, 3),               # one sample of 64 pixels, batches of 2 whole slices (the 4096-ray floor rounded up to slices)
])
def test_batches_give_the_one_batch_frame(hip, spp, group, budget_rays, batches):
    fs = load_scene("monkey_room")
    cam = camera_for(fs, W, H).c_struct()
    cfg = make_config(samples=spp, monte_carlo=True, seed=19)
    with hip.DeviceScene(fs, 0) as ds:
        ref, st0 = _render(ds, cam, cfg, sample_group=group)
        out, st = _render(ds, cam, cfg, sample_group=group, queue_budget_bytes=budget_rays * PER_PRIMARY)
    assert st0["batches"] == 1 and st["batches"] == batches >= 3
    assert_frames_identical(out, ref, f"{batches} batches")
    for k in ("primary_rays", "secondary_rays", "shadow_rays", "shaded_hits"):
        assert st[k] == st0[k], k


def test_region_off_the_origin_gives_the_frames_pixels(hip):
    """Rank 1 of 3 over 32x8 tiles at 70x50 (3 tiles across): the column of tiles from x = 32, the last one clipped to 2 rows."""
    import torch
    from rustray_amd.renderer import TiledFrame, region_pixels, render_region_torch
    fs = load_scene("monkey_room")
    w, h = 70, 50
    cam = camera_for(fs, w, h).c_struct()
    cfg = make_config(samples=64, monte_carlo=True, seed=20)
    with hip.DeviceScene(fs, 0) as ds:
        whole = ds.render(cam, cfg)
        part = render_region_torch(ds, cam, cfg, TiledFrame(w, h, 1, 3, 32, 8), aux=True)
        torch.cuda.synchronize()
        part = {k: v.cpu().numpy() for k, v in part.items()}
    xy = region_pixels(w, h, 32, 8, 3, 1)
    assert xy[0, 0] == 32 and xy[0, 1] == 0 and 0 < len(xy) < w * h
    for k in ("rgba", "normal", "depth", "object_id"):
        got = part[k][:len(xy)].reshape(len(xy), -1)
        want = whole[k][xy[:, 1], xy[:, 0]].reshape(len(xy), -1)
        if got.dtype == np.float32:
            got, want = got.view(np.uint32), want.view(np.uint32)
        assert np.array_equal(got.view(want.dtype), want), k


def test_depth_of_field_matches_oracle(hip, oracle):
    """The depth-of-field configuration of the lotus stand-in (its meta["config"]) at 64 spp: the aperture's offsets come from
    the per-sample table, the focus point from the per-slot centres."""
    from rustray_amd import synthetic
    from rustray_amd.camera import Camera
    fs = synthetic.lotus_syn(grid=6)
    st = dict(fs.meta["camera"]); st["width"], st["height"] = W, H
    cam = Camera.from_state(st).c_struct()
    cd = fs.meta["config"]
    assert cd["aperture_size"] > 1.0 and cd["focal_length"] > 1.0
    cfg = make_config(samples=64, monte_carlo=True, seed=12, focal_length=cd["focal_length"], aperture_size=cd["aperture_size"])
    with hip.DeviceScene(fs, 0) as ds:
        out = ds.render(cam, cfg)
        one, _ = _render(ds, cam, cfg, sample_group=1)
    assert_frames_identical(one, out, "sample_group 1")
    assert_parity(out, oracle.render(fs.c_struct(), cam, cfg, want_means=True, n_threads=16), "lotus_syn +DOF")


def test_pick_matches_oracle(hip, oracle):
    """rr_pick launches the level-1 kernel over one-entry tables: a hit, a miss in a corner and a hit off the centre."""
    fs = load_scene("spheres")
    cam = camera_for(fs, 256, 256).c_struct()
    hits = 0
    with hip.DeviceScene(fs, 0) as ds:
        for x, y in ((128, 128), (3, 250), (185, 150)):
            a, b = ds.pick(cam, x, y), oracle.pick(fs.c_struct(), cam, x, y)
            assert (a.hit, a.object_id, a.item_index) == (b.hit, b.object_id, b.item_index)
            assert a.distance == b.distance
            hits += a.hit
    assert hits >= 1
