"""Shared helpers for the test suite: fixture scenes, cameras, comparisons."""
from __future__ import annotations

import os

import numpy as np

from rustray_amd.camera import Camera
from rustray_amd.flat import FlatScene, make_config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENES = os.path.join(ROOT, "scenes")
GOLDEN = os.path.join(ROOT, "tests", "golden")


def load_scene(name: str) -> FlatScene:
    return FlatScene.load(os.path.join(SCENES, name + ".npz"))


def camera_for(fs: FlatScene, width: int, height: int) -> Camera:
    st = dict(fs.meta["camera"])
    st["width"], st["height"] = width, height
    return Camera.from_state(st)


def compare_frames(a: dict, b: dict, rgb_tol: int = 1):
    """Returns a dict of mismatch statistics between two renders (a = candidate, b = oracle)."""
    ra, rb = a["rgba"].astype(np.int32), b["rgba"].astype(np.int32)
    diff = np.abs(ra[..., :3] - rb[..., :3]).max(axis=-1)
    res = dict(max_rgb_diff=int(diff.max()), n_rgb_over=int((diff > rgb_tol).sum()), n_pixels=int(diff.size),
               alpha_ok=bool((ra[..., 3] == 255).all()))
    if "object_id" in a and "object_id" in b:
        res["n_id_diff"] = int((a["object_id"] != b["object_id"]).sum())
    if "depth" in a and "depth" in b:
        da, db = a["depth"].astype(np.float64), b["depth"].astype(np.float64)
        res["max_depth_rel"] = float((np.abs(da - db) / np.maximum(np.abs(db), 1e-3)).max())
    if "normal" in a and "normal" in b:
        na, nb = a["normal"], b["normal"]
        both_nan = np.isnan(na) & np.isnan(nb)
        d = np.where(both_nan, 0.0, np.abs(na.astype(np.float64) - nb.astype(np.float64)))
        res["nan_mismatch"] = int((np.isnan(na) != np.isnan(nb)).sum())
        res["max_normal_abs"] = float(np.nanmax(d)) if d.size else 0.0
    return res


def assert_frames_identical(a: dict, b: dict, what: str = ""):
    """rgba, depth, normal and object_id equal bit for bit (floats compared as their bit patterns, NaN payloads included)."""
    for k in ("rgba", "depth", "normal", "object_id"):
        x, y = np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k])
        if x.dtype == np.float32:
            x, y = x.view(np.uint32), y.view(np.uint32)
        assert x.shape == y.shape and np.array_equal(x, y), f"{what}: {k} differs in {int((x != y).sum())} values"


def item_transforms(fs: FlatScene, dx: float = 0.0):
    """(n, 4, 4) float32 transforms and inverses of the scene's items (math layout), every item moved by (dx, 0, 0)."""
    t = np.stack([np.asarray(it.trans, np.float64) for it in fs.items]) if fs.items else np.zeros((0, 4, 4))
    ti = np.stack([np.asarray(it.trans_inv, np.float64) for it in fs.items]) if fs.items else np.zeros((0, 4, 4))
    move, back = np.eye(4), np.eye(4)
    move[0, 3], back[0, 3] = dx, -dx
    return (move @ t).astype(np.float32), (ti @ back).astype(np.float32)


def with_transforms(fs: FlatScene, t, ti) -> FlatScene:
    """A copy of the scene whose items carry the given transforms (what a freshly created scene is built from)."""
    import copy
    out = copy.deepcopy(fs)
    for it, a, b in zip(out.items, t, ti):
        it.trans, it.trans_inv = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return out
