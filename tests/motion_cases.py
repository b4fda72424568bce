"""Hand-made frames, items and moved lists for the tests of rr_motion_records (tests/test_motion_host.py, tests/test_gpu_motion.py): the
inputs only, made once per size and never changed by a test."""
import functools

import numpy as np

from tests.denoise_cases import F, pack
from tests.temporal_cases import make_camera

N_ITEMS = 80
N_MOVED = (0, 1, 3, 70)
ID_NOBODY = 12345            # an object id no item has


def _rotation(rng, angle):
    axis = rng.normal(size=3)
    axis /= np.linalg.norm(axis)
    k = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(angle) * k + (1 - np.cos(angle)) * (k @ k)


def _affine(rot, scale, shift):
    m = np.eye(4)
    m[:3, :3], m[:3, 3] = rot * scale, shift
    return m


@functools.lru_cache(maxsize=None)
def motion_items():
    """80 items: object ids (uint32, no two alike; ORDER[0] has id 0xffffffff, ORDER[1] id 0), `trans` and `trans_inv` of the current
    frame and `prev_trans` of the frame before (rotations, scales 0.5 .. 2, shifts; the step between the frames is a small rotation and
    a shift), all (80, 4, 4) float32 in math layout.  ORDER is the order in which items are listed as moved: a call with n_moved
    lists ORDER[:n_moved].  ORDER[2] is scaled by 0.25, so that its trans_inv takes a far point out of the float range."""
    rng = np.random.default_rng(23)
    order = rng.permutation(N_ITEMS)
    ids = rng.choice(np.arange(1, 5000), N_ITEMS, replace=False).astype(np.uint32)
    ids[order[0]], ids[order[1]] = 0xffffffff, 0
    assert ID_NOBODY not in ids
    trans, inv, prev = (np.zeros((N_ITEMS, 4, 4), F) for _ in range(3))
    for i in range(N_ITEMS):
        scale = 0.25 if i == order[2] else rng.uniform(0.5, 2.0)
        t = _affine(_rotation(rng, rng.uniform(0, np.pi)), scale, rng.uniform(-3, 3, 3))
        step = _affine(_rotation(rng, rng.uniform(0, 0.05)), 1.0, rng.normal(0, 0.1, 3))
        trans[i], inv[i], prev[i] = t.astype(F), np.linalg.inv(t).astype(F), (np.linalg.inv(step) @ t).astype(F)
    for a in (ids, trans, inv, prev, order):
        a.setflags(write=False)
    return dict(ids=ids, trans=trans, trans_inv=inv, prev_trans=prev, order=order)


def motion_scene(trans_inv=None):
    """A flat scene whose 80 items are spheres with the ids, `trans` and `trans_inv` of motion_items() (or the given inverses): what
    gives a handle the item records rr_motion_records reads.  Materials and lights are spheres_room's."""
    import copy
    import dataclasses
    from rustray_amd.flat import RR_ITEM_SPHERE
    from tests.helpers import load_scene
    it = motion_items()
    fs = copy.deepcopy(load_scene("spheres_room"))
    ball = next(item for item in fs.items if item.kind == RR_ITEM_SPHERE)
    inv = it["trans_inv"] if trans_inv is None else trans_inv
    fs.items = [dataclasses.replace(ball, id=int(it["ids"][i]), trans=it["trans"][i].copy(), trans_inv=np.asarray(inv[i], F).copy(), name=f"moved{i}")
                for i in range(N_ITEMS)]
    return fs


def moved_list(n_moved: int):
    """(item_index (n_moved,) uint32, prev_trans (n_moved, 4, 4)) of a call that lists the first n_moved items of ORDER."""
    it = motion_items()
    idx = it["order"][:n_moved].astype(np.uint32)
    return idx, it["prev_trans"][idx]


@functools.lru_cache(maxsize=None)
def motion_frame(W: int, H: int):
    """A W x H frame of records over motion_items(): the row pairs y % 8 in (0, 1) hold ONE id each -- a wave of the kernel covers 32 x 2
    pixels, rows 2j and 2j + 1 of a 32x8 tile, so every wave there has one id (but for the three pixels below) --, the rows y % 8 in
    (2, 3) alternate between two ids lane by lane, the others hold patches of 5 x 2 pixels.  The ids are those of ORDER[:40] (listed
    by a call with n_moved = 70; the first three by the shorter calls), of ORDER[70:] (never listed) and ID_NOBODY; ids 0 and
    0xffffffff are among them.  Depths 2.5 .. 9, unit normals.  One pixel in twenty is a miss (id 0, depth 0, NaN normal; none in rows 8 and 9).  Pixel 5 has
    a NaN depth, pixel 6 an inf depth, and pixel 7, of ORDER[2], a depth of 3e38: its world point is finite and its local point is not.
    -> dict(cam, records (n, 8))."""
    rng = np.random.default_rng(31)
    it = motion_items()
    order, ids_of = it["order"], it["ids"]
    pool = np.concatenate([ids_of[order[:40]], ids_of[order[70:]], np.array([ID_NOBODY], np.uint32)]).astype(np.uint32)
    n = W * H
    y, x = np.mgrid[0:H, 0:W]
    x, y = x.reshape(-1), y.reshape(-1)
    patch = pool[rng.integers(0, len(pool), ((H + 1) // 2 + 1) * ((W + 4) // 5 + 1))]
    ids = patch[(y // 2) * ((W + 4) // 5 + 1) + x // 5]
    pair_a, pair_b = pool[rng.integers(0, len(pool), H // 2 + 1)], pool[rng.integers(0, len(pool), H // 2 + 1)]   # per pair of rows
    pair_a[0], pair_a[4] = ids_of[order[0]], ids_of[order[1]]  # rows 0, 1 and 8, 9: the ids 0xffffffff and 0, uniform
    pair_a[1], pair_b[1] = ids_of[order[0]], ids_of[order[1]]  # rows 2, 3: the two of them in turn
    pair_a[5], pair_b[5] = ids_of[order[3]], ID_NOBODY         # rows 10, 11: a listed id and nobody's in turn
    ids = np.where(y % 8 < 2, pair_a[y // 2], ids)
    ids = np.where((y % 8 == 2) | (y % 8 == 3), np.where(x % 2 == 0, pair_a[y // 2], pair_b[y // 2]), ids).astype(np.uint32)
    normal = rng.normal(size=(n, 3))
    normal = (normal / np.linalg.norm(normal, axis=1, keepdims=True)).astype(F)
    depth = (F(2.5) + rng.random(n).astype(F) * F(6.5)).astype(F)
    color = rng.random((n, 3)).astype(F)
    miss = rng.random(n) < 0.05
    miss[:8] = False
    miss[(y == 8) | (y == 9)] = False          # whole waves of one id, every lane valid
    ids[miss], depth[miss], normal[miss] = 0, 0, np.nan
    depth[5], depth[6], depth[7] = np.nan, np.inf, F(3e38)
    ids[7] = ids_of[order[2]]
    records = pack(color, depth, normal, ids)
    records.setflags(write=False)
    return dict(cam=make_camera(W, H), records=records)
