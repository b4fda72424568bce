"""Inert decoys: scenes padded with invisible items, so that the same picture is traced by another walk of the top level.

The packet form of the top level (rr_trace.h: beam_candidates, trace_closest_packet, trace_shadow_packet) runs in scenes
with RR_BEAM_MIN_ITEMS .. RR_BEAM_MAX_ITEMS (17 .. 512) items and falls back to the per-ray walk for a packet with more than 64
candidates.  An invisible item keeps its place in the top-level boxes and in a packet's candidate list: only item_passes
rejects it, per candidate.  So decoys change which walk runs and how full a packet is, and never what a ray hits.
tests/test_packet_pad.py shows that under the oracle's semantics; tests/test_gpu_packet_walk.py then holds the device to it.
"""
from __future__ import annotations

import copy

import numpy as np

from rustray_amd.flat import FlatScene, Item, Material, MeshData, RR_ITEM_MESH, RR_ITEM_SPHERE
from rustray_amd.scene import Scene, get_transformation, inverse_affine

MODES = ("copies", "scattered", "switches")
PACKET_MIN, PACKET_MAX = 17, 512   # RR_BEAM_MIN_ITEMS, RR_BEAM_MAX_ITEMS (rustray_amd/csrc/rr_device.h)
PACKET_LANES = 64                  # a packet with more candidates than lanes takes the per-ray walk


def in_packet_range(n_items: int) -> bool:
    return PACKET_MIN <= n_items <= PACKET_MAX


def world_bounds(fs: FlatScene):
    """(lo, hi) float64 of the world boxes of the corners of the items' declared boxes (affine, finite ones only)."""
    lo, hi = np.full(3, np.inf), np.full(3, -np.inf)
    for it in fs.items:
        ti = np.asarray(it.trans_inv, np.float64)
        if not (ti[3] == (0.0, 0.0, 0.0, 1.0)).all():
            continue
        c = np.asarray([[(it.bbox_max if k & (1 << a) else it.bbox_min)[a] for a in range(3)] for k in range(8)], np.float64)
        w = c @ np.asarray(it.trans, np.float64)[:3, :3].T + np.asarray(it.trans, np.float64)[:3, 3]
        if np.isfinite(w).all():
            lo, hi = np.minimum(lo, w.min(0)), np.maximum(hi, w.max(0))
    if not np.isfinite(lo).all():
        lo, hi = np.full(3, -1.0), np.full(3, 1.0)
    return lo, hi


def _decoy_material(out: FlatScene, alpha_texture: int = -1):
    m = Material(base_color=(1.0, 0.0, 1.0))
    if alpha_texture >= 0:
        m.texture[4] = alpha_texture                      # TextureType::Alpha: sets RR_IF_OCCLUDER_ALPHA_TEX
    out.materials.append(m); out.materials.append(Scene._cache_of(m))
    return len(out.materials) - 2, len(out.materials) - 1


def _decoy_quad(out: FlatScene) -> int:
    p = np.asarray([[-1, 0, 1], [1, 0, 1], [1, 0, -1], [-1, 0, -1]], np.float32)
    out.meshes.append(MeshData(positions=p, indices=np.asarray([[0, 1, 2], [0, 2, 3]], np.uint32),
                               uvs=np.asarray([[0, 0], [1, 0], [1, 1], [0, 1]], np.float32),
                               uv_indices=np.asarray([[0, 1, 2], [0, 2, 3]], np.uint32)))
    return len(out.meshes) - 1


def _placed(centre, size):
    t = get_transformation(np.eye(4, dtype=np.float32), tuple(float(v) for v in centre), (float(size),) * 3, (0.0, 0.0, 0.0))
    return t, inverse_affine(t)


def _switch_items(out: FlatScene, ids, lo, hi):
    """One invisible item per scene-wide path switch: a projective inverse (DSceneView::general_w: the dividing form of
    inverse_ray / to_local_point for every item), an alpha-mapped occluder (any_alpha_occluder: zero-term shadow rays of
    receivers whose uv may be NaN are traced) and a ball whose arithmetic overflows (RR_VIEW_NAN_BALLS: trace_shadow_blockers
    goes on past the first blocker)."""
    centre, size = 0.5 * (lo + hi), max(float((hi - lo).max()), 1e-3) * 0.05
    mi, ci = _decoy_material(out)
    # projective: origin' = (M x) / 2, compensated in the first three rows (tests/test_gpu_corners.py, projective inverse)
    s, _ = _placed(centre, size)
    si = np.linalg.inv(s.astype(np.float64)).astype(np.float32)
    si[3, :] = (0.0, 0.0, 0.0, 2.0)
    si[:3, :] *= 2.0
    items = [Item(kind=RR_ITEM_SPHERE, id=next(ids), material=mi, material_cache=ci, radius=1.0, trans=s, trans_inv=si,
                  bbox_min=(-1.0,) * 3, bbox_max=(1.0,) * 3, visible=False, name="decoy_projective")]
    tex = np.zeros((4, 4, 4), np.uint8); tex[..., :3] = 128; tex[..., 3] = 255
    out.textures.append(tex)
    ma, ca = _decoy_material(out, alpha_texture=len(out.textures) - 1)
    t, ti = _placed(centre, size)
    items.append(Item(kind=RR_ITEM_MESH, id=next(ids), material=ma, material_cache=ca, mesh=_decoy_quad(out), trans=t, trans_inv=ti,
                      bbox_min=(-1.0, 0.0, -1.0), bbox_max=(1.0, 0.0, 1.0), visible=False, name="decoy_alpha_occluder"))
    # radius 1e12 under a transform that scales it to `size` units (tests/test_gpu_item_boxes.py: the overflowing ball)
    t = get_transformation(np.eye(4, dtype=np.float32), tuple(float(v) for v in centre), (float(np.float32(1e-12 * size)),) * 3, (0.3, 0.4, 0.5))
    items.append(Item(kind=RR_ITEM_SPHERE, id=next(ids), material=mi, material_cache=ci, radius=1e12, trans=t, trans_inv=inverse_affine(t),
                      bbox_min=(-1e12,) * 3, bbox_max=(1e12,) * 3, visible=False, name="decoy_overflowing_ball"))
    return items


def pad_inert(fs: FlatScene, n_total: int, mode: str, seed: int = 0) -> FlatScene:
    """A deep copy of `fs` with invisible items appended until it holds `n_total` items.  The real items keep their indices
    (equal-toi ties are broken by index); decoys take ids the scene does not use.
      copies:    invisible copies of the scene's own items, cycled (same mesh or radius, transform and declared box): their
                 boxes and keys equal the real items', which pushes packets past 64 candidates; the extent stays.
      scattered: small invisible spheres and quads at seeded places inside the scene's world bounds: only some packets
                 see them, most stay on the packet form.
      switches:  `copies` plus one invisible item per scene-wide path switch (_switch_items)."""
    assert mode in MODES, mode
    n0 = len(fs.items)
    assert n_total >= n0, (n_total, n0)
    keep, fs._keep = fs._keep, None   # (the buffers a c_struct() view borrows: not part of the scene, and ctypes cannot be copied)
    try:
        out = copy.deepcopy(fs)
    finally:
        fs._keep = keep
    ids = iter(range(max((it.id for it in fs.items), default=0) + 1000, 1 << 31))
    lo, hi = world_bounds(fs)
    decoys = []
    if mode == "switches":
        assert n_total - n0 >= 3, "switches needs room for three switch items"
        decoys += _switch_items(out, ids, lo, hi)
    if mode == "scattered":
        rng = np.random.default_rng(seed)
        mi, ci = _decoy_material(out)
        quad = _decoy_quad(out)
        size = max(float((hi - lo).max()), 1e-3) * 0.03
        while n0 + len(decoys) < n_total:
            t, ti = _placed(rng.uniform(lo, hi), size)
            if rng.random() < 0.5:
                decoys.append(Item(kind=RR_ITEM_SPHERE, id=next(ids), material=mi, material_cache=ci, radius=1.0, trans=t, trans_inv=ti,
                                   bbox_min=(-1.0,) * 3, bbox_max=(1.0,) * 3, visible=False, name="decoy_ball"))
            else:
                decoys.append(Item(kind=RR_ITEM_MESH, id=next(ids), material=mi, material_cache=ci, mesh=quad, trans=t, trans_inv=ti,
                                   bbox_min=(-1.0, 0.0, -1.0), bbox_max=(1.0, 0.0, 1.0), visible=False, name="decoy_quad"))
    k = 0
    while n0 + len(decoys) < n_total:
        src = fs.items[k % n0]
        d = copy.deepcopy(src)
        d.id, d.visible, d.name = next(ids), False, f"decoy_copy_{src.name}"
        decoys.append(d)
        k += 1
    out.items += decoys
    assert len(out.items) == n_total and all(not d.visible for d in out.items[n0:])
    return out
