"""Host-side mirror of the reference's frame scheduler, on top of the C ABI.

`Raytracing` and `RendererManager` keep the names and call surface of the
reference (src/raytracing.rs:205-273, src/renderer.rs:38-251) so that host code
and tests read like the reference's; what changes is that `start()` issues ONE
frame-level call into librustray_hip.so instead of spawning num_cpus-2 worker
threads over a shuffled queue of 2x2-pixel cells (src/renderer.rs:105-172).

`TiledFrame` is the multi-GPU form (no reference counterpart):
one process per GPU, the frame cut into interleaved tiles, every rank renders
its tiles into a compact device buffer, one gather to rank 0 over RCCL, one
de-interleave kernel.
"""
from __future__ import annotations

import copy
import time
from typing import Optional

import numpy as np

from . import capi
from .camera import Camera
from .flat import FlatScene, make_config, rr_camera, rr_config, rr_region

# the in-place steps of Raytracing.apply_scene, in the order they run; RECREATE stands alone
IN_PLACE_STEPS = ("add_textures", "update_materials", "update_transforms", "update_item_flags", "update_lights")
# the steps of a structural plan (plan_scene_update(..., structural=True)): the item list, the material list or the mesh list differ
STRUCTURAL_STEPS = ("add_textures", "add_meshes", "set_items", "update_lights")
RECREATE = "recreate"


def _pack_records(fields: dict) -> np.ndarray:
    """The dict of render_pixels (color (..., 3), depth (...), normal (..., 3), object_id (...) uint32) as (..., 8) float32 rr_radiance records."""
    color = np.asarray(fields["color"], np.float32)
    rec = np.zeros(color.shape[:-1] + (8,), np.float32)
    rec[..., 0:3] = color
    rec[..., 3] = fields["depth"]
    rec[..., 4:7] = fields["normal"]
    rec[..., 7] = np.asarray(fields["object_id"], np.uint32).view(np.float32)
    return rec


def _bits(a, dtype=np.float32) -> bytes:
    return np.ascontiguousarray(np.asarray(a, dtype)).tobytes()


def _same_array(a, b) -> bool:
    if a is b:
        return True
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _same_mesh(a, b) -> bool:
    return a is b or all(_same_array(getattr(a, k), getattr(b, k)) for k in ("positions", "indices", "uvs", "uv_indices", "normals", "normal_indices"))


def _resident_mesh_indices(resident, new_meshes):
    """Where each of `new_meshes` sits in a mesh list that starts as `resident` and gets the unseen ones appended: meshes are
    recognised by content (_same_mesh).  Returns (index per new mesh, the meshes to append)."""
    index, appended = [], []
    pool = list(resident)
    for m in new_meshes:
        at = next((k for k, r in enumerate(pool) if _same_mesh(r, m)), None)
        if at is None:
            at = len(pool)
            pool.append(m)
            appended.append(m)
        index.append(at)
    return index, appended


def _structural_plan(old: FlatScene, new: FlatScene, resident_meshes) -> list:
    """The STRUCTURAL_STEPS that bring a handle created from `old` -- whose device holds `resident_meshes`: old.meshes and whatever was
    appended since -- to `new`; [RECREATE] when a texture image changed or disappeared (the texture list is positional: materials
    name images by index) or when a mesh of `old` is in `new` no more, changed or dropped: meshes are never removed from a handle, so
    a host that edits or drops meshes gets their memory back with a new one.  A mesh that `new` still lists and no item names (the
    mesh of a deleted item, as Scene.flatten() leaves it) is no edit; meshes in another order are only indexed anew."""
    if len(new.textures) < len(old.textures) or not all(_same_array(a, b) for a, b in zip(old.textures, new.textures)):
        return [RECREATE]
    if not all(any(_same_mesh(m, n) for n in new.meshes) for m in old.meshes):
        return [RECREATE]
    steps = []
    if len(new.textures) > len(old.textures):
        steps.append("add_textures")
    if _resident_mesh_indices(resident_meshes, new.meshes)[1]:
        steps.append("add_meshes")
    steps.append("set_items")
    if len(old.lights) != len(new.lights) or any(bytes(a.c_struct()) != bytes(b.c_struct()) for a, b in zip(old.lights, new.lights)):
        steps.append("update_lights")
    return steps


def plan_scene_update(old: FlatScene, new: FlatScene, structural: bool = False, resident_meshes=None) -> list:
    """What turns a handle created from `old` into one that renders what a handle created from `new` renders, at the least cost
    (Run::restart_rendering after a GUI edit, reference src/run.rs:395-420).  Returns [RECREATE] when the item list (count, kind,
    id, mesh or material indices, radius, local box), a mesh, the material count or an existing texture image differs, or the
    texture list got shorter; else the IN_PLACE_STEPS whose part differs, in their order (empty: nothing to do).  Values are
    compared as the bits that cross the ABI.
    structural=True: where the default answers [RECREATE] for the item list, the material count or the mesh list (the GUI's object
    "delete", "add ground plane", "add environment sphere"), the plan is made of STRUCTURAL_STEPS instead (_structural_plan) and
    [RECREATE] is left for a resident mesh or texture image that changed or disappeared; `resident_meshes` (default: old.meshes) is
    what the device holds.  When nothing structural differs the plan is the default one."""
    plan = _plan_in_place(old, new)
    if structural and plan == [RECREATE]:
        return _structural_plan(old, new, old.meshes if resident_meshes is None else resident_meshes)
    return plan


def _plan_in_place(old: FlatScene, new: FlatScene) -> list:
    if len(old.items) != len(new.items) or len(old.materials) != len(new.materials) or len(old.meshes) != len(new.meshes):
        return [RECREATE]
    if len(new.textures) < len(old.textures):
        return [RECREATE]
    for a, b in zip(old.items, new.items):
        if (a.kind, a.id, a.mesh, a.material, a.material_cache) != (b.kind, b.id, b.mesh, b.material, b.material_cache):
            return [RECREATE]
        if _bits([a.radius, *a.bbox_min, *a.bbox_max]) != _bits([b.radius, *b.bbox_min, *b.bbox_max]):
            return [RECREATE]
    if not all(_same_mesh(a, b) for a, b in zip(old.meshes, new.meshes)):
        return [RECREATE]
    if not all(_same_array(a, b) for a, b in zip(old.textures, new.textures)):
        return [RECREATE]
    steps = []
    if len(new.textures) > len(old.textures):
        steps.append("add_textures")
    if any(bytes(a.c_struct()) != bytes(b.c_struct()) for a, b in zip(old.materials, new.materials)):
        steps.append("update_materials")
    if any(_bits(a.trans) != _bits(b.trans) or _bits(a.trans_inv) != _bits(b.trans_inv) for a, b in zip(old.items, new.items)):
        steps.append("update_transforms")
    if any((bool(a.visible), bool(a.flip_normals)) != (bool(b.visible), bool(b.flip_normals)) for a, b in zip(old.items, new.items)):
        steps.append("update_item_flags")
    if len(old.lights) != len(new.lights) or any(bytes(a.c_struct()) != bytes(b.c_struct()) for a, b in zip(old.lights, new.lights)):
        steps.append("update_lights")
    return steps


class Raytracing:
    """Scene + RaytracingConfig, as reference `Raytracing` (src/raytracing.rs:205-224)."""

    def __init__(self, flat_scene: FlatScene, camera: Camera, device: int = 0):
        self.flat_scene = flat_scene
        self.camera = camera
        self.config: rr_config = make_config()
        cfg = flat_scene.meta.get("config") or {}
        # a scene file's "config" block overrides whatever the caller set before load (src/scene.rs:180-198)
        self.apply_config(**{k: v for k, v in cfg.items() if k in
                             ("samples", "monte_carlo", "focal_length", "aperture_size", "fog_density",
                              "max_recursion", "gamma_correction")})
        self.device_scene = capi.DeviceScene(flat_scene, device)
        self.resident_meshes = list(flat_scene.meshes)   # what the device holds: the meshes of creation and those appended since, in order

    def apply_config(self, **kw):
        for k, v in kw.items():
            if k == "fog_color":
                self.config.fog_color[:] = list(v)
            elif k in ("monte_carlo", "gamma_correction"):
                setattr(self.config, k, int(bool(v)))
            else:
                setattr(self.config, k, v)

    def render_frame(self, sample_xy=None, aux: bool = True) -> dict:
        """All pixels of `Raytracing::render(x, y)` (src/raytracing.rs:275-427) in one call."""
        return self.device_scene.render(self.camera.c_struct(), self.config, sample_xy=sample_xy, aux=aux)

    def render_pixels(self, pixels=None, rgba8: bool = False, sample_xy=None) -> dict:
        """`Raytracing::render(x, y)` before its clamp, as linear floats (rr_render_pixels): for `pixels`, an (n, 2) array of (x, y) or
        an (n,) uint32 array of x | y << 16, or for the whole frame in row-major order (None) -> dict(color, depth, normal, object_id
        [, rgba: the frame's own bytes])."""
        return self.device_scene.render_pixels(self.camera.c_struct(), self.config, pixels=pixels, sample_xy=sample_xy, rgba8=rgba8)

    def render_pixel_parts(self, pixels=None, n_parts: int = 2, sample_xy=None) -> dict:
        """render_pixels, and per pixel the means over its n_parts interleaved sample subsets (rr_render_pixel_parts): the dict of
        render_pixels plus parts = dict(color (n, K, 3), depth (n, K), normal (n, K, 3), object_id (n, K))."""
        return self.device_scene.render_pixel_parts(self.camera.c_struct(), self.config, pixels=pixels, n_parts=n_parts, sample_xy=sample_xy)

    def render_pixel_split(self, pixels=None, halves: bool = True, sample_xy=None) -> dict:
        """render_pixel_parts at n_parts = 2 (render_pixels with halves=False) and, as a sum of its own, the frame's direct diffuse light of the
        primary hits (rr_render_pixel_split): the dict of render_pixel_parts plus diffuse (n, 3) and, with halves, diffuse_halves (n, 2, 3).
        color - diffuse is everything else: ambient and fog, highlights, what mirrors and glass show."""
        return self.device_scene.render_pixel_split(self.camera.c_struct(), self.config, pixels=pixels, halves=halves, sample_xy=sample_xy)

    def denoise_split(self, records, diffuse, halves=None, diffuse_halves=None, albedo=None, params=None, rgba8: bool = False) -> dict:
        """rr_denoise_split_records over a frame of this camera: denoise() with the albedo applied to `diffuse` (n, 3), the direct diffuse part
        of the colour (render_pixel_split), alone; `diffuse_halves` (n, 2, 3) exactly when `halves` is given.  Returns dict(records (n, 8),
        color, depth, normal, object_id [, rgba]).  The result is, bit for bit, denoise.atrous_denoise_split of the same arrays."""
        cam = self.camera.c_struct()
        res = self.device_scene.denoise_split(int(cam.width), int(cam.height), records, diffuse, halves, diffuse_halves, albedo, params, rgba8=rgba8)
        return dict(res, **capi._records(res["records"]))

    def denoise(self, records, halves=None, albedo=None, params=None, rgba8: bool = False) -> dict:
        """rr_denoise_records over a frame of this camera: `records` (n, 8) float32 rr_radiance records in row-major order (what
        render_pixels gives, as records), `halves` (n, 2, 8) or None (render_pixel_parts at n_parts = 2), `albedo` (n, 3) or None, `params`
        a denoise.DenoiseParams or None for the defaults.  Returns dict(records (n, 8), variance (n,), color, depth, normal, object_id:
        copies of the filtered records' fields [, rgba: the frame's bytes of the filtered records]).  The result is, bit for bit,
        denoise.atrous_denoise of the same arrays."""
        cam = self.camera.c_struct()
        res = self.device_scene.denoise_records(int(cam.width), int(cam.height), records, halves, albedo, params, rgba8=rgba8)
        return dict(res, **capi._records(res["records"]))

    def surface_pixels(self, pixels=None):
        """The G-buffer of this camera (rr_surface_pixels): the rr_surface_hit record of the pixel-centre ray of every pixel of `pixels`
        (as render_pixels takes them) or of the whole frame in row-major order (None) -> a structured array (flat.SURFACE_HIT_DTYPE)."""
        return self.device_scene.surface_pixels(self.camera.c_struct(), pixels=pixels, records=True, albedo=False)

    def albedo(self) -> np.ndarray:
        """The albedo of the whole frame of this camera, (n, 3) float32 in row-major order: what denoise() takes as `albedo` (the
        base_color of surface_pixels(), 0 where the pixel's centre ray hits nothing)."""
        return self.device_scene.surface_pixels(self.camera.c_struct(), records=False, albedo=True)

    def mean_albedo(self, samples: Optional[int] = None, sample_xy=None) -> np.ndarray:
        """The albedo of the whole frame of this camera as the frame at `samples` (default: the config's) sees it, (n, 3) float32 in
        row-major order (rr_albedo_pixels): per pixel the mean over the frame's primary rays -- its sub-sample table, its depth of field --
        of the base colour at each ray's first hit.  What denoise() should take as `albedo` for a frame of that many samples: a pixel on a
        texture edge or a silhouette holds the mix its colour was modulated by, where albedo() holds the colour under its centre."""
        cfg = rr_config.from_buffer_copy(self.config)
        if samples is not None:
            cfg.samples = samples
        return self.device_scene.albedo_pixels(self.camera.c_struct(), cfg, sample_xy=sample_xy)

    def mean_albedo_torch(self, samples: Optional[int] = None, sample_xy=None):
        """mean_albedo on torch's current stream, without a host trip (rr_albedo_pixels_device): an (n, 3) float32 CUDA tensor."""
        cfg = rr_config.from_buffer_copy(self.config)
        if samples is not None:
            cfg.samples = samples
        return albedo_pixels_torch(self.device_scene, self.camera.c_struct(), cfg, None, sample_xy=sample_xy)

    def render_denoised(self, samples: Optional[int] = None, params=None, sample_xy=None, rgba8: bool = False, albedo=False) -> dict:
        """The whole frame at `samples` (default: the config's; even) in two halves, followed by the filter guided by their variance: one
        rr_render_pixel_parts call at n_parts = 2 and one rr_denoise_records call.  albedo=True: one rr_surface_pixels call between them
        makes this camera's albedo and the filter runs on albedo-demodulated colour; the result then holds it as `albedo`.  albedo="mean":
        one rr_albedo_pixels call with the frame's config and table stands in its place (mean_albedo).  albedo="diffuse": the frame comes
        from rr_render_pixel_split, the albedo is the mean one, and rr_denoise_split_records demodulates the direct diffuse part of the colour
        alone; the result then holds `diffuse` and `diffuse_halves` too, and no variance.  Returns the
        dict of denoise() plus `noisy`, the records before the filter.  render_denoised_torch is the same on the device, with no host trip."""
        cam = self.camera.c_struct()
        cfg = rr_config.from_buffer_copy(self.config)
        if samples is not None:
            cfg.samples = samples
        _check_albedo_mode(albedo)
        if _diffuse_mode(albedo):
            base = self.device_scene.render_pixel_split(cam, cfg, sample_xy=sample_xy)
            records, halves = _pack_records(base), _pack_records(base["parts"])
            guide = self.device_scene.albedo_pixels(cam, cfg, sample_xy=sample_xy)
            res = self.denoise_split(records, base["diffuse"], halves, base["diffuse_halves"], guide, params, rgba8=rgba8)
            return dict(res, noisy=records, albedo=guide, diffuse=base["diffuse"], diffuse_halves=base["diffuse_halves"])
        base = self.device_scene.render_pixel_parts(cam, cfg, n_parts=2, sample_xy=sample_xy)
        records = _pack_records(base)
        halves = _pack_records(base["parts"])
        if albedo:
            if _mean_mode(albedo):
                guide = self.device_scene.albedo_pixels(cam, cfg, sample_xy=sample_xy)
            else:
                guide = self.device_scene.surface_pixels(cam, records=False, albedo=True)
            return dict(self.denoise(records, halves, guide, params, rgba8=rgba8), noisy=records, albedo=guide)
        return dict(self.denoise(records, halves, None, params, rgba8=rgba8), noisy=records)

    def upsample(self, low_width: int, low_height: int, low, guide_low, guide, halves_low=None, params=None, rgba8: bool = False, albedo_low=None,
                 albedo=None) -> dict:
        """rr_upsample_records to a frame of this camera's size: `low` (w h, 8) and `halves_low` (w h, 2, 8) or None are the records of a
        frame traced at low_width x low_height, `guide_low` and `guide` the surface_pixels() of the small and of this camera.  Returns
        dict(records (n, 8), halves (n, 2, 8) or None, weight (n,), color, depth, normal, object_id [, rgba]); bit for bit
        upsample.upsample_records of the same arrays.  albedo_low (w h, 3) and albedo (n, 3), each or None: albedo planes in place of
        the guides' base colours (rr_upsample_albedo_records), e.g. mean_albedo() of the two cameras."""
        cam = self.camera.c_struct()
        res = self.device_scene.upsample(low_width, low_height, int(cam.width), int(cam.height), low, guide_low, guide, halves_low, params, rgba8=rgba8,
                                         albedo_low=albedo_low, albedo=albedo)
        return dict(res, **capi._records(res["records"]))

    def render_upsampled(self, scale=2, samples: Optional[int] = None, params=None, denoise_params=None, fill_holes: bool = False, rgba8: bool = False,
                         albedo=True, full_albedo_samples: Optional[int] = None, low_denoise_params=None) -> dict:
        """The frame traced at ceil(W / scale) x ceil(H / scale) with this camera's matrices and raised to W x H by the G-buffer: one
        rr_render_pixel_parts call at n_parts = 2 on the small camera, one rr_surface_pixels call on each camera, one rr_upsample_records
        call with halves, and with `denoise_params` one rr_denoise_records call at full size with the full guide's albedo.  fill_holes:
        the pixels the guide found no tap for (weight 0) on a surface (guide.hit) are traced at full resolution, one rr_render_pixel_parts
        call on their list, and written over the records and halves before the filter.  Returns dict(records, halves, weight, color,
        depth, normal, object_id, low_width, low_height, holes: the list as x | y << 16, count, albedo_low, albedo: the planes the
        upsampler took, or None [, variance][, rgba]).
        albedo: True, the guides' pixel-centre albedo; "mean": the low frame is demodulated by rr_albedo_pixels on the small camera with
        the low frame's config -- the mean over the rays that made the colour (rr_upsample_albedo_records).  full_albedo_samples: None,
        or k >= 1: rr_albedo_pixels on this camera at k samples remodulates in place of the full guide's centre albedo and, with
        `denoise_params`, is the full-size filter's albedo.  low_denoise_params: rr_denoise_records at the LOW size on the low records and
        halves before the upsampler, with the low albedo in use; the filtered records are raised without halves (`halves` is None,
        fill_holes writes records only, and the full-size filter runs without halves); `low_filtered` holds them.
        render_upsampled_torch is the same on the device, on one stream."""
        _check_upsampled_options(albedo, full_albedo_samples)
        cam = self.camera.c_struct()
        cfg = rr_config.from_buffer_copy(self.config)
        if samples is not None:
            cfg.samples = samples
        W, H = int(cam.width), int(cam.height)
        low_cam, w, h = _low_camera(cam, scale)
        ds = self.device_scene
        base = ds.render_pixel_parts(low_cam, cfg, n_parts=2)
        guide_low = ds.surface_pixels(low_cam, records=True, albedo=False)
        guide = ds.surface_pixels(cam, records=True, albedo=False)
        low, halves_low = _pack_records(base), _pack_records(base["parts"])
        albedo_low = ds.albedo_pixels(low_cam, cfg) if _mean_mode(albedo) else None
        albedo_full = ds.albedo_pixels(cam, _config_at(cfg, full_albedo_samples)) if full_albedo_samples is not None else None
        low_filtered = None
        if low_denoise_params is not None:
            guide_albedo = albedo_low if albedo_low is not None else np.ascontiguousarray(guide_low["base_color"][:, 0:3])
            low = low_filtered = ds.denoise_records(w, h, low, halves_low, guide_albedo, low_denoise_params, variance=False)["records"]
            halves_low = None
        res = ds.upsample(w, h, W, H, low, guide_low, guide, halves_low, params, rgba8=rgba8, albedo_low=albedo_low, albedo=albedo_full)
        holes = np.zeros(0, np.uint32)
        if fill_holes:
            at = np.flatnonzero((res["weight"] == 0) & (guide["hit"] != 0))
            holes = ((at % W) | ((at // W) << 16)).astype(np.uint32)
            if len(holes):
                cfg_b = rr_config.from_buffer_copy(cfg)
                cfg_b.gamma_correction = capi.upsample_params(params).gamma_correction
                fine = ds.render_pixel_parts(cam, cfg_b, pixels=holes, n_parts=2)
                res["records"][at] = _pack_records(fine)
                if res["halves"] is not None:
                    res["halves"][at] = _pack_records(fine["parts"])
                if rgba8:
                    res["rgba"][at] = ds.render_pixels(cam, cfg_b, pixels=holes, rgba8=True)["rgba"]
        res.update(low_width=w, low_height=h, holes=holes, count=len(holes), albedo_low=albedo_low, albedo=albedo_full)
        if low_filtered is not None:
            res["low_filtered"] = low_filtered
        if denoise_params is not None:
            albedo = albedo_full if albedo_full is not None else np.ascontiguousarray(guide["base_color"][:, 0:3])
            res.update(upsampled=res["records"], **self.device_scene.denoise_records(W, H, res["records"], res["halves"], albedo, denoise_params, rgba8=rgba8))
        return dict(res, **capi._records(res["records"]))

    def render_temporal(self, state: "TemporalState", samples: Optional[int] = None, denoise_params=None, accumulate_params=None, seed: Optional[int] = None,
                        motion=None, sample_xy=None, rgba8: bool = False, track_items: bool = False, albedo=False, clamp=None) -> dict:
        """One frame of a frame-after-frame loop at `samples` (default: the config's; even) and `seed` (default: the config's): the frame
        in two halves, blended into the history `state` carries from the previous call (rr_accumulate_records, reprojected through the
        camera of that call), then the filter guided by the accumulated halves.  render_temporal_torch on this scene and camera: three
        calls on one stream, no host trip; the result holds torch tensors.  Move self.camera (or the scene) between calls; give `motion`
        (n, 3) for what moved in the world, or track_items=True: the state notes `trans` of every item of self.flat_scene at each call,
        the next call lists the items whose 16 floats differ bitwise, and rr_motion_records makes their motion on the device (a fourth
        call on the same stream); a change of the item count or of any item's id resets the state, and so does a history from a call
        without track_items.  albedo=True: one more call on the same stream (rr_surface_pixels_device) makes this camera's albedo for the
        filter; the accumulation is not changed, it blends un-demodulated colour.  albedo="mean": rr_albedo_pixels_device with the frame's
        config and table in its place.  albedo="diffuse" raises ValueError: the diffuse part is accumulated over time by
        render_temporal_split, a pipeline of its own.  clamp: None or False is rr_accumulate_records; True (the library's defaults) or a
        temporal.HistoryClampParams puts rr_accumulate_clamped_records in its place, which holds the history to the current frame's colours
        around each pixel: for frames after an edit of lights, materials, textures or item flags, and under moving shadows."""
        _check_albedo_mode(albedo, temporal=True)
        return self._render_temporal(render_temporal_torch, state, samples, denoise_params, accumulate_params, seed, motion, sample_xy, rgba8, track_items,
                                     albedo=albedo, clamp=_clamp_params(clamp))

    def _render_temporal(self, pipeline, state: "TemporalState", samples, denoise_params, accumulate_params, seed, motion, sample_xy, rgba8, track_items, **kw):
        """What the three render_temporal* methods share, behind their refusals (so a refused call leaves the state as it was): the frame's
        config and the moved items, then `pipeline`, the method's render_temporal*_torch, on this scene and camera with this camera's view."""
        from .temporal import previous_view
        cfg, moved = self._temporal_frame(state, samples, seed, motion, track_items)
        return pipeline(self.device_scene, self.camera.c_struct(), cfg, state, accumulate_params, denoise_params, motion=motion, sample_xy=sample_xy, rgba8=rgba8,
                        view=previous_view(self.camera), moved=moved, **kw)

    def _temporal_frame(self, state: "TemporalState", samples, seed, motion, track_items: bool):
        """What render_temporal and render_temporal_split do before their pipeline: the frame's config, and with track_items the moved items
        against the history (the state notes this frame's) -> (cfg, moved or None)."""
        cfg = rr_config.from_buffer_copy(self.config)
        if samples is not None:
            cfg.samples = samples
        if seed is not None:
            cfg.seed = seed
        moved = None
        if track_items:
            if motion is not None:
                raise ValueError("give track_items=True (the motion is made on the device) or `motion`, not both")
            items = self.flat_scene.items
            moved = state.track([it.id for it in items], np.stack([np.asarray(it.trans, np.float32) for it in items]) if items else np.zeros((0, 4, 4), np.float32))
            if moved is None:
                moved = (np.zeros(0, np.uint32), np.zeros((0, 4, 4), np.float32))
        else:
            state.items = None
        return cfg, moved

    def render_temporal_split(self, state: "TemporalState", samples: Optional[int] = None, denoise_params=None, accumulate_params=None, seed: Optional[int] = None,
                              motion=None, sample_xy=None, rgba8: bool = False, track_items: bool = False, clamp=None) -> dict:
        """render_temporal with the frame's direct diffuse light accumulated as layers of its own and the mean albedo applied to it alone:
        rr_render_pixel_split, (with moved items) rr_motion_records, rr_accumulate_split_records, rr_albedo_pixels and
        rr_denoise_split_records -- render_temporal_split_torch on this scene and camera, on one stream with no host trip.  The arguments are
        render_temporal's, without `albedo`; `state` is a TemporalState of this pipeline's (one that render_temporal filled starts anew).
        The result holds torch tensors: render_temporal's, and diffuse, diffuse_halves, accumulated_diffuse, accumulated_diffuse_halves and
        albedo.  clamp: anything but None or False raises ValueError that names render_temporal_split_clamped, the pipeline with the clamped
        accumulation."""
        _no_split_clamp(clamp)
        return self._render_temporal(render_temporal_split_torch, state, samples, denoise_params, accumulate_params, seed, motion, sample_xy, rgba8, track_items)

    def render_temporal_split_clamped(self, state: "TemporalState", samples: Optional[int] = None, denoise_params=None, accumulate_params=None,
                                      seed: Optional[int] = None, motion=None, sample_xy=None, rgba8: bool = False, track_items: bool = False, clamp=True) -> dict:
        """render_temporal_split with the history held to the current frame (rr_accumulate_clamped_split_records in the place of
        rr_accumulate_split_records): the colour layers to the box of the current colours around each pixel, the diffuse layers to the box of
        the current diffuse layer -- render_temporal_split_clamped_torch on this scene and camera, on one stream with no host trip.  For the
        frames after an edit of lights, materials, textures or item flags, and under moving shadows; a state may go from one of the two
        pipelines to the other from frame to frame.  clamp: True (the library's defaults) or a temporal.HistoryClampParams; None or False
        raises ValueError.  The other arguments and the result are render_temporal_split's."""
        clamp = _clamp_params(clamp)         # (refused before the state notes this frame's items)
        if clamp is None:
            raise ValueError("clamp is True (the defaults) or a temporal.HistoryClampParams; without a clamp the pipeline is render_temporal_split")
        return self._render_temporal(render_temporal_split_clamped_torch, state, samples, denoise_params, accumulate_params, seed, motion, sample_xy, rgba8, track_items,
                                     clamp=clamp)


    def render_adaptive(self, base_samples: int, max_samples: int, threshold: float, sample_xy_base=None, sample_xy_max=None) -> dict:
        """Two sample counts in one frame: every pixel at `base_samples`, and at `max_samples` where the half-buffer estimate of the
        base frame's error (adaptive.half_error of the two interleaved halves, one rr_render_pixel_parts call) exceeds `threshold`
        (one rr_render_pixels call for adaptive.refine_list).  Returns the frame in row-major order: dict(color (n, 3) LINEAR, depth,
        normal, object_id, samples: the count each pixel was rendered at, error: the estimate).  Every pixel is, bit for bit, the
        rr_render_pixels pixel at the sample count `samples` names."""
        from . import adaptive
        cam = self.camera.c_struct()
        w, h = int(cam.width), int(cam.height)
        cfg = rr_config.from_buffer_copy(self.config)
        cfg.samples = base_samples
        base = self.device_scene.render_pixel_parts(cam, cfg, n_parts=2, sample_xy=sample_xy_base)
        error = adaptive.half_error(base["parts"]["color"])
        xy, count = adaptive.refine_list(error, threshold, w, h)
        res = {k: base[k].copy() for k in ("color", "depth", "normal", "object_id")}
        samples = np.full(w * h, base_samples, np.uint32)
        if count:
            cfg.samples = max_samples
            fine = self.device_scene.render_pixels(cam, cfg, pixels=xy, sample_xy=sample_xy_max)
            at = (xy[:count] >> np.uint32(16)).astype(np.int64) * w + (xy[:count] & np.uint32(0xffff)).astype(np.int64)
            for k in res:
                res[k][at] = fine[k][:count]
            samples[at] = max_samples
        res["samples"] = samples
        res["error"] = error
        return res

    def render_adaptive_on_device(self, base_samples: int, max_samples: int, threshold: float, sample_xy_base=None, sample_xy_max=None, rgba8: bool = False) -> dict:
        """render_adaptive as ONE library call (rr_render_adaptive): the estimate, the list, the fine pass and the scatter run on the device
        under one hold of the scene's lock.  Returns what render_adaptive returns, field for field and bit for bit, plus n_refined, and
        `rgba`, the frame's own bytes, with rgba8=True."""
        return self.device_scene.render_adaptive(self.camera.c_struct(), self.config, base_samples, max_samples, threshold, sample_xy_base=sample_xy_base,
                                                 sample_xy_max=sample_xy_max, rgba8=rgba8)

    def _render_ladder(self, counts, threshold: float, render_level) -> dict:
        """The host loop behind render_adaptive_levels and render_adaptive_prefix: render_level(l, pixels) renders level l of the ladder
        `counts` in two halves, for the whole frame (pixels None, level 0) or for a padded list, and returns the dict of
        render_pixel_parts.  The lists are adaptive.refine_list, then adaptive.refine_sublist, until one is empty or the top is reached."""
        from . import adaptive
        cam = self.camera.c_struct()
        w, h = int(cam.width), int(cam.height)
        base = render_level(0, None)
        res = {k: base[k].copy() for k in ("color", "depth", "normal", "object_id")}
        error = adaptive.half_error(base["parts"]["color"])
        samples = np.full(w * h, counts[0], np.uint32)
        level_pixels, padded = [w * h] + [0] * (len(counts) - 1), [w * h] + [0] * (len(counts) - 1)
        xy, count = adaptive.refine_list(error, threshold, w, h)
        for l in range(1, len(counts)):
            if not count:
                break
            fine = render_level(l, xy)
            level_pixels[l], padded[l] = count, len(xy)
            at = (xy[:count] >> np.uint32(16)).astype(np.int64) * w + (xy[:count] & np.uint32(0xffff)).astype(np.int64)
            for k in res:
                res[k][at] = fine[k][:count]
            samples[at] = counts[l]
            e = adaptive.half_error(fine["parts"]["color"])
            error[at] = e[:count]
            xy, count = adaptive.refine_sublist(e, threshold, xy, count)
        res["samples"] = samples
        res["error"] = error
        res["level_pixels"] = level_pixels
        res["padded"] = padded
        return res

    def render_adaptive_levels(self, levels, threshold: float, sample_xy_levels=None) -> dict:
        """A ladder of sample counts in one frame, as a HOST LOOP over library calls: every pixel at levels[0] in two halves (one
        rr_render_pixel_parts call), and level after level the pixels whose half-buffer error (adaptive.half_error) still exceeds
        `threshold`, again in two halves at the next count (one rr_render_pixel_parts call per list: adaptive.refine_list, then
        adaptive.refine_sublist), until the list is empty or the top count is reached.  Returns the frame in row-major order:
        dict(color (n, 3) LINEAR, depth, normal, object_id, samples: the count of the last level that rendered the pixel, error: the
        estimate at THAT count -- the residual error --, level_pixels: the pixels of each level before the pad, padded: each level's
        list length with it).  Every pixel is, bit for bit, the rr_render_pixels pixel at the count `samples` names."""
        levels = [int(v) for v in levels]
        tables = list(sample_xy_levels) if sample_xy_levels is not None else [None] * len(levels)
        cam = self.camera.c_struct()
        cfg = rr_config.from_buffer_copy(self.config)

        def render_level(l, pixels):
            cfg.samples = levels[l]
            return self.device_scene.render_pixel_parts(cam, cfg, pixels=pixels, n_parts=2, sample_xy=tables[l])
        return self._render_ladder(levels, threshold, render_level)

    def render_adaptive_levels_on_device(self, levels, threshold: float, sample_xy_levels=None, rgba8: bool = False) -> dict:
        """render_adaptive_levels as ONE library call (rr_render_adaptive_levels): every pass, list and scatter runs on the device under one
        hold of the scene's lock.  Returns what render_adaptive_levels returns, field for field and bit for bit (without `padded`), and
        `rgba`, the frame's own bytes, with rgba8=True."""
        return self.device_scene.render_adaptive_levels(self.camera.c_struct(), self.config, levels, threshold, sample_xy_levels=sample_xy_levels, rgba8=rgba8)

    def render_pixel_prefix(self, samples_used: int, pixels=None, halves: bool = False, rgba8: bool = False, sample_xy=None) -> dict:
        """render_pixels over the first `samples_used` samples of the frame of config.samples samples (rr_render_pixel_prefix): that
        frame's table, cell size and generator keys, the sums divided by samples_used; with halves=True plus `parts`, the two
        interleaved halves of those samples as render_pixel_parts gives them at n_parts = 2."""
        return self.device_scene.render_pixel_prefix(self.camera.c_struct(), self.config, pixels=pixels, samples_used=samples_used, halves=halves,
                                                     sample_xy=sample_xy, rgba8=rgba8)

    def render_adaptive_prefix(self, prefix_samples, threshold: float, sample_xy=None) -> dict:
        """A ladder of PREFIXES of one frame of config.samples samples (the last prefix), as a HOST LOOP over library calls that renders
        each prefix from scratch: every pixel over the first prefix_samples[0] samples in two halves (one rr_render_pixel_prefix call),
        and level after level the pixels whose half-buffer error (adaptive.half_error) still exceeds `threshold`, over the next
        prefix (adaptive.refine_list, then adaptive.refine_sublist), until the list is empty or the whole frame is reached.  Returns
        the dict of render_adaptive_levels.  Every pixel is, bit for bit, the rr_render_pixel_prefix pixel at the count `samples`
        names.  This is the yardstick of render_adaptive_prefix_on_device, which traces every sample once."""
        prefixes = [int(v) for v in prefix_samples]
        cam = self.camera.c_struct()
        if not prefixes or prefixes[-1] != int(self.config.samples):
            raise ValueError(f"prefix_samples {prefixes}: the last prefix must be config.samples = {int(self.config.samples)}")
        return self._render_ladder(prefixes, threshold, lambda l, pixels: self.device_scene.render_pixel_prefix(
            cam, self.config, pixels=pixels, samples_used=prefixes[l], halves=True, sample_xy=sample_xy))

    def render_adaptive_prefix_on_device(self, prefix_samples, threshold: float, sample_xy=None, rgba8: bool = False) -> dict:
        """render_adaptive_prefix as ONE library call (rr_render_adaptive_prefix): the sums of a listed pixel stay on the device and every
        level adds only the samples the pixel does not have yet.  Returns what render_adaptive_prefix returns, field for field and bit
        for bit (without `padded`), and `rgba`, the frame's own bytes, with rgba8=True."""
        return self.device_scene.render_adaptive_prefix(self.camera.c_struct(), self.config, prefix_samples, threshold, sample_xy=sample_xy, rgba8=rgba8)

    def pick(self, x: int, y: int):
        """Raytracing::pick (src/raytracing.rs:237-273): Some((id, distance)) or None."""
        r = self.device_scene.pick(self.camera.c_struct(), x, y)
        return (int(r.object_id), float(r.distance)) if r.hit else None

    def apply_scene(self, new_flat: FlatScene, structural: bool = False) -> list:
        """The host's restart after a scene edit (Run::restart_rendering, reference src/run.rs:395-420): brings the device scene
        to `new_flat` by the cheapest correct path (plan_scene_update) and returns the plan it carried out.  In-place steps run in
        order; if one fails the scene is created anew from `new_flat` and [RECREATE] is returned.  The new handle is created
        before the old one is released, so a failed re-create leaves the old scene in place (and raises).
        structural=True: an edit of the item list, the material list or the mesh list keeps the handle too (STRUCTURAL_STEPS):
        unseen meshes are appended to the resident ones and the items name meshes by their resident index."""
        resident = self.resident_meshes
        plan = plan_scene_update(self.flat_scene, new_flat, structural=structural, resident_meshes=resident)
        if plan != [RECREATE]:
            ds = self.device_scene
            try:
                for step in plan:
                    if step == "add_textures":
                        ds.add_textures(new_flat.textures[len(self.flat_scene.textures):])
                    elif step == "add_meshes":
                        ds.add_meshes(_resident_mesh_indices(resident, new_flat.meshes)[1])
                    elif step == "set_items":
                        index, appended = _resident_mesh_indices(resident, new_flat.meshes)
                        items = [copy.copy(it) for it in new_flat.items]
                        for it in items:
                            if it.mesh >= 0:
                                it.mesh = index[it.mesh]
                        ds.set_items(items, new_flat.materials)
                        resident = resident + appended
                    elif step == "update_materials":
                        ds.update_materials(new_flat.materials)
                    elif step == "update_transforms":
                        ds.update_transforms(np.stack([np.asarray(it.trans, np.float32) for it in new_flat.items]),
                                             np.stack([np.asarray(it.trans_inv, np.float32) for it in new_flat.items]))
                    elif step == "update_item_flags":
                        ds.update_item_flags([it.visible for it in new_flat.items], [it.flip_normals for it in new_flat.items])
                    elif step == "update_lights":
                        ds.update_lights(new_flat.lights)
            except capi.RustrayHipError:
                plan = [RECREATE]
        if plan == [RECREATE]:
            fresh = capi.DeviceScene(new_flat, self.device_scene.device)
            self.device_scene.close()
            self.device_scene = fresh
            resident = list(new_flat.meshes)
        self.resident_meshes = resident
        self.flat_scene = new_flat
        return plan

    def close(self):
        self.device_scene.close()


class RendererManager:
    """Call surface of reference `RendererManager` (src/renderer.rs:63-251)."""

    def __init__(self, width: int, height: int, raytracing: Raytracing):
        self.width, self.height = width, height
        self.raytracing = raytracing
        self.thread_amount = 1  # one frame-level device call replaces the worker threads
        self._running = False
        self._pixels_rendered = 0
        self._start = time.time()
        self._done_ms = 0
        self.image = self.normals = self.depth = self.objects = None

    def update_resolution(self, width: int, height: int):
        self.width, self.height = width, height

    def start(self, on_pass=None, min_passes: int = 8):
        """One frame.  With `on_pass(manager)` the frame is rendered progressively: after every device batch the
        image buffers hold the frame over the samples finished so far (what Run::apply_pixels shows while the
        reference renders, src/run.rs:506-545) and the callback may call `stop()` to end the frame early
        (RendererManager::stop, src/renderer.rs:174-198)."""
        self._start = time.time()
        self._done_ms = 0
        self._pixels_rendered = 0
        self._running = True
        self.raytracing.camera.init(self.width, self.height)
        if on_pass is not None:
            def _pass(out, done, total):
                self.image, self.normals, self.depth, self.objects = out["rgba"], out["normal"], out["depth"], out["object_id"]
                # the reference counts finished pixels; a pass finishes a share of every pixel's samples
                self._pixels_rendered = (self.width * self.height * done) // total
                on_pass(self)
                return not self._running
            try:
                out = self.raytracing.device_scene.render_progressive(self.raytracing.camera.c_struct(), self.raytracing.config,
                                                                      _pass, min_passes=min_passes)
            except capi.RustrayHipError as e:
                if e.code != -6:
                    raise
                self._done_ms = int((time.time() - self._start) * 1000.0)
                return  # stopped: the buffers keep the last preview
        else:
            out = self.raytracing.render_frame()
        # what Run::apply_pixels stores per PixelData (src/run.rs:519-541)
        self.image, self.normals, self.depth, self.objects = out["rgba"], out["normal"], out["depth"], out["object_id"]
        self._pixels_rendered = self.width * self.height
        self._done_ms = int((time.time() - self._start) * 1000.0)

    def stop(self):
        self._running = False

    def restart(self, width: int, height: int):
        self.stop()
        self.update_resolution(width, height)
        self.start()

    def is_running(self) -> bool:
        return self._running

    def is_done(self) -> bool:
        return self._pixels_rendered == self.width * self.height

    def get_rendered_pixels(self) -> int:
        return self._pixels_rendered

    def check_and_get_elapsed_time(self) -> int:
        return self._done_ms if self._done_ms > 0 else int((time.time() - self._start) * 1000.0)


# ---------------------------------------------------------------------------
# animation: the frame loop, one frame per GPU at a time
# ---------------------------------------------------------------------------
class AnimationRun:
    """The reference's animation loop (Run::render_next_frame_if_possible, src/run.rs:421-465: apply_frame, restart,
    wait for completion, next frame) over ONE resident device scene: only the item transforms change per frame
    (Scene::apply_frame, src/scene.rs:1695-1713 -> rr_scene_update_transforms), geometry, per-mesh trees and textures
    stay in HBM.  With world_size > 1 the frames are dealt round-robin to the ranks (one process per GPU, scene
    replicated): frames are independent, so the data path needs no collective; `gather()` brings the finished
    RGBA8 frames to rank 0 if one process is to write them out."""

    def __init__(self, raytracing: Raytracing, animation, rank: int = 0, world_size: int = 1, start_frame: int = 0):
        self.raytracing, self.animation = raytracing, animation
        self.rank, self.world_size = rank, world_size
        self.frames = animation.frames_to_render(start_frame)

    def my_frames(self, rank: Optional[int] = None):
        r = self.rank if rank is None else rank
        return self.frames[r::self.world_size]

    def render(self, on_frame=None, render_fn=None) -> dict:
        """{frame: out} for this rank's frames.  render_fn(frame) replaces the device call (host-logic tests)."""
        done = {}
        for f in self.my_frames():
            if render_fn is not None:
                out = render_fn(f)
            else:
                tr = self.animation.frame_transforms(self.raytracing.flat_scene, f)
                if tr is not None:
                    self.raytracing.device_scene.update_transforms(*tr)
                out = self.raytracing.render_frame()
            done[f] = out
            if on_frame is not None:
                on_frame(f, out)
        return done

    def gather(self, done: dict, via_cpu: bool = False):
        """Rank 0: list of (frame, rgba) in frame order; other ranks: None.  One gather of the stacked RGBA8 frames."""
        import torch
        import torch.distributed as dist
        mine = self.my_frames()
        if self.world_size == 1:
            return [(f, done[f]["rgba"]) for f in mine]
        on_gpu = (not via_cpu) and torch.cuda.is_available() and dist.get_backend() == "nccl"  # RCCL moves device tensors only
        h, w = (done[mine[0]]["rgba"].shape[:2]) if mine else (0, 0)
        shape = torch.tensor([h, w], dtype=torch.int64, device="cuda" if on_gpu else "cpu")
        dist.all_reduce(shape, op=dist.ReduceOp.MAX)  # a rank without frames still needs the shape
        h, w = int(shape[0]), int(shape[1])
        n_max = max(len(self.my_frames(r)) for r in range(self.world_size))
        pad = torch.zeros((n_max, h, w, 4), dtype=torch.uint8)
        for i, f in enumerate(mine):
            pad[i] = torch.from_numpy(np.ascontiguousarray(done[f]["rgba"]))
        if on_gpu:
            pad = pad.cuda()
        gl = [torch.empty_like(pad) for _ in range(self.world_size)] if self.rank == 0 else None
        dist.gather(pad, gl, dst=0)
        if self.rank != 0:
            return None
        out = []
        for r in range(self.world_size):
            for i, f in enumerate(self.my_frames(r)):
                out.append((f, gl[r][i].cpu().numpy()))
        return sorted(out, key=lambda t: t[0])


# ---------------------------------------------------------------------------
# multi-GPU tiling
# ---------------------------------------------------------------------------
def region_pixels(width: int, height: int, tile_w: int, tile_h: int, n_ranks: int, rank: int) -> np.ndarray:
    """(n, 2) array of (x, y) in the order `rr_region` defines (include/rustray_hip.h)."""
    tx, ty = (width + tile_w - 1) // tile_w, (height + tile_h - 1) // tile_h
    out = []
    for t in range(rank, tx * ty, n_ranks):
        x0, y0 = (t % tx) * tile_w, (t // tx) * tile_h
        x1, y1 = min(x0 + tile_w, width), min(y0 + tile_h, height)
        ys, xs = np.mgrid[y0:y1, x0:x1]
        out.append(np.stack([xs.ravel(), ys.ravel()], axis=1))
    return np.concatenate(out).astype(np.int64) if out else np.zeros((0, 2), np.int64)


class TiledFrame:
    """One rank of a tiled multi-GPU frame.

    render_fn(region, n_pixels) must return a dict of compact per-rank torch tensors
    {"rgba": (n,4) uint8, ["normal": (n,3) f32, "depth": (n,) f32, "object_id": (n,) int32]}.
    `gather()` collects them on rank 0 (torch.distributed; backend "nccl" is RCCL on ROCm, "gloo"
    on CPU) and returns full frames there, None elsewhere.
    """

    def __init__(self, width: int, height: int, rank: int, world_size: int, tile_w: int = 32, tile_h: int = 8):
        self.width, self.height = width, height
        self.rank, self.world_size = rank, world_size
        self.tile_w, self.tile_h = tile_w, tile_h
        self.counts = [len(region_pixels(width, height, tile_w, tile_h, world_size, r)) for r in range(world_size)]
        self.max_count = max(self.counts) if self.counts else 0
        self._index = None

    def region(self) -> rr_region:
        return rr_region(self.tile_w, self.tile_h, self.world_size, self.rank)

    def n_pixels(self) -> int:
        return self.counts[self.rank]

    def _frame_index(self, device):
        """index[y*W + x] = position of that pixel in the rank-ordered concatenation of compact buffers."""
        import torch
        if self._index is None or self._index.device != device:
            idx = np.zeros(self.width * self.height, np.int64)
            base = 0
            for r in range(self.world_size):
                xy = region_pixels(self.width, self.height, self.tile_w, self.tile_h, self.world_size, r)
                idx[xy[:, 1] * self.width + xy[:, 0]] = base + np.arange(len(xy))
                base += len(xy)
            self._index = torch.from_numpy(idx).to(device)
        return self._index

    # bytes per pixel of the buffers a rank can render, in packing order
    _SPEC = (("rgba", "uint8", 4, 4), ("normal", "float32", 3, 12), ("depth", "float32", 1, 4), ("object_id", "int32", 1, 4))

    def alloc(self, device, aux: bool, via_cpu: bool = False) -> dict:
        """Persistent buffers of this rank, allocated ONCE (outside any timed region) and reused every frame:
        `pack` = one byte buffer with a section of max_count pixels per rendered buffer (every section starts 4-byte
        aligned on every rank); the returned compact views into it are what `rr_render_region_device` fills, so the
        gather sends the pack as it is.  Rank 0 also holds the gather target (world x pack), the rank-ordered
        concatenation per buffer and the frame-order outputs."""
        import torch
        key = (str(device), bool(aux), bool(via_cpu))
        if getattr(self, "_alloc_key", None) == key:
            return self._parts
        spec = [sp for sp in self._SPEC if aux or sp[0] == "rgba"]
        pack_bytes = self.max_count * sum(sp[3] for sp in spec)
        self._pack = torch.zeros(max(pack_bytes, 4), dtype=torch.uint8, device=device)
        self._parts, self._section, off = {}, {}, 0
        n = self.n_pixels()
        for name, dt, comps, width in spec:
            self._section[name] = (off, width, getattr(torch, dt), comps)
            view = self._pack[off: off + n * width].view(getattr(torch, dt))
            self._parts[name] = view.reshape(n, comps) if comps > 1 else view.reshape(n)
            off += self.max_count * width
        self._pack_cpu = torch.zeros_like(self._pack, device="cpu").pin_memory() if (via_cpu and torch.cuda.is_available()) else (torch.zeros_like(self._pack, device="cpu") if via_cpu else None)
        self._gbuf = self._gbuf_dev = self._frame = None
        if self.world_size > 1 and self.rank == 0:
            self._gbuf = torch.zeros((self.world_size, max(pack_bytes, 4)), dtype=torch.uint8, device="cpu" if via_cpu else device)
            if via_cpu and torch.device(device).type == "cuda":
                self._gbuf_dev = torch.zeros_like(self._gbuf, device=device)   # gloo rehearsal: the gathered packs copied to the card once
        if self.rank == 0:
            self._frame = {name: torch.zeros((self.height * self.width, comps), dtype=getattr(torch, dt), device=device) for name, dt, comps, _ in spec}
        self._alloc_key = key
        return self._parts

    def gather(self, parts: dict, use_device_kernel: bool = False, via_cpu: bool = False) -> Optional[dict]:
        """ONE collective per frame: every rank sends its pack (RGBA8 and whichever aux buffers were rendered, one byte
        buffer), rank 0 gathers them (backend "nccl" = RCCL over xGMI, device tensors; `via_cpu` stages through host
        memory for "gloo", which cannot gather device tensors) and de-interleaves each buffer into frame order.
        With `parts` from `alloc()` nothing is allocated or packed here: the views ARE the pack's sections.

        ALIASING (device-kernel path): the returned tensors are reshaped VIEWS of this object's persistent frame buffers; the next
        `gather` overwrites them in place.  A caller that keeps a frame across calls -- to compare two consecutive frames, say --
        must `.clone()` it first (comparing two returned dicts without a copy always compares a buffer with itself)."""
        import torch
        import torch.distributed as dist
        keys = list(parts.keys())
        persistent = getattr(self, "_alloc_key", None) is not None and all(parts[k] is self._parts.get(k) for k in keys)
        if not persistent:   # ad-hoc tensors (tests, one-off frames): pack them into freshly allocated buffers
            dev = parts[keys[0]].device
            self.alloc(dev, aux=len(keys) > 1, via_cpu=via_cpu)
            for k in keys:
                self._parts[k].copy_(parts[k].reshape(self._parts[k].shape))
        dev = self._pack.device
        gathered, packs = None, self._pack   # world_size 1: this rank's own pack is the only one
        if self.world_size > 1:
            send = self._pack
            if via_cpu:
                self._pack_cpu.copy_(self._pack)
                send = self._pack_cpu
            gl = list(self._gbuf.unbind(0)) if self.rank == 0 else None
            dist.gather(send, gl, dst=0)
            if self.rank != 0:
                return None
            packs = self._gbuf
            if via_cpu and use_device_kernel and dev.type == "cuda":
                self._gbuf_dev.copy_(self._gbuf)
                packs = self._gbuf_dev
        out = {}
        if use_device_kernel and packs.is_cuda:
            # ONE launch for all buffers, straight from the gather target (rr_deinterleave_packed_device): no concatenation pass
            names = [sp[0] for sp in self._SPEC]
            so = [self._section[n][0] if n in keys else 0 for n in names]
            eb = [self._section[n][1] if n in keys else 0 for n in names]
            dp = [self._frame[n].data_ptr() if n in keys else 0 for n in names]
            capi.deinterleave_packed_device(self.width, self.height, self.tile_w, self.tile_h, self.world_size, packs.data_ptr(),
                                            packs.stride(0) if packs.dim() == 2 else packs.numel(), so, eb, dp,
                                            packs.device.index or 0, torch.cuda.current_stream().cuda_stream)
            for k in keys:
                out[k] = self._frame[k].reshape(self.height, self.width, -1)
            return out
        for k in keys:
            off, width, dt, comps = self._section[k]
            if self.world_size > 1:
                rows = [packs[r, off: off + self.counts[r] * width] for r in range(self.world_size)]
                cat = torch.cat(rows).view(dt).reshape(-1, comps)
            else:
                cat = self._parts[k].reshape(self.n_pixels(), comps)
            out[k] = cat.index_select(0, self._frame_index(cat.device)).reshape(self.height, self.width, -1)
        return out


def render_region_torch(device_scene: capi.DeviceScene, cam, cfg, tf: TiledFrame, aux: bool = False, sample_xy=None, via_cpu: bool = False) -> dict:
    """Render this rank's tiles on torch's current stream, straight into the sections of the rank's persistent pack
    buffer (TiledFrame.alloc): nothing is allocated per frame and `tf.gather` sends the pack as it is.

    ALIASING: the returned tensors are VIEWS of that persistent pack; the next call renders over them.  `.clone()` what must outlive
    the next frame."""
    import torch
    dev = torch.device("cuda", device_scene.device)
    parts = tf.alloc(dev, aux, via_cpu=via_cpu)
    ptrs = [parts["rgba"].data_ptr(), None, None, None]
    if aux:
        ptrs = [parts["rgba"].data_ptr(), parts["normal"].data_ptr(), parts["depth"].data_ptr(), parts["object_id"].data_ptr()]
    device_scene.render_region_device(cam, cfg, tf.region(), ptrs, torch.cuda.current_stream(dev).cuda_stream, sample_xy)
    return parts


# ---------------------------------------------------------------------------
# the ray queries on torch tensors: rays produced on the GPU are traced where they are, on torch's current stream
# ---------------------------------------------------------------------------
def _ray_tensor(device_scene: capi.DeviceScene, t, name: str, shape_tail=(3,), dtype=None):
    """`t` as the library reads it: a contiguous CUDA tensor of `dtype` (float32) and shape (n, *shape_tail) on the scene's device; raises otherwise."""
    import torch
    dtype = torch.float32 if dtype is None else dtype
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name}: a torch tensor is required, got {type(t).__name__}")
    if not t.is_cuda or (t.device.index or 0) != device_scene.device:
        raise ValueError(f"{name}: the tensor is on {t.device}, the scene on cuda:{device_scene.device}")
    if t.dtype != dtype:
        raise TypeError(f"{name}: dtype {t.dtype}, {dtype} is required")
    if t.dim() != 1 + len(shape_tail) or tuple(t.shape[1:]) != tuple(shape_tail):
        raise ValueError(f"{name}: shape {tuple(t.shape)}, (n, {', '.join(map(str, shape_tail))}) is required" if shape_tail else f"{name}: shape {tuple(t.shape)}, (n,) is required")
    if not t.is_contiguous():
        raise ValueError(f"{name}: the tensor must be contiguous")
    return t


def _frame_tensors(device_scene: capi.DeviceScene, width: int, height: int, tensors: dict, required=()) -> dict:
    """{name: (tensor or None, shape_tail)} as {name: what _ray_tensor makes of it, or None where the caller left it out and it is not
    `required`}: every tensor holds the width * height entries of the frame; raises otherwise."""
    n = int(width) * int(height)
    checked = {}
    for name, (value, tail) in tensors.items():
        checked[name] = t = _ray_tensor(device_scene, value, name, shape_tail=tail) if value is not None or name in required else None
        if t is not None and int(t.shape[0]) != n:
            raise ValueError(f"{name}: {int(t.shape[0])} entries for a frame of {int(width)}x{int(height)}")
    return checked


def _hit_views(rec, first: str) -> dict:
    """An (n, 5) int32 tensor of 20-byte hit records and its named column views (no copy): `first` (hit / occluded), item_index,
    object_id, face_id as int32 and distance viewed as float32."""
    import torch
    return {"records": rec, first: rec[:, 0], "item_index": rec[:, 1], "object_id": rec[:, 2], "face_id": rec[:, 3],
            "distance": rec.view(torch.float32)[:, 4]}


def trace_rays_torch(device_scene: capi.DeviceScene, origins, directions, depth: int = 2) -> dict:
    """rr_trace_rays_device on torch's current stream of the scene's device: `origins` / `directions` are contiguous float32 CUDA tensors
    of shape (n, 3) on that device (anything else raises).  Returns torch tensors, without a host copy and without a synchronisation
    of the results: dict(records (n, 5) int32, hit, item_index (-1 = nothing hit), object_id, face_id, distance (float32 view))."""
    import torch
    o = _ray_tensor(device_scene, origins, "origins")
    d = _ray_tensor(device_scene, directions, "directions")
    if d.shape[0] != o.shape[0]:
        raise ValueError(f"{o.shape[0]} origins, {d.shape[0]} directions")
    dev = torch.device("cuda", device_scene.device)
    n = int(o.shape[0])
    with torch.cuda.device(dev):
        rec = torch.empty((n, 5), dtype=torch.int32, device=dev)
        if n:
            device_scene.trace_rays_device(o.data_ptr(), d.data_ptr(), n, depth, rec.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
    return _hit_views(rec, "hit")


def surface_rays_torch(device_scene: capi.DeviceScene, origins, directions, depth: int = 1) -> dict:
    """rr_surface_rays_device on torch's current stream: as trace_rays_torch (depth 1 = a frame's primary ray).  Returns torch tensors,
    without a host copy and without a synchronisation of the results: dict(records (n, 32) float32 = n rr_surface_hit records, and
    views of it named as the struct's fields: hit, item_index, object_id, face_id, material, has_uv as int32 views; position, normal,
    shading_normal, ambient_color, specular_color (n, 3), base_color (n, 4), uv (n, 2), distance, alpha, reflectivity, roughness,
    ambient_occlusion (n,))."""
    import torch
    o = _ray_tensor(device_scene, origins, "origins")
    d = _ray_tensor(device_scene, directions, "directions")
    if d.shape[0] != o.shape[0]:
        raise ValueError(f"{o.shape[0]} origins, {d.shape[0]} directions")
    dev = torch.device("cuda", device_scene.device)
    n = int(o.shape[0])
    with torch.cuda.device(dev):
        rec = torch.empty((n, 32), dtype=torch.float32, device=dev)   # (torch allocations are at least 512-byte aligned)
        if n:
            device_scene.surface_rays_device(o.data_ptr(), d.data_ptr(), n, depth, rec.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
    return _surface_views(rec)


def _surface_views(rec) -> dict:
    """`records`, (n, 32) float32 = n rr_surface_hit records on the device, and the views of its fields"""
    import torch
    i = rec.view(torch.int32)
    return {"records": rec, "hit": i[:, 0], "item_index": i[:, 1], "object_id": i[:, 2], "face_id": i[:, 3],
            "position": rec[:, 4:7], "distance": rec[:, 7], "normal": rec[:, 8:11], "material": i[:, 11],
            "shading_normal": rec[:, 12:15], "has_uv": i[:, 15], "base_color": rec[:, 16:20],
            "ambient_color": rec[:, 20:23], "alpha": rec[:, 23], "specular_color": rec[:, 24:27], "reflectivity": rec[:, 27],
            "uv": rec[:, 28:30], "roughness": rec[:, 30], "ambient_occlusion": rec[:, 31]}


def surface_pixels_torch(device_scene: capi.DeviceScene, cam, pixels=None, records: bool = True, albedo: bool = True) -> dict:
    """rr_surface_pixels_device on torch's current stream: the G-buffer of `cam`'s pixel-centre rays and the albedo denoise_torch takes.
    `pixels` as render_pixels_torch takes them, or None for every pixel of the frame in row-major order -- that form is only enqueued: no
    host copy, no synchronisation.  Returns torch tensors: with records=True the dict of surface_rays_torch (records (n, 32) float32 and
    the views of its fields), with albedo=True `albedo` (n, 3) float32 (the records' base_color, 0 for a miss)."""
    import torch
    if not records and not albedo:
        raise ValueError("surface_pixels_torch: neither records nor albedo")
    n, xy = int(cam.width) * int(cam.height), None
    if pixels is not None:
        dtype = torch.int32 if not isinstance(pixels, torch.Tensor) or pixels.dtype != getattr(torch, "uint32", None) else pixels.dtype
        xy = _ray_tensor(device_scene, pixels, "pixels", shape_tail=(), dtype=dtype)
        n = int(xy.shape[0])
    dev = torch.device("cuda", device_scene.device)
    with torch.cuda.device(dev):
        rec = torch.empty((n, 32), dtype=torch.float32, device=dev) if records else None   # (torch allocations are at least 512-byte aligned)
        alb = torch.empty((n, 3), dtype=torch.float32, device=dev) if albedo else None
        if n:
            device_scene.surface_pixels_device(cam, xy.data_ptr() if xy is not None else None, n, rec.data_ptr() if records else None,
                                               alb.data_ptr() if albedo else None, torch.cuda.current_stream(dev).cuda_stream)
    out = _surface_views(rec) if records else {}
    if albedo:
        out["albedo"] = alb
    return out


def _check_albedo_mode(albedo, temporal: bool = False) -> None:
    """The `albedo` argument of the pipelines: False, True (the pixel-centre albedo, rr_surface_pixels), "mean" (rr_albedo_pixels) or, in the
    single-frame pipelines only, "diffuse" (the mean albedo applied to the direct diffuse part alone: rr_render_pixel_split and
    rr_denoise_split_records)."""
    if isinstance(albedo, str) and albedo not in ("mean", "diffuse"):
        raise ValueError(f'albedo must be False, True, "mean" or "diffuse", not {albedo!r}')
    if temporal and _diffuse_mode(albedo):
        raise ValueError('albedo="diffuse" is for the single-frame pipelines; over time the diffuse part is accumulated by render_temporal_split '
                         '(render_temporal_split_torch), a pipeline of its own')


def _mean_mode(albedo) -> bool:
    return isinstance(albedo, str) and albedo == "mean"


def _diffuse_mode(albedo) -> bool:
    return isinstance(albedo, str) and albedo == "diffuse"


def albedo_pixels_torch(device_scene: capi.DeviceScene, cam, cfg: rr_config, pixels=None, sample_xy=None):
    """rr_albedo_pixels_device on torch's current stream: the albedo of `cam`'s pixels as the frame of `cfg` sees them (the mean over the
    frame's primary rays of the base colour at each first hit).  `pixels` as render_pixels_torch takes them, or None for every pixel of the
    frame in row-major order.  Returns an (n, 3) float32 CUDA tensor, what denoise_torch takes as `albedo`; no host copy of the result."""
    import torch
    n, xy = int(cam.width) * int(cam.height), None
    if pixels is not None:
        dtype = torch.int32 if not isinstance(pixels, torch.Tensor) or pixels.dtype != getattr(torch, "uint32", None) else pixels.dtype
        xy = _ray_tensor(device_scene, pixels, "pixels", shape_tail=(), dtype=dtype)
        n = int(xy.shape[0])
    dev = torch.device("cuda", device_scene.device)
    with torch.cuda.device(dev):
        alb = torch.empty((n, 3), dtype=torch.float32, device=dev)
        if n:
            device_scene.albedo_pixels_device(cam, cfg, xy.data_ptr() if xy is not None else None, n, alb.data_ptr(),
                                              torch.cuda.current_stream(dev).cuda_stream, sample_xy=sample_xy)
    return alb


def trace_shadow_rays_torch(device_scene: capi.DeviceScene, origins, directions, max_distance=None, depth: int = 2) -> dict:
    """rr_trace_shadow_rays_device on torch's current stream: as trace_rays_torch, with `max_distance` a contiguous float32 CUDA tensor of
    shape (n,) or None (no limit).  Returns dict(records (n, 5) int32, occluded, item_index (-1 = lit), object_id, face_id, distance)."""
    import torch
    o = _ray_tensor(device_scene, origins, "origins")
    d = _ray_tensor(device_scene, directions, "directions")
    if d.shape[0] != o.shape[0]:
        raise ValueError(f"{o.shape[0]} origins, {d.shape[0]} directions")
    lim = None
    if max_distance is not None:
        lim = _ray_tensor(device_scene, max_distance, "max_distance", shape_tail=())
        if lim.shape[0] != o.shape[0]:
            raise ValueError(f"{o.shape[0]} rays, {lim.shape[0]} distances")
    dev = torch.device("cuda", device_scene.device)
    n = int(o.shape[0])
    with torch.cuda.device(dev):
        rec = torch.empty((n, 5), dtype=torch.int32, device=dev)
        if n:
            device_scene.trace_shadow_rays_device(o.data_ptr(), d.data_ptr(), lim.data_ptr() if lim is not None else None, n, depth, rec.data_ptr(),
                                                  torch.cuda.current_stream(dev).cuda_stream)
    return _hit_views(rec, "occluded")


def shade_rays_torch(device_scene: capi.DeviceScene, origins, directions, cfg: rr_config, rays_per_result: int = 1, stream_ids=None) -> dict:
    """rr_shade_rays_device on torch's current stream: `origins` / `directions` hold n_results * rays_per_result rays as contiguous float32
    CUDA tensors of shape (n, 3), `stream_ids` n_results ids as a contiguous int32 CUDA tensor (the 32 bits are the id) or None.  Returns
    dict(records (n_results, 8) float32, color (n_results, 3) LINEAR, depth, normal (n_results, 3), object_id (int32 view)), views of `records`."""
    import torch
    o = _ray_tensor(device_scene, origins, "origins")
    d = _ray_tensor(device_scene, directions, "directions")
    if d.shape[0] != o.shape[0]:
        raise ValueError(f"{o.shape[0]} origins, {d.shape[0]} directions")
    rpr = int(rays_per_result)
    if rpr < 1 or o.shape[0] % rpr:
        raise ValueError(f"{o.shape[0]} rays are not whole results of {rpr} rays")
    n = int(o.shape[0]) // rpr
    ids = None
    if stream_ids is not None:
        ids = _ray_tensor(device_scene, stream_ids, "stream_ids", shape_tail=(), dtype=torch.int32)
        if ids.shape[0] != n:
            raise ValueError(f"{n} results, {ids.shape[0]} stream ids")
    dev = torch.device("cuda", device_scene.device)
    with torch.cuda.device(dev):
        rec = torch.empty((n, 8), dtype=torch.float32, device=dev)
        if n:
            device_scene.shade_rays_device(cfg, o.data_ptr(), d.data_ptr(), n, rpr, ids.data_ptr() if ids is not None else None, rec.data_ptr(),
                                           torch.cuda.current_stream(dev).cuda_stream)
    return _record_views(rec)


def render_pixels_torch(device_scene: capi.DeviceScene, cam, cfg: rr_config, pixels=None, sample_xy=None, rgba8: bool = False) -> dict:
    """rr_render_pixels_device on torch's current stream: `pixels` holds n entries x | y << 16 as a contiguous int32 or uint32 CUDA tensor of
    shape (n,) (the 32 bits are the entry), or None for every pixel of the frame in row-major order.  Returns torch tensors, without a
    host copy and without a synchronisation of the results: dict(records (n, 8) float32, color (n, 3) LINEAR, depth, normal (n, 3),
    object_id (int32 view)), views of `records`, and with rgba8=True rgba (n, 4) uint8, the frame's own bytes."""
    import torch
    n, xy = int(cam.width) * int(cam.height), None
    if pixels is not None:
        dtype = torch.int32 if not isinstance(pixels, torch.Tensor) or pixels.dtype != getattr(torch, "uint32", None) else pixels.dtype
        xy = _ray_tensor(device_scene, pixels, "pixels", shape_tail=(), dtype=dtype)
        n = int(xy.shape[0])
    dev = torch.device("cuda", device_scene.device)
    with torch.cuda.device(dev):
        rec = torch.empty((n, 8), dtype=torch.float32, device=dev)   # (torch allocations are at least 512-byte aligned)
        rgba = torch.empty((n, 4), dtype=torch.uint8, device=dev) if rgba8 else None
        if n:
            device_scene.render_pixels_device(cam, cfg, xy.data_ptr() if xy is not None else None, n, rec.data_ptr(), rgba.data_ptr() if rgba8 else None,
                                              torch.cuda.current_stream(dev).cuda_stream, sample_xy=sample_xy)
    out = _record_views(rec)
    if rgba8:
        out["rgba"] = rgba
    return out


def render_pixel_parts_torch(device_scene: capi.DeviceScene, cam, cfg: rr_config, pixels=None, n_parts: int = 2, sample_xy=None) -> dict:
    """rr_render_pixel_parts_device on torch's current stream: `pixels` as render_pixels_torch takes them.  Returns torch tensors, without a
    host copy and without a synchronisation of the results: the dict of render_pixels_torch (records (n, 8) float32 and its views) plus
    part_records (n, K, 8) float32 and parts = dict(color (n, K, 3) LINEAR, depth (n, K), normal (n, K, 3), object_id (int32 view)), views of it."""
    import torch
    n, xy = int(cam.width) * int(cam.height), None
    if pixels is not None:
        dtype = torch.int32 if not isinstance(pixels, torch.Tensor) or pixels.dtype != getattr(torch, "uint32", None) else pixels.dtype
        xy = _ray_tensor(device_scene, pixels, "pixels", shape_tail=(), dtype=dtype)
        n = int(xy.shape[0])
    K = int(n_parts)
    dev = torch.device("cuda", device_scene.device)
    with torch.cuda.device(dev):
        rec = torch.empty((n, 8), dtype=torch.float32, device=dev)   # (torch allocations are at least 512-byte aligned)
        prec = torch.empty((n, max(min(K, 64), 1), 8), dtype=torch.float32, device=dev)
        if n:
            device_scene.render_pixel_parts_device(cam, cfg, xy.data_ptr() if xy is not None else None, n, K, rec.data_ptr(), prec.data_ptr(),
                                                   torch.cuda.current_stream(dev).cuda_stream, sample_xy=sample_xy)
    parts = _record_views(prec)
    return dict(_record_views(rec), part_records=parts.pop("records"), parts=parts)


def render_pixel_split_torch(device_scene: capi.DeviceScene, cam, cfg: rr_config, pixels=None, halves: bool = True, sample_xy=None) -> dict:
    """rr_render_pixel_split_device on torch's current stream: `pixels` as render_pixels_torch takes them.  Returns torch tensors, without a host
    copy and without a synchronisation of the results: the dict of render_pixel_parts_torch at n_parts = 2 (that of render_pixels_torch with
    halves=False) plus diffuse (n, 3) float32 and, with halves, diffuse_halves (n, 2, 3)."""
    import torch
    n, xy = int(cam.width) * int(cam.height), None
    if pixels is not None:
        dtype = torch.int32 if not isinstance(pixels, torch.Tensor) or pixels.dtype != getattr(torch, "uint32", None) else pixels.dtype
        xy = _ray_tensor(device_scene, pixels, "pixels", shape_tail=(), dtype=dtype)
        n = int(xy.shape[0])
    dev = torch.device("cuda", device_scene.device)
    with torch.cuda.device(dev):
        rec = torch.empty((n, 8), dtype=torch.float32, device=dev)   # (torch allocations are at least 512-byte aligned)
        prec = torch.empty((n, 2, 8), dtype=torch.float32, device=dev) if halves else None
        dif = torch.empty((n, 3), dtype=torch.float32, device=dev)
        dif_h = torch.empty((n, 2, 3), dtype=torch.float32, device=dev) if halves else None
        if n:
            device_scene.render_pixel_split_device(cam, cfg, xy.data_ptr() if xy is not None else None, n, rec.data_ptr(), prec.data_ptr() if halves else None,
                                                   dif.data_ptr(), dif_h.data_ptr() if halves else None, torch.cuda.current_stream(dev).cuda_stream,
                                                   sample_xy=sample_xy)
    out = dict(_record_views(rec), diffuse=dif)
    if halves:
        parts = _record_views(prec)
        out.update(part_records=parts.pop("records"), parts=parts, diffuse_halves=dif_h)
    return out


def _record_views(rec) -> dict:
    """`records`, (..., 8) float32 rr_radiance on the device, and the views of its fields"""
    import torch
    return {"records": rec, "color": rec[..., 0:3], "depth": rec[..., 3], "normal": rec[..., 4:7], "object_id": rec.view(torch.int32)[..., 7]}


def _fused_torch(device_scene: capi.DeviceScene, cam, rgba8: bool, samples: bool, error: bool, counts_key: str, call) -> dict:
    """The body of the three fused calls on torch's current stream: the outputs as torch tensors, `call(out, rgba8, samples, error, stream)`
    on their raw pointers (None where one is not asked for), and the dict they return; what `call` returns goes under `counts_key`."""
    import torch
    n = int(cam.width) * int(cam.height)
    dev = torch.device("cuda", device_scene.device)
    with torch.cuda.device(dev):
        rec = torch.empty((n, 8), dtype=torch.float32, device=dev)   # (torch allocations are at least 512-byte aligned)
        rgba = torch.empty((n, 4), dtype=torch.uint8, device=dev) if rgba8 else None
        smp = torch.empty((n,), dtype=torch.int16, device=dev) if samples else None
        err = torch.empty((n,), dtype=torch.float32, device=dev) if error else None
        counts = call(rec.data_ptr(), rgba.data_ptr() if rgba8 else None, smp.data_ptr() if samples else None, err.data_ptr() if error else None,
                      torch.cuda.current_stream(dev).cuda_stream)
    out = dict(_record_views(rec), **{counts_key: counts})
    if rgba8:
        out["rgba"] = rgba
    if samples:
        out["samples"] = smp
    if error:
        out["error"] = err
    return out


def render_adaptive_torch(device_scene: capi.DeviceScene, cam, cfg: rr_config, base_samples: int, max_samples: int, threshold: float, sample_xy_base=None,
                          sample_xy_max=None, rgba8: bool = False, samples: bool = True, error: bool = True) -> dict:
    """rr_render_adaptive_device on torch's current stream: the frame at `base_samples`, and at `max_samples` where the half-buffer error
    of the base frame exceeds `threshold`.  Returns torch tensors in row-major order, without a host copy of the results: the dict of
    render_pixels_torch (records (n, 8) float32 and its views), n_refined (an int: the call waits for it), and on request samples (n,)
    int16 (the sample count per pixel), error (n,) float32 and rgba (n, 4) uint8."""
    return _fused_torch(device_scene, cam, rgba8, samples, error, "n_refined", lambda out, rgba, smp, err, stream: device_scene.render_adaptive_device(
        cam, cfg, base_samples, max_samples, threshold, out, rgba, smp, err, stream, sample_xy_base=sample_xy_base, sample_xy_max=sample_xy_max))


def render_adaptive_levels_torch(device_scene: capi.DeviceScene, cam, cfg: rr_config, levels, threshold: float, sample_xy_levels=None, rgba8: bool = False,
                                 samples: bool = True, error: bool = True) -> dict:
    """rr_render_adaptive_levels_device on torch's current stream: the frame at levels[0], and level after level the pixels whose
    half-buffer error still exceeds `threshold` at the next count.  Returns torch tensors in row-major order, without a host copy of the
    results: the dict of render_pixels_torch (records (n, 8) float32 and its views), level_pixels (a list of ints: the call waits for
    them), and on request samples (n,) int16 (the count of the last level that rendered the pixel), error (n,) float32 (the residual
    error, at that count) and rgba (n, 4) uint8."""
    return _fused_torch(device_scene, cam, rgba8, samples, error, "level_pixels", lambda out, rgba, smp, err, stream: device_scene.render_adaptive_levels_device(
        cam, cfg, levels, threshold, out, rgba, smp, err, stream, sample_xy_levels=sample_xy_levels))


def render_adaptive_prefix_torch(device_scene: capi.DeviceScene, cam, cfg: rr_config, prefix_samples, threshold: float, sample_xy=None, rgba8: bool = False,
                                 samples: bool = True, error: bool = True) -> dict:
    """rr_render_adaptive_prefix_device on torch's current stream: the frame over its first prefix_samples[0] samples, and level after
    level only the samples up to the next prefix for the pixels whose half-buffer error still exceeds `threshold`.  Returns what
    render_adaptive_levels_torch returns."""
    return _fused_torch(device_scene, cam, rgba8, samples, error, "level_pixels", lambda out, rgba, smp, err, stream: device_scene.render_adaptive_prefix_device(
        cam, cfg, prefix_samples, threshold, out, rgba, smp, err, stream, sample_xy=sample_xy))


# ---------------------------------------------------------------------------
# the a-trous filter on torch tensors: records rendered on the GPU are filtered where they are, on torch's current stream
# ---------------------------------------------------------------------------
def denoise_torch(device_scene: capi.DeviceScene, width: int, height: int, records, halves=None, albedo=None, params=None, rgba8: bool = False,
                  variance: bool = True, in_place: bool = False) -> dict:
    """rr_denoise_records_device on torch's current stream of the scene's device: `records` (n, 8), `halves` (n, 2, 8) or None and `albedo`
    (n, 3) or None are contiguous float32 CUDA tensors on that device, n = width * height (anything else raises).  Returns torch tensors,
    without a host copy and without a synchronisation: dict(records (n, 8) float32 and its views color, depth, normal, object_id; on
    request variance (n,) float32 and rgba (n, 4) uint8).  in_place: the filtered records are written over `records`."""
    import torch
    n = int(width) * int(height)
    t = _frame_tensors(device_scene, width, height, dict(records=(records, (8,)), halves=(halves, (2, 8)), albedo=(albedo, (3,))),
                       required=("records",))
    rec, hv, al = t["records"], t["halves"], t["albedo"]
    dev = torch.device("cuda", device_scene.device)
    with torch.cuda.device(dev):
        out = rec if in_place else torch.empty((n, 8), dtype=torch.float32, device=dev)   # (torch allocations are at least 512-byte aligned)
        rgba = torch.empty((n, 4), dtype=torch.uint8, device=dev) if rgba8 else None
        var = torch.empty((n,), dtype=torch.float32, device=dev) if variance else None
        device_scene.denoise_records_device(width, height, rec.data_ptr(), hv.data_ptr() if hv is not None else None, al.data_ptr() if al is not None else None,
                                            out.data_ptr(), rgba.data_ptr() if rgba8 else None, var.data_ptr() if variance else None, params,
                                            torch.cuda.current_stream(dev).cuda_stream)
    res = _record_views(out)
    if variance:
        res["variance"] = var
    if rgba8:
        res["rgba"] = rgba
    return res


def denoise_split_torch(device_scene: capi.DeviceScene, width: int, height: int, records, diffuse, halves=None, diffuse_halves=None, albedo=None, params=None,
                        rgba8: bool = False, in_place: bool = False) -> dict:
    """rr_denoise_split_records_device on torch's current stream of the scene's device: the tensors of denoise_torch plus `diffuse` (n, 3) and
    `diffuse_halves` (n, 2, 3) or None (exactly when `halves` is).  Returns torch tensors, without a host copy and without a synchronisation:
    dict(records (n, 8) float32 and its views; on request rgba (n, 4) uint8)."""
    import torch
    n = int(width) * int(height)
    t = _frame_tensors(device_scene, width, height, dict(records=(records, (8,)), halves=(halves, (2, 8)), albedo=(albedo, (3,)), diffuse=(diffuse, (3,)),
                                                         diffuse_halves=(diffuse_halves, (2, 3))), required=("records", "diffuse"))
    ptr = lambda k: t[k].data_ptr() if t[k] is not None else None
    dev = torch.device("cuda", device_scene.device)
    with torch.cuda.device(dev):
        out = t["records"] if in_place else torch.empty((n, 8), dtype=torch.float32, device=dev)   # (torch allocations are at least 512-byte aligned)
        rgba = torch.empty((n, 4), dtype=torch.uint8, device=dev) if rgba8 else None
        device_scene.denoise_split_device(width, height, ptr("records"), ptr("halves"), ptr("diffuse"), ptr("diffuse_halves"), ptr("albedo"), out.data_ptr(),
                                          rgba.data_ptr() if rgba8 else None, params, torch.cuda.current_stream(dev).cuda_stream)
    res = _record_views(out)
    if rgba8:
        res["rgba"] = rgba
    return res


def _albedo_guide_torch(device_scene: capi.DeviceScene, cam, cfg: rr_config, sample_xy, albedo):
    """The albedo guide of a device pipeline on torch's current stream: None, the pixel-centre albedo (True) or the frame's mean ("mean")."""
    _check_albedo_mode(albedo)
    if not albedo:
        return None
    if _mean_mode(albedo):
        return albedo_pixels_torch(device_scene, cam, cfg, None, sample_xy=sample_xy)
    return surface_pixels_torch(device_scene, cam, None, records=False, albedo=True)["albedo"]


def render_denoised_torch(device_scene: capi.DeviceScene, cam, cfg: rr_config, params=None, sample_xy=None, rgba8: bool = False, albedo=False) -> dict:
    """Raytracing.render_denoised on the device, with no host trip: rr_render_pixel_parts_device at n_parts = 2 (cfg.samples even) and
    rr_denoise_records_device on the same stream, the second reading what the first wrote without a synchronisation.  albedo=True:
    rr_surface_pixels_device between the two, on the same stream, makes the camera's albedo for the filter (three calls, still no host
    trip); albedo="mean": rr_albedo_pixels_device with the frame's config and table in its place.  Returns the dict of denoise_torch plus
    noisy (n, 8) and halves (n, 2, 8), the tensors the filter read, and with an albedo albedo (n, 3).  albedo="diffuse": three calls on the
    stream, rr_render_pixel_split_device, rr_albedo_pixels_device (the mean albedo) and rr_denoise_split_records_device, which demodulates the
    direct diffuse part of the colour alone; the result then holds diffuse (n, 3) and diffuse_halves (n, 2, 3) too, and no variance."""
    _check_albedo_mode(albedo)
    if _diffuse_mode(albedo):
        base = render_pixel_split_torch(device_scene, cam, cfg, None, True, sample_xy=sample_xy)
        guide = albedo_pixels_torch(device_scene, cam, cfg, None, sample_xy=sample_xy)
        res = denoise_split_torch(device_scene, int(cam.width), int(cam.height), base["records"], base["diffuse"], base["part_records"], base["diffuse_halves"], guide,
                                  params, rgba8=rgba8)
        return dict(res, noisy=base["records"], halves=base["part_records"], albedo=guide, diffuse=base["diffuse"], diffuse_halves=base["diffuse_halves"])
    base = render_pixel_parts_torch(device_scene, cam, cfg, None, 2, sample_xy=sample_xy)
    guide = _albedo_guide_torch(device_scene, cam, cfg, sample_xy, albedo)
    res = denoise_torch(device_scene, int(cam.width), int(cam.height), base["records"], base["part_records"], guide, params, rgba8=rgba8)
    res = dict(res, noisy=base["records"], halves=base["part_records"])
    if albedo:
        res["albedo"] = guide
    return res


# ---------------------------------------------------------------------------
# the joint-bilateral upsampler on torch tensors: a frame traced at a low resolution is raised where it is, on torch's current stream
# ---------------------------------------------------------------------------
def _check_upsampled_options(albedo, full_albedo_samples) -> None:
    """The `albedo` and `full_albedo_samples` arguments of the upsampling pipelines: True (the guides' pixel-centre albedo) or "mean"
    (rr_albedo_pixels on the small camera); None or a whole number of samples, at least 1."""
    if not (albedo is True or _mean_mode(albedo)):
        raise ValueError(f'albedo must be True or "mean", not {albedo!r}')
    if full_albedo_samples is not None:
        k = full_albedo_samples
        if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or k < 1:
            raise ValueError(f"full_albedo_samples must be None or a whole number of samples, at least 1, not {k!r}")


def _config_at(cfg: rr_config, samples) -> rr_config:
    """`cfg` at `samples` samples."""
    c = rr_config.from_buffer_copy(cfg)
    c.samples = int(samples)
    return c


def _low_camera(cam, scale):
    """(`cam` with its matrices at ceil(width / scale) x ceil(height / scale), that width, that height); scale >= 1, whole or not."""
    import math
    if not float(scale) >= 1.0:
        raise ValueError(f"scale {scale}: at least 1")
    low = rr_camera.from_buffer_copy(cam)
    low.width, low.height = max(1, math.ceil(int(cam.width) / scale)), max(1, math.ceil(int(cam.height) / scale))
    return low, int(low.width), int(low.height)


def upsample_torch(device_scene: capi.DeviceScene, low_width: int, low_height: int, width: int, height: int, low, halves_low, guide_low, guide, params=None,
                   rgba8: bool = False, weight: bool = True, albedo_low=None, albedo=None) -> dict:
    """rr_upsample_records_device on torch's current stream of the scene's device: `low` (w h, 8), `halves_low` (w h, 2, 8) or None,
    `guide_low` (w h, 32) and `guide` (W H, 32) (the `records` of surface_pixels_torch) are contiguous float32 CUDA tensors on that device
    (anything else raises).  Returns torch tensors, without a host copy and without a synchronisation: dict(records (W H, 8) float32 and
    its views color, depth, normal, object_id; halves (W H, 2, 8) or None; on request weight (W H,) float32 and rgba (W H, 4) uint8).
    albedo_low (w h, 3) and albedo (W H, 3), each or None: albedo planes in place of the guides' base colours, tensors of the same kind
    (rr_upsample_albedo_records_device; a view that is only 4-byte aligned will do)."""
    import torch
    n = int(width) * int(height)
    lo = _frame_tensors(device_scene, low_width, low_height, dict(low=(low, (8,)), halves_low=(halves_low, (2, 8)), guide_low=(guide_low, (32,)),
                                                                  albedo_low=(albedo_low, (3,))), required=("low", "guide_low"))
    fl = _frame_tensors(device_scene, width, height, dict(guide=(guide, (32,)), albedo=(albedo, (3,))), required=("guide",))
    gf, al, af = fl["guide"], lo["albedo_low"], fl["albedo"]
    hv = lo["halves_low"]
    dev = torch.device("cuda", device_scene.device)
    with torch.cuda.device(dev):
        out = torch.empty((n, 8), dtype=torch.float32, device=dev)   # (torch allocations are at least 512-byte aligned)
        hout = torch.empty((n, 2, 8), dtype=torch.float32, device=dev) if hv is not None else None
        rgba = torch.empty((n, 4), dtype=torch.uint8, device=dev) if rgba8 else None
        wt = torch.empty((n,), dtype=torch.float32, device=dev) if weight else None
        device_scene.upsample_device(low_width, low_height, width, height, lo["low"].data_ptr(), hv.data_ptr() if hv is not None else None, lo["guide_low"].data_ptr(),
                                     gf.data_ptr(), out.data_ptr(), hout.data_ptr() if hout is not None else None, rgba.data_ptr() if rgba8 else None,
                                     wt.data_ptr() if weight else None, params, torch.cuda.current_stream(dev).cuda_stream,
                                     albedo_low=al.data_ptr() if al is not None else None, albedo=af.data_ptr() if af is not None else None)
    res = dict(_record_views(out), halves=hout)
    if weight:
        res["weight"] = wt
    if rgba8:
        res["rgba"] = rgba
    return res


def render_upsampled_torch(device_scene: capi.DeviceScene, cam, cfg: rr_config, scale=2, params=None, denoise_params=None, fill_holes: bool = False,
                           rgba8: bool = False, sample_xy=None, albedo=True, full_albedo_samples: Optional[int] = None, low_denoise_params=None) -> dict:
    """Raytracing.render_upsampled on the device, on torch's current stream with no host trip: rr_render_pixel_parts_device at n_parts = 2
    on the camera at ceil(W / scale) x ceil(H / scale), rr_surface_pixels_device on both cameras, rr_upsample_records_device with halves
    and, with `denoise_params`, rr_denoise_records_device at full size with the full guide's albedo, each reading what the one before
    wrote without a synchronisation.  fill_holes: the pixels with weight 0 on a surface (guide.hit) become a list x | y << 16, made with
    torch on the device (its length is read on the host: one wait), are traced at full resolution by rr_render_pixel_parts_device and
    written over the records and the halves before the filter.  Returns the dict of upsample_torch plus low (w h, 8), halves_low,
    guide_low, guide (the tensors the upsampler read), low_width, low_height, holes (the list, int32 bits) and count; with
    `denoise_params` the records are the filtered ones, `upsampled` those before the filter, and `variance` is there.
    albedo, full_albedo_samples and low_denoise_params as Raytracing.render_upsampled takes them: rr_albedo_pixels_device on the small
    camera (with the low frame's cfg and sample_xy) and on `cam` at full_albedo_samples, rr_upsample_albedo_records_device, and
    rr_denoise_records_device at the low size before it, all on the same stream; the result holds albedo_low and albedo (the planes the
    upsampler took, or None) and with low_denoise_params low_filtered."""
    _check_upsampled_options(albedo, full_albedo_samples)
    import torch
    W, H = int(cam.width), int(cam.height)
    low_cam, w, h = _low_camera(cam, scale)
    base = render_pixel_parts_torch(device_scene, low_cam, cfg, None, 2, sample_xy=sample_xy)
    mean = _mean_mode(albedo)
    guide_low = surface_pixels_torch(device_scene, low_cam, None, records=True, albedo=low_denoise_params is not None and not mean)
    guide = surface_pixels_torch(device_scene, cam, None, records=True, albedo=denoise_params is not None and full_albedo_samples is None)
    albedo_low = albedo_pixels_torch(device_scene, low_cam, cfg, None, sample_xy=sample_xy) if mean else None
    albedo_full = albedo_pixels_torch(device_scene, cam, _config_at(cfg, full_albedo_samples), None) if full_albedo_samples is not None else None
    low, halves_low, low_filtered = base["records"], base["part_records"], None
    if low_denoise_params is not None:
        low = low_filtered = denoise_torch(device_scene, w, h, low, halves_low, albedo_low if mean else guide_low["albedo"], low_denoise_params,
                                           variance=False)["records"]
        halves_low = None
    res = upsample_torch(device_scene, w, h, W, H, low, halves_low, guide_low["records"], guide["records"], params, rgba8=rgba8, albedo_low=albedo_low,
                         albedo=albedo_full)
    dev = torch.device("cuda", device_scene.device)
    with torch.cuda.device(dev):
        holes = torch.empty((0,), dtype=torch.int32, device=dev)
        if fill_holes:
            at = torch.nonzero((res["weight"] == 0) & (guide["hit"] != 0)).reshape(-1)
            xy = (at % W) | ((at // W) << 16)                       # int64; as the 32 bits of an int32
            holes = torch.where(xy >= (1 << 31), xy - (1 << 32), xy).to(torch.int32).contiguous()
    if int(holes.shape[0]):
        cfg_b = rr_config.from_buffer_copy(cfg)
        cfg_b.gamma_correction = capi.upsample_params(params).gamma_correction
        fine = render_pixel_parts_torch(device_scene, cam, cfg_b, holes, 2, sample_xy=sample_xy)
        res["records"][at] = fine["records"]
        if res["halves"] is not None:
            res["halves"][at] = fine["part_records"]
        if rgba8:
            res["rgba"][at] = render_pixels_torch(device_scene, cam, cfg_b, holes, sample_xy=sample_xy, rgba8=True)["rgba"]
    res.update(low=base["records"], halves_low=base["part_records"], guide_low=guide_low["records"], guide=guide["records"], low_width=w, low_height=h,
               holes=holes, count=int(holes.shape[0]), albedo_low=albedo_low, albedo=albedo_full)
    if low_filtered is not None:
        res["low_filtered"] = low_filtered
    if denoise_params is not None:
        filtered = denoise_torch(device_scene, W, H, res["records"], res["halves"], albedo_full if albedo_full is not None else guide["albedo"], denoise_params,
                                 rgba8=rgba8)
        res.update(upsampled=res["records"], **filtered)
    return res


# ---------------------------------------------------------------------------
# temporal reprojection on torch tensors: the history lives on the device from frame to frame
# ---------------------------------------------------------------------------
class TemporalState:
    """What a frame-after-frame loop carries from one rr_accumulate_records call to the next: two sets of device tensors (records (n, 8),
    halves (n, 2, 8), length (n,); for the split pipeline also diffuse (n, 3) and diffuse_halves (n, 2, 3)) used in turn -- the call gathers
    from one set and writes the other --, which of them holds the history, and the view (world_to_clip, eye) the history was rendered
    from.  reset() forgets the history: the next frame is a first frame."""

    def __init__(self):
        self.sets = [None, None]
        self.current = None      # index of the set that holds the history, or None
        self.view = None
        self.frames = 0
        self.items = None        # (ids (k,) uint32, trans (k, 4, 4) float32) of the items the history was rendered with (track)

    def reset(self):
        self.current, self.view, self.frames, self.items = None, None, 0, None

    def track(self, ids, trans):
        """Takes note of the items the frame about to be rendered is traced with -- object ids (k,) and `trans` (k, 4, 4) in math
        layout -- and returns what rr_motion_records needs against the history: (item_index (m,) uint32, prev_trans (m, 4, 4)) of the
        items whose 16 floats differ bitwise from the ones noted at the call before; None when there is no history.  A change of
        the item count or of any item's id resets the state first; so does a history whose items were not noted (a frame rendered
        without tracking): nobody knows what moved since, and the frame starts anew rather than treat every item as static."""
        ids = np.array(ids, np.uint32).reshape(-1)
        trans = np.array(trans, np.float32).reshape(len(ids), 4, 4)
        if (self.items is None and self.current is not None) or (self.items is not None and not np.array_equal(self.items[0], ids)):
            self.reset()
        moved = None
        if self.items is not None and self.current is not None:
            changed = np.flatnonzero((self.items[1].view(np.uint32) != trans.view(np.uint32)).reshape(len(ids), 16).any(1))
            moved = (changed.astype(np.uint32), self.items[1][changed])
        self.items = (ids, trans)
        return moved

    def history(self):
        return self.sets[self.current] if self.current is not None else None

    def target(self, n: int, halves: bool, device, diffuse: bool = False) -> dict:
        """The set the next call writes: the one that does not hold the history, (re)allocated when the frame's size changed.  diffuse:
        the set of the split pipeline, with diffuse (n, 3) and, with halves, diffuse_halves (n, 2, 3)."""
        import torch
        k = 0 if self.current is None else self.current ^ 1
        t = self.sets[k]
        if (t is None or int(t["records"].shape[0]) != n or t["records"].device != device or (t["halves"] is not None) != halves
                or (t.get("diffuse") is not None) != diffuse):
            t = dict(records=torch.empty((n, 8), dtype=torch.float32, device=device),
                     halves=torch.empty((n, 2, 8), dtype=torch.float32, device=device) if halves else None,
                     length=torch.empty((n,), dtype=torch.float32, device=device))
            if diffuse:
                t.update(diffuse=torch.empty((n, 3), dtype=torch.float32, device=device),
                         diffuse_halves=torch.empty((n, 2, 3), dtype=torch.float32, device=device) if halves else None)
            self.sets[k] = t
        return t

    def advance(self, written: dict, view):
        self.current = next(k for k, t in enumerate(self.sets) if t is written)
        self.view, self.frames = view, self.frames + 1


def _accumulate_torch(device_scene: capi.DeviceScene, split: bool, clamped: bool, cam, tensors, params, clamp, rgba8: bool, in_place: bool, out) -> dict:
    """The four accumulate*_torch functions, over the rows of capi.ACCUMULATE_ROWS the call has: `tensors` holds the inputs by row name
    (the caller's own arguments), checked by _frame_tensors; an output is its input (in_place), the tensor of its key in `out`, or fresh,
    and None where its input is; the call is the binding's one device body on torch's current stream."""
    import torch
    n = int(cam.width) * int(cam.height)
    rows = capi.accumulate_rows(split)
    t = _frame_tensors(device_scene, cam.width, cam.height, {r.name: (tensors[r.name], r.shape) for r in rows if r.key is None},
                       required=("records", "diffuse") if split else ())
    dev = torch.device("cuda", device_scene.device)
    with torch.cuda.device(dev):
        for r in (r for r in rows if r.key is not None):
            fresh = lambda: torch.empty((n,) + r.shape, dtype=torch.uint8 if r.dtype is np.uint8 else torch.float32, device=dev)   # (at least 512-byte aligned)
            if r.key == "rgba":
                t[r.name] = fresh() if rgba8 else None
            elif r.key == "length":
                t[r.name] = out["length"] if out is not None else fresh()
            elif in_place or t[r.key] is None:
                t[r.name] = t[r.key]
            else:
                t[r.name] = out[r.key] if out is not None else fresh()
        device_scene._accumulate_device(split, capi.history_clamp_params(clamp) if clamped else None, cam,
                                        {r.name + "_ptr": t[r.name].data_ptr() if t[r.name] is not None else None for r in rows}, params,
                                        torch.cuda.current_stream(dev).cuda_stream)
    result = dict(_record_views(t["out"]), **{r.key: t[r.name] for r in rows if r.key not in (None, "records", "rgba")})
    if rgba8:
        result["rgba"] = t["rgba8"]
    return result


def accumulate_torch(device_scene: capi.DeviceScene, cam, records, halves=None, history=None, history_halves=None, history_length=None, motion=None, params=None,
                     rgba8: bool = False, in_place: bool = False, out: Optional[dict] = None) -> dict:
    """rr_accumulate_records_device on torch's current stream of the scene's device: `records` (n, 8), `halves` (n, 2, 8) or None, `history`
    (n, 8), `history_halves` (n, 2, 8) and `history_length` (n,) (all None: the first frame) and `motion` (n, 3) or None are contiguous
    float32 CUDA tensors on that device, n = cam.width * cam.height (anything else raises); params: a temporal.AccumulateParams.  Returns
    torch tensors, without a host copy and without a synchronisation: dict(records (n, 8) and its views, halves (n, 2, 8) or None, length
    (n,) [, rgba (n, 4) uint8]).  in_place: written over `records` and `halves`; out: dict(records, halves, length) of tensors to write."""
    return _accumulate_torch(device_scene, False, False, cam, locals(), params, None, rgba8, in_place, out)


def _clamp_params(clamp):
    """The `clamp` keyword of the temporal pipelines -> None (off: clamp is None or False) or the clamp to use: the library's defaults as
    the C struct for True, a temporal.HistoryClampParams (checked) or a C struct as given.  Anything else raises ValueError."""
    from .temporal import HistoryClampParams
    if clamp is None or clamp is False:
        return None
    if clamp is True:
        return capi.history_clamp_default_params()
    if isinstance(clamp, HistoryClampParams):
        clamp.check()
        return clamp
    if isinstance(clamp, capi.rr_history_clamp_params):
        return clamp
    raise ValueError("clamp is None or False (off), True (the defaults) or a temporal.HistoryClampParams")


def _no_split_clamp(clamp) -> None:
    if clamp is not None and clamp is not False:
        raise ValueError("clamp: the split pipeline with the clamped accumulation is a function of its own, render_temporal_split_clamped "
                         "(render_temporal_split_clamped_torch); render_temporal_split (render_temporal_split_torch) takes no clamp")


def accumulate_clamped_torch(device_scene: capi.DeviceScene, cam, records, halves=None, history=None, history_halves=None, history_length=None, motion=None,
                             params=None, clamp=None, rgba8: bool = False, out: Optional[dict] = None) -> dict:
    """rr_accumulate_clamped_records_device on torch's current stream of the scene's device: the tensors and the result of accumulate_torch,
    and clamp: a temporal.HistoryClampParams or None (the library's defaults).  There is no in_place: `out` may not be `records`, whose
    neighbours the window reads.  out: dict(records, halves, length) of tensors to write."""
    return _accumulate_torch(device_scene, False, True, cam, locals(), params, clamp, rgba8, False, out)


def accumulate_split_torch(device_scene: capi.DeviceScene, cam, records, halves, diffuse, diffuse_halves, history=None, history_halves=None, history_diffuse=None,
                           history_diffuse_halves=None, history_length=None, motion=None, params=None, rgba8: bool = False, in_place: bool = False,
                           out: Optional[dict] = None) -> dict:
    """rr_accumulate_split_records_device on torch's current stream of the scene's device: the tensors of accumulate_torch, and `diffuse`
    (n, 3), `diffuse_halves` (n, 2, 3) or None (exactly when `halves` is), `history_diffuse` (n, 3) and `history_diffuse_halves` (n, 2, 3):
    the previous call's.  Returns torch tensors, without a host copy and without a synchronisation: the dict of accumulate_torch plus
    diffuse (n, 3) and diffuse_halves (n, 2, 3) or None.  in_place: written over the four current tensors; out: dict(records, halves,
    diffuse, diffuse_halves, length) of tensors to write."""
    return _accumulate_torch(device_scene, True, False, cam, locals(), params, None, rgba8, in_place, out)


def accumulate_clamped_split_torch(device_scene: capi.DeviceScene, cam, records, halves, diffuse, diffuse_halves, history=None, history_halves=None,
                                   history_diffuse=None, history_diffuse_halves=None, history_length=None, motion=None, params=None, clamp=None,
                                   rgba8: bool = False, out: Optional[dict] = None) -> dict:
    """rr_accumulate_clamped_split_records_device on torch's current stream of the scene's device: the tensors and the result of
    accumulate_split_torch, and clamp: a temporal.HistoryClampParams or None (the library's defaults).  There is no in_place: `out` may not
    be `records` and `diffuse_out` not `diffuse`, whose neighbours the windows read.  out: dict(records, halves, diffuse, diffuse_halves,
    length) of tensors to write."""
    return _accumulate_torch(device_scene, True, True, cam, locals(), params, clamp, rgba8, False, out)


def motion_torch(device_scene: capi.DeviceScene, cam, records, item_index, prev_trans, world: bool = False) -> dict:
    """rr_motion_records_device on torch's current stream of the scene's device: `records` (n, 8) is a contiguous float32 CUDA tensor on
    that device, n = cam.width * cam.height (anything else raises); item_index (k,) and prev_trans (k, 4, 4, math layout) are host arrays:
    the moved items and their `trans` in the frame the history was rendered from.  Returns torch tensors, without a host copy and without
    a synchronisation: dict(motion (n, 3), world (n, 3) or None) -- motion is what accumulate_torch takes."""
    import torch
    n = int(cam.width) * int(cam.height)
    rec = _frame_tensors(device_scene, cam.width, cam.height, dict(records=(records, (8,))), required=("records",))["records"]
    dev = torch.device("cuda", device_scene.device)
    with torch.cuda.device(dev):
        motion = torch.empty((n, 3), dtype=torch.float32, device=dev)
        wout = torch.empty((n, 3), dtype=torch.float32, device=dev) if world else None
        device_scene.motion_records_device(cam, item_index, prev_trans, rec.data_ptr(), motion.data_ptr(), wout.data_ptr() if world else None,
                                           torch.cuda.current_stream(dev).cuda_stream)
    return dict(motion=motion, world=wout)


def _temporal_frame_torch(device_scene, cam, cfg, state, params, denoise_params, motion, sample_xy, rgba8, view, moved, split: bool, clamp, albedo=False) -> dict:
    """The frame of the three render_temporal*_torch functions, their refusals behind it: the frame's own records, the history check, with
    moved items the motion, the accumulation into the state's other set, the guide, the filter -- in that order on torch's current stream.
    split: the arm with the diffuse layers (its producer, a history with a diffuse set, the mean albedo as the guide, the split filter);
    clamp: None, or the checked clamp of the clamped accumulation; albedo: the guide of the plain arm."""
    import dataclasses
    import torch
    from .temporal import AccumulateParams, previous_view
    if moved is not None and motion is not None:
        raise ValueError("give `moved` (the motion is made on the device) or `motion`, not both")
    if split:
        base = render_pixel_split_torch(device_scene, cam, cfg, None, True, sample_xy=sample_xy)
    else:
        base = render_pixel_parts_torch(device_scene, cam, cfg, None, 2, sample_xy=sample_xy)
    n = int(cam.width) * int(cam.height)
    hist = state.history()
    if hist is not None and (int(hist["records"].shape[0]) != n or hist["halves"] is None or (split and hist.get("diffuse") is None)):
        items = state.items
        state.reset()
        state.items = items      # (the items noted for this frame are those of the history it becomes)
        hist = None
    prm = dataclasses.replace(params) if params is not None else AccumulateParams()
    if hist is not None:
        prm.prev_world_to_clip, prm.prev_eye = state.view
    target = state.target(n, True, torch.device("cuda", device_scene.device), diffuse=split)
    if moved is not None and hist is not None and len(moved[0]):
        motion = motion_torch(device_scene, cam, base["records"], moved[0], moved[1])["motion"]
    h = lambda k: hist.get(k) if hist else None
    acc = _accumulate_torch(device_scene, split, clamp is not None, cam,
                            dict(records=base["records"], halves=base["part_records"], diffuse=base.get("diffuse"), diffuse_halves=base.get("diffuse_halves"),
                                 history=h("records"), history_halves=h("halves"), history_diffuse=h("diffuse"), history_diffuse_halves=h("diffuse_halves"),
                                 history_length=h("length"), motion=motion), prm, clamp, False, False, target)
    res = dict(noisy=base["records"], halves=base["part_records"], accumulated=acc["records"], accumulated_halves=acc["halves"], length=acc["length"], motion=motion)
    if split:
        guide = albedo_pixels_torch(device_scene, cam, cfg, None, sample_xy=sample_xy)
        out = denoise_split_torch(device_scene, int(cam.width), int(cam.height), acc["records"], acc["diffuse"], acc["halves"], acc["diffuse_halves"], guide,
                                  denoise_params, rgba8=rgba8)
        res.update(diffuse=base["diffuse"], diffuse_halves=base["diffuse_halves"], accumulated_diffuse=acc["diffuse"],
                   accumulated_diffuse_halves=acc["diffuse_halves"], albedo=guide)
    else:
        guide = _albedo_guide_torch(device_scene, cam, cfg, sample_xy, albedo)
        out = denoise_torch(device_scene, int(cam.width), int(cam.height), acc["records"], acc["halves"], guide, denoise_params, rgba8=rgba8)
        if albedo:
            res["albedo"] = guide
    state.advance(target, view if view is not None else previous_view(cam))
    return dict(out, **res)


def render_temporal_torch(device_scene: capi.DeviceScene, cam, cfg: rr_config, state: TemporalState, params=None, denoise_params=None, motion=None,
                          sample_xy=None, rgba8: bool = False, view=None, moved=None, albedo=False, clamp=None) -> dict:
    """One frame of a frame-after-frame loop on the device, with no host trip: rr_render_pixel_parts_device at n_parts = 2 (cfg.samples
    even), rr_accumulate_records_device against the history in `state`, rr_denoise_records_device with the accumulated halves -- three
    calls on torch's current stream, each reading what the one before wrote without a synchronisation.  params: a
    temporal.AccumulateParams whose scalars are used (its previous view is replaced by the state's); view: (world_to_clip, eye) of `cam`
    for the NEXT call (default: temporal.previous_view(cam), the float64 inverse of its inverses).  moved: (item_index (k,), prev_trans
    (k, 4, 4)) of the items that moved since the history was rendered and their `trans` then -- with a history and k > 0
    rr_motion_records_device makes the motion on the same stream, the second of four calls; together with `motion` it is a ValueError.
    Returns the dict of denoise_torch plus noisy (n, 8) and halves (n, 2, 8), the frame's own records, accumulated (n, 8),
    accumulated_halves (n, 2, 8) and length (n,): what the filter read, which `state` now holds as the history; and motion (n, 3) or None:
    what the accumulation read.  albedo=True: rr_surface_pixels_device on the same stream, one call more, makes the albedo of `cam` for the
    filter (returned as `albedo`); the accumulation itself blends un-demodulated colour, as without it.  albedo="mean":
    rr_albedo_pixels_device with the frame's config and table in its place.  albedo="diffuse" raises ValueError: the diffuse part is
    accumulated over time by render_temporal_split_torch.  clamp: None or False is rr_accumulate_records_device; True (the library's defaults) or a
    temporal.HistoryClampParams puts rr_accumulate_clamped_records_device in its place, on the same stream and the same buffers."""
    _check_albedo_mode(albedo, temporal=True)
    clamp = _clamp_params(clamp)         # (refused before anything is rendered)
    return _temporal_frame_torch(device_scene, cam, cfg, state, params, denoise_params, motion, sample_xy, rgba8, view, moved, False, clamp, albedo)


def render_temporal_split_torch(device_scene: capi.DeviceScene, cam, cfg: rr_config, state: TemporalState, params=None, denoise_params=None, motion=None,
                                sample_xy=None, rgba8: bool = False, view=None, moved=None, clamp=None) -> dict:
    """render_temporal_torch for the split arm, with no host trip: rr_render_pixel_split_device (cfg.samples even), with moved items
    rr_motion_records_device, rr_accumulate_split_records_device against the history in `state`, rr_albedo_pixels_device (the mean albedo,
    as render_denoised_torch(albedo="diffuse") uses) and rr_denoise_split_records_device on the accumulated layers -- four or five calls on
    torch's current stream, each reading what the ones before wrote without a synchronisation.  The arguments are render_temporal_torch's.
    A history without a diffuse part (a state render_temporal_torch filled), without halves or of another size resets the state, the
    items noted for this frame kept.  Returns the dict of render_temporal_torch (without a variance) plus diffuse (n, 3) and diffuse_halves
    (n, 2, 3), the frame's own, accumulated_diffuse and accumulated_diffuse_halves, what the filter read and `state` now holds, and
    albedo (n, 3).  clamp: anything but None or False raises ValueError that names render_temporal_split_clamped_torch, the pipeline with
    the clamped accumulation."""
    _no_split_clamp(clamp)
    return _temporal_frame_torch(device_scene, cam, cfg, state, params, denoise_params, motion, sample_xy, rgba8, view, moved, True, None)


def render_temporal_split_clamped_torch(device_scene: capi.DeviceScene, cam, cfg: rr_config, state: TemporalState, params=None, denoise_params=None, motion=None,
                                        sample_xy=None, rgba8: bool = False, view=None, moved=None, clamp=True) -> dict:
    """render_temporal_split_torch with the call of accumulate_clamped_split_torch in the place of rr_accumulate_split_records_device, on
    the same stream, the same buffers and the state's same diffuse sets: the split frame, with moved items the motion, the clamped split
    accumulation, the mean albedo, the split filter, with no host trip.  For the frames after an edit of lights, materials, textures or
    item flags, and under moving shadows.  clamp: True (the library's defaults) or a temporal.HistoryClampParams; None or False is a
    ValueError here (that is render_temporal_split_torch).  The arguments and the result are render_temporal_split_torch's."""
    clamp = _clamp_params(clamp)         # (refused before anything is rendered)
    if clamp is None:
        raise ValueError("clamp is True (the defaults) or a temporal.HistoryClampParams; without a clamp the pipeline is render_temporal_split_torch")
    return _temporal_frame_torch(device_scene, cam, cfg, state, params, denoise_params, motion, sample_xy, rgba8, view, moved, True, clamp)
