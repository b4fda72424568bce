"""ctypes binding of librustray_hip.so (the C ABI of include/rustray_hip.h).

This is the only way Python reaches the trace loop: there is no CPU or PyTorch
fallback.  If the HIP library has not been built, or no GPU is present, the
calls below raise — they never silently compute something else.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess
from typing import NamedTuple, Optional

import numpy as np

from .flat import (RR_ABI_VERSION, FlatScene, rr_camera, rr_config, rr_flat_scene, rr_frame, rr_frame_stats, rr_light, rr_material, rr_pick_result,
                   rr_radiance, rr_region, rr_surface_hit, rr_texture, rr_tuning, SURFACE_HIT_DTYPE)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("RUSTRAY_HIP_LIB") or os.path.join(_HERE, "librustray_hip.so")  # override: developer A/B builds
_LIB = None

class rr_shadow_hit(C.Structure):
    """include/rustray_hip.h: one record of rr_trace_shadow_rays."""
    _fields_ = [("occluded", C.c_uint32), ("item_index", C.c_uint32), ("object_id", C.c_uint32), ("face_id", C.c_uint32), ("distance", C.c_float)]


class rr_denoise_params(C.Structure):
    """include/rustray_hip.h: the parameters of rr_denoise_records."""
    _fields_ = [("struct_size", C.c_uint32), ("iterations", C.c_uint32), ("normal_power_log2", C.c_uint32), ("sigma_depth", C.c_float),
                ("sigma_luminance", C.c_float), ("gamma_correction", C.c_uint32)]


class rr_upsample_params(C.Structure):
    """include/rustray_hip.h: the parameters of rr_upsample_records."""
    _fields_ = [("struct_size", C.c_uint32), ("normal_power_log2", C.c_uint32), ("sigma_depth", C.c_float), ("use_albedo", C.c_uint32),
                ("gamma_correction", C.c_uint32)]


class rr_accumulate_params(C.Structure):
    """include/rustray_hip.h: the parameters of rr_accumulate_records."""
    _fields_ = [("struct_size", C.c_uint32), ("prev_world_to_clip", C.c_float * 16), ("prev_eye", C.c_float * 3), ("max_history", C.c_float),
                ("normal_min", C.c_float), ("sigma_depth", C.c_float), ("snap", C.c_float), ("gamma_correction", C.c_uint32)]


class rr_history_clamp_params(C.Structure):
    """include/rustray_hip.h: the clamp parameters of rr_accumulate_clamped_records."""
    _fields_ = [("struct_size", C.c_uint32), ("radius", C.c_uint32), ("sigma_scale", C.c_float)]


class RustrayHipError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"rustray_hip error {code}: {msg}")
        self.code = code


PASS_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_uint64, C.c_uint64)

# THE list of the files under csrc/ that librustray_hip.so is built from: rr_bvh.cpp and everything rr_api.hip includes.  The
# Makefile rule's prerequisites name the same files (tests/test_host.py compares both with the #include lines), and the developer
# tools that copy or read the sources (tools/ablate.py, tools/static_cost.py, tools/valu_mix.py) import this tuple.
LIB_SOURCES = ("rr_api.hip", "rr_api_base.h", "rr_sample_table.h", "rr_schedule_log.h", "rr_api_handle.h", "rr_api_scene.h", "rr_api_frame.h", "rr_api_multi.h", "rr_api_post.h", "rr_api_query.h", "rr_api_parts.h", "rr_api_adaptive.h", "rr_api_levels.h", "rr_api_prefix.h", "rr_api_denoise.h", "rr_api_temporal.h", "rr_api_motion.h", "rr_api_surface_pixels.h", "rr_api_albedo_pixels.h", "rr_api_pixel_split.h", "rr_api_upsample.h", "rr_api_probe.h", "rr_api_schedule_probe.h",
               "rr_kernels.hip", "rr_frame_plan.h", "rr_primary_setup.h", "rr_pixel_list.h", "rr_adaptive.h", "rr_denoise.h", "rr_temporal.h", "rr_history_clamp.h", "rr_motion.h", "rr_upsample.h", "rr_query_pointers.h", "rr_arg_ranges.h", "rr_scene_build.h", "rr_beam.h", "rr_bvh.cpp", "rr_bvh.h", "rr_device.h", "rr_math.h",
               "rr_primitives.h", "rr_walk.h", "rr_trace.h", "rr_surface.h", "rr_accumulate.h")


def source_id() -> str:
    """Identity of the kernel sources next to the library (sha256 over LIB_SOURCES + the header, 16 hex digits): what ties a committed
    counter profile (profiles/*_sq_counters.json) to the build a bench run measures."""
    import hashlib
    h = hashlib.sha256()
    files = [os.path.join(_HERE, "csrc", f) for f in LIB_SOURCES]
    files.append(os.path.join(os.path.dirname(_HERE), "include", "rustray_hip.h"))
    for f in files:
        with open(f, "rb") as fh:
            h.update(fh.read())
    return h.hexdigest()[:16]


def build(force: bool = False) -> str:
    """Compile librustray_hip.so for gfx950 with hipcc (cross-compiles without a GPU)."""
    csrc = os.path.join(_HERE, "csrc")
    if force and os.path.exists(LIB_PATH):
        os.remove(LIB_PATH)
    subprocess.check_call(["make", "-C", csrc], stdout=subprocess.DEVNULL)
    return LIB_PATH


class AccumulateRow(NamedTuple):
    """One buffer of the temporal calls: `name` is the header's parameter (the device forms append _dev, and the methods below _ptr), `shape`
    and `dtype` those of one pixel, `diffuse` says whether it is one of the six rows only the split calls have.  An output names in `key`
    its entry of the result dict, which is also the input it may be written over in place."""
    name: str
    shape: tuple
    diffuse: bool
    key: Optional[str] = None
    dtype: type = np.float32


# THE buffers of rr_accumulate[_clamped][_split]_records[_device], in the order of their arguments: the mirror of AccumulateIo and
# accumulate_rows in csrc/rr_api_temporal.h.  The calls that are not split take this table without its diffuse rows; that is the only
# difference between the argument lists.  Signatures, host arrays, device pointers and the torch wrappers (renderer.py) are read off it.
ACCUMULATE_ROWS = (
    AccumulateRow("records", (8,), False), AccumulateRow("halves", (2, 8), False),
    AccumulateRow("diffuse", (3,), True), AccumulateRow("diffuse_halves", (2, 3), True),
    AccumulateRow("history", (8,), False), AccumulateRow("history_halves", (2, 8), False),
    AccumulateRow("history_diffuse", (3,), True), AccumulateRow("history_diffuse_halves", (2, 3), True),
    AccumulateRow("history_length", (), False), AccumulateRow("motion", (3,), False),
    AccumulateRow("out", (8,), False, "records"), AccumulateRow("halves_out", (2, 8), False, "halves"),
    AccumulateRow("diffuse_out", (3,), True, "diffuse"), AccumulateRow("diffuse_halves_out", (2, 3), True, "diffuse_halves"),
    AccumulateRow("length_out", (), False, "length"), AccumulateRow("rgba8", (4,), False, "rgba", np.uint8))


def accumulate_rows(split: bool) -> tuple:
    """The rows of ACCUMULATE_ROWS a call has, in the order of its arguments."""
    return tuple(r for r in ACCUMULATE_ROWS if split or not r.diffuse)


def _accumulate_fn(split: bool, clamped: bool, device: bool) -> str:
    return "rr_accumulate" + ("_clamped" if clamped else "") + ("_split" if split else "") + "_records" + ("_device" if device else "")


def _accumulate_signatures() -> dict:
    """The eight temporal calls: scene, camera, params [, clamp], one pointer per row of the table [, the stream]."""
    sigs = {}
    for split in (False, True):
        for clamped in (False, True):
            args = [_V, _CAM, C.POINTER(rr_accumulate_params)] + ([C.POINTER(rr_history_clamp_params)] if clamped else []) + [_V] * len(accumulate_rows(split))
            sigs[_accumulate_fn(split, clamped, False)] = (args, C.c_int)
            sigs[_accumulate_fn(split, clamped, True)] = (args + [_V], C.c_int)
    return sigs


_V, _I, _F, _U16, _U32, _U64 = C.c_void_p, C.c_int, C.c_float, C.c_uint16, C.c_uint32, C.c_uint64
_CAM, _CFG, _DN, _COUNT = C.POINTER(rr_camera), C.POINTER(rr_config), C.POINTER(rr_denoise_params), C.POINTER(C.c_uint32)
_PIXELS = [_V, _CAM, _CFG, _V, _V, _U32]            # scene, camera, config, sample table, pixel list, n_pixels: how the pixel queries begin
_PROGRESSIVE = [_V, _CAM, _CFG, _V, C.POINTER(rr_frame), _U32, PASS_FN, _V, _V]
_ADAPTIVE = [_V, _CAM, _CFG, _U16, _U16, _F, _V, _V, _V, _V, _V, _V, _COUNT, _V]

# every function include/rustray_hip.h declares: name -> (argtypes, restype).  tests/test_temporal_binding_host.py compares the lengths
# with the header's parameter lists; EXPORTS, what build() and tests/test_abi.py look for in the library, is this table's names.
_PUBLIC = {
    "rr_abi_version": ([], _U32), "rr_device_count": ([], _I), "rr_last_error": ([], C.c_char_p),
    "rr_scene_create": ([C.POINTER(rr_flat_scene), _I, C.POINTER(_V)], _I), "rr_scene_destroy": ([_V], None),
    "rr_scene_update_transforms": ([_V, _V, _V], _I), "rr_scene_update_materials": ([_V, _V, _U32], _I), "rr_scene_update_lights": ([_V, _V, _U32], _I),
    "rr_scene_update_item_flags": ([_V, _V, _V, _U32], _I), "rr_scene_add_textures": ([_V, _V, _U32, _COUNT], _I),
    "rr_scene_add_meshes": ([_V, _V, _U32, _COUNT], _I), "rr_scene_set_items": ([_V, _V, _U32, _V, _U32], _I),
    "rr_scene_set_tuning": ([_V, C.POINTER(rr_tuning)], _I), "rr_scene_get_tuning": ([_V, C.POINTER(rr_tuning)], _I), "rr_scene_set_compat": ([_V, _U32], _I),
    "rr_scene_last_stats": ([_V, C.POINTER(rr_frame_stats)], _I), "rr_scene_overlap_stages": ([_V, _COUNT], _I),
    "rr_sample_table": ([_U16, _V, _COUNT], _I),
    "rr_render": ([_V, _CAM, _CFG, _V, C.POINTER(rr_frame), _V], _I),
    "rr_render_multi": ([C.POINTER(_V), _U32, _CAM, _CFG, _V, C.POINTER(rr_frame), _V], _I), "rr_multi_lock_order": ([C.POINTER(_V), _U32, _COUNT], _I),
    "rr_render_progressive": (_PROGRESSIVE, _I), "rr_render_progressive_tiles": (_PROGRESSIVE, _I),
    "rr_region_pixel_count": ([_U32, _U32, C.POINTER(rr_region)], _U64),
    "rr_render_region_device": ([_V, _CAM, _CFG, _V, C.POINTER(rr_region), C.POINTER(rr_frame), _V, _V], _I),
    "rr_deinterleave_device": ([_U32] * 6 + [_V, _V, _I, _V], _I),
    "rr_deinterleave_packed_device": ([_U32] * 5 + [_V, _U64, C.POINTER(_U64), _COUNT, C.POINTER(_V), _I, _V], _I),
    "rr_pick": ([_V, _CAM, _I, _I, C.POINTER(rr_pick_result)], _I),
    "rr_trace_rays": ([_V, _V, _V, _U32, _U32, _V], _I), "rr_trace_rays_device": ([_V, _V, _V, _U32, _U32, _V, _V], _I),
    "rr_trace_shadow_rays": ([_V, _V, _V, _V, _U32, _U32, C.POINTER(rr_shadow_hit)], _I), "rr_trace_shadow_rays_device": ([_V, _V, _V, _V, _U32, _U32, _V, _V], _I),
    "rr_shade_rays": ([_V, _CFG, _V, _V, _U32, _U32, _V, _V, _V], _I), "rr_shade_rays_device": ([_V, _CFG, _V, _V, _U32, _U32, _V, _V, _V, _V], _I),
    "rr_surface_rays": ([_V, _V, _V, _U32, _U32, _V], _I), "rr_surface_rays_device": ([_V, _V, _V, _U32, _U32, _V, _V], _I),
    "rr_render_pixels": (_PIXELS + [_V] * 3, _I), "rr_render_pixels_device": (_PIXELS + [_V] * 4, _I),
    "rr_render_pixel_parts": (_PIXELS + [_U32] + [_V] * 3, _I), "rr_render_pixel_parts_device": (_PIXELS + [_U32] + [_V] * 4, _I),
    "rr_refine_list_capacity": ([_U32, _U32], _U64), "rr_refine_list_device": ([_V, _U32, _U32, _V, _F, _V, _V, _COUNT, _V], _I),
    "rr_render_adaptive": (_ADAPTIVE, _I), "rr_render_adaptive_device": (_ADAPTIVE + [_V], _I),
    "rr_refine_sublist_device": ([_V, _V, _U32, _V, _F, _V, _V, _COUNT, _V], _I),
    "rr_render_adaptive_levels": ([_V, _CAM, _CFG, _V, _U32, _F] + [_V] * 7, _I), "rr_render_adaptive_levels_device": ([_V, _CAM, _CFG, _V, _U32, _F] + [_V] * 8, _I),
    "rr_render_pixel_prefix": (_PIXELS + [_U32] + [_V] * 4, _I), "rr_render_pixel_prefix_device": (_PIXELS + [_U32] + [_V] * 5, _I),
    "rr_render_adaptive_prefix": ([_V, _CAM, _CFG, _V, _V, _U32, _F] + [_V] * 6, _I), "rr_render_adaptive_prefix_device": ([_V, _CAM, _CFG, _V, _V, _U32, _F] + [_V] * 7, _I),
    "rr_denoise_default_params": ([_DN], _I),
    "rr_denoise_records": ([_V, _U32, _U32, _DN] + [_V] * 6, _I), "rr_denoise_records_device": ([_V, _U32, _U32, _DN] + [_V] * 7, _I),
    "rr_denoise_split_records": ([_V, _U32, _U32, _DN] + [_V] * 7, _I), "rr_denoise_split_records_device": ([_V, _U32, _U32, _DN] + [_V] * 8, _I),
    "rr_accumulate_default_params": ([C.POINTER(rr_accumulate_params)], _I), "rr_history_clamp_default_params": ([C.POINTER(rr_history_clamp_params)], _I),
    **_accumulate_signatures(),
    "rr_motion_records": ([_V, _CAM, _V, _V, _U32, _V, _V, _V], _I), "rr_motion_records_device": ([_V, _CAM, _V, _V, _U32, _V, _V, _V, _V], _I),
    "rr_surface_pixels": ([_V, _CAM, _V, _U32, _V, _V], _I), "rr_surface_pixels_device": ([_V, _CAM, _V, _U32, _V, _V, _V], _I),
    "rr_albedo_pixels": (_PIXELS + [_V] * 2, _I), "rr_albedo_pixels_device": (_PIXELS + [_V] * 3, _I),
    "rr_render_pixel_split": (_PIXELS + [_V] * 5, _I), "rr_render_pixel_split_device": (_PIXELS + [_V] * 6, _I),
    "rr_upsample_default_params": ([C.POINTER(rr_upsample_params)], _I),
    "rr_upsample_records": ([_V] + [_U32] * 4 + [C.POINTER(rr_upsample_params)] + [_V] * 8, _I),
    "rr_upsample_records_device": ([_V] + [_U32] * 4 + [C.POINTER(rr_upsample_params)] + [_V] * 9, _I),
    "rr_upsample_albedo_records": ([_V] + [_U32] * 4 + [C.POINTER(rr_upsample_params)] + [_V] * 10, _I),
    "rr_upsample_albedo_records_device": ([_V] + [_U32] * 4 + [C.POINTER(rr_upsample_params)] + [_V] * 11, _I),
    "rr_post_process": ([_U32, _U32, _I, _I, _V, _V, _V, _V, _I], _I), "rr_post_process_device": ([_U32, _U32, _I, _I, _V, _V, _V, _V, _I, _V], _I),
}
# the test entry points the binding calls: exported by the library, declared in no public header
_TEST_ONLY = {
    "rr_test_denoise_forms": ([_U32], None),
    "rr_test_schedule_record": ([_V, _I], _I), "rr_test_schedule_read": ([_V, _V, _U64, C.POINTER(_U64)], _I),
    "rr_math_probe": ([_I, _V, _V, _V, _I, _V, _V, _V, _U64, _I], _I),
}
SIGNATURES = {**_PUBLIC, **_TEST_ONLY}
EXPORTS = list(_PUBLIC)


def lib():
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                               "or `make -C rustray_amd/csrc` — there is no fallback path")
        L = C.CDLL(LIB_PATH)
        developer = bool(os.environ.get("RUSTRAY_HIP_LIB"))   # a developer A/B build of an older revision is the caller's business:
        got = 1                                               # it may speak another version and lack symbols
        if hasattr(L, "rr_abi_version"):
            L.rr_abi_version.restype = C.c_uint32
            got = L.rr_abi_version()
        if got != RR_ABI_VERSION and not developer:
            raise RuntimeError(f"{LIB_PATH} speaks ABI version {got}, this binding {RR_ABI_VERSION}: rebuild the library")
        for name, (argtypes, restype) in SIGNATURES.items():
            if developer and not hasattr(L, name):
                continue
            fn = getattr(L, name)   # (the shipped library lacks none of them: AttributeError)
            fn.argtypes, fn.restype = argtypes, restype
        _LIB = L
    return _LIB


def pack_pixels(pixels) -> np.ndarray:
    """The pixel list of rr_render_pixels: an (n, 2) integer array of (x, y) -> (n,) uint32 of x | y << 16; an (n,) array is taken as packed."""
    a = np.asarray(pixels)
    if a.ndim == 2 and a.shape[1] == 2:
        if len(a) and (a.min() < 0 or a.max() > 65535):
            raise ValueError("pixel coordinates must lie in 0 .. 65535")
        a = a.astype(np.uint32)
        return np.ascontiguousarray(a[:, 0] | (a[:, 1] << np.uint32(16)), np.uint32)
    if a.ndim != 1:
        raise ValueError(f"pixels of shape {a.shape}: (n, 2) of (x, y), or (n,) packed x | y << 16")
    return np.ascontiguousarray(a, np.uint32)


def _check(rc: int):
    if rc != 0:
        raise RustrayHipError(rc, lib().rr_last_error().decode("utf-8", "replace"))


def device_count() -> int:
    return int(lib().rr_device_count())


def sample_table(samples: int):
    """Built-in sub-sample table of the library (reference src/raytracing.rs:290-313)."""
    xy = np.zeros((max(samples, 1), 2), np.uint16)
    cs = C.c_uint32(0)
    _check(lib().rr_sample_table(C.c_uint16(samples), xy.ctypes.data_as(C.c_void_p), C.byref(cs)))
    return xy[:samples], int(cs.value)


def refine_list_capacity(width: int, height: int) -> int:
    """rr_refine_list_capacity: entries a refinement list of a width x height frame may need (every pixel, padded to a multiple of 64)."""
    return int(lib().rr_refine_list_capacity(C.c_uint32(width), C.c_uint32(height)))


def denoise_default_params() -> rr_denoise_params:
    """rr_denoise_default_params: 5 iterations, power 5, sigma_depth 0.05, sigma_luminance 4, no gamma (never touches a device)."""
    p = rr_denoise_params()
    _check(lib().rr_denoise_default_params(C.byref(p)))
    return p


def denoise_params(params=None) -> rr_denoise_params:
    """A denoise.DenoiseParams (or None: the library's defaults) as the C struct; a C struct is passed through."""
    if isinstance(params, rr_denoise_params):
        return params
    p = denoise_default_params()
    if params is not None:
        p.iterations, p.normal_power_log2 = int(params.iterations), int(params.normal_power_log2)
        p.sigma_depth, p.sigma_luminance = float(params.sigma_depth), float(params.sigma_luminance)
        p.gamma_correction = 1 if params.gamma_correction else 0
    return p


def upsample_default_params() -> rr_upsample_params:
    """rr_upsample_default_params: power 5, sigma_depth 0.05, albedo on, no gamma (never touches a device)."""
    p = rr_upsample_params()
    _check(lib().rr_upsample_default_params(C.byref(p)))
    return p


def upsample_params(params=None) -> rr_upsample_params:
    """An upsample.UpsampleParams (or None: the library's defaults) as the C struct; a C struct is passed through."""
    if isinstance(params, rr_upsample_params):
        return params
    p = upsample_default_params()
    if params is not None:
        p.normal_power_log2, p.sigma_depth = int(params.normal_power_log2), float(params.sigma_depth)
        p.use_albedo, p.gamma_correction = (1 if params.use_albedo else 0), (1 if params.gamma_correction else 0)
    return p


def accumulate_default_params() -> rr_accumulate_params:
    """rr_accumulate_default_params: max_history 32, normal_min 0.9, sigma_depth 0.05, snap 1/64, no gamma, the identity as the previous
    view and an eye of 0 (never touches a device)."""
    p = rr_accumulate_params()
    _check(lib().rr_accumulate_default_params(C.byref(p)))
    return p


def accumulate_params(params=None) -> rr_accumulate_params:
    """A temporal.AccumulateParams (or None: the library's defaults) as the C struct; a C struct is passed through."""
    if isinstance(params, rr_accumulate_params):
        return params
    p = accumulate_default_params()
    if params is not None:
        p.prev_world_to_clip[:] = np.asarray(params.prev_world_to_clip, np.float32).T.reshape(16).tolist()   # column-major
        p.prev_eye[:] = np.asarray(params.prev_eye, np.float32).reshape(3).tolist()
        p.max_history, p.normal_min = float(params.max_history), float(params.normal_min)
        p.sigma_depth, p.snap = float(params.sigma_depth), float(params.snap)
        p.gamma_correction = 1 if params.gamma_correction else 0
    return p


def history_clamp_default_params() -> rr_history_clamp_params:
    """rr_history_clamp_default_params: the radius and sigma_scale DESIGN.md's sweep chose (never touches a device)."""
    p = rr_history_clamp_params()
    _check(lib().rr_history_clamp_default_params(C.byref(p)))
    return p


def history_clamp_params(clamp=None) -> rr_history_clamp_params:
    """A temporal.HistoryClampParams (or None: the library's defaults) as the C struct; a C struct is passed through."""
    if isinstance(clamp, rr_history_clamp_params):
        return clamp
    p = history_clamp_default_params()
    if clamp is not None:
        p.radius, p.sigma_scale = int(clamp.radius), float(clamp.sigma_scale)
    return p


# the forms a pass of rr_denoise_records can run in (rustray_amd/csrc/rr_denoise.h)
DENOISE_FORM_AUTO, DENOISE_FORM_GATHER, DENOISE_FORM_TILE, DENOISE_FORM_LATTICE = 0, 1, 2, 3


def denoise_forms(forms=None):
    """The tuning hook of rr_denoise_records, process-wide: forms[i] is the form of pass i (DENOISE_FORM_*; a form that does not exist
    at that pass's step leaves it automatic); None = every pass automatic, the shipped choice.  The bits do not depend on it: for the
    tests that say so and for tools/denoise_time.py."""
    word = 0
    for i, f in enumerate(forms or ()):
        if not 0 <= int(f) <= 3 or i >= 6:
            raise ValueError(f"forms {forms}")
        word |= int(f) << (4 * i)
    lib().rr_test_denoise_forms(C.c_uint32(word))


def region_pixel_count(width: int, height: int, tile_w: int, tile_h: int, n_ranks: int, rank: int) -> int:
    rg = rr_region(tile_w, tile_h, n_ranks, rank)
    return int(lib().rr_region_pixel_count(width, height, C.byref(rg)))


def _sxy(sample_xy):
    if sample_xy is None:
        return None, None
    a = np.ascontiguousarray(sample_xy, np.uint16)
    return a, a.ctypes.data_as(C.c_void_p)


def _levels(levels, sample_xy_levels):
    """The sample counts of rr_render_adaptive_levels as a uint16 array, and its table pointers: (counts, what must stay alive, the
    array of n_levels pointers or None).  Values a uint16 cannot hold are refused here: the library would see other numbers."""
    lv = [int(v) for v in levels]
    if any(v < 0 or v > 0xffff for v in lv):
        raise ValueError(f"levels {lv}: sample counts are uint16")
    counts = np.ascontiguousarray(lv, np.uint16)
    if sample_xy_levels is None:
        return counts, None, None
    if len(sample_xy_levels) != len(lv):
        raise ValueError(f"{len(sample_xy_levels)} tables for {len(lv)} levels")
    keep = [_sxy(t)[0] for t in sample_xy_levels]
    ptrs = (C.c_void_p * max(len(lv), 1))(*[k.ctypes.data if k is not None else None for k in keep])
    return counts, (keep, ptrs), C.cast(ptrs, C.c_void_p)


def _ptr(p):
    """A raw pointer (an int) as a ctypes argument; None or 0 is NULL."""
    return C.c_void_p(p) if p else None


def _flag(cancel):
    """The optional cancel flag, a ctypes c_int, as a ctypes argument."""
    return C.byref(cancel) if cancel is not None else None


def _data(a):
    """A host array's memory as a ctypes argument; None is NULL."""
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _pixel_list(cam, pixels):
    """What a list call works on: (n, the packed list -- it must stay alive during the call --, its pointer); None is the whole frame."""
    if pixels is None:
        return int(cam.width) * int(cam.height), None, None
    xy = pack_pixels(pixels)
    return len(xy), xy, xy.ctypes.data_as(C.c_void_p)


def _records(a):
    """(..., 8) float32 rr_radiance records as the dict of shade_rays: copies, one array per field."""
    return dict(color=a[..., 0:3].copy(), depth=a[..., 3].copy(), normal=a[..., 4:7].copy(), object_id=a[..., 7].copy().view(np.uint32))


class _FusedOutputs:
    """The host outputs of a fused adaptive call over the frame of `cam`: records, sample counts, errors, on request the bytes, and
    n_counts uint32 words (n_refined, or level_pixels)."""

    def __init__(self, cam, rgba8: bool, n_counts: int):
        self.n = n = int(cam.width) * int(cam.height)
        self.out = np.zeros((max(n, 1), 8), np.float32)
        self.samples = np.zeros(max(n, 1), np.uint16)
        self.error = np.zeros(max(n, 1), np.float32)
        self.rgba = np.zeros((max(n, 1), 4), np.uint8) if rgba8 else None
        self.counts = np.zeros(max(n_counts, 1), np.uint32)

    def args(self):
        """out, rgba8_out, samples_out, error_out and the counts, in the order every fused entry point takes them"""
        return _data(self.out), _data(self.rgba), _data(self.samples), _data(self.error), self.counts.ctypes.data_as(C.POINTER(C.c_uint32))

    def result(self, **counts) -> dict:
        n = self.n
        res = dict(_records(self.out[:n]), samples=self.samples[:n].astype(np.uint32), error=self.error[:n], **counts)
        if self.rgba is not None:
            res["rgba"] = self.rgba[:n]
        return res


class DeviceScene:
    """Owns one `rr_scene*` (scene uploaded to one GPU, acceleration structures built)."""

    def __init__(self, flat_scene, device: int = 0):
        self._h = C.c_void_p(None)
        self.device = device
        self._flat = flat_scene               # keeps host arrays alive during the call
        fs = flat_scene.c_struct() if hasattr(flat_scene, "c_struct") else flat_scene
        _check(lib().rr_scene_create(C.byref(fs), device, C.byref(self._h)))

    def close(self):
        if self._h:
            lib().rr_scene_destroy(self._h)
            self._h = C.c_void_p(None)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    # -- whole frame into host arrays -------------------------------------------
    def render(self, cam: rr_camera, cfg: rr_config, sample_xy=None, aux: bool = True):
        w, h = cam.width, cam.height
        rgba = np.zeros((h, w, 4), np.uint8)
        out = dict(rgba=rgba)
        fr = rr_frame(rgba.ctypes.data, None, None, None)
        if aux:
            out["normal"] = np.zeros((h, w, 3), np.float32)
            out["depth"] = np.zeros((h, w), np.float32)
            out["object_id"] = np.zeros((h, w), np.uint32)
            fr = rr_frame(rgba.ctypes.data, out["normal"].ctypes.data, out["depth"].ctypes.data, out["object_id"].ctypes.data)
        keep, p = _sxy(sample_xy)
        _check(lib().rr_render(self._h, C.byref(cam), C.byref(cfg), p, C.byref(fr), None))
        return out

    def render_progressive(self, cam: rr_camera, cfg: rr_config, on_pass, min_passes: int = 8, sample_xy=None, aux: bool = True, tiles: bool = False):
        """rr_render_progressive: `on_pass(out, samples_done, samples_total)` sees the frame resolved over the samples
        finished so far after every device batch; a truthy return stops the frame (RustrayHipError, code -6).
        tiles=True: rr_render_progressive_tiles -- `min_passes` passes of interleaved 32x8 tiles, every pixel final when it appears."""
        w, h = cam.width, cam.height
        rgba = np.zeros((h, w, 4), np.uint8)
        out = dict(rgba=rgba)
        fr = rr_frame(rgba.ctypes.data, None, None, None)
        if aux:
            out["normal"] = np.zeros((h, w, 3), np.float32)
            out["depth"] = np.zeros((h, w), np.float32)
            out["object_id"] = np.zeros((h, w), np.uint32)
            fr = rr_frame(rgba.ctypes.data, out["normal"].ctypes.data, out["depth"].ctypes.data, out["object_id"].ctypes.data)
        keep, p = _sxy(sample_xy)
        errors = []

        def _cb(user, done, total):
            try:
                return 1 if on_pass(out, int(done), int(total)) else 0
            except BaseException as e:  # an exception must not unwind through the C frames
                errors.append(e)
                return 1
        cb = PASS_FN(_cb)
        fn = lib().rr_render_progressive_tiles if tiles else lib().rr_render_progressive
        rc = fn(self._h, C.byref(cam), C.byref(cfg), p, C.byref(fr), int(min_passes), cb, None, None)
        if errors:
            raise errors[0]
        _check(rc)
        return out

    # -- one rank's region into device (torch) tensors ----------------------------
    def render_region_device(self, cam, cfg, region: rr_region, out_ptrs, stream_ptr=None, sample_xy=None):
        """out_ptrs: (rgba8, normal, depth, object_id) device pointers (ints, None allowed for aux)."""
        fr = rr_frame(*[_ptr(p) for p in out_ptrs])
        keep, p = _sxy(sample_xy)
        _check(lib().rr_render_region_device(self._h, C.byref(cam), C.byref(cfg), p, C.byref(region), C.byref(fr),
                                             _ptr(stream_ptr), None))

    def update_transforms(self, trans: np.ndarray, trans_inv: np.ndarray):
        """trans / trans_inv: (n_items, 4, 4) in math layout."""
        t = np.ascontiguousarray(np.transpose(np.asarray(trans, np.float32), (0, 2, 1)))
        ti = np.ascontiguousarray(np.transpose(np.asarray(trans_inv, np.float32), (0, 2, 1)))
        _check(lib().rr_scene_update_transforms(self._h, t.ctypes.data_as(C.c_void_p), ti.ctypes.data_as(C.c_void_p)))

    def pick(self, cam: rr_camera, x: int, y: int) -> rr_pick_result:
        r = rr_pick_result()
        _check(lib().rr_pick(self._h, C.byref(cam), x, y, C.byref(r)))
        return r

    def update_materials(self, materials):
        """rr_scene_update_materials: `materials` = the flat scene's material list (same length and order), edited."""
        arr = (rr_material * len(materials))(*[m.c_struct() if hasattr(m, "c_struct") else m for m in materials])
        _check(lib().rr_scene_update_materials(self._h, arr, len(materials)))

    def update_lights(self, lights):
        """rr_scene_update_lights: the whole light list (flat.Light or rr_light), any length, in the order that gives each light its RNG stream."""
        n = len(lights)
        arr = (rr_light * max(n, 1))(*[l.c_struct() if hasattr(l, "c_struct") else l for l in lights])
        _check(lib().rr_scene_update_lights(self._h, arr if n else None, n))

    def update_item_flags(self, visible, flip_normals):
        """rr_scene_update_item_flags: ShapeBasics::visible / flip_normals of every item (sequences of the scene's item count)."""
        v = np.ascontiguousarray([1 if x else 0 for x in visible], np.uint8)
        f = np.ascontiguousarray([1 if x else 0 for x in flip_normals], np.uint8)
        if len(v) != len(f):
            raise ValueError(f"{len(v)} visible flags, {len(f)} flip_normals flags")
        _check(lib().rr_scene_update_item_flags(self._h, v.ctypes.data_as(C.c_void_p), f.ctypes.data_as(C.c_void_p), len(v)))

    def add_textures(self, images) -> int:
        """rr_scene_add_textures: appends (H, W, 4) uint8 images to the texture list; returns the index of the first."""
        keep = [np.ascontiguousarray(t, np.uint8) for t in images]
        arr = (rr_texture * max(len(keep), 1))()
        for i, t in enumerate(keep):
            assert t.ndim == 3 and t.shape[2] == 4
            arr[i].width, arr[i].height = t.shape[1], t.shape[0]
            arr[i].rgba8 = t.ctypes.data if t.size else None
        first = C.c_uint32(0)
        _check(lib().rr_scene_add_textures(self._h, arr, len(keep), C.byref(first)))
        return int(first.value)

    def add_meshes(self, meshes) -> int:
        """rr_scene_add_meshes: appends flat.MeshData meshes to the mesh list; returns the index of the first."""
        fs = FlatScene()
        fs.meshes = list(meshes)
        c = fs.c_struct()                     # (fs keeps the arrays alive during the call)
        first = C.c_uint32(0)
        _check(lib().rr_scene_add_meshes(self._h, c.meshes if len(fs.meshes) else None, len(fs.meshes), C.byref(first)))
        return int(first.value)

    def set_items(self, items, materials):
        """rr_scene_set_items: the whole item list (flat.Item; `mesh` = an index into the scene's resident meshes) and the whole
        material list (flat.Material or rr_material) that the items name, together."""
        fs = FlatScene()
        fs.items = list(items)
        c = fs.c_struct()
        arr = (rr_material * max(len(materials), 1))(*[m.c_struct() if hasattr(m, "c_struct") else m for m in materials])
        _check(lib().rr_scene_set_items(self._h, c.items if len(fs.items) else None, len(fs.items), arr if len(materials) else None, len(materials)))

    def set_tuning(self, **kw):
        """rr_scene_set_tuning: sample_group, queue_budget_bytes, shade_chunk_rays, kernel_timing, multi_force_staged, bin_min_rays (others keep their value)."""
        t = rr_tuning()
        _check(lib().rr_scene_get_tuning(self._h, C.byref(t)))
        for k, v in kw.items():
            if k not in ("sample_group", "queue_budget_bytes", "shade_chunk_rays", "kernel_timing", "multi_force_staged", "bin_min_rays"):
                raise TypeError(f"unknown tuning field {k}")
            setattr(t, k, int(v) & 0xffffffffffffffff)
        t.struct_size = C.sizeof(rr_tuning)
        _check(lib().rr_scene_set_tuning(self._h, C.byref(t)))

    def trace_rays(self, origins, dirs, depth: int = 2):
        """rr_trace_rays: closest hits of caller-supplied rays -> (found, item, face, toi) arrays."""
        o = np.ascontiguousarray(origins, np.float32); d = np.ascontiguousarray(dirs, np.float32)
        n = len(o)
        out = np.zeros((n, 5), np.uint32)
        _check(lib().rr_trace_rays(self._h, o.ctypes.data_as(C.c_void_p), d.ctypes.data_as(C.c_void_p), C.c_uint32(n), C.c_uint32(depth), out.ctypes.data_as(C.c_void_p)))
        return out[:, 0].astype(bool), out[:, 1].astype(np.int32), out[:, 3].copy(), out[:, 4].copy().view(np.float32)

    def trace_shadow_rays(self, origins, dirs, max_distance=None, depth: int = 2):
        """rr_trace_shadow_rays: shadow queries of caller-supplied rays, `max_distance` per ray or None for no limit ->
        (occluded bool, item int32 (-1 when not occluded), face uint32, toi float32) arrays."""
        o = np.ascontiguousarray(origins, np.float32); d = np.ascontiguousarray(dirs, np.float32)
        n = len(o)
        if len(d) != n:
            raise ValueError(f"{n} origins, {len(d)} directions")
        lim, lim_p = None, None
        if max_distance is not None:
            lim = np.ascontiguousarray(max_distance, np.float32).reshape(-1)
            if len(lim) != n:
                raise ValueError(f"{n} rays, {len(lim)} distances")
            lim_p = lim.ctypes.data_as(C.c_void_p)
        out = (rr_shadow_hit * max(n, 1))()
        _check(lib().rr_trace_shadow_rays(self._h, o.ctypes.data_as(C.c_void_p), d.ctypes.data_as(C.c_void_p), lim_p, C.c_uint32(n), C.c_uint32(depth), out))
        a = np.frombuffer(out, np.uint32, 5 * n).reshape(n, 5)
        return a[:, 0].astype(bool), a[:, 1].astype(np.int32), a[:, 3].copy(), a[:, 4].copy().view(np.float32)

    def shade_rays(self, origins, dirs, cfg: rr_config, rays_per_result: int = 1, stream_ids=None, cancel=None):
        """rr_shade_rays: get_color_depth_normal_id(scene, ray, 1) of caller-supplied rays, averaged over each result's
        `rays_per_result` consecutive rays -> dict(color (n, 3) float32 LINEAR, depth (n,), normal (n, 3), object_id (n,) uint32).
        stream_ids: the RNG pixel id of every result (default: its index); cancel: a ctypes c_int polled between launches."""
        o = np.ascontiguousarray(origins, np.float32).reshape(-1, 3); d = np.ascontiguousarray(dirs, np.float32).reshape(-1, 3)
        if len(d) != len(o):
            raise ValueError(f"{len(o)} origins, {len(d)} directions")
        rpr = int(rays_per_result)
        if rpr < 1 or len(o) % rpr:
            raise ValueError(f"{len(o)} rays are not whole results of {rpr} rays")
        n = len(o) // rpr
        ids, ids_p = None, None
        if stream_ids is not None:
            ids = np.ascontiguousarray(stream_ids, np.uint32).reshape(-1)
            if len(ids) != n:
                raise ValueError(f"{n} results, {len(ids)} stream ids")
            ids_p = ids.ctypes.data_as(C.c_void_p)
        out = np.zeros((max(n, 1), 8), np.float32)
        _check(lib().rr_shade_rays(self._h, C.byref(cfg), o.ctypes.data_as(C.c_void_p), d.ctypes.data_as(C.c_void_p), C.c_uint32(n), C.c_uint32(rpr), ids_p,
                                   out.ctypes.data_as(C.c_void_p), _flag(cancel)))
        return _records(out[:n])

    def surface_rays(self, origins, dirs, depth: int = 1):
        """rr_surface_rays: position, normals, uv and material of the closest hits of caller-supplied rays (depth 1 = a frame's primary
        ray) -> a structured array of n rr_surface_hit records (flat.SURFACE_HIT_DTYPE)."""
        o = np.ascontiguousarray(origins, np.float32).reshape(-1, 3); d = np.ascontiguousarray(dirs, np.float32).reshape(-1, 3)
        if len(d) != len(o):
            raise ValueError(f"{len(o)} origins, {len(d)} directions")
        n = len(o)
        out = np.zeros(max(n, 1), SURFACE_HIT_DTYPE)
        _check(lib().rr_surface_rays(self._h, o.ctypes.data_as(C.c_void_p), d.ctypes.data_as(C.c_void_p), C.c_uint32(n), C.c_uint32(depth), out.ctypes.data_as(C.c_void_p)))
        return out[:n]

    def surface_pixels(self, cam: rr_camera, pixels=None, records: bool = True, albedo: bool = True):
        """rr_surface_pixels: rr_surface_rays for the pixel-centre rays of `cam` (pixel_rays.pixel_rays), made on the device, for the pixels
        named in `pixels` (as render_pixels takes them) or for every pixel of the frame in row-major order (None).  Returns the structured
        array of n rr_surface_hit records (flat.SURFACE_HIT_DTYPE), the (n, 3) float32 albedo rr_denoise_records takes (the records'
        base_color, 0 for a miss), or with both the tuple (records, albedo)."""
        if not records and not albedo:
            raise ValueError("surface_pixels: neither records nor albedo")
        n, xy, xy_p = _pixel_list(cam, pixels)
        out = np.zeros(max(n, 1), SURFACE_HIT_DTYPE) if records else None
        alb = np.zeros((max(n, 1), 3), np.float32) if albedo else None
        _check(lib().rr_surface_pixels(self._h, C.byref(cam), xy_p, C.c_uint32(n), _data(out), _data(alb)))
        if records and albedo:
            return out[:n], alb[:n]
        return out[:n] if records else alb[:n]

    def surface_pixels_device(self, cam: rr_camera, pixel_xy_ptr, n: int, out_ptr, albedo_ptr, stream_ptr=None):
        """rr_surface_pixels_device: n uint32 entries x | y << 16 (None = the whole frame, n = width * height), n 128-byte rr_surface_hit
        records (16-byte aligned, or None) and n x 3 float32 of albedo (or None), all raw device pointers; enqueued on `stream_ptr`.  The
        whole-frame form is not waited for."""
        _check(lib().rr_surface_pixels_device(self._h, C.byref(cam), _ptr(pixel_xy_ptr), C.c_uint32(n), _ptr(out_ptr), _ptr(albedo_ptr), _ptr(stream_ptr)))

    def albedo_pixels(self, cam: rr_camera, cfg: rr_config, pixels=None, sample_xy=None, cancel=None):
        """rr_albedo_pixels: the frame's albedo per pixel -- the mean over the cfg.samples primary rays render_pixels traces for the pixel of
        the base colour at each ray's first hit (albedo.mean_albedo states the sum), for the pixels named in `pixels` (as render_pixels takes
        them) or for every pixel of the frame in row-major order (None) -> (n, 3) float32, the array rr_denoise_records takes as `albedo`."""
        n, xy, xy_p = _pixel_list(cam, pixels)
        alb = np.zeros((max(n, 1), 3), np.float32)
        keep, p = _sxy(sample_xy)
        _check(lib().rr_albedo_pixels(self._h, C.byref(cam), C.byref(cfg), p, xy_p, C.c_uint32(n), _data(alb), _flag(cancel)))
        return alb[:n]

    def albedo_pixels_device(self, cam: rr_camera, cfg: rr_config, pixel_xy_ptr, n_pixels: int, albedo_ptr, stream_ptr=None, sample_xy=None, cancel=None):
        """rr_albedo_pixels_device: n_pixels uint32 entries x | y << 16 (None = the whole frame, n_pixels = width * height) and n_pixels x 3
        float32 of albedo, raw device pointers, both 4-byte aligned; enqueued on `stream_ptr`."""
        keep, p = _sxy(sample_xy)
        _check(lib().rr_albedo_pixels_device(self._h, C.byref(cam), C.byref(cfg), p, _ptr(pixel_xy_ptr), C.c_uint32(n_pixels), _ptr(albedo_ptr),
                                             _ptr(stream_ptr), _flag(cancel)))

    def render_pixels(self, cam: rr_camera, cfg: rr_config, pixels=None, sample_xy=None, rgba8: bool = False, cancel=None):
        """rr_render_pixels: Raytracing::render(x, y) before its clamp, for the pixels named in `pixels` -- an (n, 2) integer array of
        (x, y) or an (n,) uint32 array of x | y << 16, in any order, duplicates allowed -- or for every pixel of the frame in row-major
        order (None) -> the dict of shade_rays (color LINEAR), plus `rgba` (n, 4) uint8, the frame's own bytes, with rgba8=True."""
        n, xy, xy_p = _pixel_list(cam, pixels)
        out = np.zeros((max(n, 1), 8), np.float32)
        rgba = np.zeros((max(n, 1), 4), np.uint8) if rgba8 else None
        keep, p = _sxy(sample_xy)
        _check(lib().rr_render_pixels(self._h, C.byref(cam), C.byref(cfg), p, xy_p, C.c_uint32(n), _data(out), _data(rgba), _flag(cancel)))
        res = _records(out[:n])
        if rgba8:
            res["rgba"] = rgba[:n]
        return res

    def render_pixels_device(self, cam: rr_camera, cfg: rr_config, pixel_xy_ptr, n_pixels: int, out_ptr, rgba8_ptr=None, stream_ptr=None, sample_xy=None, cancel=None):
        """rr_render_pixels_device: n_pixels uint32 entries x | y << 16 (None = the whole frame, n_pixels = width * height), n_pixels 32-byte
        rr_radiance records (16-byte aligned) and, optionally, n_pixels x 4 bytes, all raw device pointers; enqueued on `stream_ptr`."""
        keep, p = _sxy(sample_xy)
        _check(lib().rr_render_pixels_device(self._h, C.byref(cam), C.byref(cfg), p, _ptr(pixel_xy_ptr), C.c_uint32(n_pixels), _ptr(out_ptr), _ptr(rgba8_ptr),
                                             _ptr(stream_ptr), _flag(cancel)))

    def render_pixel_parts(self, cam: rr_camera, cfg: rr_config, pixels=None, n_parts: int = 2, sample_xy=None, cancel=None):
        """rr_render_pixel_parts: the pixels of render_pixels (a list, or None for the whole frame in row-major order) and, per pixel, the
        means over its n_parts interleaved sample subsets (part h = the samples s with s % n_parts == h) -> the dict of render_pixels
        plus parts = dict(color (n, K, 3) LINEAR, depth (n, K), normal (n, K, 3))."""
        n, xy, xy_p = _pixel_list(cam, pixels)
        K = int(n_parts)
        if K < 0 or K > 0xffffffff:
            raise ValueError(f"n_parts {n_parts}")
        out = np.zeros((max(n, 1), 8), np.float32)
        parts = np.zeros((max(n, 1), max(min(K, 64), 1), 8), np.float32)
        keep, p = _sxy(sample_xy)
        _check(lib().rr_render_pixel_parts(self._h, C.byref(cam), C.byref(cfg), p, xy_p, C.c_uint32(n), C.c_uint32(K), _data(out), _data(parts), _flag(cancel)))
        return dict(_records(out[:n]), parts=_records(parts[:n]))

    def render_pixel_parts_device(self, cam: rr_camera, cfg: rr_config, pixel_xy_ptr, n_pixels: int, n_parts: int, out_ptr, parts_ptr, stream_ptr=None,
                                  sample_xy=None, cancel=None):
        """rr_render_pixel_parts_device: n_pixels uint32 entries x | y << 16 (None = the whole frame, n_pixels = width * height), n_pixels and
        n_pixels * n_parts 32-byte rr_radiance records (both 16-byte aligned), all raw device pointers; enqueued on `stream_ptr`."""
        keep, p = _sxy(sample_xy)
        _check(lib().rr_render_pixel_parts_device(self._h, C.byref(cam), C.byref(cfg), p, _ptr(pixel_xy_ptr), C.c_uint32(n_pixels), C.c_uint32(n_parts), _ptr(out_ptr),
                                                  _ptr(parts_ptr), _ptr(stream_ptr), _flag(cancel)))

    def render_pixel_split(self, cam: rr_camera, cfg: rr_config, pixels=None, halves: bool = True, sample_xy=None, cancel=None):
        """rr_render_pixel_split: the dict of render_pixel_parts at n_parts = 2 (without `parts` when halves=False: the dict of render_pixels)
        plus diffuse (n, 3) float32, the direct diffuse light of the primary hits summed on its own, and with halves diffuse_halves (n, 2, 3)."""
        n, xy, xy_p = _pixel_list(cam, pixels)
        out = np.zeros((max(n, 1), 8), np.float32)
        parts = np.zeros((max(n, 1), 2, 8), np.float32) if halves else None
        dif = np.zeros((max(n, 1), 3), np.float32)
        dif_h = np.zeros((max(n, 1), 2, 3), np.float32) if halves else None
        keep, p = _sxy(sample_xy)
        _check(lib().rr_render_pixel_split(self._h, C.byref(cam), C.byref(cfg), p, xy_p, C.c_uint32(n), _data(out), _data(parts), _data(dif), _data(dif_h), _flag(cancel)))
        res = dict(_records(out[:n]), diffuse=dif[:n])
        if halves:
            res["parts"] = _records(parts[:n])
            res["diffuse_halves"] = dif_h[:n]
        return res

    def render_pixel_split_device(self, cam: rr_camera, cfg: rr_config, pixel_xy_ptr, n_pixels: int, out_ptr, halves_ptr, diffuse_ptr, diffuse_halves_ptr,
                                  stream_ptr=None, sample_xy=None, cancel=None):
        """rr_render_pixel_split_device: n_pixels uint32 entries x | y << 16 (None = the whole frame, n_pixels = width * height), n_pixels and
        (or None) n_pixels * 2 32-byte rr_radiance records (16-byte aligned), n_pixels x 3 and (None exactly when halves_ptr is) n_pixels x 2 x 3
        float32, all raw device pointers; enqueued on `stream_ptr`."""
        keep, p = _sxy(sample_xy)
        _check(lib().rr_render_pixel_split_device(self._h, C.byref(cam), C.byref(cfg), p, _ptr(pixel_xy_ptr), C.c_uint32(n_pixels), _ptr(out_ptr), _ptr(halves_ptr),
                                                  _ptr(diffuse_ptr), _ptr(diffuse_halves_ptr), _ptr(stream_ptr), _flag(cancel)))

    # -- adaptive sampling on the device ----------------------------------------------
    def refine_list_device(self, width: int, height: int, parts_ptr, threshold: float, error_ptr, list_ptr, stream_ptr=None) -> int:
        """rr_refine_list_device: adaptive.refine_list(adaptive.half_error(parts), threshold, width, height) on the device.  parts_ptr: the
        width * height * 2 part records of a whole frame at n_parts = 2 (16-byte aligned); error_ptr: width * height float32 or None; list_ptr:
        refine_list_capacity(width, height) uint32, of which the padded list is written; raw device pointers, enqueued on `stream_ptr`.  Returns
        the number of entries before the pad (the call waits for it)."""
        count = C.c_uint32(0)
        _check(lib().rr_refine_list_device(self._h, C.c_uint32(width), C.c_uint32(height), _ptr(parts_ptr), C.c_float(threshold), _ptr(error_ptr), _ptr(list_ptr),
                                           C.byref(count), _ptr(stream_ptr)))
        return int(count.value)

    def render_adaptive(self, cam: rr_camera, cfg: rr_config, base_samples: int, max_samples: int, threshold: float, sample_xy_base=None, sample_xy_max=None,
                        rgba8: bool = False, cancel=None) -> dict:
        """rr_render_adaptive: every pixel at `base_samples`, and at `max_samples` where the half-buffer error of the base frame exceeds
        `threshold` -- estimate, list, fine pass and scatter in one call on the device.  Returns the dict of Raytracing.render_adaptive in
        row-major order (color (n, 3) LINEAR, depth, normal, object_id, samples uint32, error) plus n_refined, and `rgba` (n, 4) uint8, the
        frame's own bytes, with rgba8=True.  cfg.samples is ignored."""
        f = _FusedOutputs(cam, rgba8, 1)
        keep_b, pb = _sxy(sample_xy_base)
        keep_m, pm = _sxy(sample_xy_max)
        _check(lib().rr_render_adaptive(self._h, C.byref(cam), C.byref(cfg), C.c_uint16(base_samples), C.c_uint16(max_samples), C.c_float(threshold), pb, pm,
                                        *f.args(), _flag(cancel)))
        return f.result(n_refined=int(f.counts[0]))

    def render_adaptive_device(self, cam: rr_camera, cfg: rr_config, base_samples: int, max_samples: int, threshold: float, out_ptr, rgba8_ptr=None, samples_ptr=None,
                               error_ptr=None, stream_ptr=None, sample_xy_base=None, sample_xy_max=None, cancel=None) -> int:
        """rr_render_adaptive_device: width * height 32-byte rr_radiance records (16-byte aligned) and, optionally, as many x 4 bytes, uint16
        sample counts and float32 errors, all raw device pointers; enqueued on `stream_ptr`.  Returns the number of refined pixels."""
        keep_b, pb = _sxy(sample_xy_base)
        keep_m, pm = _sxy(sample_xy_max)
        count = C.c_uint32(0)
        _check(lib().rr_render_adaptive_device(self._h, C.byref(cam), C.byref(cfg), C.c_uint16(base_samples), C.c_uint16(max_samples), C.c_float(threshold), pb, pm,
                                               _ptr(out_ptr), _ptr(rgba8_ptr), _ptr(samples_ptr), _ptr(error_ptr), C.byref(count), _ptr(stream_ptr), _flag(cancel)))
        return int(count.value)

    # -- refinement level by level -----------------------------------------------------
    def refine_sublist_device(self, list_ptr, count: int, parts_ptr, threshold: float, error_ptr, list_out_ptr, stream_ptr=None) -> int:
        """rr_refine_sublist_device: adaptive.refine_sublist(adaptive.half_error(parts), threshold, list, count) on the device.  list_ptr:
        `count` uint32 entries; parts_ptr: their count * 2 part records at n_parts = 2 (16-byte aligned); error_ptr: count float32 or None;
        list_out_ptr: count rounded up to a multiple of 64 uint32, of which the padded result is written; raw device pointers, enqueued
        on `stream_ptr`.  Returns the number of entries before the pad (the call waits for it)."""
        taken = C.c_uint32(0)
        _check(lib().rr_refine_sublist_device(self._h, _ptr(list_ptr), C.c_uint32(count), _ptr(parts_ptr), C.c_float(threshold), _ptr(error_ptr), _ptr(list_out_ptr),
                                              C.byref(taken), _ptr(stream_ptr)))
        return int(taken.value)

    def render_adaptive_levels(self, cam: rr_camera, cfg: rr_config, levels, threshold: float, sample_xy_levels=None, rgba8: bool = False, cancel=None) -> dict:
        """rr_render_adaptive_levels: every pixel at levels[0], and level after level the pixels whose half-buffer error still exceeds
        `threshold` at the next count (even, strictly increasing, 2 to 8 of them) -- one call on the device.  sample_xy_levels: None, or
        one table or None per level.  Returns the dict of Raytracing.render_adaptive_levels in row-major order (color (n, 3) LINEAR,
        depth, normal, object_id, samples uint32, error: the RESIDUAL error at the pixel's own count, level_pixels), and `rgba` (n, 4)
        uint8, the frame's own bytes, with rgba8=True.  cfg.samples is ignored."""
        lv, keep, tables = _levels(levels, sample_xy_levels)
        f = _FusedOutputs(cam, rgba8, len(lv))
        _check(lib().rr_render_adaptive_levels(self._h, C.byref(cam), C.byref(cfg), _data(lv), C.c_uint32(len(lv)), C.c_float(threshold), tables, *f.args(),
                                               _flag(cancel)))
        return f.result(level_pixels=[int(v) for v in f.counts[:len(lv)]])

    def render_adaptive_levels_device(self, cam: rr_camera, cfg: rr_config, levels, threshold: float, out_ptr, rgba8_ptr=None, samples_ptr=None, error_ptr=None,
                                      stream_ptr=None, sample_xy_levels=None, cancel=None) -> list:
        """rr_render_adaptive_levels_device: width * height 32-byte rr_radiance records (16-byte aligned) and, optionally, as many x 4 bytes,
        uint16 sample counts and float32 errors, all raw device pointers; enqueued on `stream_ptr`.  Returns level_pixels, a list of ints."""
        lv, keep, tables = _levels(levels, sample_xy_levels)
        level_pixels = np.zeros(max(len(lv), 1), np.uint32)
        _check(lib().rr_render_adaptive_levels_device(self._h, C.byref(cam), C.byref(cfg), _data(lv), C.c_uint32(len(lv)), C.c_float(threshold), tables, _ptr(out_ptr),
                                                      _ptr(rgba8_ptr), _ptr(samples_ptr), _ptr(error_ptr), _data(level_pixels), _ptr(stream_ptr), _flag(cancel)))
        return [int(v) for v in level_pixels[:len(lv)]]

    # -- refinement that keeps its samples ---------------------------------------------
    def render_pixel_prefix(self, cam: rr_camera, cfg: rr_config, pixels=None, samples_used: int = 1, halves: bool = False, sample_xy=None, rgba8: bool = False,
                            cancel=None):
        """rr_render_pixel_prefix: render_pixels over samples 0 .. samples_used - 1 of the frame of cfg.samples samples (its table, its cell
        size, its generator keys), the sums divided by samples_used -> the dict of render_pixels; with halves=True (samples_used even) plus
        parts = the dict render_pixel_parts gives at n_parts = 2: half h = the samples s < samples_used with s % 2 == h."""
        n, xy, xy_p = _pixel_list(cam, pixels)
        k = int(samples_used)
        if k < 0 or k > 0xffffffff:
            raise ValueError(f"samples_used {samples_used}")
        out = np.zeros((max(n, 1), 8), np.float32)
        parts = np.zeros((max(n, 1), 2, 8), np.float32) if halves else None
        rgba = np.zeros((max(n, 1), 4), np.uint8) if rgba8 else None
        keep, p = _sxy(sample_xy)
        _check(lib().rr_render_pixel_prefix(self._h, C.byref(cam), C.byref(cfg), p, xy_p, C.c_uint32(n), C.c_uint32(k), _data(out), _data(parts), _data(rgba),
                                            _flag(cancel)))
        res = _records(out[:n])
        if halves:
            res["parts"] = _records(parts[:n])
        if rgba8:
            res["rgba"] = rgba[:n]
        return res

    def render_pixel_prefix_device(self, cam: rr_camera, cfg: rr_config, pixel_xy_ptr, n_pixels: int, samples_used: int, out_ptr, halves_ptr=None, rgba8_ptr=None,
                                   stream_ptr=None, sample_xy=None, cancel=None):
        """rr_render_pixel_prefix_device: n_pixels uint32 entries x | y << 16 (None = the whole frame, n_pixels = width * height), n_pixels
        and, optionally, n_pixels * 2 32-byte rr_radiance records (16-byte aligned) and n_pixels x 4 bytes, all raw device pointers; enqueued
        on `stream_ptr`."""
        keep, p = _sxy(sample_xy)
        _check(lib().rr_render_pixel_prefix_device(self._h, C.byref(cam), C.byref(cfg), p, _ptr(pixel_xy_ptr), C.c_uint32(n_pixels), C.c_uint32(samples_used),
                                                   _ptr(out_ptr), _ptr(halves_ptr), _ptr(rgba8_ptr), _ptr(stream_ptr), _flag(cancel)))

    def render_adaptive_prefix(self, cam: rr_camera, cfg: rr_config, prefix_samples, threshold: float, sample_xy=None, rgba8: bool = False, cancel=None) -> dict:
        """rr_render_adaptive_prefix: every pixel over the first prefix_samples[0] samples of the frame of cfg.samples samples, and level
        after level ONLY the samples up to the next prefix (even, strictly increasing, 2 to 8 of them, the last one cfg.samples) for the
        pixels whose half-buffer error still exceeds `threshold`, added to the sums those pixels have -- one call on the device.  sample_xy:
        ONE table of cfg.samples entries or None.  Returns the dict of render_adaptive_levels."""
        lv, _, _ = _levels(prefix_samples, None)
        f = _FusedOutputs(cam, rgba8, len(lv))
        keep, p = _sxy(sample_xy)
        _check(lib().rr_render_adaptive_prefix(self._h, C.byref(cam), C.byref(cfg), p, _data(lv), C.c_uint32(len(lv)), C.c_float(threshold), *f.args(), _flag(cancel)))
        return f.result(level_pixels=[int(v) for v in f.counts[:len(lv)]])

    def render_adaptive_prefix_device(self, cam: rr_camera, cfg: rr_config, prefix_samples, threshold: float, out_ptr, rgba8_ptr=None, samples_ptr=None, error_ptr=None,
                                      stream_ptr=None, sample_xy=None, cancel=None) -> list:
        """rr_render_adaptive_prefix_device: the buffers of render_adaptive_levels_device.  Returns level_pixels, a list of ints."""
        lv, _, _ = _levels(prefix_samples, None)
        level_pixels = np.zeros(max(len(lv), 1), np.uint32)
        keep, p = _sxy(sample_xy)
        _check(lib().rr_render_adaptive_prefix_device(self._h, C.byref(cam), C.byref(cfg), p, _data(lv), C.c_uint32(len(lv)), C.c_float(threshold), _ptr(out_ptr),
                                                      _ptr(rgba8_ptr), _ptr(samples_ptr), _ptr(error_ptr), _data(level_pixels), _ptr(stream_ptr), _flag(cancel)))
        return [int(v) for v in level_pixels[:len(lv)]]

    # -- the a-trous filter over a frame of records ------------------------------------
    def denoise_records(self, width: int, height: int, records, halves=None, albedo=None, params=None, rgba8: bool = False, variance: bool = True,
                        in_place: bool = False) -> dict:
        """rr_denoise_records: denoise.atrous_denoise on the device, host arrays in and out.  records: (n, 8) float32 rr_radiance records of
        the whole frame in row-major order; halves: (n, 2, 8) or None; albedo: (n, 3) or None; params: a denoise.DenoiseParams or None.
        Returns dict(records (n, 8) float32, and on request variance (n,) float32 and rgba (n, 4) uint8); in_place filters a copy of
        `records` in place (out == records)."""
        n = int(width) * int(height)
        rec = np.array(records, np.float32, order="C").reshape(n, 8) if in_place else np.ascontiguousarray(records, np.float32).reshape(n, 8)
        hv = None if halves is None else np.ascontiguousarray(halves, np.float32).reshape(n, 2, 8)
        al = None if albedo is None else np.ascontiguousarray(albedo, np.float32).reshape(n, 3)
        out = rec if in_place else np.zeros((n, 8), np.float32)
        rgba = np.zeros((n, 4), np.uint8) if rgba8 else None
        var = np.zeros(n, np.float32) if variance else None
        p = denoise_params(params)
        _check(lib().rr_denoise_records(self._h, C.c_uint32(width), C.c_uint32(height), C.byref(p), _data(rec), _data(hv), _data(al), _data(out), _data(rgba), _data(var)))
        res = dict(records=out)
        if variance:
            res["variance"] = var
        if rgba8:
            res["rgba"] = rgba
        return res

    def denoise_records_device(self, width: int, height: int, records_ptr, halves_ptr, albedo_ptr, out_ptr, rgba8_ptr=None, variance_ptr=None, params=None,
                               stream_ptr=None):
        """rr_denoise_records_device: width * height 32-byte records in and out (16-byte aligned; out_ptr may be records_ptr), optionally
        twice as many half records, width * height * 3 float32 of albedo, width * height x 4 bytes and as many float32 of variance, all raw
        device pointers; enqueued on `stream_ptr`, not waited for."""
        p = denoise_params(params)
        _check(lib().rr_denoise_records_device(self._h, C.c_uint32(width), C.c_uint32(height), C.byref(p), _ptr(records_ptr), _ptr(halves_ptr), _ptr(albedo_ptr),
                                               _ptr(out_ptr), _ptr(rgba8_ptr), _ptr(variance_ptr), _ptr(stream_ptr)))

    def denoise_split(self, width: int, height: int, records, diffuse, halves=None, diffuse_halves=None, albedo=None, params=None, rgba8: bool = False,
                      in_place: bool = False) -> dict:
        """rr_denoise_split_records: denoise.atrous_denoise_split on the device, host arrays in and out.  records, halves, albedo and params
        as denoise_records takes them; diffuse: (n, 3) float32, diffuse_halves: (n, 2, 3) or None (exactly when halves is).  Returns
        dict(records (n, 8) float32, and on request rgba (n, 4) uint8)."""
        n = int(width) * int(height)
        rec = np.array(records, np.float32, order="C").reshape(n, 8) if in_place else np.ascontiguousarray(records, np.float32).reshape(n, 8)
        hv = None if halves is None else np.ascontiguousarray(halves, np.float32).reshape(n, 2, 8)
        df = None if diffuse is None else np.ascontiguousarray(diffuse, np.float32).reshape(n, 3)
        dh = None if diffuse_halves is None else np.ascontiguousarray(diffuse_halves, np.float32).reshape(n, 2, 3)
        al = None if albedo is None else np.ascontiguousarray(albedo, np.float32).reshape(n, 3)
        out = rec if in_place else np.zeros((n, 8), np.float32)
        rgba = np.zeros((n, 4), np.uint8) if rgba8 else None
        p = denoise_params(params)
        _check(lib().rr_denoise_split_records(self._h, C.c_uint32(width), C.c_uint32(height), C.byref(p), _data(rec), _data(hv), _data(df), _data(dh), _data(al),
                                              _data(out), _data(rgba)))
        res = dict(records=out)
        if rgba8:
            res["rgba"] = rgba
        return res

    def denoise_split_device(self, width: int, height: int, records_ptr, halves_ptr, diffuse_ptr, diffuse_halves_ptr, albedo_ptr, out_ptr, rgba8_ptr=None, params=None,
                             stream_ptr=None):
        """rr_denoise_split_records_device: the buffers of denoise_records_device without the variance, plus width * height x 3 float32 of
        diffuse and (None exactly when halves_ptr is) width * height x 2 x 3 of its halves, all raw device pointers; enqueued on `stream_ptr`,
        not waited for."""
        p = denoise_params(params)
        _check(lib().rr_denoise_split_records_device(self._h, C.c_uint32(width), C.c_uint32(height), C.byref(p), _ptr(records_ptr), _ptr(halves_ptr), _ptr(diffuse_ptr),
                                                     _ptr(diffuse_halves_ptr), _ptr(albedo_ptr), _ptr(out_ptr), _ptr(rgba8_ptr), _ptr(stream_ptr)))

    # -- the joint-bilateral upsampler: a low-resolution frame raised by the G-buffer -------
    def upsample(self, low_width: int, low_height: int, width: int, height: int, low, guide_low, guide, halves_low=None, params=None, rgba8: bool = False,
                 weight: bool = True, albedo_low=None, albedo=None) -> dict:
        """rr_upsample_records: upsample.upsample_records on the device, host arrays in and out.  low: (w h, 8) float32 rr_radiance records
        of the low frame in row-major order; halves_low: (w h, 2, 8) or None; guide_low, guide: w h and W H rr_surface_hit records
        (flat.SURFACE_HIT_DTYPE, what surface_pixels returns); params: an upsample.UpsampleParams or None.  Returns dict(records (W H, 8)
        float32, halves (W H, 2, 8) or None, and on request weight (W H,) float32 and rgba (W H, 4) uint8).  albedo_low (w h, 3) and
        albedo (W H, 3) float32, each or None: the caller's albedo planes, and the call is rr_upsample_albedo_records; with both None it is
        rr_upsample_records itself (the same bits either way: the older symbol, so that a library without the newer one still serves)."""
        from .upsample import guide_array
        nl, n = int(low_width) * int(low_height), int(width) * int(height)
        rec = np.ascontiguousarray(low, np.float32).reshape(nl, 8)
        hv = None if halves_low is None else np.ascontiguousarray(halves_low, np.float32).reshape(nl, 2, 8)
        gl, gf = guide_array(guide_low, nl), guide_array(guide, n)
        out = np.zeros((n, 8), np.float32)
        hout = None if hv is None else np.zeros((n, 2, 8), np.float32)
        rgba = np.zeros((n, 4), np.uint8) if rgba8 else None
        wt = np.zeros(n, np.float32) if weight else None
        p = upsample_params(params)
        size = (C.c_uint32(low_width), C.c_uint32(low_height), C.c_uint32(width), C.c_uint32(height))
        if albedo_low is None and albedo is None:
            _check(lib().rr_upsample_records(self._h, *size, C.byref(p), _data(rec), _data(hv), _data(gl), _data(gf), _data(out), _data(hout), _data(rgba), _data(wt)))
        else:
            al = None if albedo_low is None else np.ascontiguousarray(albedo_low, np.float32).reshape(nl, 3)
            af = None if albedo is None else np.ascontiguousarray(albedo, np.float32).reshape(n, 3)
            _check(lib().rr_upsample_albedo_records(self._h, *size, C.byref(p), _data(rec), _data(hv), _data(gl), _data(gf), _data(al), _data(af), _data(out),
                                                    _data(hout), _data(rgba), _data(wt)))
        res = dict(records=out, halves=hout)
        if weight:
            res["weight"] = wt
        if rgba8:
            res["rgba"] = rgba
        return res

    def upsample_device(self, low_width: int, low_height: int, width: int, height: int, low_ptr, halves_low_ptr, guide_low_ptr, guide_ptr, out_ptr, halves_out_ptr=None,
                        rgba8_ptr=None, weight_out_ptr=None, params=None, stream_ptr=None, albedo_low=None, albedo=None):
        """rr_upsample_records_device: low_width * low_height 32-byte records (and optionally twice as many half records) and as many
        128-byte rr_surface_hit records in, width * height surface records in, width * height records (and twice as many half records,
        exactly when the low halves are given) out, all 16-byte aligned; optionally width * height x 4 bytes and as many float32 of
        weight; all raw device pointers, none overlapping another; enqueued on `stream_ptr`, not waited for.  albedo_low and albedo: raw
        device pointers too (albedo_low_dev and albedo_dev of rr_upsample_albedo_records_device: low_width * low_height x 3 and width *
        height x 3 float32, 4-byte aligned), each or None; with both None the call is rr_upsample_records_device itself."""
        p = upsample_params(params)
        size = (C.c_uint32(low_width), C.c_uint32(low_height), C.c_uint32(width), C.c_uint32(height))
        if albedo_low is None and albedo is None:
            _check(lib().rr_upsample_records_device(self._h, *size, C.byref(p), _ptr(low_ptr), _ptr(halves_low_ptr), _ptr(guide_low_ptr), _ptr(guide_ptr), _ptr(out_ptr),
                                                    _ptr(halves_out_ptr), _ptr(rgba8_ptr), _ptr(weight_out_ptr), _ptr(stream_ptr)))
        else:
            _check(lib().rr_upsample_albedo_records_device(self._h, *size, C.byref(p), _ptr(low_ptr), _ptr(halves_low_ptr), _ptr(guide_low_ptr), _ptr(guide_ptr),
                                                           _ptr(albedo_low), _ptr(albedo), _ptr(out_ptr), _ptr(halves_out_ptr), _ptr(rgba8_ptr), _ptr(weight_out_ptr),
                                                           _ptr(stream_ptr)))

    # -- temporal reprojection of a frame of records -----------------------------------
    # The four calls in their two forms are ONE host body and ONE device body over ACCUMULATE_ROWS; the eight methods below are their
    # signatures and docstrings, and hand their own arguments over by name (locals()), so no buffer is listed by position anywhere.
    def _accumulate_call(self, split: bool, clamp, device: bool, cam, params, buffers):
        """rr_accumulate[_clamped][_split]_records[_device]: the variant by (split, clamp: the clamped pair's C struct, else None, device);
        `buffers`: what follows scene, camera, params and the clamp, in the order of accumulate_rows(split)."""
        p = accumulate_params(params)
        head = [self._h, C.byref(cam), C.byref(p)] + ([C.byref(clamp)] if clamp is not None else [])
        _check(getattr(lib(), _accumulate_fn(split, clamp is not None, device))(*head, *buffers))

    def _accumulate(self, split: bool, clamp, cam, arrays, params, rgba8: bool, in_place=()) -> dict:
        """The host form.  arrays: the inputs by row name (None where the call has none), as contiguous float32 views of one pixel's shape
        per row; in_place: the input rows accumulated into private copies, each then the output that names it as its key.  The other
        outputs are made where their input is present, the length always, the bytes with rgba8 -> the result dict by the outputs' keys."""
        n = int(cam.width) * int(cam.height)
        rows, buf = accumulate_rows(split), {}
        for r in rows:
            if r.key is None:
                a = arrays[r.name]
                if a is not None:
                    a = (np.array(a, np.float32, order="C") if r.name in in_place else np.ascontiguousarray(a, np.float32)).reshape((n,) + r.shape)
                buf[r.name] = a
            elif r.key in in_place:
                buf[r.name] = buf[r.key]
            else:
                wanted = rgba8 if r.key == "rgba" else r.key == "length" or buf[r.key] is not None
                buf[r.name] = np.zeros((n,) + r.shape, r.dtype) if wanted else None
        self._accumulate_call(split, clamp, False, cam, params, [_data(buf[r.name]) for r in rows])
        res = {r.key: buf[r.name] for r in rows if r.key is not None and (r.key != "rgba" or rgba8)}
        return dict(records=res.pop("records"), length=res.pop("length"), **res)   # (the keys in the order they have always had)

    def _accumulate_device(self, split: bool, clamp, cam, pointers, params, stream_ptr):
        """The device form.  pointers: raw device pointers by row name + "_ptr" (None where the call has none), then the stream."""
        self._accumulate_call(split, clamp, True, cam, params, [_ptr(pointers[r.name + "_ptr"]) for r in accumulate_rows(split)] + [_ptr(stream_ptr)])

    def accumulate_records(self, cam: rr_camera, records, halves=None, history=None, history_halves=None, history_length=None, motion=None, params=None,
                           rgba8: bool = False, in_place: bool = False) -> dict:
        """rr_accumulate_records: temporal.accumulate_records on the device, host arrays in and out.  records (n, 8) float32 rr_radiance
        records of the whole frame of `cam` in row-major order; halves (n, 2, 8) or None; history (n, 8), history_halves (n, 2, 8) and
        history_length (n,): the previous call's records, halves and length, or None on the first frame; motion (n, 3) or None; params: a
        temporal.AccumulateParams or None.  Returns dict(records (n, 8), length (n,), halves (n, 2, 8) or None [, rgba (n, 4) uint8]);
        in_place accumulates into copies of `records` and `halves` (out == records, halves_out == halves)."""
        return self._accumulate(False, None, cam, locals(), params, rgba8, ("records", "halves") if in_place else ())

    def accumulate_records_device(self, cam: rr_camera, records_ptr, halves_ptr, history_ptr, history_halves_ptr, history_length_ptr, motion_ptr, out_ptr,
                                  halves_out_ptr, length_out_ptr, rgba8_ptr=None, params=None, stream_ptr=None):
        """rr_accumulate_records_device: width * height 32-byte records in, as history and out (16-byte aligned; out_ptr may be records_ptr
        and halves_out_ptr halves_ptr), optionally twice as many half records each, width * height float32 of length in and out,
        width * height * 3 float32 of motion and width * height x 4 bytes, all raw device pointers (None where the call has none);
        enqueued on `stream_ptr`, not waited for."""
        self._accumulate_device(False, None, cam, locals(), params, stream_ptr)

    def accumulate_split(self, cam: rr_camera, records, halves, diffuse, diffuse_halves, history=None, history_halves=None, history_diffuse=None,
                         history_diffuse_halves=None, history_length=None, motion=None, params=None, rgba8: bool = False, in_place: bool = False) -> dict:
        """rr_accumulate_split_records: temporal.accumulate_split_records on the device, host arrays in and out.  The arguments of
        accumulate_records, and diffuse (n, 3) float32, diffuse_halves (n, 2, 3) or None (exactly when halves is), history_diffuse (n, 3) and
        history_diffuse_halves (n, 2, 3): the previous call's diffuse and diffuse_halves.  Returns dict(records (n, 8), length (n,), halves
        (n, 2, 8) or None, diffuse (n, 3), diffuse_halves (n, 2, 3) or None [, rgba (n, 4) uint8]); in_place accumulates into copies of the
        four current arrays (every output is its input)."""
        return self._accumulate(True, None, cam, locals(), params, rgba8, ("records", "halves", "diffuse", "diffuse_halves") if in_place else ())

    def accumulate_split_device(self, cam: rr_camera, records_ptr, halves_ptr, diffuse_ptr, diffuse_halves_ptr, history_ptr, history_halves_ptr, history_diffuse_ptr,
                                history_diffuse_halves_ptr, history_length_ptr, motion_ptr, out_ptr, halves_out_ptr, diffuse_out_ptr, diffuse_halves_out_ptr,
                                length_out_ptr, rgba8_ptr=None, params=None, stream_ptr=None):
        """rr_accumulate_split_records_device: the buffers of accumulate_records_device, plus width * height x 3 float32 of diffuse and
        twice as many of its halves, current, history and out (4-byte aligned; an output may be its current input), all raw device pointers
        (None where the call has none), in the order of the C arguments; enqueued on `stream_ptr`, not waited for."""
        self._accumulate_device(True, None, cam, locals(), params, stream_ptr)

    def accumulate_clamped(self, cam: rr_camera, records, halves=None, history=None, history_halves=None, history_length=None, motion=None, params=None,
                           clamp=None, rgba8: bool = False, halves_in_place: bool = False) -> dict:
        """rr_accumulate_clamped_records: temporal.accumulate_clamped_records on the device, host arrays in and out.  The arguments of
        accumulate_records, and clamp: a temporal.HistoryClampParams or None (the library's defaults).  Returns dict(records (n, 8), length
        (n,), halves (n, 2, 8) or None [, rgba (n, 4) uint8]); halves_in_place accumulates into a copy of `halves` (halves_out == halves;
        out can never be records)."""
        return self._accumulate(False, history_clamp_params(clamp), cam, locals(), params, rgba8, ("halves",) if halves_in_place else ())

    def accumulate_clamped_device(self, cam: rr_camera, records_ptr, halves_ptr, history_ptr, history_halves_ptr, history_length_ptr, motion_ptr, out_ptr,
                                  halves_out_ptr, length_out_ptr, rgba8_ptr=None, params=None, clamp=None, stream_ptr=None):
        """rr_accumulate_clamped_records_device: the buffers of accumulate_records_device (out_ptr may NOT be records_ptr; halves_out_ptr
        may be halves_ptr), all raw device pointers (None where the call has none); enqueued on `stream_ptr`, not waited for."""
        self._accumulate_device(False, history_clamp_params(clamp), cam, locals(), params, stream_ptr)

    def accumulate_clamped_split(self, cam: rr_camera, records, halves, diffuse, diffuse_halves, history=None, history_halves=None, history_diffuse=None,
                                 history_diffuse_halves=None, history_length=None, motion=None, params=None, clamp=None, rgba8: bool = False,
                                 halves_in_place: bool = False) -> dict:
        """rr_accumulate_clamped_split_records: temporal.accumulate_clamped_split_records on the device, host arrays in and out.  The
        arguments of accumulate_split, and clamp: a temporal.HistoryClampParams or None (the library's defaults).  Returns accumulate_split's
        dict; halves_in_place accumulates into copies of `halves` and `diffuse_halves` (out can never be records, diffuse_out never diffuse)."""
        return self._accumulate(True, history_clamp_params(clamp), cam, locals(), params, rgba8, ("halves", "diffuse_halves") if halves_in_place else ())

    def accumulate_clamped_split_device(self, cam: rr_camera, records_ptr, halves_ptr, diffuse_ptr, diffuse_halves_ptr, history_ptr, history_halves_ptr,
                                        history_diffuse_ptr, history_diffuse_halves_ptr, history_length_ptr, motion_ptr, out_ptr, halves_out_ptr, diffuse_out_ptr,
                                        diffuse_halves_out_ptr, length_out_ptr, rgba8_ptr=None, params=None, clamp=None, stream_ptr=None):
        """rr_accumulate_clamped_split_records_device: the buffers of accumulate_split_device (out_ptr may NOT be records_ptr and
        diffuse_out_ptr NOT diffuse_ptr; the two halves outputs may be their inputs), all raw device pointers (None where the call has none),
        in the order of the C arguments; enqueued on `stream_ptr`, not waited for."""
        self._accumulate_device(True, history_clamp_params(clamp), cam, locals(), params, stream_ptr)

    # -- the motion of moved items per pixel -------------------------------------------
    @staticmethod
    def _moved(item_index, prev_trans):
        """The host arrays of rr_motion_records: item indices (k,) uint32 and their previous transforms (k, 4, 4) in math layout ->
        (k, uint32 array or None, column-major float32 array or None)."""
        idx = np.ascontiguousarray(np.asarray(item_index if item_index is not None else [], np.int64).reshape(-1))
        if len(idx) and (idx.min() < 0 or idx.max() > 0xffffffff):
            raise ValueError("item indices must lie in 0 .. 2^32 - 1")
        idx = idx.astype(np.uint32)
        t = np.asarray(prev_trans if prev_trans is not None else np.zeros((0, 4, 4)), np.float32).reshape(-1, 4, 4)
        if len(t) != len(idx):
            raise ValueError(f"{len(idx)} moved items with {len(t)} previous transforms")
        t = np.ascontiguousarray(np.transpose(t, (0, 2, 1)))
        return len(idx), (idx if len(idx) else None), (t if len(idx) else None)

    def motion_records(self, cam: rr_camera, item_index, prev_trans, records, world: bool = False):
        """rr_motion_records: temporal.motion_records on the device, host arrays in and out.  item_index (k,) names the moved items,
        prev_trans (k, 4, 4) is each one's `trans` in the frame the history was rendered from (math layout); records (n, 8) float32 of the
        whole frame of `cam`.  Returns (motion (n, 3) float32, world (n, 3) float32 or None)."""
        n = int(cam.width) * int(cam.height)
        rec = np.ascontiguousarray(records, np.float32).reshape(n, 8)
        k, idx, t = self._moved(item_index, prev_trans)
        motion = np.zeros((n, 3), np.float32)
        wout = np.zeros((n, 3), np.float32) if world else None
        _check(lib().rr_motion_records(self._h, C.byref(cam), _data(idx), _data(t), C.c_uint32(k), _data(rec), _data(motion), _data(wout)))
        return motion, wout

    def motion_records_device(self, cam: rr_camera, item_index, prev_trans, records_ptr, motion_ptr, world_ptr=None, stream_ptr=None):
        """rr_motion_records_device: item_index and prev_trans as motion_records takes them (host arrays, read before the call returns);
        width * height 32-byte records in (16-byte aligned), width * height * 3 float32 of motion and optionally as many of world out,
        all raw device pointers; enqueued on `stream_ptr`, not waited for."""
        k, idx, t = self._moved(item_index, prev_trans)
        _check(lib().rr_motion_records_device(self._h, C.byref(cam), _data(idx), _data(t), C.c_uint32(k), _ptr(records_ptr), _ptr(motion_ptr), _ptr(world_ptr),
                                              _ptr(stream_ptr)))

    # -- the ray queries on device buffers, in stream order ---------------------------
    def surface_rays_device(self, origins_ptr, dirs_ptr, n: int, depth: int, out_ptr, stream_ptr=None):
        """rr_surface_rays_device: as trace_rays_device, with n 128-byte rr_surface_hit records (16-byte aligned)."""
        _check(lib().rr_surface_rays_device(self._h, C.c_void_p(origins_ptr), C.c_void_p(dirs_ptr), C.c_uint32(n), C.c_uint32(depth), C.c_void_p(out_ptr),
                                            _ptr(stream_ptr)))

    def trace_rays_device(self, origins_ptr, dirs_ptr, n: int, depth: int, out_ptr, stream_ptr=None):
        """rr_trace_rays_device: raw device pointers (ints) of n * 3 float32 origins and directions and of n 20-byte rr_ray_hit records;
        enqueued on `stream_ptr` (a hipStream_t as int, None = the default stream).  Synchronise before reading the records on the host."""
        _check(lib().rr_trace_rays_device(self._h, C.c_void_p(origins_ptr), C.c_void_p(dirs_ptr), C.c_uint32(n), C.c_uint32(depth), C.c_void_p(out_ptr),
                                          _ptr(stream_ptr)))

    def trace_shadow_rays_device(self, origins_ptr, dirs_ptr, max_distance_ptr, n: int, depth: int, out_ptr, stream_ptr=None):
        """rr_trace_shadow_rays_device: as trace_rays_device, with n float32 limits (None = no limit) and n 20-byte rr_shadow_hit records."""
        _check(lib().rr_trace_shadow_rays_device(self._h, C.c_void_p(origins_ptr), C.c_void_p(dirs_ptr), _ptr(max_distance_ptr),
                                                 C.c_uint32(n), C.c_uint32(depth), C.c_void_p(out_ptr), _ptr(stream_ptr)))

    def shade_rays_device(self, cfg: rr_config, origins_ptr, dirs_ptr, n_results: int, rays_per_result: int, stream_ids_ptr, out_ptr, stream_ptr=None, cancel=None):
        """rr_shade_rays_device: n_results * rays_per_result rays, n_results uint32 stream ids (None = the result's index) and n_results
        32-byte rr_radiance records (16-byte aligned), all raw device pointers; enqueued on `stream_ptr`."""
        _check(lib().rr_shade_rays_device(self._h, C.byref(cfg), C.c_void_p(origins_ptr), C.c_void_p(dirs_ptr), C.c_uint32(n_results), C.c_uint32(rays_per_result),
                                          _ptr(stream_ids_ptr), C.c_void_p(out_ptr),
                                          _ptr(stream_ptr), _flag(cancel)))

    def set_profiling(self, on: bool):
        self.set_tuning(kernel_timing=1 if on else 0)

    def set_compat(self, flags: int):
        """rr_scene_set_compat: behaviours of earlier reference binaries (1 = shadows attenuated by the occluder's alpha)."""
        _check(lib().rr_scene_set_compat(self._h, C.c_uint32(flags)))

    def overlap_stages(self) -> int:
        """rr_scene_overlap_stages: level-1 stages of the last frame whose shade and shadow launches ran on two streams (0 = serial)."""
        n = C.c_uint32(0)
        _check(lib().rr_scene_overlap_stages(self._h, C.byref(n)))
        return n.value

    def schedule_record(self, on: bool = True):
        """rr_test_schedule_record (rr_api_schedule_probe.h, a test entry point outside include/rustray_hip.h): empty the handle's schedule log and
        record what every frame call enqueues from now on (False: stop)."""
        _check(lib().rr_test_schedule_record(self._h, 1 if on else 0))

    def schedule_log(self) -> str:
        """rr_test_schedule_read: the log as text, one operation per line in host order (tests/launch_order.py parses and checks it)."""
        L = lib()
        need = C.c_uint64(0)
        _check(L.rr_test_schedule_read(self._h, None, 0, C.byref(need)))
        buf = C.create_string_buffer(need.value)
        _check(L.rr_test_schedule_read(self._h, buf, need.value, C.byref(need)))
        return buf.value.decode()

    def stats(self) -> dict:
        st = rr_frame_stats()
        _check(lib().rr_scene_last_stats(self._h, C.byref(st)))
        return {k: getattr(st, k) for k, _ in rr_frame_stats._fields_ if not k.startswith("_")}


def render_multi(device_scenes, cam: rr_camera, cfg: rr_config, sample_xy=None, aux: bool = True):
    """rr_render_multi: one frame over several DeviceScene handles (one per GPU) from this one process, into host arrays."""
    w, h = cam.width, cam.height
    rgba = np.zeros((h, w, 4), np.uint8)
    out = dict(rgba=rgba)
    fr = rr_frame(rgba.ctypes.data, None, None, None)
    if aux:
        out["normal"] = np.zeros((h, w, 3), np.float32)
        out["depth"] = np.zeros((h, w), np.float32)
        out["object_id"] = np.zeros((h, w), np.uint32)
        fr = rr_frame(rgba.ctypes.data, out["normal"].ctypes.data, out["depth"].ctypes.data, out["object_id"].ctypes.data)
    keep, p = _sxy(sample_xy)
    handles = (C.c_void_p * len(device_scenes))(*[ds._h for ds in device_scenes])
    _check(lib().rr_render_multi(handles, len(device_scenes), C.byref(cam), C.byref(cfg), p, C.byref(fr), None))
    return out


def deinterleave_device(width, height, tile_w, tile_h, n_ranks, elem_bytes, src_ptr, dst_ptr, device, stream_ptr=None):
    _check(lib().rr_deinterleave_device(width, height, tile_w, tile_h, n_ranks, elem_bytes, C.c_void_p(src_ptr),
                                        C.c_void_p(dst_ptr), device, _ptr(stream_ptr)))


def deinterleave_packed_device(width, height, tile_w, tile_h, n_ranks, packs_ptr, pack_stride, section_offset, elem_bytes, dst_ptrs, device, stream_ptr=None):
    """rr_deinterleave_packed_device: the gathered packs of all ranks -> the frame-order buffers, one launch.  section_offset / elem_bytes /
    dst_ptrs: 4 entries (rgba, normal, depth, object id); elem_bytes 0 = absent."""
    so = (C.c_uint64 * 4)(*[int(v) for v in section_offset])
    eb = (C.c_uint32 * 4)(*[int(v) for v in elem_bytes])
    dp = (C.c_void_p * 4)(*[C.c_void_p(int(v)) if v else None for v in dst_ptrs])
    _check(lib().rr_deinterleave_packed_device(width, height, tile_w, tile_h, n_ranks, C.c_void_p(packs_ptr), C.c_uint64(pack_stride), so, eb, dp,
                                               device, _ptr(stream_ptr)))


def post_process(rgba: np.ndarray, normal, object_id, cavity: bool, outline: bool, device: int = 0) -> np.ndarray:
    """run_post_processing (reference src/post_processing.rs:123-181) on the GPU, host arrays in and out."""
    h, w = rgba.shape[:2]
    src = np.ascontiguousarray(rgba, np.uint8)
    out = np.zeros_like(src)
    nrm = np.ascontiguousarray(normal, np.float32) if normal is not None else None
    ids = np.ascontiguousarray(object_id, np.uint32) if object_id is not None else None
    _check(lib().rr_post_process(w, h, int(cavity), int(outline), src.ctypes.data_as(C.c_void_p),
                                 nrm.ctypes.data_as(C.c_void_p) if nrm is not None else None,
                                 ids.ctypes.data_as(C.c_void_p) if ids is not None else None,
                                 out.ctypes.data_as(C.c_void_p), device))
    return out


def post_process_device(w, h, cavity, outline, rgba_ptr, normal_ptr, id_ptr, out_ptr, device=0, stream_ptr=None):
    _check(lib().rr_post_process_device(w, h, int(cavity), int(outline), C.c_void_p(rgba_ptr), _ptr(normal_ptr),
                                        _ptr(id_ptr), C.c_void_p(out_ptr), device,
                                        _ptr(stream_ptr)))


def math_probe(op: int, a, b=None, c=None, seed: int = 0, device: int = 0):
    a = np.ascontiguousarray(a, np.float32)
    n = len(a)
    b = np.ascontiguousarray(b, np.float32) if b is not None else None
    c = np.ascontiguousarray(c, np.float32) if c is not None else None
    outs = [np.zeros(n, np.float32) for _ in range(3)]
    _check(lib().rr_math_probe(op, a.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p) if b is not None else None,
                               c.ctypes.data_as(C.c_void_p) if c is not None else None, n,
                               *[o.ctypes.data_as(C.c_void_p) for o in outs], C.c_uint64(seed), device))
    return outs


def wave_sums_probe(entry: int, sum_pix, rgb, aux_pix, aux, depth_hi=None, device: int = 0):
    """rr_math_probe op 13: the wave merges of rr_accumulate.h on one workgroup of 256 lanes (four waves).  `entry`: 0 accum_merged,
    1 accum_aux_merged, 2 accum_hit_merged, 3 accum_depth_wide_merged.  `sum_pix`, `aux_pix`: (256,) uint32 slots below 128 or
    0xffffffff; `rgb`: (256, 3) int32; `aux`: (256, 4) int32 (nx, ny, nz, depth); `depth_hi`: (256,) the depth's high words for
    entry 3.  Returns the int64 sums {"rgb": (3, 128), "normal": (3, 128), "depth": (128,)}."""
    rgb = np.ascontiguousarray(rgb, np.int32).reshape(256, 3)
    aux = np.ascontiguousarray(aux, np.int32).reshape(256, 4)
    words = np.concatenate([np.ascontiguousarray(sum_pix, np.uint32).reshape(256), rgb.T.reshape(-1).view(np.uint32),
                            np.ascontiguousarray(aux_pix, np.uint32).reshape(256), aux.T.reshape(-1).view(np.uint32)])
    hi = np.zeros(9 * 256, np.uint32)
    if depth_hi is not None:
        hi[:256] = np.ascontiguousarray(depth_hi).astype(np.int64).astype(np.uint32).reshape(256)
    out0, _, _ = math_probe(13, words.view(np.float32), hi.view(np.float32), None, seed=int(entry), device=device)
    planes = out0.view(np.int64)[:7 * 128].reshape(7, 128)
    return {"rgb": planes[0:3].copy(), "normal": planes[3:6].copy(), "depth": planes[6].copy()}


def philox_probe(op: int, counters, key, device: int = 0):
    """rr_math_probe ops 12 (device) and 14 (host) of philox4x32_10: `counters` is (m, 4) uint32
    (pixel, sample, node, stream), `key` two uint32 words; returns the (m, 2) uint32 words jitter() uses."""
    ctr = np.ascontiguousarray(counters, np.uint32).reshape(-1, 4)
    m = len(ctr)
    a = np.concatenate([ctr[:, 0], ctr[:, 3]]).view(np.float32)
    b = np.concatenate([ctr[:, 1], np.zeros(m, np.uint32)]).view(np.float32)
    c = np.concatenate([ctr[:, 2], np.zeros(m, np.uint32)]).view(np.float32)
    seed = (int(key[0]) & 0xffffffff) | ((int(key[1]) & 0xffffffff) << 32)
    r0, r1, _ = math_probe(op, a, b, c, seed=seed, device=device)
    return np.stack([r0.view(np.uint32)[:m], r1.view(np.uint32)[:m]], axis=1)

