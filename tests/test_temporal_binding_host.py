"""The ctypes binding against include/rustray_hip.h, without a GPU.

1: every function the header declares has a signature in the binding, with the header's number of parameters.
2: the eight DeviceScene.accumulate* methods hand their buffers to the C function in the order of the header's parameter names.  A swap
of two void* among nineteen positional arguments is invisible to the compiler and to ctypes, so the library is replaced by a fake that
records what it is called with: the device forms get a distinct integer per pointer, the host forms arrays whose memory is looked for."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from rustray_amd import capi
from rustray_amd.flat import rr_camera
from tests.helpers import ROOT, arglist_after, n_params
from tests.test_abi import declared_functions

W, H = 3, 2
N = W * H
HANDLE = 0x5c3e0
# the host arrays of the calls, by the header's parameter name, with their documented shapes
SHAPES = dict(records=(N, 8), halves=(N, 2, 8), diffuse=(N, 3), diffuse_halves=(N, 2, 3), history=(N, 8), history_halves=(N, 2, 8), history_diffuse=(N, 3),
              history_diffuse_halves=(N, 2, 3), history_length=(N,), motion=(N, 3))
# the header's output parameter -> the key of the result dict, and the input an in-place call writes it over
RESULT = dict(out="records", halves_out="halves", diffuse_out="diffuse", diffuse_halves_out="diffuse_halves", length_out="length", rgba8_out="rgba")
PARTNER = dict(out="records", halves_out="halves", diffuse_out="diffuse", diffuse_halves_out="diffuse_halves")
# method, C function, split, clamped, the keyword of its in-place form and the inputs that keyword covers
HOST = (("accumulate_records", "rr_accumulate_records", False, False, "in_place", ("records", "halves")),
        ("accumulate_split", "rr_accumulate_split_records", True, False, "in_place", ("records", "halves", "diffuse", "diffuse_halves")),
        ("accumulate_clamped", "rr_accumulate_clamped_records", False, True, "halves_in_place", ("halves",)),
        ("accumulate_clamped_split", "rr_accumulate_clamped_split_records", True, True, "halves_in_place", ("halves", "diffuse_halves")))
DEVICE = (("accumulate_records_device", "rr_accumulate_records_device", False), ("accumulate_split_device", "rr_accumulate_split_records_device", False),
          ("accumulate_clamped_device", "rr_accumulate_clamped_records_device", True),
          ("accumulate_clamped_split_device", "rr_accumulate_clamped_split_records_device", True))


def _header() -> str:
    with open(os.path.join(ROOT, "include", "rustray_hip.h")) as fh:
        return re.sub(r"/\*.*?\*/", "", fh.read(), flags=re.S)


def _arglist(hdr: str, name: str) -> str:
    return arglist_after(hdr, re.search(r"\b" + name + r"\s*\(", hdr).end())


def _param_names(hdr: str, name: str) -> list:
    """The header's parameter names of `name`, in order (none of these functions takes a callback)."""
    return [re.findall(r"[A-Za-z_]\w*", p)[-1] for p in _arglist(hdr, name).split(",")]


# ---- 1: signatures against the header -----------------------------------------------------------------------------------------------
def test_every_declared_function_has_a_signature_of_the_headers_length():
    hdr = _header()
    L = capi.lib()
    names = declared_functions()
    assert len(names) >= 70
    for name in names:
        want = n_params(_arglist(hdr, name))
        got = getattr(L, name).argtypes
        assert got is not None, f"{name} is declared in the header and the binding sets no signature for it"
        assert len(got) == want, f"{name}: header has {want} parameters, the binding's argtypes {len(got)}"


# ---- 2: the argument order of the eight accumulate methods --------------------------------------------------------------------------
class _Recorder:
    """Stands in for the loaded library: every attribute is a function that stores its arguments and returns 0."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append((name, args))
            return 0
        return fn


@pytest.fixture
def recorder(monkeypatch):
    rec = _Recorder()
    monkeypatch.setattr(capi, "_LIB", rec)
    return rec


@pytest.fixture
def scene(recorder):
    """A DeviceScene around a handle that is never dereferenced (and, set back to NULL while the fake is still in place, never destroyed)."""
    ds = object.__new__(capi.DeviceScene)
    ds._h = C.c_void_p(HANDLE)
    yield ds
    ds._h = C.c_void_p(None)


def _structs():
    cam = rr_camera()
    cam.width, cam.height = W, H
    prm, clamp = capi.rr_accumulate_params(), capi.rr_history_clamp_params()
    prm.struct_size, clamp.struct_size = C.sizeof(prm), C.sizeof(clamp)
    return cam, prm, clamp


def _address(v):
    """A recorded pointer argument as an integer; NULL is 0."""
    if v is None:
        return 0
    return int((v.value if isinstance(v, C.c_void_p) else v) or 0)


def _one_call(recorder, fn_name, names):
    assert len(recorder.calls) == 1 and recorder.calls[0][0] == fn_name, [c[0] for c in recorder.calls]
    args = recorder.calls.pop()[1]
    assert len(args) == len(names), f"{fn_name}: {len(args)} arguments for the header's {len(names)}"
    return dict(zip(names, args))


def _check_head(got, cam, prm, clamp, clamped, what):
    """scene, camera, params and, for the clamped pair, clamp: the handle and the caller's own structs, each in its place"""
    assert _address(got["scene"]) == HANDLE, what
    assert got["camera"]._obj is cam and got["params"]._obj is prm, what
    if clamped:
        assert got["clamp"]._obj is clamp, what
    else:
        assert "clamp" not in got, what


@pytest.mark.parametrize("method,fn_name,clamped", DEVICE)
def test_device_forms_pass_every_pointer_in_the_headers_order(recorder, scene, method, fn_name, clamped):
    names = _param_names(_header(), fn_name)
    assert names[:3] == ["scene", "camera", "params"] and names[-1] == "hip_stream" and (names[3] == "clamp") == clamped
    fn = getattr(capi.DeviceScene, method)
    pointers = [p for p in inspect.signature(fn).parameters if p.endswith("_ptr")]
    header_name = lambda p: dict(rgba8_ptr="rgba8_out_dev", stream_ptr="hip_stream").get(p, p[:-4] + "_dev")
    assert sorted(header_name(p) for p in pointers) == sorted(names[4 if clamped else 3:])
    cam, prm, clamp = _structs()
    values = {p: 0x1000 * (k + 1) for k, p in enumerate(pointers)}
    optional = [p for p in pointers if p not in ("records_ptr", "out_ptr", "length_out_ptr")]
    for absent in [None] + optional:
        kw = dict(values, params=prm, **(dict(clamp=clamp) if clamped else {}))
        if absent:
            kw[absent] = None
        fn(scene, cam, **kw)
        got = _one_call(recorder, fn_name, names)
        _check_head(got, cam, prm, clamp, clamped, fn_name)
        for p in pointers:
            assert _address(got[header_name(p)]) == (kw[p] or 0), f"{fn_name}: {header_name(p)} with {absent} absent"


def _arrays(split, without=()):
    rng = np.random.default_rng(5)
    keys = [k for k in SHAPES if split or "diffuse" not in k]
    return {k: None if k in without else rng.random(SHAPES[k], np.float32) for k in keys}


@pytest.mark.parametrize("method,fn_name,split,clamped,in_place_kw,in_place_rows", HOST)
def test_host_forms_pass_the_callers_arrays_and_the_results_in_the_headers_order(recorder, scene, method, fn_name, split, clamped, in_place_kw, in_place_rows):
    names = _param_names(_header(), fn_name)
    outs = [k for k in RESULT if split or "diffuse" not in k]
    assert names == ["scene", "camera", "params"] + (["clamp"] if clamped else []) + [k for k in SHAPES if split or "diffuse" not in k] + outs
    fn = getattr(capi.DeviceScene, method)
    cam, prm, clamp = _structs()
    extra = dict(clamp=clamp) if clamped else {}
    absent_sets = ((), ("halves", "diffuse_halves", "history_halves", "history_diffuse_halves"), ("motion",),
                   ("history", "history_halves", "history_diffuse", "history_diffuse_halves", "history_length"))
    for without in absent_sets:
        for rgba8 in (False, True):
            a = _arrays(split, without)
            res = fn(scene, cam, params=prm, rgba8=rgba8, **a, **extra)
            got = _one_call(recorder, fn_name, names)
            what = f"{fn_name} without {without} rgba8={rgba8}"
            _check_head(got, cam, prm, clamp, clamped, what)
            for k, v in a.items():       # the caller's own memory, no copy; NULL where the caller has none
                assert _address(got[k]) == (v.ctypes.data if v is not None else 0), f"{what}: {k}"
            assert list(res) == ["records", "length", "halves"] + (["diffuse", "diffuse_halves"] if split else []) + (["rgba"] if rgba8 else []), what
            for o in outs:               # the memory of the array returned under the matching key; NULL where there is none
                r = res.get(RESULT[o])
                present = (PARTNER[o] not in without) if o in PARTNER else (o == "length_out" or rgba8)
                assert (r is not None) == present, f"{what}: {o}"
                assert _address(got[o]) == (r.ctypes.data if present else 0), f"{what}: {o}"
                if present:
                    dtype, shape = (np.uint8, (N, 4)) if o == "rgba8_out" else (np.float32, SHAPES.get(PARTNER.get(o), (N,)))
                    assert r.dtype == dtype and r.shape == shape and r.flags.c_contiguous, f"{what}: {o}"
                    assert all(_address(got[o]) != _address(got[k]) for k in a), f"{what}: {o} is an input"
    # in place: the named outputs are their inputs, and both are private copies of the caller's arrays
    for without in ((), ("halves", "diffuse_halves", "history_halves", "history_diffuse_halves")):
        a = _arrays(split, without)
        before = {k: v.copy() for k, v in a.items() if v is not None}
        res = fn(scene, cam, params=prm, **a, **extra, **{in_place_kw: True})
        got = _one_call(recorder, fn_name, names)
        for o, k in PARTNER.items():
            if k not in a or a[k] is None:
                continue
            if k in in_place_rows:
                assert _address(got[o]) == _address(got[k]) == res[RESULT[o]].ctypes.data != a[k].ctypes.data, f"{fn_name} {in_place_kw}: {o}"
                assert np.array_equal(res[RESULT[o]], before[k]), f"{fn_name} {in_place_kw}: {o} is no copy of {k}"
            else:
                assert _address(got[k]) == a[k].ctypes.data and _address(got[o]) == res[RESULT[o]].ctypes.data != a[k].ctypes.data, f"{fn_name} {in_place_kw}: {o}"
        for k, v in a.items():
            if v is not None and k not in in_place_rows:
                assert _address(got[k]) == v.ctypes.data, f"{fn_name} {in_place_kw}: {k}"
            if v is not None:
                assert np.array_equal(v, before[k]), f"{fn_name} {in_place_kw}: the caller's {k} was written"
