"""rr_surface_rays without a GPU: the 128-byte record as a C99 host, the ctypes struct and the numpy dtype see it, and the argument
errors that are decided before any device is touched (tests/native/surface_c99.c)."""
import ctypes as C
import os
import subprocess

import numpy as np

from rustray_amd import capi
from rustray_amd.flat import SURFACE_HIT_DTYPE, rr_surface_hit
from tests.helpers import ROOT

# the issue's layout: eight 16-byte rows
WANT = [("hit", 0, 4), ("item_index", 4, 4), ("object_id", 8, 4), ("face_id", 12, 4),
        ("position", 16, 12), ("distance", 28, 4),
        ("normal", 32, 12), ("material", 44, 4),
        ("shading_normal", 48, 12), ("has_uv", 60, 4),
        ("base_color", 64, 16),
        ("ambient_color", 80, 12), ("alpha", 92, 4),
        ("specular_color", 96, 12), ("reflectivity", 108, 4),
        ("uv", 112, 8), ("roughness", 120, 4), ("ambient_occlusion", 124, 4)]


def _run_c99(tmp_path):
    exe = str(tmp_path / "surface_c99")
    libdir = os.path.dirname(capi.LIB_PATH)
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "native", "surface_c99.c"),
                           "-L" + libdir, "-lrustray_hip", "-Wl,-rpath," + libdir])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "surface c99 OK" in out.stdout, out.stdout + out.stderr
    return out.stdout.splitlines()


def test_layout_in_c_ctypes_and_numpy(tmp_path):
    lines = _run_c99(tmp_path)
    assert lines[0] == "sizeof 128"
    got = [(a, int(b), int(c)) for a, b, c in (l.split() for l in lines[1:1 + len(WANT)])]
    assert got == WANT
    assert C.sizeof(rr_surface_hit) == 128 and SURFACE_HIT_DTYPE.itemsize == 128
    assert [(n, getattr(rr_surface_hit, n).offset, getattr(rr_surface_hit, n).size) for n, _ in rr_surface_hit._fields_] == WANT
    assert [(n, SURFACE_HIT_DTYPE.fields[n][1], SURFACE_HIT_DTYPE.fields[n][0].itemsize) for n in SURFACE_HIT_DTYPE.names] == WANT
    kinds = {n: SURFACE_HIT_DTYPE.fields[n][0].base for n in SURFACE_HIT_DTYPE.names}
    assert all(kinds[n] == np.uint32 for n in ("hit", "item_index", "object_id", "face_id", "has_uv")) and kinds["material"] == np.int32
    assert all(k == np.float32 for n, k in kinds.items() if n not in ("hit", "item_index", "object_id", "face_id", "has_uv", "material"))


def test_argument_errors_that_need_no_device():
    """NULL scene, depth 0 and 256, NULL buffers with n > 0, the size bound, n == 0 -- through the binding, with the codes and messages of
    rr_trace_rays (the C program of the layout test makes the same calls from C)."""
    L = capi.lib()
    assert "rr_surface_rays" in capi.EXPORTS and "rr_surface_rays_device" in capi.EXPORTS
    o = np.zeros((1, 3), np.float32); d = np.zeros((1, 3), np.float32); out = np.full(1, 0x5a, np.uint8).repeat(128)
    po, pd, pout = (C.c_void_p(a.ctypes.data) for a in (o, d, out))
    fake = C.c_void_p(out.ctypes.data)   # never dereferenced: every call below is refused by its arguments alone
    for call in (lambda *a: L.rr_surface_rays(*a), lambda *a: L.rr_surface_rays_device(*a, None)):
        assert call(None, po, pd, 1, 1, pout) == -1 and b"NULL" in L.rr_last_error()
        for depth in (0, 256):
            assert call(fake, po, pd, 1, depth, pout) == -1 and b"depth" in L.rr_last_error()
        for args in ((None, pd, pout), (po, None, pout), (po, pd, None)):
            assert call(fake, args[0], args[1], 1, 1, args[2]) == -1 and b"NULL" in L.rr_last_error()
        assert call(fake, po, pd, 0x7fffff01, 1, pout) == -2
        assert call(fake, None, None, 0, 1, None) == 0
    assert L.rr_surface_rays(fake, po, pd, 1, 0, pout) == L.rr_trace_rays(fake, po, pd, 1, 0, pout) == -1
    assert (out == 0x5a).all()
