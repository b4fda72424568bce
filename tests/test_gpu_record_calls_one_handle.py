"""The record calls -- rr_denoise_records, rr_accumulate_records, rr_motion_records -- interleaved on ONE handle.  Their host forms share
one staging path and one pool of device buffers in the handle, argument k of whichever call in slot k; all six forms share one entry.
Here every call runs with and without its optional arguments, host forms between device forms of the other calls, at 37x19, then at
70x41 (every slot grows), then at 37x19 again (every slot is larger than the call needs, and holds another call's bytes): every
host-form result must be, bit for bit, what the device form gives on the same inputs and what the same call gives as the first call of
a fresh handle.  At the end one refused call per function -- an overlap for the device forms, a bad struct_size for the host forms of the
two calls that have one and a refused list for rr_motion_records, which has none -- each followed by a good call: a refusal leaves
the pool usable.
The frames are tests/denoise_cases.py's random_frame (NaN and inf colours, misses) with the ids of spheres_room's items."""
import functools

import numpy as np
import pytest

from rustray_amd.denoise import DenoiseParams
from rustray_amd.temporal import AccumulateParams, previous_view
from tests.denoise_cases import F, random_frame
from tests.helpers import camera_for, item_transforms, load_scene

pytestmark = pytest.mark.gpu

SIZES = ((37, 19), (70, 41), (37, 19))     # odd sizes: partial tiles both ways, several workgroups at the larger one
MOVED = (0, 2, 5)                          # the items rr_motion_records is told have moved


@functools.lru_cache(maxsize=None)
def _scene():
    return load_scene("spheres_room")


@functools.lru_cache(maxsize=None)
def _inputs(W, H):
    """Everything the three calls read at one size, made once and never written."""
    fs, n = _scene(), W * H
    ids = np.array([0] + [it.id for it in fs.items[:5]], np.uint32)        # random_frame's ids 1 .. 5 as ids of the scene; 0 stays a miss

    def of_scene(a):
        a = a.copy()
        a[..., 7] = ids[a[..., 7].view(np.uint32)].view(F)
        return a
    (records, halves, albedo), (history, history_halves, _) = random_frame(W, H), random_frame(W, H, seed=6)
    history, history_halves = history.copy(), history_halves.copy()        # other colours on the same surfaces: most of the history is taken
    history[:, 3:], history_halves[:, :, 3:] = records[:, 3:], halves[:, :, 3:]
    rng = np.random.default_rng(W * 1000 + H)
    cam = camera_for(fs, W, H)
    view = previous_view(cam)
    res = dict(cam=cam.c_struct(), records=of_scene(records), halves=of_scene(halves), albedo=albedo, history=of_scene(history),
               history_halves=of_scene(history_halves), history_length=rng.integers(0, 9, n).astype(F),
               motion=((rng.random((n, 3)) - 0.5) * 0.05).astype(F), prev_trans=item_transforms(fs, dx=0.3)[0][list(MOVED)],
               accumulate=AccumulateParams(prev_world_to_clip=view[0], prev_eye=view[1]), denoise=DenoiseParams(iterations=2))
    for v in res.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return res


def _on_device(call, inputs: dict, outputs: dict) -> dict:
    """call(pointers) on device copies of the host arrays `inputs` and on device buffers of the shapes and dtypes in `outputs` (None
    where the call has none) -> the outputs as host arrays."""
    import torch
    dev_in = {k: None if v is None else torch.from_numpy(np.array(v)).cuda() for k, v in inputs.items()}
    dev_out = {k: None if v is None else torch.zeros(v[0], dtype=v[1], device="cuda") for k, v in outputs.items()}
    torch.cuda.synchronize()
    call({k: None if v is None else v.data_ptr() for k, v in {**dev_in, **dev_out}.items()})
    torch.cuda.synchronize()
    return {k: None if v is None else v.cpu().numpy() for k, v in dev_out.items()}


# ---- the calls: name -> (host form, device form), each taking (handle, W, H) and returning a dict of host arrays
def _denoise(full: bool):
    def args(W, H):
        i = _inputs(W, H)
        return i, dict(records=i["records"], halves=i["halves"] if full else None, albedo=i["albedo"] if full else None)

    def host(ds, W, H):
        i, a = args(W, H)
        return ds.denoise_records(W, H, a["records"], a["halves"], a["albedo"], i["denoise"], rgba8=full, variance=full)

    def device(ds, W, H):
        import torch
        i, a = args(W, H)
        n = W * H
        got = _on_device(lambda p: ds.denoise_records_device(W, H, p["records"], p["halves"], p["albedo"], p["out"], p["rgba"], p["variance"], i["denoise"]), a,
                         dict(out=((n, 8), torch.float32), variance=((n,), torch.float32) if full else None, rgba=((n, 4), torch.uint8) if full else None))
        return {k: v for k, v in dict(records=got["out"], variance=got["variance"], rgba=got["rgba"]).items() if v is not None}
    return host, device


def _accumulate(full: bool):
    keys = ("records", "halves", "history", "history_halves", "history_length", "motion")

    def args(W, H):
        i = _inputs(W, H)
        return i, {k: i[k] if full or k == "records" else None for k in keys}

    def host(ds, W, H):
        i, a = args(W, H)
        return ds.accumulate_records(i["cam"], *(a[k] for k in keys), i["accumulate"], rgba8=full)

    def device(ds, W, H):
        import torch
        i, a = args(W, H)
        n = W * H
        got = _on_device(lambda p: ds.accumulate_records_device(i["cam"], *(p[k] for k in keys), p["out"], p["halves_out"], p["length"], p["rgba"], i["accumulate"]), a,
                         dict(out=((n, 8), torch.float32), halves_out=((n, 2, 8), torch.float32) if full else None, length=((n,), torch.float32),
                              rgba=((n, 4), torch.uint8) if full else None))
        res = dict(records=got["out"], length=got["length"], halves=got["halves_out"])
        return dict(res, rgba=got["rgba"]) if full else res
    return host, device


def _motion(world: bool):
    def host(ds, W, H):
        i = _inputs(W, H)
        motion, wout = ds.motion_records(i["cam"], MOVED, i["prev_trans"], i["records"], world=world)
        return dict(motion=motion, world=wout)

    def device(ds, W, H):
        import torch
        i = _inputs(W, H)
        n = W * H
        return _on_device(lambda p: ds.motion_records_device(i["cam"], MOVED, i["prev_trans"], p["records"], p["motion"], p["world"]), dict(records=i["records"]),
                          dict(motion=((n, 3), torch.float32), world=((n, 3), torch.float32) if world else None))
    return host, device


CALLS = {"denoise_full": _denoise(True), "accumulate_full": _accumulate(True), "motion_world": _motion(True),
         "denoise_bare": _denoise(False), "accumulate_first": _accumulate(False), "motion_plain": _motion(False)}


def _same(got: dict, want: dict, what: str):
    assert list(got) == list(want), what
    for k, w in want.items():
        g = got[k]
        assert (g is None) == (w is None), f"{what}.{k}"
        if w is not None:
            assert g.shape == w.shape and g.dtype == w.dtype, f"{what}.{k}"
            assert g.tobytes() == w.tobytes(), f"{what}.{k} differs in {int((g.view(np.uint8) != w.view(np.uint8)).sum())} bytes"


def test_interleaved_record_calls_on_one_handle(hip):
    fs = _scene()
    names = list(CALLS)
    want = {}
    for W, H in sorted(set(SIZES)):                # each host form as the first call of a handle of its own
        for name in names:
            with hip.DeviceScene(fs, 0) as fresh:
                want[name, W, H] = CALLS[name][0](fresh, W, H)
    # the inputs do something: the filter changes colours, a history is taken, the moved items cover pixels
    big = _inputs(70, 41)
    assert want["denoise_full", 70, 41]["records"].tobytes() != big["records"].tobytes() and want["denoise_full", 70, 41]["rgba"].any()
    assert (want["accumulate_full", 70, 41]["length"] > 1).any() and (want["accumulate_first", 70, 41]["length"] <= 1).all()   # (0: a non-finite colour)
    assert (want["motion_world", 70, 41]["motion"] != 0).any() and np.isfinite(want["motion_world", 70, 41]["world"]).any()
    with hip.DeviceScene(fs, 0) as ds:
        for W, H in SIZES:
            for k, name in enumerate(names):       # a host form, then the device form of the NEXT call, on the same handle
                other = names[(k + 1) % len(names)]
                host = CALLS[name][0](ds, W, H)
                device = CALLS[other][1](ds, W, H)
                _same(host, want[name, W, H], f"{name} {W}x{H}, host form against a fresh handle")
                _same(device, want[other, W, H], f"{other} {W}x{H}, device form against the host form")
        # ---- one refusal per function, each followed by a good call of the same form
        import torch
        W, H = SIZES[0]
        i, n = _inputs(W, H), W * H
        rec, hist = torch.from_numpy(np.array(i["records"])).cuda(), torch.from_numpy(np.array(i["history"])).cuda()
        out, length, motion = torch.zeros((n + 1, 8), device="cuda"), torch.zeros(n, device="cuda"), torch.zeros((2 * n, 3), device="cuda")
        torch.cuda.synchronize()
        with pytest.raises(hip.RustrayHipError, match="out overlaps records"):
            ds.denoise_records_device(W, H, rec.data_ptr(), None, None, rec.data_ptr() + 32, None, None, i["denoise"])
        _same(CALLS["denoise_bare"][1](ds, W, H), want["denoise_bare", W, H], "denoise, device form after a refusal")
        with pytest.raises(hip.RustrayHipError, match="length_out overlaps history_length"):
            ds.accumulate_records_device(i["cam"], rec.data_ptr(), None, hist.data_ptr(), None, length.data_ptr(), None, out.data_ptr(), None, length.data_ptr(), None,
                                         i["accumulate"])
        _same(CALLS["accumulate_first"][1](ds, W, H), want["accumulate_first", W, H], "accumulate, device form after a refusal")
        with pytest.raises(hip.RustrayHipError, match="world_out overlaps motion_out"):
            ds.motion_records_device(i["cam"], MOVED, i["prev_trans"], rec.data_ptr(), motion.data_ptr(), motion.data_ptr() + 12)
        _same(CALLS["motion_world"][1](ds, W, H), want["motion_world", W, H], "motion, device form after a refusal")
        bad_d, bad_a = hip.denoise_params(i["denoise"]), hip.accumulate_params(i["accumulate"])
        bad_d.struct_size, bad_a.struct_size = bad_d.struct_size - 4, bad_a.struct_size + 4
        with pytest.raises(hip.RustrayHipError, match="struct_size"):
            ds.denoise_records(W, H, i["records"], i["halves"], i["albedo"], bad_d)
        _same(CALLS["denoise_full"][0](ds, W, H), want["denoise_full", W, H], "denoise, host form after a refusal")
        with pytest.raises(hip.RustrayHipError, match="struct_size"):
            ds.accumulate_records(i["cam"], i["records"], params=bad_a)
        _same(CALLS["accumulate_full"][0](ds, W, H), want["accumulate_full", W, H], "accumulate, host form after a refusal")
        with pytest.raises(hip.RustrayHipError, match="entries 0 and 2"):          # (under the lock, before anything is staged)
            ds.motion_records(i["cam"], (MOVED[0], MOVED[1], MOVED[0]), i["prev_trans"], i["records"])
        _same(CALLS["motion_plain"][0](ds, W, H), want["motion_plain", W, H], "motion, host form after a refusal")
        torch.cuda.synchronize()
        assert not out.any() and not length.any() and not motion.any(), "a refused call wrote an output"
