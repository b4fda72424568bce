"""The one harness of tests/test_gpu_temporal.py, _split.py, _clamp.py and _clamp_split.py: a device call of any of the four temporal
calls with every buffer watched, and the word comparison against the yardstick.  The pointers are handed over by keyword, so the
harness does not depend on the order of the binding's parameters."""
import numpy as np

from rustray_amd.temporal import HistoryClampParams
from tests.denoise_cases import differing_words
from tests.test_gpu_pixel_parts import SENTINEL

# variant -> (the DeviceScene method, the call has the diffuse buffers, the call takes a clamp)
VARIANTS = dict(plain=("accumulate_records_device", False, False), split=("accumulate_split_device", True, False),
                clamped=("accumulate_clamped_device", False, True), clamped_split=("accumulate_clamped_split_device", True, True))
# output -> (32-bit words per pixel, the input it may be written over in place, its key in the result)
OUTPUTS = dict(out=(8, "records", "records"), halves_out=(16, "halves", "halves"), diffuse_out=(3, "diffuse", "diffuse"),
               diffuse_halves_out=(6, "diffuse_halves", "diffuse_halves"), length_out=(1, None, "length"), rgba8=(1, None, "rgba"))
SHAPES = dict(records=(8,), halves=(2, 8), diffuse=(3,), diffuse_halves=(2, 3), length=())
DIFFUSE_INPUTS = ("diffuse", "diffuse_halves", "history_diffuse", "history_diffuse_halves")


def device_call(ds, variant, cam, prm, arrays, clamp=None, in_place=(), rgba8=False, stream=None, produce=False):
    """One device call of `variant` (a key of VARIANTS) on the host arrays `arrays` (by the name of the C argument, None where the call
    has none; the diffuse arrays may be there for a call that does not take them: it is then made on the colour buffers alone) ->
    dict(records, halves, length [, diffuse, diffuse_halves] [, rgba]) as numpy words.  clamp: (radius, sigma_scale) of the clamped
    calls; in_place: the inputs whose output is the same memory (where the input is there); produce: the inputs are made by copy kernels
    on `stream` and the call follows them without a synchronisation.
    Asserted for every call: the eight words behind each of the six outputs keep their sentinel; an output the call does not have -- the
    halves' without halves, the bytes without rgba8, the diffuse ones of a call that is not split -- is untouched throughout; every
    input holds afterwards the bits it held before, except those given in place."""
    import torch
    method, split, clamped = VARIANTS[variant]
    n = int(cam.width) * int(cam.height)
    use_halves = arrays["halves"] is not None
    ctx = torch.cuda.stream(stream) if stream is not None else torch.cuda.device(0)
    with ctx:
        src = {k: torch.from_numpy(np.ascontiguousarray(v).copy()).cuda() if v is not None else None for k, v in arrays.items()}
        torch.cuda.synchronize()
        if produce:
            src = {k: t.clone() if t is not None else None for k, t in src.items()}      # (copy kernels on `stream`; the call is enqueued behind them)
        words = {o: w * n for o, (w, _, _) in OUTPUTS.items()}
        out = {o: torch.full((w + 8,), SENTINEL, dtype=torch.int32, device="cuda") for o, w in words.items()}
        ptr = {k: (t.data_ptr() if t is not None else None) for k, t in src.items()}
        written_over = [k for k in in_place if src[k] is not None]
        for o, (_, k, _) in OUTPUTS.items():
            if k in written_over:
                out[o][:words[o]] = src[k].view(torch.int32).reshape(-1)
                ptr[k] = out[o].data_ptr()
        if not produce:
            torch.cuda.synchronize()
        absent = {o for o, (_, k, _) in OUTPUTS.items() if (k in ("halves", "diffuse_halves") and not use_halves) or (o == "rgba8" and not rgba8)
                  or (k in DIFFUSE_INPUTS and not split)}
        kw = {k + "_ptr": p for k, p in ptr.items() if split or k not in DIFFUSE_INPUTS}
        kw.update({o + "_ptr": None if o in absent else out[o].data_ptr() for o in OUTPUTS if split or OUTPUTS[o][1] not in DIFFUSE_INPUTS})
        if clamped:
            kw["clamp"] = HistoryClampParams(*clamp)
        getattr(ds, method)(cam, params=prm, stream_ptr=stream.cuda_stream if stream is not None else None, **kw)
    torch.cuda.synchronize()
    got = {o: t.cpu().numpy().view(np.uint32) for o, t in out.items()}
    for o, w in words.items():
        assert (got[o][w:] == SENTINEL).all(), f"words behind {o} were written"
        if o in absent:
            assert (got[o] == SENTINEL).all(), f"{o} is absent and was written"
    for k, v in arrays.items():          # the inputs are what they were
        if v is not None and k not in written_over:
            assert np.array_equal(src[k].cpu().numpy().view(np.uint32), np.ascontiguousarray(v).view(np.uint32)), k
    res = {}
    for o, (_, _, key) in OUTPUTS.items():
        if key == "rgba":
            if rgba8:
                res[key] = got[o][:n].view(np.uint8).reshape(n, 4)
        elif split or key not in DIFFUSE_INPUTS:
            res[key] = None if o in absent else got[o][:words[o]].reshape((n,) + SHAPES[key])
    return res


def check_words(got, want, what, diffuse=True):
    """Every word equal.  In records, halves and length a word that is a NaN on both sides counts as equal whatever its other bits (a NaN
    the arithmetic generated has no specified sign or payload); the diffuse words, where `want` has them and diffuse is True, are
    compared bitwise: the header rules out a generated NaN there."""
    for key in ("records", "halves", "length"):
        if want[key] is None:
            assert got[key] is None, what
            continue
        differ, nans = differing_words(got[key], want[key])
        if nans:
            print(f"{what}: {nans} words of {key} are NaNs of other bits on both sides")
        assert differ == 0, f"{what}: {differ} of {np.asarray(want[key]).size} words of {key} differ"
    for key in ("diffuse", "diffuse_halves") if diffuse and "diffuse" in want else ():
        if want[key] is None:
            assert got[key] is None, what
            continue
        g, w = np.ascontiguousarray(got[key]).view(np.uint32), np.ascontiguousarray(want[key]).view(np.uint32)
        assert g.shape == w.shape and np.array_equal(g, w), f"{what}: {int((g != w).sum())} of {w.size} words of {key} differ"
