"""The wave merges of rr_accumulate.h, called as the kernels call them (rr_math_probe op 13, run with -m gpu on an MI355X).

One workgroup of 256 lanes = four waves, each wave a case of its own: lane l adds (r, g, b) to its colour pixel and (nx, ny, nz, depth) to
its aux pixel, a pixel being a slot of a zeroed 128-slot DAccum or 0xffffffff for "nothing to add".  accum_merged, accum_aux_merged,
accum_hit_merged and accum_depth_wide_merged must leave in the planes exactly the int64 sums per slot that numpy forms -- whichever path
a wave takes: the plain wave sum of a one-pixel wave, the segmented scan of every other wave, 32-bit or 64-bit values.  Integer adds
commute, so there is no tolerance."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NONE = 0xffffffff
LO, HI = -(1 << 25), (1 << 25) - 1          # the ends of fits25i: 64 terms of either stay inside an int
GARBAGE = np.array([0x7fffffff, -(1 << 31), 0x12345678, -7], np.int64)


def _wave(pix, rgb=None, aux=None, aux_pix=None, rng=None, garbage=True):
    """One wave: `pix` (64,) colour pixels (aux pixels too unless given); values random below 2^25 unless given.  Lanes without a
    pixel hold garbage that must not count."""
    rng = rng or np.random.default_rng(1)
    pix = np.asarray(pix, np.int64).astype(np.uint32)
    aux_pix = pix.copy() if aux_pix is None else np.asarray(aux_pix, np.int64).astype(np.uint32)
    rgb = rng.integers(LO, HI + 1, (64, 3)) if rgb is None else np.broadcast_to(np.asarray(rgb, np.int64), (64, 3)).copy()
    aux = rng.integers(LO, HI + 1, (64, 4)) if aux is None else np.broadcast_to(np.asarray(aux, np.int64), (64, 4)).copy()
    if garbage:
        rgb[pix == NONE] = GARBAGE[:3]
        aux[aux_pix == NONE] = GARBAGE
    return dict(sum_pix=pix, aux_pix=aux_pix, rgb=rgb.astype(np.int32), aux=aux.astype(np.int32))


def _launch(waves):
    assert len(waves) == 4
    return {k: np.concatenate([w[k] for w in waves]) for k in ("sum_pix", "aux_pix", "rgb", "aux")}


def _expected(entry, L, depth64=None):
    rgb, normal, depth = np.zeros((3, 128), np.int64), np.zeros((3, 128), np.int64), np.zeros(128, np.int64)
    s, a = L["sum_pix"] != NONE, L["aux_pix"] != NONE
    if entry in (0, 2):
        for c in range(3):
            np.add.at(rgb[c], L["sum_pix"][s], L["rgb"][s, c].astype(np.int64))
    if entry in (1, 2):
        for c in range(3):
            np.add.at(normal[c], L["aux_pix"][a], L["aux"][a, c].astype(np.int64))
        np.add.at(depth, L["aux_pix"][a], L["aux"][a, 3].astype(np.int64))
    if entry == 3:
        np.add.at(depth, L["aux_pix"][a], depth64[a])
    return dict(rgb=rgb, normal=normal, depth=depth)


def _check(hip, entry, L, what, depth64=None):
    aux, hi = L["aux"], None
    if depth64 is not None:
        aux = L["aux"].copy()
        aux[:, 3] = (depth64 & 0xffffffff).astype(np.uint32).view(np.int32)
        hi = depth64 >> 32
    got = hip.wave_sums_probe(entry, L["sum_pix"], L["rgb"], L["aux_pix"], aux, depth_hi=hi)
    want = _expected(entry, L, depth64)
    for k in ("rgb", "normal", "depth"):
        bad = np.argwhere(got[k] != want[k])
        assert bad.size == 0, f"{what}, entry {entry}, {k}: first difference at {bad[0]}: {got[k][tuple(bad[0])]} != {want[k][tuple(bad[0])]}"
    return got


def _holes(rng, p, keep=0.5):
    pix = np.full(64, p, np.int64)
    pix[rng.random(64) > keep] = NONE
    return pix


def _split(at, p, q):
    return np.where(np.arange(64) < at, p, q)


def _single(lane, p):
    pix = np.full(64, NONE, np.int64)
    pix[lane] = p
    return pix


def _named_launches():
    rng = np.random.default_rng(24)
    none = np.full(64, NONE, np.int64)
    wide = rng.integers(LO, HI + 1, (64, 3))
    wide[41, 1] = 1 << 25                                  # one lane one step past the 32-bit bound: the 64-bit path
    wide_aux = rng.integers(LO, HI + 1, (64, 4))
    wide_aux[5, 3] = -(1 << 25) - 1
    return {
        "one pixel, holes, single lane, no lane": _launch([
            _wave(np.full(64, 3), rng=rng), _wave(_holes(rng, 40), rng=rng), _wave(_single(37, 70), rng=rng), _wave(none, rng=rng)]),
        "single lanes at the wave's ends and a row's": _launch([
            _wave(_single(0, 9), rng=rng), _wave(_single(63, 9), rng=rng), _wave(_single(15, 100), rng=rng), _wave(_single(16, 127), rng=rng)]),
        "two pixels split at 16 and at 20, 64 pixels, zeros": _launch([
            _wave(_split(16, 1, 2), rng=rng), _wave(_split(20, 34, 35), rng=rng), _wave((np.arange(64) + 50) % 128, rng=rng),
            _wave(np.full(64, 120), rgb=0, aux=0)]),
        "the ends of the 32-bit bound and one step past": _launch([
            _wave(np.full(64, 0), rgb=LO, aux=LO), _wave(np.full(64, 127), rgb=HI, aux=HI),
            _wave(np.full(64, 64), rgb=wide, aux=wide_aux), _wave(_holes(rng, 65, 0.8), rgb=wide, aux=wide_aux)]),
        "colour lanes and aux lanes that differ": _launch([
            _wave(_holes(rng, 7, 0.4), aux_pix=np.full(64, 7), rng=rng),            # some hits add no colour of their own
            _wave(np.full(64, 8), aux_pix=np.full(64, 9), rng=rng),                # two pixels between the two sets: the fallback
            _wave(none, aux_pix=_holes(rng, 10), rng=rng), _wave(_holes(rng, 11), aux_pix=none, rng=rng)]),
        "one pixel beside another pixel with holes between": _launch([
            _wave(np.where(np.arange(64) % 3 == 0, NONE, _split(32, 20, 21)), rng=rng), _wave(_split(63, 22, 23), rng=rng),
            _wave(_split(1, 24, 25), rng=rng), _wave(np.where(np.arange(64) == 30, 27, 26), rng=rng)]),
    }


NAMED = _named_launches()


@pytest.mark.parametrize("entry", [0, 1, 2])
@pytest.mark.parametrize("name", list(NAMED))
def test_merges_leave_the_sums_per_pixel(hip, name, entry):
    got = _check(hip, entry, NAMED[name], name)
    if name.startswith("the ends") and entry in (0, 2):
        # 64 terms of -2^25 and of 2^25 - 1: the totals at the ends of an int, widened once (rr_accumulate.h, fits25)
        assert got["rgb"][0, 0] == -(1 << 31) and got["rgb"][2, 127] == (1 << 31) - 64
    if name.startswith("two pixels") and entry != 1:
        assert not got["rgb"][:, 120].any()    # zeros add nothing


@pytest.mark.parametrize("seed", range(6))
def test_random_pixel_patterns_and_values(hip, seed):
    """Runs of random length over a few slots, holes, values up to the bound and now and then beyond it."""
    rng = np.random.default_rng(1000 + seed)
    waves = []
    for w in range(4):
        kind = rng.integers(0, 4)
        if kind == 0:
            pix = np.full(64, rng.integers(0, 128))
        elif kind == 1:
            pix = _holes(rng, rng.integers(0, 128), rng.random())
        else:
            pix = np.repeat(rng.integers(0, 128, 64), rng.integers(1, 24, 64))[:64]
            if kind == 3:
                pix = np.where(rng.random(64) < 0.2, NONE, pix)
        aux_pix = pix if rng.random() < 0.5 else np.where(rng.random(64) < 0.3, NONE, pix)
        wv = _wave(pix, aux_pix=aux_pix, rng=rng)
        if rng.random() < 0.3:                     # a few terms beyond 2^25 in magnitude
            k = rng.integers(0, 64, 3)
            wv["rgb"][k, rng.integers(0, 3, 3)] = rng.integers(-(1 << 31), 1 << 31, 3).astype(np.int64).astype(np.int32)
            wv["aux"][k, rng.integers(0, 4, 3)] = rng.integers(-(1 << 31), 1 << 31, 3).astype(np.int64).astype(np.int32)
        waves.append(wv)
    L = _launch(waves)
    for entry in (0, 1, 2):
        _check(hip, entry, L, f"seed {seed}")


def test_wide_depth_terms_in_64_bits(hip):
    """accum_depth_wide_merged: depth terms of 2^25 .. 1e9 * 2^16 (and their negatives), one pixel per wave, with holes, two pixels, one lane."""
    rng = np.random.default_rng(7)
    none = np.full(64, NONE, np.int64)
    L = _launch([_wave(none, aux_pix=np.full(64, 5), rng=rng), _wave(none, aux_pix=_holes(rng, 6), rng=rng),
                 _wave(none, aux_pix=_split(20, 7, 8), rng=rng), _wave(none, aux_pix=_single(63, 9), rng=rng)])
    depth64 = rng.integers(1 << 25, 65536 * 10 ** 9, 256)
    depth64[::5] *= -1
    depth64[3] = 65536 * 10 ** 9                  # the clamp of the kernels' to_fix call
    depth64[L["aux_pix"] == NONE] = -1            # garbage in both words
    got = _check(hip, 3, L, "wide depth", depth64)
    assert abs(int(got["depth"][5])) > 1 << 32 and not got["rgb"].any() and not got["normal"].any()
    L0 = _launch([_wave(none, rng=rng)] * 4)     # no lane anywhere
    _check(hip, 3, L0, "wide depth, no lane", np.full(256, -1, np.int64))
