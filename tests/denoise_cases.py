"""Hand-made frames of rr_radiance records for the denoiser's tests (tests/test_denoise_host.py, tests/test_gpu_denoise.py): the inputs
only, made once per size and never changed by a test."""
import functools

import numpy as np

F = np.float32


def pack(color, depth, normal, ids):
    """(n, 8) float32 records of (n, 3) colours, (n,) depths, (n, 3) normals and (n,) uint32 ids."""
    n = len(depth)
    rec = np.zeros((n, 8), F)
    rec[:, 0:3], rec[:, 3], rec[:, 4:7] = color, depth, normal
    rec[:, 7] = np.asarray(ids, np.uint32).view(F)
    return rec


@functools.lru_cache(maxsize=None)
def quality_frame():
    """The 64x48 frame of the quality check: two ids split by a diagonal, a normal per id, a sloped depth, a colour ramp; the halves are
    the truth plus Gaussian noise of sigma 0.1 (default_rng(1)), the records their mean.  -> (truth (n, 3), records, halves)."""
    W, H = 64, 48
    y, x = np.mgrid[0:H, 0:W]
    x, y = x.reshape(-1), y.reshape(-1)
    right = (x * H > y * W)
    ids = np.where(right, 7, 3).astype(np.uint32)
    normal = np.where(right[:, None], np.array([0.0, 0.6, 0.8], F), np.array([0.0, 0.0, 1.0], F)).astype(F)
    depth = (F(4) + F(0.02) * x.astype(F) + F(0.01) * y.astype(F) + np.where(right, F(1.5), F(0))).astype(F)
    ramp = (F(0.1) + F(0.8) * x.astype(F) / F(W - 1)).astype(F)
    truth = np.stack([ramp, (ramp * F(0.5) + F(0.2)).astype(F), np.where(right, F(0.7), F(0.3)).astype(F)], axis=1).astype(F)
    rng = np.random.default_rng(1)
    halves = np.zeros((W * H, 2, 8), F)
    for h in range(2):
        halves[:, h] = pack((truth + rng.normal(0.0, 0.1, truth.shape)).astype(F), depth, normal, ids)
    color = ((halves[:, 0, 0:3] + halves[:, 1, 0:3]) * F(0.5)).astype(F)
    records = pack(color, depth, normal, ids)
    for a in (truth, records, halves):
        a.setflags(write=False)
    return truth, records, halves


@functools.lru_cache(maxsize=None)
def random_frame(W: int, H: int, seed: int = 5, bad: bool = True):
    """A W x H frame of 5 ids in irregular patches, unit normals, depths 1 .. 9, colours in [0, 2^10] (most below 2), halves around them,
    and an albedo with zeros, tiny values and ones.  With `bad`: some NaN / inf colours, some non-finite halves, some all-miss pixels
    (NaN normals, id 0, depth 0).  -> (records (n, 8), halves (n, 2, 8), albedo (n, 3))."""
    rng = np.random.default_rng(seed)
    n = W * H
    bad = bad and n >= 64           # (a tiny frame has no room for them)
    y, x = np.mgrid[0:H, 0:W]
    x, y = x.reshape(-1), y.reshape(-1)
    ids = (1 + ((x // 5 + 2 * (y // 4) + (x * y) // 23) % 5)).astype(np.uint32)
    nrm = rng.normal(size=(5, 3))
    nrm = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(F)
    normal = (nrm[ids - 1] + rng.normal(0, 0.05, (n, 3))).astype(F)
    normal = (normal / np.linalg.norm(normal, axis=1, keepdims=True).astype(F)).astype(F)
    depth = (F(1) + ids.astype(F) * F(1.5) + rng.random(n).astype(F) * F(0.5)).astype(F)
    base = rng.random((n, 3)).astype(F) * F(2)
    base[rng.random(n) < 0.02] *= F(400)          # a few bright pixels, still below 2^10
    noise = (rng.random((n, 3)).astype(F) - F(0.5)) * F(0.4)
    a = np.clip(base + noise, 0, 1023).astype(F)
    b = np.clip(base - noise, 0, 1023).astype(F)
    color = ((a + b) * F(0.5)).astype(F)
    albedo = (F(0.05) + rng.random((n, 3)).astype(F)).astype(F)
    albedo[rng.random(n) < 0.1] = 0
    albedo[rng.random(n) < 0.05, 1] = F(2.0 ** -10)       # not above the limit: left as it is
    albedo[rng.random(n) < 0.05, 2] = F(2.0 ** -9)
    if bad:
        k = rng.permutation(n)
        color[k[0:3], 0] = np.nan
        color[k[3:5], 2] = np.inf
        color[k[5], 1] = -np.inf
        a[k[6:9], 1] = np.nan                       # a non-finite half under a finite record: no variance seed there
        b[k[9], 0] = np.inf
        miss = k[10:10 + max(3, n // 20)]
        ids[miss], depth[miss], normal[miss] = 0, 0, np.nan
        albedo[k[30 % n], 0] = np.nan
    records = pack(color, depth, normal, ids)
    halves = np.zeros((n, 2, 8), F)
    halves[:, 0], halves[:, 1] = pack(a, depth, normal, ids), pack(b, depth, normal, ids)
    for arr in (records, halves, albedo):
        arr.setflags(write=False)
    return records, halves, albedo


def same_bits(a, b) -> bool:
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()
