"""philox4x32_10 (rr_math.h) on 64-bit products, as the kernels evaluate it (rr_math_probe op 12), against the HOST build of the same
function (op 14) and the oracle's generator, which tests/test_oracle_kat.py pins to the Random123 vectors.  Bit for bit."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KAT = [  # Random123 kat_vectors, philox4x32_10: counter, key, output
    ([0, 0, 0, 0], [0, 0], [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]),
    ([0xffffffff] * 4, [0xffffffff] * 2, [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]),
    ([0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344], [0xa4093822, 0x299f31d0], [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1]),
]
DEVICE_OPS = (12,)


def _oracle_words(oracle, counters, key):
    out = np.zeros((len(counters), 2), np.uint32)
    k, o = np.asarray(key, np.uint32), np.zeros(4, np.uint32)
    for i, c in enumerate(np.ascontiguousarray(counters, np.uint32)):
        oracle.lib().rro_philox(c.ctypes.data_as(C.c_void_p), k.ctypes.data_as(C.c_void_p), o.ctypes.data_as(C.c_void_p))
        out[i] = o[:2]
    return out


def test_known_answer_vectors(hip):
    for ctr, key, want in KAT:
        host = hip.philox_probe(14, [ctr], key)
        assert host[0].tolist() == want[:2]
        for op in DEVICE_OPS:
            assert hip.philox_probe(op, [ctr], key)[0].tolist() == want[:2], op


def test_random_keys_and_edges(hip, oracle):
    rng = np.random.default_rng(22)
    random_ctr = rng.integers(0, 2 ** 32, (4096, 4), dtype=np.uint64).astype(np.uint32)
    edges = np.asarray([(p, s, n, st) for p in (0, 0xffffffff) for s in (0, 63, 127) for n in (1, 2 ** 31) for st in (0, 1, 2, 3)], np.uint32)
    # a wave of one pixel, node and stream, as a level-1 packet is keyed: 128 samples
    packet = np.asarray([(1280 * 360 + 640, s, 1, 2) for s in range(128)], np.uint32)
    ctr = np.concatenate([random_ctr, edges, packet])
    seeds = [(0, 0), (0xffffffff, 0xffffffff), (0, 0xffffffff), (0x67890, 0x12345)] + [tuple(int(v) for v in rng.integers(0, 2 ** 32, 2)) for _ in range(2)]
    for key in seeds:
        host = hip.philox_probe(14, ctr, key)
        # the host build against the oracle's generator on the edges and a sample of the random keys (one call per key)
        sub = np.concatenate([np.arange(0, 4096, 64), np.arange(4096, 4096 + len(edges))])
        assert np.array_equal(host[sub], _oracle_words(oracle, ctr[sub], key)), key
        for op in DEVICE_OPS:
            assert np.array_equal(hip.philox_probe(op, ctr, key), host), (op, key)


def test_jitter_on_the_new_products(hip, oracle):
    """op 5 (jitter) on the inputs of tests/test_gpu_math.py::test_jitter_bit_exact, every entry checked."""
    rng = np.random.default_rng(6)
    n = 5000
    d = rng.standard_normal((n, 3)).astype(np.float32)
    seed = 0x1234567890
    gx, gy, gz = hip.math_probe(5, d[:, 0].copy(), d[:, 1].copy(), d[:, 2].copy(), seed=seed)
    out = np.zeros(3, np.float32)
    for i in range(n):
        oracle.lib().rro_jitter(d[i].copy().ctypes.data_as(C.c_void_p), C.c_float(0.05), C.c_uint64(seed), i, i & 7, 1 + i % 5, i % 3, out.ctypes.data_as(C.c_void_p))
        assert (out[0], out[1], out[2]) == (gx[i], gy[i], gz[i]), i
