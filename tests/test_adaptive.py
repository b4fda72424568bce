"""rustray_amd/adaptive.py: the half-buffer error estimate and the refinement list, on hand-made arrays (pure numpy, no GPU)."""
import numpy as np
import pytest

from rustray_amd import adaptive


def test_half_error():
    parts = np.array([
        [[0.25, 0.5, 0.0], [0.75, 0.5, 0.0]],        # one channel differs by 0.5
        [[0.0, 0.0, 0.0], [0.0, 0.0, 0.0]],          # no noise
        [[3.0, 0.0, 0.0], [1.5, 0.0, 0.0]],          # both halves above 1: the frame shows 1 and 1
        [[2.0, 0.25, 0.0], [0.5, 0.0, 0.0]],         # min(2, 1) - 0.5 = 0.5 beats 0.25
        [[np.nan, 0.0, 0.0], [0.5, 0.9, 0.0]],       # a non-finite channel: more samples cannot cure it
        [[0.0, np.inf, 0.0], [0.0, 0.0, 1.0]],
        [[0.0, 0.0, 0.0], [0.0, 0.0, -np.inf]],
        [[-0.5, 0.0, 0.0], [0.5, 0.0, 0.0]],         # nothing clamps from below
    ], np.float32)
    err = adaptive.half_error(parts)
    assert err.dtype == np.float32 and err.shape == (8,)
    assert err.tolist() == [0.25, 0.0, 0.0, 0.25, 0.0, 0.0, 0.0, 0.5]
    assert adaptive.half_error(np.zeros((0, 2, 3), np.float32)).shape == (0,)
    with pytest.raises(ValueError):
        adaptive.half_error(np.zeros((4, 4, 3), np.float32))   # the estimate is for two halves


def test_refine_list_order_padding_and_count():
    w, h = 20, 12
    err = np.zeros((h, w), np.float32)
    picked = [(0, 0), (7, 7), (8, 0), (19, 3), (3, 8), (4, 8), (3, 9), (16, 11), (9, 1), (1, 9)]
    for x, y in picked:
        err[y, x] = 0.5
    err[5, 5] = 0.25        # at the threshold: not above it
    err[6, 6] = np.nan      # no estimate: not refined
    xy, count = adaptive.refine_list(err.reshape(-1), 0.25, w, h)
    assert count == len(picked) and xy.dtype == np.uint32 and len(xy) == 64
    # 8x8 blocks row-major (3 x 2 of them, the last column 4 wide, the last row 4 high), row-major inside a block
    expect = [(0, 0), (7, 7), (8, 0), (9, 1), (19, 3), (3, 8), (4, 8), (1, 9), (3, 9), (16, 11)]
    assert [(int(v) & 0xffff, int(v) >> 16) for v in xy[:count]] == expect
    assert (xy[count:] == xy[count - 1]).all()                  # padded with the last entry
    assert adaptive.refine_list(err, 0.25, w, h)[0].tolist() == xy.tolist()   # (height, width) is taken as well
    # exactly 64 and 65 entries: no pad, then a pad to 128
    full = np.zeros((h, w), np.float32); full[:8, :8] = 1.0
    xy64, c64 = adaptive.refine_list(full, 0.5, w, h)
    assert c64 == 64 and len(xy64) == 64 and xy64.tolist() == [x | (y << 16) for y in range(8) for x in range(8)]
    full[0, 8] = 1.0
    xy65, c65 = adaptive.refine_list(full, 0.5, w, h)
    assert c65 == 65 and len(xy65) == 128 and int(xy65[64]) == 8 and (xy65[64:] == 8).all()
    # nothing above the threshold: an empty list
    none, c0 = adaptive.refine_list(full, 2.0, w, h)
    assert c0 == 0 and len(none) == 0 and none.dtype == np.uint32
