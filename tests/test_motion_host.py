"""rr_motion_records without a GPU: the host loop over rustray_amd/csrc/rr_motion.h (the functions the kernel applies per lane) against
the numpy yardstick temporal.motion_records, bit for bit; the yardstick against the float64 temporal.item_motion within a derived bound;
the call's table builder (once more under AddressSanitizer + UBSan, as a plain program); the Python glue; and what the entry points
refuse before they touch a device."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

from rustray_amd import capi
from rustray_amd.temporal import item_motion, motion_records, world_positions
from tests.denoise_cases import F, differing_words, same_bits
from tests.helpers import ROOT
from tests.motion_cases import ID_NOBODY, N_ITEMS, N_MOVED, motion_frame, motion_items, moved_list

SIZES = ((37, 19), (130, 70))
FLAGS = ["-std=c++17", "-O2", "-g", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off"]


def _build(tmp_path_factory, name, extra):
    exe = str(tmp_path_factory.mktemp(name) / "motion_test")
    subprocess.check_call(["g++"] + FLAGS + extra + ["-o", exe, os.path.join(ROOT, "tests", "native", "motion_test.cpp")])
    return exe


@pytest.fixture(scope="module")
def plain_exe(tmp_path_factory):
    return _build(tmp_path_factory, "motion", [])


@pytest.fixture(scope="module")
def sanitized_exe(tmp_path_factory):
    return _build(tmp_path_factory, "motion_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


def _colmajor(m):
    return np.ascontiguousarray(np.transpose(np.asarray(m, F).reshape(-1, 4, 4), (0, 2, 1)))


def run_program(exe, tmp_path, cam, ids, trans_inv, item_index, prev_trans, records):
    """-> (returncode, stdout, dict(table (n_moved, 28) uint32, motion (n, 3), world (n, 3)) or None)."""
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    c = cam.c_struct()
    W, H = int(c.width), int(c.height)
    item_index = np.asarray(item_index, np.uint32)
    with open(src, "wb") as fh:
        fh.write(struct.pack("<4I", W, H, len(ids), len(item_index)))
        fh.write(np.array(c.projection_inverse[:], F).tobytes() + np.array(c.view_inverse[:], F).tobytes())
        fh.write(np.asarray(ids, np.uint32).tobytes() + _colmajor(trans_inv).tobytes())
        fh.write(item_index.tobytes() + _colmajor(prev_trans).tobytes())
        fh.write(np.ascontiguousarray(records, F).tobytes())
    if os.path.exists(dst):
        os.remove(dst)
    out = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=600)
    if out.returncode != 0:
        return out.returncode, out.stdout + out.stderr, None
    assert "motion test OK" in out.stdout
    raw = np.fromfile(dst, np.uint32)
    n, k = W * H, len(item_index)
    assert raw.size == 28 * k + 6 * n
    return 0, out.stdout, dict(table=raw[:28 * k].reshape(k, 28), motion=raw[28 * k:28 * k + 3 * n].view(F).reshape(n, 3), world=raw[28 * k + 3 * n:].view(F).reshape(n, 3))


def yardstick(W, H, n_moved):
    it, case = motion_items(), motion_frame(W, H)
    idx, prev = moved_list(n_moved)
    return motion_records(case["records"], case["cam"], it["ids"][idx], prev, it["trans_inv"][idx])


def assert_same(got_motion, got_world, want, what):
    """Every word equal; in `world` a word that is a NaN on both sides counts as equal (a NaN the arithmetic generated has no specified
    sign or payload); the motion holds no NaN at all."""
    assert same_bits(np.ascontiguousarray(got_motion).view(np.uint32), want[0].view(np.uint32)), f"{what}: {int((np.ascontiguousarray(got_motion).view(np.uint32) != want[0].view(np.uint32)).sum())} words of motion differ"
    differ, nans = differing_words(got_world, want[1])
    assert differ == 0, f"{what}: {differ} words of world differ"
    return nans


# ---- the cases ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", SIZES)
def test_the_generated_case_has_what_it_promises(size):
    W, H = size
    it, case = motion_items(), motion_frame(W, H)
    rec, order = case["records"], it["order"]
    ids = rec[:, 7].view(np.uint32)
    listed = it["ids"][order[:70]]
    assert len(np.unique(it["ids"])) == N_ITEMS and it["ids"][order[0]] == 0xffffffff and it["ids"][order[1]] == 0
    valid = np.isfinite(rec[:, 3]) & np.isfinite(rec[:, 4:7]).all(-1)
    assert (np.isin(ids, listed) & valid).any() and (~np.isin(ids, it["ids"])).any() and (ids == ID_NOBODY).any()
    assert np.isin(ids[valid], it["ids"][order[70:]]).any()                      # items of the scene that are never listed
    assert ((ids == 0) & valid).any() and ((ids == 0) & np.isnan(rec[:, 4])).any() and ((ids == 0xffffffff) & valid).any()
    assert np.isnan(rec[5, 3]) and np.isinf(rec[6, 3]) and rec[7, 3] == F(3e38) and ids[7] == it["ids"][order[2]]
    rows, ok = ids.reshape(H, W), valid.reshape(H, W)
    # a wave of the kernel is rows 2j, 2j + 1 of 32 columns (32x8 tiles, 64 lanes): waves whose valid lanes carry ONE id ...
    waves = [(rows[y:y + 2, x:x + 32][ok[y:y + 2, x:x + 32]], y) for y in range(0, H, 2) for x in range(0, W, 32)]
    one_id = [(v, y) for v, y in waves if len(v) and len(np.unique(v)) == 1 and y % 8 == 0]
    assert len(one_id) >= (3 if W < 64 else 8) and sum(len(v) == 64 for v, _ in one_id) >= (1 if W < 64 else 4)    # (whole waves among them)
    uniform_ids = {int(v[0]) for v, _ in one_id}
    assert {0, 0xffffffff} <= uniform_ids and any(i in set(listed.tolist()) for i in uniform_ids)
    assert sum(len(np.unique(v)) > 1 for v, y in waves if y % 8 != 0) > 0.5 * sum(y % 8 != 0 for _, y in waves)      # most other waves mix ids
    # ... and waves whose ids alternate lane by lane
    both = ok[:, 0:W - 1:2] & ok[:, 1:W:2]
    assert all((rows[y, 0:W - 1:2] != rows[y, 1:W:2])[both[y]].mean() > 0.9 for y in range(H) if y % 8 in (2, 3))
    motion, world = yardstick(W, H, 70)
    assert (motion[valid & np.isin(ids, listed)] != 0).any(1).mean() > 0.95 and not motion[~valid].any() and not motion[~np.isin(ids, listed)].any()
    # pixel 7: the world point is finite, the point in the item's space is not, and rule 3's zero is taken
    assert np.isfinite(world[7]).all() and not motion[7].any()
    k = int(order[2])
    with np.errstate(all="ignore"):
        local = it["trans_inv"][k][:3, :3] @ world[7] + it["trans_inv"][k][:3, 3]
    assert not np.isfinite(local.astype(F)).all()
    assert np.isnan(world[5]).all() and not np.isfinite(world[6]).all()


# ---- the host loop against the yardstick --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("n_moved", N_MOVED)
def test_host_loop_equals_the_yardstick(plain_exe, tmp_path, size, n_moved):
    W, H = size
    it, case = motion_items(), motion_frame(W, H)
    idx, prev = moved_list(n_moved)
    rc, text, got = run_program(plain_exe, tmp_path, case["cam"], it["ids"], it["trans_inv"], idx, prev, case["records"])
    assert rc == 0, text
    want = yardstick(W, H, n_moved)
    assert_same(got["motion"], got["world"], want, f"{size} n_moved={n_moved}")
    assert (want[0] != 0).any() == (n_moved > 0)
    # the table: sorted by id as unsigned, rows 0 .. 2 of each listed item's trans_inv and prev_trans
    ids = got["table"][:, 0]
    assert (np.diff(ids.astype(np.int64)) > 0).all() and set(ids.tolist()) == set(it["ids"][idx].tolist())
    at = {int(it["ids"][i]): (i, k) for k, i in enumerate(idx)}
    for row in got["table"]:
        i, k = at[int(row[0])]
        assert not row[1:4].any()
        assert same_bits(row[4:16].view(F).reshape(3, 4), np.ascontiguousarray(it["trans_inv"][i][:3]))
        assert same_bits(row[16:28].view(F).reshape(3, 4), np.ascontiguousarray(prev[k][:3]))


def test_the_sanitized_program_runs_clean(sanitized_exe, tmp_path):
    """The same program under AddressSanitizer + UBSan: the largest list on the frame with partial tiles, and a refused list."""
    it, case = motion_items(), motion_frame(37, 19)
    idx, prev = moved_list(70)
    rc, text, got = run_program(sanitized_exe, tmp_path, case["cam"], it["ids"], it["trans_inv"], idx, prev, case["records"])
    assert rc == 0, text
    assert_same(got["motion"], got["world"], yardstick(37, 19, 70), "sanitized")
    rc, text, _ = run_program(sanitized_exe, tmp_path, case["cam"], it["ids"], it["trans_inv"], np.append(idx, idx[3]), np.concatenate([prev, prev[3:4]]), case["records"])
    assert rc == 3 and "entries 3 and 70" in text, text
    rc, text, got = run_program(sanitized_exe, tmp_path, case["cam"], it["ids"], it["trans_inv"], idx[:0], prev[:0], case["records"])
    assert rc == 0 and not got["motion"].any(), text


# ---- the table builder --------------------------------------------------------------------------------------------------------------
def test_the_table_builder_refuses(plain_exe, tmp_path):
    it, case = motion_items(), motion_frame(37, 19)
    idx, prev = moved_list(3)
    run = lambda ids, index, p: run_program(plain_exe, tmp_path, case["cam"], ids, it["trans_inv"], index, p, case["records"])
    # two listed items with one id: both entries are named
    ids = it["ids"].copy()
    ids[idx[2]] = ids[idx[0]]
    rc, text, _ = run(ids, idx, prev)
    assert rc == 3 and "refused:" in text and "entries 0 and 2" in text and "same object id 4294967295" in text, text
    # an unlisted item may share a listed id: the caller's contract, not a refusal
    ids = it["ids"].copy()
    ids[it["order"][50]] = ids[idx[0]]
    assert run(ids, idx, prev)[0] == 0
    # a prev_trans that is not finite, naming the entry
    for bad in (np.nan, np.inf, -np.inf):
        p = prev.copy()
        p[1, 2, 3] = bad
        rc, text, _ = run(it["ids"], idx, p)
        assert rc == 3 and "prev_trans of entry 1 is not finite" in text, text
    # an index out of range
    rc, text, _ = run(it["ids"], np.array([idx[0], N_ITEMS, idx[1]], np.uint32), prev)
    assert rc == 3 and f"item_index[1] = {N_ITEMS}" in text, text
    rc, text, _ = run(it["ids"], np.array([0xffffffff], np.uint32), prev[:1])
    assert rc == 3 and "item_index[0] = 4294967295" in text, text


# ---- the yardstick against float64 --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", SIZES)
def test_yardstick_against_float64(size):
    """motion_records (float32, in the header's order) against item_motion (float64, rounded once) on the same float32 inputs.  With
    u = 2^-24 the running error of the two chained 4-term rows is, per row r,
        e_local_r = 4u * sum_c |inv_rc| |w_c|                           (w = (world, 1): three additions and a product per term)
        e_prev_r  = 4u * sum_c |P_rc| |local_c| + sum_c |P_rc| e_local_c  (its own rounding, and what it inherits)
    and u * |m_r| more for the subtraction; times 1.01 for the second-order terms.  item_motion rounds its float64 result to float32
    once more: another u * |m_r|.  Where the float32 chain leaves the float range the yardstick writes 0 and float64 does not: those
    pixels are counted, not compared."""
    W, H = size
    it, case = motion_items(), motion_frame(W, H)
    idx, prev = moved_list(70)
    rec = case["records"]
    motion, world = yardstick(W, H, 70)
    ids_p = rec[:, 7].view(np.uint32)
    valid = np.isfinite(rec[:, 3]) & np.isfinite(rec[:, 4:7]).all(-1)
    inv = it["trans_inv"][idx]
    with np.errstate(all="ignore"):
        ref = item_motion(world, np.where(valid, ids_p, ID_NOBODY), it["ids"][idx], prev, inv)
    u = 2.0 ** -24
    checked = overflowed = 0
    for ident, P, B in zip(it["ids"][idx], prev.astype(np.float64), inv.astype(np.float64)):
        at = np.flatnonzero(valid & (ids_p == ident))
        if not len(at):
            continue
        w = np.concatenate([world[at].astype(np.float64), np.ones((len(at), 1))], axis=1)          # (k, 4)
        local = w @ B.T
        with np.errstate(over="ignore"):
            over = ~np.isfinite(local.astype(F)).all(-1) | ~np.isfinite(ref[at]).all(-1)
        e_local = 4 * u * (np.abs(w) @ np.abs(B).T)                                                   # (k, 4); row 3 unused
        local[:, 3] = 1.0
        e_prev = 4 * u * (np.abs(local) @ np.abs(P).T) + e_local[:, :3] @ np.abs(P[:, :3]).T
        m = (local @ P.T)[:, :3] - w[:, :3]
        bound = 1.01 * (e_prev[:, :3] + u * np.abs(m)) + u * np.abs(m)
        err = np.abs(motion[at].astype(np.float64) - ref[at].astype(np.float64))
        assert (motion[at][over] == 0).all()
        assert (err[~over] <= bound[~over]).all(), (int(ident), float((err[~over] / bound[~over]).max()))
        checked += int((~over).sum()); overflowed += int(over.sum())
    print(f"{size}: {checked} pixels within the bound, {overflowed} out of the float range")
    assert checked > 0.3 * valid.sum() and overflowed >= 1
    other = ~(valid & np.isin(ids_p, it["ids"][idx]))
    assert not motion[other].any() and not ref[other].any()


# ---- the Python glue ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", SIZES)
def test_world_is_world_positions(size):
    case = motion_frame(*size)
    for n_moved in (0, 3):
        _, world = yardstick(*size, n_moved)
        assert same_bits(world, world_positions(case["records"], case["cam"]))


def test_motion_records_refuses_a_repeated_id():
    it, case = motion_items(), motion_frame(37, 19)
    idx, prev = moved_list(3)
    with pytest.raises(ValueError):
        motion_records(case["records"], case["cam"], [5, 7, 5], prev, it["trans_inv"][idx])


def test_temporal_state_lists_exactly_the_items_that_changed():
    from rustray_amd.renderer import TemporalState
    it = motion_items()
    ids, t0 = it["ids"][:6], it["trans"][:6]
    state = TemporalState()
    assert state.track(ids, t0) is None                        # no history yet
    state.sets[0] = dict(records=None)
    state.current, state.frames = 0, 1                         # (what advance() leaves behind a frame)
    idx, prev = state.track(ids, t0)
    assert len(idx) == 0 and prev.shape == (0, 4, 4)           # nothing moved
    t1 = t0.copy()
    t1[4, 0, 3] = np.nextafter(t1[4, 0, 3], F(np.inf))         # one ulp in one float
    t1[1] = it["prev_trans"][1]
    t1[2, 3, 3] = F(-0.0) if t1[2, 3, 3] == 0 else -t1[2, 3, 3]    # bitwise: a sign is a change
    idx, prev = state.track(ids, t1)
    assert idx.dtype == np.uint32 and idx.tolist() == [1, 2, 4] and same_bits(prev, t0[[1, 2, 4]])
    idx, prev = state.track(ids, t0)                            # and back: the previous transforms are those of the call before
    assert idx.tolist() == [1, 2, 4] and same_bits(prev, t1[[1, 2, 4]])
    assert state.frames == 1 and state.current == 0
    # a changed id resets; so does a changed count
    other = ids.copy()
    other[3] += 1
    assert state.track(other, t0) is None and state.current is None and state.frames == 0
    state.current, state.frames = 0, 1
    assert state.track(other, t0)[0].tolist() == []
    assert state.track(other[:5], t0[:5]) is None and state.current is None
    state.reset()
    assert state.items is None
    # a history whose items nobody noted (a frame without tracking): the state starts anew, nothing is taken for static
    state.current, state.frames = 0, 3
    assert state.track(ids, t0) is None and state.current is None and state.frames == 0 and state.items is not None


# ---- what the entry points refuse before they touch a device -------------------------------------------------------------------------
def test_refusals_without_a_device():
    L = capi.lib()
    cam = motion_frame(37, 19)["cam"].c_struct()
    fake = C.c_void_p(0x1000)                                  # never dereferenced: every check here precedes the scene
    rec, mo = C.c_void_p(0x200000), C.c_void_p(0x400000)
    idx, prev = (C.c_uint32 * 1)(0), (C.c_float * 16)()
    dev = lambda *a: L.rr_motion_records_device(*a, None)
    for fn in (L.rr_motion_records, dev):
        assert fn(None, C.byref(cam), None, None, 0, rec, mo, None) == -1 and b"scene is NULL" in L.rr_last_error()
        assert fn(fake, None, None, None, 0, rec, mo, None) == -1 and b"camera is NULL" in L.rr_last_error()
        assert fn(fake, C.byref(cam), None, None, 0, None, mo, None) == -1 and b"records is NULL" in L.rr_last_error()
        assert fn(fake, C.byref(cam), None, None, 0, rec, None, None) == -1 and b"motion_out is NULL" in L.rr_last_error()
        assert fn(fake, C.byref(cam), None, prev, 1, rec, mo, None) == -1 and b"item_index is NULL" in L.rr_last_error()
        assert fn(fake, C.byref(cam), idx, None, 1, rec, mo, None) == -1 and b"prev_trans is NULL" in L.rr_last_error()
        for w, h in ((0, 19), (37, 0), (65536, 19), (37, 65536)):
            bad = type(cam).from_buffer_copy(cam)
            bad.width, bad.height = w, h
            assert fn(fake, C.byref(bad), None, None, 0, rec, mo, None) == -1 and b"bad frame size" in L.rr_last_error()
        big = type(cam).from_buffer_copy(cam)
        big.width, big.height = 65535, 65535
        assert fn(fake, C.byref(big), None, None, 0, rec, mo, None) == -2 and b"2^30" in L.rr_last_error()
        assert fn(fake, C.byref(cam), None, None, 0, rec, C.c_void_p(0x200000 + 32 * 37 * 19 - 4), None) == -1 and b"motion_out overlaps records" in L.rr_last_error()
        assert fn(fake, C.byref(cam), None, None, 0, rec, mo, C.c_void_p(0x400000 + 8)) == -1 and b"world_out overlaps motion_out" in L.rr_last_error()
    assert dev(fake, C.byref(cam), None, None, 0, C.c_void_p(0x200008), mo, None) == -1 and b"16-byte aligned" in L.rr_last_error()
    assert dev(fake, C.byref(cam), None, None, 0, rec, C.c_void_p(0x400002), None) == -1 and b"4-byte aligned" in L.rr_last_error()
    assert dev(fake, C.byref(cam), None, None, 0, rec, mo, C.c_void_p(0x600001)) == -1 and b"4-byte aligned" in L.rr_last_error()
