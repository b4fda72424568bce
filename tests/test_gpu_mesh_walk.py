"""The per-mesh tree walks (rustray_amd/csrc/rr_walk.h: blas_closest, blas_any, blas_closest_packet on the trees of rr_bvh.cpp)
against the oracle's brute-force form, bit for bit, on the rays of tests/aimed_rays.py: aimed at shared vertices and edges (several
triangles, in several leaves, report ONE toi: the lowest face must win whatever order the leaves are visited in), a few
float32 spacings off them, in mesh planes and node-box planes, axis-parallel with either sign of zero, and grazing near edges (D12's
envelope).  The box test of the walks is a filter that must never remove a triangle the exact test accepts; tests/test_aimed_rays.py
shows on the CPU that the oracle's own padded tree loses none of these rays, so a difference here is the device's filter.

Every case runs on the bare scene (fewer than 17 items: the per-ray walks) and padded with invisible decoys to 40 items (the packet
form of the top level: blas_closest_packet), in two lane orders: sorted by direction octant and target triangle (coherent waves,
wave-uniform leaves, packets) and one seeded permutation (vector loads, parked leaves, lanes of one wave in different meshes)."""
import functools

import numpy as np
import pytest

from tests import aimed_rays as ar
from tests.packet_pad import in_packet_range, pad_inert
from tests.shadow_ray_cases import describe, mismatches
from tests.test_gpu_packet_walk import _assert_hits_equal, packet_groups

pytestmark = pytest.mark.gpu
CASES = [(m, i) for m in ar.MESHES for i in ar.INSTANCES]
N_PADDED = 40
SHADOW_FAMILIES = ("V", "E", "U")


@functools.lru_cache(maxsize=None)
def _case(oracle, mesh_name, inst_name, families=ar.FAMILIES):
    """(scene, rays, the oracle's brute-force closest hits of the rays in generation order): once per case, shared, left unchanged."""
    fs = ar.scene(mesh_name, inst_name)
    R = ar.all_rays(mesh_name, inst_name, families)
    ref = oracle.trace_rays(fs.c_struct(), R.o, R.d, 1, brute_force=True)
    return fs, R, ref


def _scenes(fs):
    padded = pad_inert(fs, N_PADDED, "scattered")     # decoys never change what a ray hits (tests/test_packet_pad.py)
    assert len(fs.items) < 17 and not in_packet_range(len(fs.items)) and in_packet_range(len(padded.items))
    return (("bare", fs), (f"padded to {N_PADDED}", padded))


def _per_ray(n, order, got):
    """The records of a run in lane order `order` (an index array, repeats allowed) as arrays per ray."""
    out = []
    for a in got:
        x = np.zeros(n, a.dtype)
        x[order] = a
        out.append(x)
    return tuple(out)


@pytest.mark.parametrize("mesh_name,inst_name", CASES)
def test_closest_hit_walks_equal_brute_force(hip, oracle, mesh_name, inst_name):
    """found, item, face and the bits of toi of rr_trace_rays equal the oracle's brute-force form for every family, on the bare and on
    the padded scene, in both lane orders; and the two lane orders agree ray by ray."""
    fs, R, ref = _case(oracle, mesh_name, inst_name)
    orders = (("sorted", R.sorted_order()), ("permuted", R.permuted_order()))
    family = np.asarray([l.split(":")[0] for l in R.label])
    for where, scene in _scenes(fs):
        if scene is not fs:
            s = orders[0][1]
            share = packet_groups(R.o[s], R.d[s]).mean()
            assert share >= 0.5, (mesh_name, inst_name, share)     # otherwise this run does not test blas_closest_packet
        runs = {}
        with hip.DeviceScene(scene, 0) as ds:
            for name, order in orders:
                g = ds.trace_rays(R.o[order], R.d[order], 1)
                for f in ar.FAMILIES:
                    m = family[order] == f
                    if m.any():
                        _assert_hits_equal(tuple(a[m] for a in g), tuple(a[order][m] for a in ref), f"{mesh_name} {inst_name} {where} {name} {f}")
                runs[name] = _per_ray(len(R), order, g)
        _assert_hits_equal(runs["sorted"], runs["permuted"], f"{mesh_name} {inst_name} {where}: sorted vs permuted")
    assert ref[0][R.label == "V:diag"].all() and not ref[0][R.must_miss].any()


def _limits(toi, found, k):
    """Limit class k of 5 around the closest toi t: t, the float below, the float above, +inf, 0 (t = 1 where nothing is hit)."""
    t = np.where(found & np.isfinite(toi), toi, np.float32(1.0)).astype(np.float32)
    return (t, np.nextafter(t, np.float32(0.0)), np.nextafter(t, np.float32(np.inf)), np.full_like(t, np.inf), np.zeros_like(t))[k]


@pytest.mark.parametrize("mesh_name,inst_name", CASES)
def test_shadow_walk_at_the_limit(hip, oracle, mesh_name, inst_name):
    """rr_trace_shadow_rays on V, E and U with a limit per ray out of {toi, the float below, the float above, +inf, 0}, toi the
    oracle's closest toi: occluded = found and not toi > limit, judged as tools/fuzz_rays.py --shadow does against the oracle's shadow
    trace in its brute-force form, and an occluded ray's item, face and toi are the oracle's.  V and E take every limit, U rays one
    each in turn.  `t <= limit` holds AT the limit (RR_LEAF_ANY), also where several triangles tie there, and blas_any goes on pruning
    with the limit once any hit is known."""
    fs, R, closest = _case(oracle, mesh_name, inst_name, SHADOW_FAMILIES)
    f, it, fc, t = oracle.trace_rays(fs.c_struct(), R.o, R.d, 1, for_shadow=True, brute_force=True)
    all_five = np.flatnonzero(R.label != "U")
    idx = np.concatenate([np.tile(all_five, 5), np.flatnonzero(R.label == "U")])
    cls = np.concatenate([np.repeat(np.arange(5), len(all_five)), np.arange((R.label == "U").sum()) % 5])
    lim = np.zeros(len(idx), np.float32)
    for k in range(5):
        lim[cls == k] = _limits(closest[3], closest[0], k)[idx[cls == k]]
    rays = dict(origin=R.o[idx], dir=R.d[idx], depth=np.ones(len(idx), np.uint32), found=f[idx], item=it[idx], face=fc[idx], toi=t[idx])
    at_limit = rays["found"] & (rays["toi"] == lim)
    assert at_limit.sum() >= len(idx) // 10                      # the equality case is there, in numbers
    assert len(idx) <= 20000
    rng = np.random.default_rng(3)
    T = ar.Rays(); T.o, T.d, T.label, T.item, T.face = rays["origin"], rays["dir"], R.label[idx], R.item[idx], R.face[idx]
    for where, scene in _scenes(fs):
        with hip.DeviceScene(scene, 0) as ds:
            for name, order in (("sorted", T.sorted_order()), ("permuted", rng.permutation(len(idx)))):
                sub = {k: v[order] for k, v in rays.items()}
                got = ds.trace_shadow_rays(sub["origin"], sub["dir"], lim[order], 1)
                bad = mismatches(got, sub, lim[order])
                assert len(bad) == 0, describe(f"{mesh_name} {inst_name} {where} {name}", sub, lim[order], bad, got)
