"""The temporal reprojection on the device against float64 geometry with the camera moving: tests/test_reprojection_host.py's checks
applied to what the kernels write.  The frames are the device's own (rr_render_pixels at 1 sample, monte_carlo off) of spheres_room from
the camera pairs of tests/reprojection_truth.py, at 64x48 and at 37x29 (partial workgroups, LDS tile seams in the clamped kernels).

1: per pair and size the four calls with halves on the ramp inputs -- every output word the yardstick's, and position, completeness and
behind / outside asserted on the device's outputs directly; one case through the four _device forms on a non-null stream.  2: a moved
sphere and wall under the strafing camera, rr_motion_records_device -> rr_accumulate_records_device on one stream.  3: the pipelines
Raytracing.render_temporal, render_temporal_split and render_temporal_split_clamped over two frames with the camera changed in between:
frame 2 is the explicit call with previous_view(A), bit for bit, and not the one with previous_view(B).

One sample per pixel and no depth of field, as on the host: with more samples the mean depth is not the centre ray's."""
import numpy as np
import pytest

from rustray_amd import temporal
from rustray_amd.flat import make_config
from rustray_amd.temporal import AccumulateParams, HistoryClampParams, previous_view
from tests import reprojection_truth as rt
from tests.denoise_cases import differing_words
from tests.helpers import load_scene
from tests.test_reprojection_host import CASES, IDS, KEYS, SPLIT_KEYS, conditions, make_case, make_motion_case, moved_conditions

pytestmark = pytest.mark.gpu

F = np.float32
LAYERS = ("records", "halves", "diffuse", "diffuse_halves", "length")
_cases = {}


@pytest.fixture(scope="module")
def scene(hip):
    with hip.DeviceScene(load_scene("spheres_room"), 0) as ds:
        yield ds


def _frames(ds):
    """frames(fs, camera) of make_case: the device's one-sample frame as records."""
    from rustray_amd.renderer import _pack_records
    return lambda fs, camera: _pack_records(ds.render_pixels(camera.c_struct(), rt.frame_config()))


def _case(ds, pair, size):
    if (pair, size) not in _cases:
        _cases[pair, size] = make_case(None, pair, size, frames=_frames(ds))
    return _cases[pair, size]


def _same_words(got, want, what):
    """Every word of every layer the yardstick has.  The ramp inputs hold no NaN colour and the arithmetic makes none: plain bit equality."""
    for key in LAYERS:
        if want.get(key) is None:
            continue
        g, w = np.ascontiguousarray(got[key]).view(np.uint32).reshape(-1), np.ascontiguousarray(want[key]).view(np.uint32).reshape(-1)
        assert np.array_equal(g, w), f"{what}: {int((g != w).sum())} of {w.size} words of {key} differ"


def _calls(ds, c, device_forms=False):
    """(name, the device's outputs, the yardstick's, the inputs) of the four calls with halves on the case's ramp inputs, the clamped ones at
    both radii.  device_forms: through the _device entry points on torch's current stream, device tensors in and out."""
    cam, prm, B = c["B"].c_struct(), c["prm"], c["B"]
    i, k = c["inputs"], c["checker"]
    if device_forms:
        import torch
        from rustray_amd import renderer
        up = lambda d, keys: [torch.from_numpy(np.ascontiguousarray(d[key]).copy()).cuda() for key in keys]
        down = lambda res: {key: res[key].cpu().numpy() for key in LAYERS if res.get(key) is not None}
        plain = lambda d: down(renderer.accumulate_torch(ds, cam, *up(d, KEYS), None, prm))
        split = lambda d: down(renderer.accumulate_split_torch(ds, cam, *up(d, SPLIT_KEYS), None, prm))
        clamped = lambda d, cl: down(renderer.accumulate_clamped_torch(ds, cam, *up(d, KEYS), None, prm, cl))
        clamped_split = lambda d, cl: down(renderer.accumulate_clamped_split_torch(ds, cam, *up(d, SPLIT_KEYS), None, prm, cl))
    else:
        plain = lambda d: ds.accumulate_records(cam, *(d[key] for key in KEYS), None, prm)
        split = lambda d: ds.accumulate_split(cam, *(d[key] for key in SPLIT_KEYS), None, prm)
        clamped = lambda d, cl: ds.accumulate_clamped(cam, *(d[key] for key in KEYS), None, prm, cl)
        clamped_split = lambda d, cl: ds.accumulate_clamped_split(cam, *(d[key] for key in SPLIT_KEYS), None, prm, cl)
    yield "accumulate_records", plain(i), temporal.accumulate_records(*(i[key] for key in KEYS), None, B, prm), i
    yield "accumulate_split", split(i), temporal.accumulate_split_records(*(i[key] for key in SPLIT_KEYS), None, B, prm), i
    for radius in (1, 2):
        cl = HistoryClampParams(radius=radius, sigma_scale=65536.0)
        yield f"accumulate_clamped radius {radius}", clamped(k, cl), temporal.accumulate_clamped_records(*(k[key] for key in KEYS), None, B, prm, cl), k
        yield (f"accumulate_clamped_split radius {radius}", clamped_split(k, cl),
               temporal.accumulate_clamped_split_records(*(k[key] for key in SPLIT_KEYS), None, B, prm, cl), k)


# ---- 1: the four calls per pair and size ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pair,size", CASES, ids=IDS)
def test_the_four_calls_against_the_truth(scene, pair, size):
    c = _case(scene, pair, size)
    W, H = size
    fig = conditions(c, pair, f"device frames, {pair} {W}x{H}")
    worst = []
    for name, got, want, inputs in _calls(scene, c):
        what = f"{pair} {W}x{H} {name}"
        _same_words(got, want, what)
        if "clamped" in name:
            assert not want["clamped"].any() and set(np.unique(got["length"])) <= {1.0, 2.0}, what
        res = rt.check_outputs(got, inputs, c["tr"], c["pred"], c["inside"], W, H, c["prm"].snap, what)
        worst.append(res["worst"])
    print(f"device, {pair} {W}x{H}: largest position error {worst[0]:.3g} px (accumulate_records), {max(worst):.3g} px (all four calls, every layer) over "
          f"{res['four']} four-tap pixels (bound {rt.POS_TOL:.3g}); {fig['interior']} interior pixels; {100 * fig['borderline']:.3f} % of the taps borderline")
    assert res["four"] >= 100


def test_the_device_forms_on_a_non_null_stream(scene):
    import torch
    pair, size = "all", rt.SIZES[1]
    c = _case(scene, pair, size)
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        for name, got, want, inputs in _calls(scene, c, device_forms=True):
            what = f"{pair} {size} {name}, device form"
            _same_words(got, want, what)
            rt.check_outputs(got, inputs, c["tr"], c["pred"], c["inside"], *size, c["prm"].snap, what)
    torch.cuda.synchronize()


# ---- 2: motion and camera together ------------------------------------------------------------------------------------------------------
def test_moved_items_under_a_moving_camera(hip):
    """A's frame, rr_scene_update_transforms, B's frame; then the motion and the accumulation on one stream, device buffers throughout."""
    import torch
    from rustray_amd import renderer
    from rustray_amd.renderer import _pack_records
    size = rt.SIZES[0]
    W, H = size
    fs = load_scene("spheres_room")
    edit = rt.moved_scene(fs)[3]
    rendered = []
    with hip.DeviceScene(fs, 0) as ds:
        def frames(_, camera):
            if rendered:                                          # A's frame first, B's behind the edit
                ds.update_transforms(*edit)
            rendered.append(camera)
            return _pack_records(ds.render_pixels(camera.c_struct(), rt.frame_config()))
        c = make_motion_case(None, size, frames=frames)
        assert rendered == [c["A"], c["B"]]
        what = f"device frames, moved items {W}x{H}"
        moved_conditions(c, what)
        i, cam = c["inputs"], c["B"].c_struct()
        st = torch.cuda.Stream()
        with torch.cuda.stream(st):
            dev = {key: torch.from_numpy(np.ascontiguousarray(i[key]).copy()).cuda() for key in KEYS}
            motion = renderer.motion_torch(ds, cam, dev["records"], c["index"], c["prev"])["motion"]
            acc = renderer.accumulate_torch(ds, cam, *(dev[key] for key in KEYS), motion, c["prm"])
            got = dict(records=acc["records"].cpu().numpy(), halves=acc["halves"].cpu().numpy(), length=acc["length"].cpu().numpy())
            got_motion = motion.cpu().numpy()
        torch.cuda.synchronize()
    t, ti = c["trans"]
    want_motion, _ = temporal.motion_records(i["records"], c["B"], c["ids"], c["prev"], ti[c["index"]])
    assert np.array_equal(got_motion.view(np.uint32), want_motion.view(np.uint32))
    _same_words(got, temporal.accumulate_records(*(i[key] for key in KEYS), want_motion, c["B"], c["prm"]), what)
    res = rt.check_outputs(got, i, c["tr"], c["pred"], c["inside"], W, H, c["prm"].snap, what)
    on = rt.position_errors(rt.history_means(got, i["current"])["records"][:, 0:2], c["tr"], c["pred"], got["length"])
    print(f"{what}: largest position error {res['worst']:.3g} px; {int((on['four'] & c['on_moved']).sum())} four-tap pixels on the moved items")
    assert (on["four"] & c["on_moved"]).sum() >= 50


# ---- 3: the pipelines hand on the right view ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pipeline", ("render_temporal", "render_temporal_split", "render_temporal_split_clamped"))
def test_a_pipeline_reprojects_through_the_camera_of_the_frame_before(hip, pipeline):
    """Two frames with rt.camera changed from A to B in between: what frame 2 accumulated is the explicit call on frame 2's own records
    against frame 1's outputs with previous_view(A), every word; with previous_view(B) (the mistake of handing on the current view) the
    explicit call gives something else."""
    import torch
    from rustray_amd.renderer import Raytracing, TemporalState
    size = rt.SIZES[0]
    fs = load_scene("spheres_room")
    A, B = rt.camera_pairs(fs, *size)["all"]
    split = pipeline != "render_temporal"
    out_keys = dict(records="accumulated", halves="accumulated_halves", length="length", **(dict(diffuse="accumulated_diffuse", diffuse_halves="accumulated_diffuse_halves") if split else {}))
    cur_keys = dict(records="noisy", halves="halves", **(dict(diffuse="diffuse", diffuse_halves="diffuse_halves") if split else {}))
    host = lambda res, keys: {k: res[v].cpu().numpy() for k, v in keys.items()}
    rtr = Raytracing(fs, A, 0)
    try:
        rtr.config = make_config(samples=2, monte_carlo=True, seed=3)
        state = TemporalState()
        run = getattr(rtr, pipeline)
        first = host(run(state, samples=2, seed=11), out_keys)
        torch.cuda.synchronize()
        rtr.camera = B
        res = run(state, samples=2, seed=12)
        torch.cuda.synchronize()
        second, cur = host(res, out_keys), host(res, cur_keys)
        ds, cam = rtr.device_scene, B.c_struct()

        def explicit(view):
            prm = AccumulateParams(prev_world_to_clip=view[0], prev_eye=view[1])
            if pipeline == "render_temporal":
                return ds.accumulate_records(cam, cur["records"], cur["halves"], first["records"], first["halves"], first["length"], None, prm)
            args = (cur["records"], cur["halves"], cur["diffuse"], cur["diffuse_halves"], first["records"], first["halves"], first["diffuse"], first["diffuse_halves"], first["length"], None, prm)
            return ds.accumulate_split(cam, *args) if pipeline == "render_temporal_split" else ds.accumulate_clamped_split(cam, *args)
        want, other = explicit(previous_view(A)), explicit(previous_view(B))
    finally:
        rtr.device_scene.close()
    assert set(np.unique(first["length"])) <= {0.0, 1.0} and (second["length"] > 1).mean() > 0.3      # frame 2 found history
    for key in out_keys:
        differ, _ = differing_words(second[key], want[key])
        assert differ == 0, f"{pipeline}: {differ} words of {key} are not the explicit call's with the view of the frame before"
    off = sum(differing_words(second[key], other[key])[0] for key in out_keys)
    print(f"{pipeline}: {off} words differ from the explicit call with the current view as the previous one")
    assert off > 1000
