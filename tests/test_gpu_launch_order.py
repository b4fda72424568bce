"""The launch schedule of a frame, recorded (rr_schedule_log.h, off unless a test switches it on) and checked by tests/launch_order.py: every
pair of operations whose declared address ranges overlap, other than atomic add against atomic add, must be ordered by the stream they
share, by an event, or by a wait of the host; every operation must be ordered before the call's return; and every wait and record must
be NEEDED -- deleted from the log (never from the device's queue), it must leave a race behind.  The bit-exact comparisons of the
staged frames (test_gpu_level1_overlap.py, test_gpu_level1_closest_stages.py, test_gpu_tail_overlap.py) cannot see a missing wait at
these sizes, where the device finishes a launch long before the host enqueues the next; this check does not depend on timing at all.

The frames are small ones those files use: tail_scene at 160 x 120 in 65 536-ray stages at 8, 11, 16 and 19 spp (3, 4, 5 and 6 stages
in 3 buffers), the cases (a) to (f) of test_gpu_tail_overlap.py as they stand, the 152 x 120 x 16 frame of the rich scene (5 stages,
the last ragged); each on the null stream through rr_render and through rr_render_region_device on a torch stream; a progressive
frame whose pass hook resolves between two batches, and an rr_render_pixels list frame.  Each test prints its tables (run with -s)."""
import ctypes as C

import numpy as np
import pytest

from rustray_amd.flat import make_config, rr_frame, rr_region
from tests import launch_order as lo
from tests.helpers import assert_frames_identical, camera_for
from tests.test_gpu_tail_overlap import TWO_BATCHES, tail_scene

pytestmark = pytest.mark.gpu

CHUNK = 65536
INT_STATS = ("primary_rays", "secondary_rays", "shadow_rays", "shaded_hits", "batches", "sliced_levels", "launches_trace_closest", "launches_trace_shadow", "launches_shade",
             "launches_trace_closest_level1", "launches_shade_level1", "launches_trace_shadow_level1")

# the categories of ordered cross-stream hazards: (earlier operation, later operation, the event the later one's stream waited for)
SHADE_SHADOW = ("k_shade<true>", "k_trace_shadow<true>", "stage_shaded")       # shade k -> shadow k
SHADOW_SHADE = ("k_trace_shadow<true>", "k_shade<true>", "stage_traced")       # shadow k -> shade k + n_buf: more than n_buf stages
CLOSEST_SHADE = ("k_trace_closest<true>", "k_shade<true>", "stage_closest")    # closest k -> shade k
POOL_CLOSEST = ("counter pool", "k_trace_closest<true>", "stage_fork")         # the pool's memset -> the closest-hit launches' head words
TAIL = ("k_trace_shadow<true>", ("k_resolve", "counter pool", "k_shade<false>"), "stage_tail")   # the pending shadow launches -> whatever joins them: one of ...
TAIL_RESOLVE = ("k_trace_shadow<true>", "k_resolve", "stage_tail")             # ... the resolve (it reads the planes they add to),
TAIL_BATCH = ("k_trace_shadow<true>", "counter pool", "stage_tail")            # ... the next batch's start_batch (it zeroes their counters),
TAIL_CHUNK = ("k_trace_shadow<true>", "k_shade<false>", "stage_tail")          # ... a chunk of level 2 that is not clear of their buffers
REST_CHUNK = ("k_trace_shadow<true>", "k_shade<false>", "shadow_rest")         # the clear chunk -> the shadow launch that last read buffer 0
COUNT_HOST = ("child_count -> h_count", "h_count[HC_LEVEL]", "count_ready")    # the level size's D2H -> the host's read
STAGED = (SHADE_SHADOW, CLOSEST_SHADE, POOL_CLOSEST, TAIL, TAIL_RESOLVE)

# name -> (scene, width, height, spp, max_recursion, tuning, level-1 stages, the categories the frame is built to contain)
# 160 x 120 = 19 200 pixels: 8, 11, 16, 19 spp = 153 600, 211 200, 307 200, 364 800 primary rays = 3, 4, 5, 6 stages of 65 536.
# The last two stages of 3 and of 6 use buffers 1 and 2: level 2's 65 536-ray chunk fits buffer 0 and is clear of them (REST_CHUNK); of 4 and 5
# stages they use buffer 0: every chunk of level 2 waits for the tail (TAIL_CHUNK), as with two stages per batch.
CASES = {
    "spp8": ("mixed", 160, 120, 8, 4, {}, 3, STAGED + (REST_CHUNK, COUNT_HOST)),
    "spp11": ("mixed", 160, 120, 11, 4, {}, 4, STAGED + (SHADOW_SHADE, TAIL_CHUNK, COUNT_HOST)),
    "spp16": ("mixed", 160, 120, 16, 4, {}, 5, STAGED + (SHADOW_SHADE, TAIL_CHUNK, COUNT_HOST)),
    "spp19": ("mixed", 160, 120, 19, 4, {}, 6, STAGED + (SHADOW_SHADE, REST_CHUNK, COUNT_HOST)),
    "a_deeper_levels_timed": ("mixed", 160, 120, 8, 4, {"kernel_timing": 1}, 3, STAGED + (REST_CHUNK, COUNT_HOST)),
    "b_level_2_empty": ("plain", 160, 120, 8, 4, {}, 3, STAGED + (COUNT_HOST,)),
    "c_spawns_nothing": ("mixed", 160, 120, 8, 0, {}, 3, STAGED),
    "d_no_light": ("nolight", 160, 120, 8, 4, {}, 0, (COUNT_HOST,)),
    "e_two_batches": ("mixed", 160, 120, 8, 4, {"queue_budget_bytes": TWO_BATCHES}, 4, STAGED + (TAIL_BATCH, TAIL_CHUNK, COUNT_HOST)),
    "f_sliced_level": ("glass", 160, 120, 8, 4, {"queue_budget_bytes": TWO_BATCHES}, 4, STAGED + (TAIL_BATCH, TAIL_CHUNK, COUNT_HOST)),
    "closest_152": ("rich", 152, 120, 16, 4, {}, 5, STAGED + (SHADOW_SHADE, COUNT_HOST)),
}

# A deleted wait or record that leaves NO race behind, by (case or "*", E = record / W = wait, tag) -> (why, how many per frame at most).
# Everything else must make a race.  For a wait the test prints the path that implies its order (the hazards it ordered, and what orders them now).
EXCUSED = {
    # records nobody waits for inside the call: the frame's and the launches' timers are read by rr_scene_last_stats afterwards
    ("*", "E", "frame_a"): ("the frame's timer, read after the call", 1),
    ("*", "E", "frame_b"): ("the frame's timer, read after the call", 1),
    ("*", "E", "timer"): ("a launch's timer, read after the call", 10 ** 6),
}
# stage_traced[b] is recorded behind EVERY shadow launch of the staged level 1.  Its waiters are the shade launch n_buf = 3 stages later, the
# second stream's join of the last stage (stage_tail) and, for the stage that last read buffer 0, a clear chunk of level 2 (shadow_rest).  The
# record behind a stage that has none of the three -- the last n_buf stages but the very last, less the one shadow_rest names -- is taken by
# no wait: the stage's own stream order in front of stage_tail covers its launch.  By stages per level: which buffers those are.
_NO_WAITER = "no wait takes it: its stage's buffer is not written again in this level, and stage_tail follows its launch on the same stream"
for _case, _buffers in {"spp8": (1,), "a_deeper_levels_timed": (1,), "pixel_list": (1,),              # 3 stages, stage 0 named by shadow_rest: stage 1
                        "b_level_2_empty": (0, 1), "c_spawns_nothing": (0, 1),                        # 3 stages, no level 2: stages 0 and 1
                        "spp11": (1, 2), "spp16": (2, 0), "closest_152": (2, 0),                      # 4 stages: 1 and 2; 5 stages: 2 and 3
                        "spp19": (1,),                                                                # 6 stages, stage 3 named by shadow_rest: stage 4
                        "e_two_batches": (0,), "f_sliced_level": (0,), "progressive": (0,)}.items():  # 2 stages per batch: stage 0, twice
    for _b in _buffers:
        EXCUSED[(_case, "E", f"stage_traced[{_b}]")] = (_NO_WAITER, 2 if _case[0] in "efp" and _case != "pixel_list" else 1)


def scene_of(kind):
    if kind == "rich":
        from tools.fuzz_parity import rich_scene   # as tests/test_gpu_level1_closest_stages.py builds it
        return rich_scene(9119)
    return {"mixed": lambda: tail_scene(), "plain": lambda: tail_scene("plain"), "nolight": lambda: tail_scene(lights=False), "glass": lambda: tail_scene("glass")}[kind]()


@pytest.fixture(scope="module")
def scenes():
    made = {}

    def get(kind):
        if kind not in made:
            made[kind] = scene_of(kind)
        return made[kind]
    return get


def config_of(case):
    _, _, _, spp, max_recursion, _, _, _ = CASES[case]
    return make_config(samples=spp, monte_carlo=True, seed=4242 if case != "closest_152" else 9119, max_recursion=max_recursion)


def render_case(hip, fs, case, stream, record):
    """One frame of `case` on a fresh handle (a sliced frame changes the next frame's arena: every frame here is a handle's first)
    -> (frame buffers, integer statistics, stages, the log's text or None).  stream: "null" = rr_render, "torch" = rr_render_region_device."""
    import torch
    _, w, h, _, _, tuning, _, _ = CASES[case]
    cam, cfg = camera_for(fs, w, h).c_struct(), config_of(case)
    with hip.DeviceScene(fs, 0) as ds:
        ds.set_tuning(shade_chunk_rays=CHUNK, **tuning)
        if record:
            ds.schedule_record(True)
        if stream == "null":
            out = ds.render(cam, cfg)
        else:
            dev = torch.device("cuda:0")
            t = dict(rgba=torch.zeros((h, w, 4), dtype=torch.uint8, device=dev), normal=torch.zeros((h, w, 3), dtype=torch.float32, device=dev),
                     depth=torch.zeros((h, w), dtype=torch.float32, device=dev), object_id=torch.zeros((h, w), dtype=torch.int32, device=dev))
            st = torch.cuda.Stream()
            torch.cuda.synchronize()   # (the zero fills above ran on torch's current stream)
            ds.render_region_device(cam, cfg, rr_region(8, 8, 1, 0), [t[k].data_ptr() for k in ("rgba", "normal", "depth", "object_id")], st.cuda_stream)
            st.synchronize()
            out = {k: v.cpu().numpy() for k, v in t.items()}
            out["object_id"] = out["object_id"].view(np.uint32)
        text = ds.schedule_log() if record else None
        stats = ds.stats()
        return out, {k: stats[k] for k in INT_STATS}, ds.overlap_stages(), text


def streams_with_launches(ops):
    return {o.stream for o in ops if o.kind == "L"}


def category_table(report, categories):
    rows = [(c, lo.count(report, *c)) for c in categories]
    return rows, "\n".join(f"  {a:24s} -> {b if isinstance(b, str) else ' | '.join(b):24s} behind {tag:14s}: {n}" for (a, b, tag), n in rows)


def implying_path(base, mutated):
    """For a deleted wait whose absence is not noticed: the hazards it ordered, and the event that orders them now."""
    now = {(a.index, b.index): tag for tag, pairs in mutated.ordered.items() for a, b, _, _ in pairs}
    lines = []
    for tag, pairs in base.ordered.items():
        for a, b, _, _ in pairs:
            if now.get((a.index, b.index), tag) != tag:
                lines.append(f"      {a.name} -> {b.name}: behind {tag}, without it behind {now[(a.index, b.index)]}")
    return "\n".join(sorted(set(lines))[:6])


def mutation_table(case, frame, idle_at_return=False, schedule=None):
    """Every wait and record deleted in turn -> (text, [(kind, tag) deleted without a race and without an excuse])."""
    schedule = schedule or lo.Schedule(frame.ops)
    base = lo.check(frame.ops, frame.stream, idle_at_return, schedule=schedule)
    counts, unnoticed, lines = {}, {}, []
    for op, races in lo.mutate(frame.ops, schedule):
        key = (op.kind, op.name)
        n, caught = counts.get(key, (0, 0))
        counts[key] = (n + 1, caught + bool(races))
        if not races:
            unnoticed.setdefault(key, []).append(op)
    bad = []
    for (kind, tag), (n, caught) in sorted(counts.items()):
        line = f"  {'record' if kind == 'E' else 'wait  '} {tag:18s}: {n:3d} deleted, {caught:3d} leave a race"
        missed = unnoticed.get((kind, tag), [])
        if missed:
            excuse = EXCUSED.get((case, kind, tag)) or EXCUSED.get(("*", kind, tag))
            if excuse and len(missed) <= excuse[1]:
                line += f", {len(missed)} excused: {excuse[0]}"
            else:
                line += f", {len(missed)} UNNOTICED"
                bad.append((kind, tag))
            for op in missed[:3]:
                if kind == "E":
                    line += f"\n      #{op.index}: " + ("no wait takes this record" if op.index not in base.consumed_records() else "a wait takes it, and nothing it orders is a hazard")
                else:
                    rep = lo.check(frame.ops, frame.stream, idle_at_return, skip=(op.index,))
                    line += f"\n      #{op.index} on stream {op.stream:#x}:\n" + (implying_path(base, rep) or "      it orders no hazard")
        lines.append(line)
    return "\n".join(lines), bad


def check_frame(case, frame, n_stages, categories, idle_at_return=False, call_streams=1):
    """The assertions every recorded frame gets; prints its tables."""
    ops = frame.ops
    schedule = lo.Schedule(ops)
    rep = lo.check(ops, frame.stream, idle_at_return, schedule=schedule)
    print(f"\n[{case}] stream {frame.stream:#x}, returned {frame.code}: {rep.summary()}")
    # not vacuous: launches on all three streams where the frame is staged
    n_streams = len(streams_with_launches(ops))
    assert n_streams == (3 if n_stages else 1), (case, n_streams)
    rows, text = category_table(rep, categories)
    print(text)
    for c, n in rows:
        assert n > 0, (case, "no ordered hazard of the category", c)
    assert not rep.races, f"{case}: {len(rep.races)} unordered hazards\n" + rep.describe_races()
    assert not rep.unjoined, f"{case}: not ordered before the return: " + ", ".join(str(o) for o in rep.unjoined[:8])
    text, bad = mutation_table(case, frame, idle_at_return, schedule)
    print(text)
    assert not bad, f"{case}: deleted without a race: {bad}"
    return rep


@pytest.mark.parametrize("stream", ["null", "torch"])
@pytest.mark.parametrize("case", list(CASES))
def test_recorded_frame(hip, scenes, case, stream):
    kind, w, h, spp, _, _, n_stages, categories = CASES[case]
    fs = scenes(kind)
    plain, stats0, stages0, _ = render_case(hip, fs, case, stream, record=False)
    logged, stats1, stages1, text = render_case(hip, fs, case, stream, record=True)
    # recording changes nothing: the frame's bytes, its counters and its launch counts
    assert_frames_identical(plain, logged, f"{case}: recording on")
    if stats0["sliced_levels"] and stats1["sliced_levels"]:
        # (f) Which children land in which slice follows the order of the atomic appends, which differs from run to run with or without the
        # recorder: the rays, the batches and the frame are the same, the NUMBER of slices is not (226 and 229 in two runs on one MI355X).
        stats0, stats1 = dict(stats0, sliced_levels=1), dict(stats1, sliced_levels=1)
    assert stats0 == stats1 and stages0 == stages1 == n_stages, (case, stats0, stats1, stages0, stages1)
    frames = lo.parse(text)
    assert len(frames) == 1 and frames[0].code == "0"
    frame = frames[0]
    if stream == "torch":
        assert frame.stream != 0
    check_frame(case, frame, n_stages, categories)
    if CASES[case][5].get("kernel_timing"):   # the log holds every launch the timers counted
        names = [o.name for o in frame.ops if o.kind == "L"]
        for prefix, key in (("k_trace_closest", "launches_trace_closest"), ("k_shade", "launches_shade"), ("k_trace_shadow", "launches_trace_shadow")):
            assert sum(1 for n in names if n.startswith(prefix)) == stats1[key], (prefix, stats1[key])


def test_progressive_frame_resolves_between_two_batches(hip, scenes):
    """The pass hook's join, resolve and copy in front of the second batch: two batches of two stages, both resolves behind stage_tail."""
    fs = scenes("mixed")
    cam, cfg = camera_for(fs, 160, 120).c_struct(), make_config(samples=8, monte_carlo=True, seed=4242, max_recursion=4)
    passes = []
    with hip.DeviceScene(fs, 0) as ds:
        ds.set_tuning(shade_chunk_rays=CHUNK, queue_budget_bytes=TWO_BATCHES)
        ref = ds.render(cam, cfg)
        ds.schedule_record(True)
        out = ds.render_progressive(cam, cfg, lambda frame, done, total: passes.append((done, total)) and False, min_passes=2)
        text = ds.schedule_log()
    assert passes == [(160 * 120 * 4, 160 * 120 * 8)]
    assert_frames_identical(ref, out, "progressive, recording on")
    frames = lo.parse(text)
    assert len(frames) == 1 and frames[0].code == "0"
    rep = check_frame("progressive", frames[0], 4, STAGED + (TAIL_BATCH, TAIL_CHUNK, COUNT_HOST))
    assert sum(1 for o in frames[0].ops if o.kind == "L" and o.name == "k_resolve") == 2
    assert sum(1 for o in frames[0].ops if o.kind == "D" and o.name == "frame -> host") == 4   # the hook's copy of the four buffers
    assert lo.count(rep, *TAIL_RESOLVE) >= 4   # two pending launches in front of each resolve


def test_pixel_list_frame(hip, scenes):
    """rr_render_pixels with a list: the list's slot table (k_pixel_slots), the wait for its first bad index, then the staged frame."""
    fs = scenes("mixed")
    w, h = 160, 120
    cam, cfg = camera_for(fs, w, h).c_struct(), make_config(samples=8, monte_carlo=True, seed=4242, max_recursion=4)
    ys, xs = np.mgrid[0:h, 0:w]
    pixels = np.stack([xs.ravel()[::-1], ys.ravel()[::-1]], axis=1)   # every pixel, last to first: 153 600 primary rays, three stages
    with hip.DeviceScene(fs, 0) as ds:
        ds.set_tuning(shade_chunk_rays=CHUNK)
        ref = ds.render_pixels(cam, cfg, pixels)
        assert ds.overlap_stages() == 3
        ds.schedule_record(True)
        got = ds.render_pixels(cam, cfg, pixels)
        text = ds.schedule_log()
    for k in ref:
        assert np.array_equal(ref[k], got[k], equal_nan=True), k
    frames = lo.parse(text)
    assert len(frames) == 1 and frames[0].code == "0"
    rep = check_frame("pixel_list", frames[0], 3, (SHADE_SHADOW, CLOSEST_SHADE, POOL_CLOSEST, ("k_trace_shadow<true>", "k_resolve_pixels", "stage_tail"), REST_CHUNK, COUNT_HOST,
                                                    ("pixel_bad -> h_count", "h_count[HC_PIXEL_BAD]", "fill_pixel_slots"), ("k_pixel_slots", "k_trace_closest<true>", "stage_fork")))
    assert rep.clean


@pytest.mark.parametrize("skip", [1, 2])
def test_exception_between_two_stages_leaves_the_handle_idle(hip, scenes, skip):
    """A bad_alloc thrown in enqueue_level1_stages in front of stage skip + 1 of five (the fault point level1_stages.stage; the ABI guard turns
    it into RR_ERR_OUT_OF_MEMORY): the launches of the earlier stages are complete, valid ones on all three streams, and the header promises a
    usable handle.  The log must show every one of them ordered before the return -- by the host, the call failed -- and the next frame on
    the handle is the serial frame.  (The device is synchronized before anything else touches the handle, whatever the log says.)"""
    import torch
    fs = scenes("mixed")
    w, h = 160, 120
    cam, cfg = camera_for(fs, w, h).c_struct(), make_config(samples=16, monte_carlo=True, seed=4242, max_recursion=4)
    L = hip.lib()
    L.rr_test_fault.argtypes = [C.c_char_p, C.c_int, C.c_int]
    with hip.DeviceScene(fs, 0) as ds:
        ds.set_tuning(shade_chunk_rays=0)
        serial = ds.render(cam, cfg)
        ds.set_tuning(shade_chunk_rays=CHUNK)
        out = dict(rgba=np.zeros((h, w, 4), np.uint8), normal=np.zeros((h, w, 3), np.float32), depth=np.zeros((h, w), np.float32), object_id=np.zeros((h, w), np.uint32))
        fr = rr_frame(out["rgba"].ctypes.data, out["normal"].ctypes.data, out["depth"].ctypes.data, out["object_id"].ctypes.data)
        ds.schedule_record(True)
        assert L.rr_test_fault(b"level1_stages.stage", 1, skip) == 0
        try:
            rc = L.rr_render(ds._h, C.byref(cam), C.byref(cfg), None, C.byref(fr), None)
        finally:
            L.rr_test_fault(b"", 0, 0)
            torch.cuda.synchronize()
        assert rc == -5 and b"memory" in L.rr_last_error()
        frames = lo.parse(ds.schedule_log())
        ds.schedule_record(False)
        assert len(frames) == 1 and frames[0].code == "unwound"
        ops = frames[0].ops
        assert len(streams_with_launches(ops)) == 3 and sum(1 for o in ops if o.kind == "L" and o.name == "k_shade<true>") == skip
        rep = lo.check(ops, frames[0].stream, idle_at_return=True)
        print(f"\n[fault in front of stage {skip + 1}] {rep.summary()}")
        print("  synchronized on the way out: " + ", ".join(f"{o.name} ({o.stream:#x})" for o in ops if o.kind == "S" and o.name == "frame left early"))
        assert not rep.races, rep.describe_races()
        assert not rep.unjoined, "pending at the return: " + ", ".join(str(o) for o in rep.unjoined)
        after = ds.render(cam, cfg)
        assert ds.overlap_stages() == 5
    assert_frames_identical(serial, after, "the frame after the failed one")
