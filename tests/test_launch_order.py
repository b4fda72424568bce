"""tests/launch_order.py on hand-written schedules: the seeded mistakes of the model itself.  Each schedule is the smallest that holds the
property; what the checker says about the frames the library records is tests/test_gpu_launch_order.py."""
from tests import launch_order as lo
from tests.launch_order import A, R, W, check, launch, memset, record, wait

S1, S2, S3 = 0x10, 0x20, 0x30
EV, EV2 = 0x100, 0x200
BUF = (0x1000, 0x2000)


def _names(report):
    return [(a.name, b.name) for a, b, _, _ in report.races]


def test_two_streams_write_then_read_without_an_event_race():
    rep = check([launch(S1, "producer", W(*BUF)), launch(S2, "consumer", R(*BUF))], call_stream=S1)
    assert _names(rep) == [("producer", "consumer")] and rep.n_hazards == 1
    assert "producer" in rep.describe_races() and "0x1000" in rep.describe_races()   # both names and the range are reported


def test_record_and_wait_order_them():
    ops = [launch(S1, "producer", W(*BUF)), record(S1, EV, "ready"), wait(S2, EV, "ready"), launch(S2, "consumer", R(*BUF))]
    rep = check(ops, call_stream=S1)
    assert rep.clean and rep.n_hazards == 1
    assert [(a.name, b.name) for a, b, _, _ in rep.ordered["ready"]] == [("producer", "consumer")]   # grouped by the event that orders them
    assert rep.credited == {2: 1}
    # ... and the consumer's stream was never joined: not everything happens-before the return
    assert [o.name for o in rep.unjoined] == ["consumer"]
    joined = check(ops + [record(S2, EV2, "done"), wait(S1, EV2, "done")], call_stream=S1)
    assert joined.clean and not joined.unjoined
    # a call that must leave the handle idle needs the host to have waited
    assert [o.name for o in check(ops, call_stream=S1, idle_at_return=True).unjoined] == ["producer", "consumer"]


def test_a_wait_issued_before_the_record_orders_nothing():
    ops = [launch(S1, "producer", W(*BUF)), wait(S2, EV, "ready"), record(S1, EV, "ready"), launch(S2, "consumer", R(*BUF))]
    rep = check(ops, call_stream=S1)
    assert _names(rep) == [("producer", "consumer")] and rep.credited == {1: None}


def test_a_wait_takes_the_latest_record_in_host_order():
    """The event is recorded behind the producer and AGAIN behind a later launch before the wait is issued: the wait is credited with the
    later record, which follows the producer on the same stream -- clean -- and orders the later launch as well."""
    ops = [launch(S1, "producer", W(*BUF)), record(S1, EV, "ready"), launch(S1, "later", W(0x5000, 0x6000)), record(S1, EV, "ready"), wait(S2, EV, "ready"),
           launch(S2, "consumer", R(*BUF), R(0x5000, 0x6000))]
    rep = check(ops, call_stream=S1)
    assert rep.clean and rep.credited[4] == 3
    assert sorted((a.name, b.name) for a, b, _, _ in rep.ordered["ready"]) == [("later", "consumer"), ("producer", "consumer")]
    # had the wait kept the FIRST record, `later` would race: that is what deleting the second record shows
    assert _names(check(ops, call_stream=S1, skip=(3,))) == [("later", "consumer")]
    # ... and a re-record on ANOTHER stream in between takes the order away (the earlier record is forgotten)
    ops = [launch(S1, "producer", W(*BUF)), record(S1, EV, "ready"), record(S3, EV, "ready"), wait(S2, EV, "ready"), launch(S2, "consumer", R(*BUF))]
    rep = check(ops, call_stream=S1)
    assert _names(rep) == [("producer", "consumer")] and rep.credited[3] == 2


def test_atomic_adds_to_one_range_commute():
    rep = check([launch(S1, "shade", A(*BUF)), launch(S2, "shadow", A(*BUF))], call_stream=S1)
    assert rep.clean and rep.n_hazards == 0


def test_an_atomic_add_against_a_memset_races_unless_ordered():
    assert _names(check([memset(S1, "zero", *BUF), launch(S2, "shadow", A(*BUF))], call_stream=S1)) == [("zero", "shadow")]
    rep = check([memset(S1, "zero", *BUF), record(S1, EV, "zeroed"), wait(S2, EV, "zeroed"), launch(S2, "shadow", A(*BUF))], call_stream=S1)
    assert rep.clean and len(rep.ordered["zeroed"]) == 1
    # ... and against a plain read or write as well
    assert len(check([launch(S1, "resolve", R(*BUF)), launch(S2, "shadow", A(*BUF))], call_stream=S1).races) == 1
    assert len(check([launch(S1, "store", W(*BUF)), launch(S2, "shadow", A(*BUF))], call_stream=S1).races) == 1


def test_disjoint_ranges_are_clean():
    rep = check([launch(S1, "a", W(0x1000, 0x2000)), launch(S2, "b", W(0x2000, 0x3000), R(0x0, 0x1000))], call_stream=S1)   # [lo, hi): touching is not overlapping
    assert rep.clean and rep.n_hazards == 0
    assert len(check([launch(S1, "a", W(0x1000, 0x2001)), launch(S2, "b", W(0x2000, 0x3000))], call_stream=S1).races) == 1
    # a device range and a host range with the same numbers are different memory
    assert check([lo.d2h(S1, "copy", (0x9000, 0x9004), BUF), launch(S2, "b", W(*BUF))], call_stream=S1).clean


def _rotation(n_stages, n_buf, with_wait):
    """The staged level 1 in small: stage k is written on S1 into buffer k % n_buf and read on S2 behind `written[b]`; writer k waits for the
    reader of stage k - n_buf (`read[b]`) -- or does not."""
    ops = []
    for k in range(n_stages):
        b = k % n_buf
        buf = (0x1000 * (b + 1), 0x1000 * (b + 2))
        if k >= n_buf and with_wait:
            ops.append(wait(S1, 0x300 + b, f"read[{b}]"))
        ops += [launch(S1, f"write {k}", W(*buf)), record(S1, 0x200 + b, f"written[{b}]"), wait(S2, 0x200 + b, f"written[{b}]"), launch(S2, f"read {k}", R(*buf)),
                record(S2, 0x300 + b, f"read[{b}]")]
    return ops


def test_three_buffer_rotation_with_its_wait():
    rep = check(_rotation(5, 3, True), call_stream=S1, exhaustive=True)
    assert rep.clean
    assert [(a.name, b.name) for a, b, _, _ in rep.ordered["read[0]"]] == [("read 0", "write 3")]
    assert [(a.name, b.name) for a, b, _, _ in rep.ordered["read[1]"]] == [("read 1", "write 4")]
    # writer k -> reader k, five times; and writers 0 and 1 -> readers 3 and 4 of the same buffers, which the first wait of the readers' stream already orders
    assert sum(len(rep.ordered[f"written[{b}]"]) for b in range(3)) == 5 + 2
    assert lo.count(rep, "write", "read", "written") == 7 and lo.count(rep, "read", "write", "read[") == 2
    # the frontier lists the five and the two rotations: writers 0 and 1 -> readers 3 and 4 are implied by writer 0 -> writer 3 -> reader 3
    front = check(_rotation(5, 3, True), call_stream=S1)
    assert front.clean and lo.count(front, "write", "read", "written") == 5 and lo.count(front, "read", "write", "read[") == 2
    # every wait and every record that somebody waits for is needed: deleting it makes a race.  The records behind the last three readers have no waiter.
    ops = _rotation(5, 3, True)
    unnoticed = [(o.kind, o.name) for o, races in lo.mutate(ops) if not races]
    assert unnoticed == [("E", "read[2]"), ("E", "read[0]"), ("E", "read[1]")]


def test_three_buffer_rotation_without_its_wait_races():
    rep = check(_rotation(5, 3, False), call_stream=S1)
    assert sorted(_names(rep)) == [("read 0", "write 3"), ("read 1", "write 4")]


def test_order_through_a_host_synchronize():
    ops = [launch(S1, "producer", W(*BUF)), lo.sync_stream(S1, "wait for the producer"), launch(S2, "consumer", R(*BUF))]
    rep = check(ops, call_stream=S1)
    assert rep.clean and [(a.name, b.name) for a, b, _, _ in rep.ordered["host:wait for the producer"]] == [("producer", "consumer")]
    # through an event synchronize, and for a host read of what a copy brought
    ops = [lo.d2h(S1, "count -> host", (0x9000, 0x9004), (0x7000, 0x7004)), record(S1, EV, "count_ready"), lo.sync_event(EV, "count_ready"), lo.host_read("count", 0x7000, 0x7004)]
    rep = check(ops, call_stream=S1)
    assert rep.clean and len(rep.ordered["count_ready"]) == 1
    assert len(check(ops, call_stream=S1, skip=(1,)).races) == 1 and len(check(ops, call_stream=S1, skip=(2,)).races) == 1
    # the next copy into the same word is enqueued after the host has read it
    rep = check(ops + [lo.d2h(S1, "count -> host", (0x9000, 0x9004), (0x7000, 0x7004))], call_stream=S1)
    assert rep.clean and rep.n_hazards == 3 and len(rep.ordered["host order"]) == 1
    # a synchronize of ANOTHER stream orders nothing
    assert len(check([launch(S1, "producer", W(*BUF)), lo.sync_stream(S3), launch(S2, "consumer", R(*BUF))], call_stream=S1).races) == 1


def test_the_null_stream_is_a_stream_like_any_other():
    """No implicit ordering between the legacy null stream and the others is credited (the handle's streams are non-blocking)."""
    assert len(check([memset(0, "zero", *BUF), launch(S2, "shadow", A(*BUF))], call_stream=0).races) == 1
    assert check([memset(0, "zero", *BUF), launch(0, "shade", A(*BUF))], call_stream=0).clean


def test_parse_reads_the_recorders_text():
    text = ("S\t0\t0\toutside a frame\t\n"
            "B\t10\t0\trender_region_locked\t\n"
            "M\t10\t0\tacc_rgb\tW,d,1000,2000,acc_rgb\n"
            "E\t10\t100\tstage_shaded[0]\t\n"
            "W\t20\t100\tstage_shaded[0]\t\n"
            "L\t20\t0\tk_trace_shadow<true>\tR,d,3000,4000,shadow s0;A,d,1000,2000,acc_rgb\n"
            "D\t10\t0\tchild_count -> h_count\tR,d,5000,5004,child_count -> h_count;W,h,7000,7004,child_count -> h_count\n"
            "X\t10\t0\t0\t\n"
            "B\t0\t0\trender_region_locked\t\n"
            "X\t0\t0\tunwound\t\n")
    frames = lo.parse(text)
    assert [(f.stream, f.code, len(f.ops)) for f in frames] == [(0x10, "0", 5), (0, "unwound", 0)]
    ops = frames[0].ops
    assert ops[3].name == "k_trace_shadow<true>" and ops[3].acc[1] == lo.Access("A", 0x1000, 0x2000, "acc_rgb", False) and ops[4].acc[1].host
    rep = check(ops, call_stream=0x10)
    assert rep.clean and lo.count(rep, "acc_rgb", "k_trace_shadow", "stage_shaded") == 1 and [o.name for o in rep.unjoined] == ["k_trace_shadow<true>"]


def _schedules():
    yield _rotation(5, 3, True)
    yield _rotation(7, 3, True)
    yield _rotation(5, 2, True)
    yield _rotation(5, 3, False)
    # atomic adds from two streams onto a zeroed plane, a resolve behind a join, a second round on the same plane.  ("level 2" adds behind the
    # join and in front of the resolve: were it to replace the other stream's add on the frontier, deleting the join would go unseen.)
    ops = []
    for r in range(2):
        ops += [memset(S1, "zero", *BUF), record(S1, EV, "zeroed"), wait(S2, EV, "zeroed"), launch(S1, "shade", A(*BUF), W(0x5000, 0x6000)), record(S1, EV2, "shaded"),
                wait(S2, EV2, "shaded"), launch(S2, "shadow", A(*BUF), R(0x5000, 0x5800)), launch(S1, "shade2", A(0x1800, 0x2000)), record(S2, 0x300, "tail"),
                wait(S1, 0x300, "tail"), launch(S1, "level 2", A(*BUF)), launch(S1, "resolve", R(*BUF)), lo.d2h(S1, "count", (0x9000, 0x9004), (0x7000, 0x7004)), record(S1, 0x400, "count_ready"),
                lo.sync_event(0x400, "count_ready"), lo.host_read("count", 0x7000, 0x7004)]
    yield ops
    with open(GOLDEN) as fh:
        yield lo.parse(fh.read())[0].ops


GOLDEN = __import__("os").path.join(__import__("os").path.dirname(__file__), "golden", "launch_order_staged_frame.log")


def test_the_frontier_lists_a_race_exactly_when_the_definition_has_one():
    """frontier_hazards against hazards, the definition pair by pair: on every schedule here, on a frame the library recorded (three stages
    on three streams, levels 2 to 4 behind them: tests/golden/launch_order_staged_frame.log), and on each of them with every wait and every record
    deleted in turn -- the same verdict, every listed hazard one of the definition's, and the incremental walk of mutate() the same races
    as checking the shortened schedule from scratch."""
    n_mutations = 0
    for ops in _schedules():
        full, front = check(ops, call_stream=ops[0].stream, exhaustive=True), check(ops, call_stream=ops[0].stream)
        assert front.clean == full.clean and front.n_hazards <= full.n_hazards
        every = {(a.index, b.index) for a, b, _, _ in full.races}
        assert {(a.index, b.index) for a, b, _, _ in front.races} <= every
        for op, races in lo.mutate(ops):
            full = check(ops, call_stream=ops[0].stream, skip=(op.index,), exhaustive=True)
            front = check(ops, call_stream=ops[0].stream, skip=(op.index,))
            assert front.clean == full.clean, str(op)
            if check(ops).clean:   # mutate() lists what the deletion breaks in a schedule that was in order
                assert bool(races) == (not full.clean), str(op)
                assert {(a.index, b.index) for a, b, _, _ in races} <= {(a.index, b.index) for a, b, _, _ in full.races}, str(op)
            n_mutations += 1
    assert n_mutations > 100


def test_a_recorded_staged_frame_is_in_order_and_needs_its_waits():
    """The recorded frame of the golden file (tail_scene, 160 x 120 x 8 in three 65 536-ray stages, the null stream): no unordered hazard, all
    ordered before the return, and the only deletions that go unnoticed are records that no wait takes."""
    with open(GOLDEN) as fh:
        frame = lo.parse(fh.read())[0]
    rep = check(frame.ops, frame.stream)
    assert rep.clean and not rep.unjoined and len({o.stream for o in frame.ops if o.kind == "L"}) == 3
    assert lo.count(rep, "k_shade<true>", "k_trace_shadow<true>", "stage_shaded") == 3 and lo.count(rep, "k_trace_shadow<true>", "k_resolve", "stage_tail") >= 1
    unnoticed = [o for o, races in lo.mutate(frame.ops) if not races]
    assert sorted(o.name for o in unnoticed) == ["frame_a", "frame_b", "stage_traced[1]"]
    assert all(o.kind == "E" and o.index not in rep.consumed_records() for o in unnoticed)
