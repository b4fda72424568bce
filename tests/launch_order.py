"""A happens-before checker for a recorded launch schedule (rr_schedule_log.h: what render_region_locked enqueued, in host order).

THE MODEL.  One vector clock per stream and one for the host; a component per timeline (a stream, or the host), counting its operations.
  * An operation enqueued on stream S first merges the HOST's clock into S's (everything enqueued after a host synchronize inherits
    what the host has waited for), then takes the next tick of S.  Operations of one stream are ordered by their ticks.
  * An event record gives the event S's clock.  An event carries the clock of its LATEST record in host order at the moment a wait on
    it is issued -- the HIP rule: a wait captures the event's state when it is called, a later record does not move it, an earlier
    record that was overwritten is forgotten.  The log is in host order, so processing it in order implements the rule.
  * A wait on an event that has never been recorded (in this log) orders nothing.
  * hipStreamWaitEvent merges the event's clock into the stream.  hipStreamSynchronize merges the stream's clock into the host,
    hipEventSynchronize the event's.  A host read (what a D2H copy brought) is an operation of the host's timeline.
  * a happens-before b  <=>  b's clock has reached a's tick on a's timeline.

WHAT IS NOT CREDITED (conservative: a schedule that needs one of these is reported as a race).
  * The legacy null stream is a timeline like any other.  Its implicit synchronization with blocking streams is not modelled: the
    handle's own streams are created hipStreamNonBlocking, and a caller's stream may be too.
  * hipMalloc and hipFree (DevBuf::reserve) order nothing, although the runtime may wait inside them.
  * hipMemcpy is a copy on the null stream followed by a host synchronize of the null stream (the recorder logs it as the two).
  * An event recorded before the log began is "never recorded": every frame is checked on its own, from `B` to `X`.
  * Kernel boundaries only: nothing is said about the order of accesses inside one launch.

HAZARDS.  Two work operations form a hazard when two of their ranges overlap in the same address space (device or host) and the pair
of modes is neither R-R nor A-A (A: an integer atomic add / or / min / max, which commutes with every other A).  Every hazard must be
ordered.

THE RETURN.  A call on the caller's stream is asynchronous: at its return every operation must happen-before the host OR the tail of
the call's stream (whoever then waits for the stream has waited for everything).  A call that fails promises an idle handle: then
(`idle_at_return`) the host alone counts.
"""
from dataclasses import dataclass, field

HOST = "host"
WORK_KINDS = "LMUDH"   # launch, memset, copy to the device, copy to the host, host read
KIND_NAMES = {"L": "launch", "M": "memset", "U": "H2D", "D": "D2H", "E": "record", "W": "wait", "S": "sync stream", "Y": "sync event", "H": "host read",
              "B": "begin", "X": "end"}


@dataclass(frozen=True)
class Access:
    mode: str      # R, W, A
    lo: int
    hi: int
    what: str = ""
    host: bool = False

    def __str__(self):
        return f"{self.mode} {'host ' if self.host else ''}[{self.lo:#x}, {self.hi:#x}) {self.what}"


@dataclass
class Op:
    kind: str
    stream: int = 0
    event: int = 0
    name: str = ""
    acc: tuple = ()
    index: int = -1

    def timeline(self):
        return HOST if self.kind == "H" else self.stream

    def __str__(self):
        where = "host" if self.kind == "H" else f"stream {self.stream:#x}"
        return f"#{self.index} {KIND_NAMES[self.kind]} {self.name} on {where}"


# ---- builders for hand-written schedules
def R(lo, hi, what=""): return Access("R", lo, hi, what)
def W(lo, hi, what=""): return Access("W", lo, hi, what)
def A(lo, hi, what=""): return Access("A", lo, hi, what)
def launch(stream, name, *acc): return Op("L", stream, 0, name, tuple(acc))
def memset(stream, name, lo, hi): return Op("M", stream, 0, name, (W(lo, hi, name),))
def d2h(stream, name, src, dst): return Op("D", stream, 0, name, (Access("R", src[0], src[1], name), Access("W", dst[0], dst[1], name, True)))
def record(stream, event, tag=""): return Op("E", stream, event, tag or f"event {event}")
def wait(stream, event, tag=""): return Op("W", stream, event, tag or f"event {event}")
def sync_stream(stream, name="sync"): return Op("S", stream, 0, name)
def sync_event(event, tag=""): return Op("Y", 0, event, tag or f"event {event}")
def host_read(name, lo, hi): return Op("H", 0, 0, name, (Access("R", lo, hi, name, True),))


@dataclass
class Frame:
    ops: list
    stream: int      # the call's stream
    code: str        # the return code as text, "unwound" for an exception, "" when the log ends inside the call


def parse(text: str) -> list:
    """The text of rr_test_schedule_read -> the frames it holds (`B` .. `X`), operations outside a frame dropped."""
    frames, cur = [], None
    for line in text.splitlines():
        if not line:
            continue
        kind, stream, event, name, acc = (line.split("\t") + [""])[:5]
        if kind == "B":
            cur = Frame([], int(stream, 16), "")
            frames.append(cur)
            continue
        if cur is None:
            continue
        if kind == "X":
            cur.code = name
            cur = None
            continue
        accs = []
        for a in filter(None, acc.split(";")):
            mode, space, lo, hi, what = a.split(",", 4)
            accs.append(Access(mode, int(lo, 16), int(hi, 16), what, space == "h"))
        cur.ops.append(Op(kind, int(stream, 16), int(event, 16), name, tuple(accs)))
    return frames


def hazards(ops):
    """THE DEFINITION, pair by pair: every (i, j), i < j in host order, of work operations with overlapping ranges whose modes conflict
    -> [(i, j, access of i, access of j)], one entry per pair of operations (the first conflicting pair of ranges found).  Quadratic in the
    launches that share a buffer: for frames of a few hundred operations, and for checking frontier_hazards against."""
    flat = []
    for i, o in enumerate(ops):
        if o.kind in WORK_KINDS:
            for a in o.acc:
                if a.hi > a.lo:
                    flat.append((a.host, a.lo, a.hi, i, a))
    flat.sort(key=lambda t: (t[0], t[1]))
    found = {}
    for x, (host, lo, hi, i, a) in enumerate(flat):
        for y in range(x + 1, len(flat)):
            host2, lo2, _, j, b = flat[y]
            if host2 != host or lo2 >= hi:
                break
            if i == j or (a.mode == b.mode and a.mode in "RA"):
                continue
            key = (i, j) if i < j else (j, i)
            if key not in found:
                found[key] = (a, b) if i < j else (b, a)
    return [(i, j, ab[0], ab[1]) for (i, j), ab in sorted(found.items())]


def frontier_hazards(ops, before):
    """The hazards that imply all others, in time linear in the accesses (a sliced level records thousands of launches over the same planes).
    before(i, j): operation i happens-before operation j > i, in the schedule AS RECORDED.
    Per group of overlapping ranges a frontier of accesses is kept.  A new access x of operation j is paired with every frontier entry it
    overlaps and conflicts with, and then REPLACES every entry e that lies inside x's range and happens-before j, provided x conflicts with
    at least what e conflicts with AND the order of e and x cannot be lost unseen: x writes (then e -> x is itself a listed hazard), or x
    has e's mode and runs on e's timeline (a stream's own order cannot be deleted).  Whatever conflicts with e later conflicts with x
    too, and being ordered behind x it is ordered behind e.  So every hazard of the definition that is not listed is implied by a chain
    whose links are listed hazards or one timeline's own order.  That stays true when orderings are taken AWAY (a deleted wait or
    record): the implied hazard is ordered while every link of its chain is, and a link that breaks is in the list.  (An atomic add
    that replaced an atomic add of ANOTHER stream would be such a chain with an unlisted link: A against A is no hazard.)  Hence: no
    listed hazard unordered <=> no hazard unordered, for the schedule and for every mutation of it -- tests/test_launch_order.py holds
    the two lists to that on every schedule it has."""
    flat = []
    for i, o in enumerate(ops):
        if o.kind in WORK_KINDS:
            for a in o.acc:
                if a.hi > a.lo:
                    flat.append((a.host, a.lo, a.hi, i, a))
    order = sorted(range(len(flat)), key=lambda k: (flat[k][0], flat[k][1]))
    group_of, group, reach, space = [0] * len(flat), -1, -1, None
    for k in order:   # groups of ranges connected by overlap
        host, lo, hi, _, _ = flat[k]
        if host != space or lo >= reach:
            group, reach, space = group + 1, hi, host
        reach = max(reach, hi)
        group_of[k] = group
    frontier = [[] for _ in range(group + 1)]
    lines = [o.timeline() for o in ops]
    found = {}
    for k, (_, lo, hi, j, x) in enumerate(flat):   # in host order: flat was filled operation by operation
        f = frontier[group_of[k]]
        keep = []
        for e in f:
            elo, ehi, i, a = e
            if i == j or elo >= hi or ehi <= lo:
                keep.append(e)
                continue
            conflict = not (a.mode == x.mode and a.mode in "RA")
            if conflict and (i, j) not in found:
                found[(i, j)] = (a, x)
            if lo <= elo and ehi <= hi and (x.mode == "W" or (x.mode == a.mode and lines[i] == lines[j])) and before(i, j):
                continue   # replaced by x
            keep.append(e)
        keep.append((lo, hi, j, x))
        frontier[group_of[k]] = keep
    return [(i, j, ab[0], ab[1]) for (i, j), ab in sorted(found.items())]


@dataclass
class Report:
    ops: list
    races: list = field(default_factory=list)        # (op a, op b, access a, access b): a hazard that nothing orders
    ordered: dict = field(default_factory=dict)      # tag of the ordering event (or "host:<sync>", "host order") -> [(op a, op b, access a, access b)], cross-timeline hazards only
    unjoined: list = field(default_factory=list)     # work operations that do not happen-before the return
    credited: dict = field(default_factory=dict)     # index of a wait / event synchronize -> index of the record it took its clock from (None: never recorded)
    n_hazards: int = 0

    @property
    def clean(self):
        return not self.races

    def consumed_records(self):
        return {r for r in self.credited.values() if r is not None}

    def describe_races(self, limit=20):
        return "\n".join(f"RACE {a} ({x})  ||  {b} ({y})" for a, b, x, y in self.races[:limit])

    def summary(self):
        lines = [f"{len(self.ops)} operations, {self.n_hazards} hazards, {len(self.races)} unordered, {len(self.unjoined)} not ordered before the return"]
        for tag in sorted(self.ordered):
            lines.append(f"  ordered behind {tag}: {len(self.ordered[tag])}")
        return "\n".join(lines)


def _join(a, b):
    return a if a == b else tuple(map(max, a, b))


class Schedule:
    """The clocks of one frame's operations (`ops` in host order), and of the frame with one ordering operation deleted."""

    def __init__(self, ops):
        self.ops = list(ops)
        for i, o in enumerate(self.ops):
            o.index = i
        self.lines = {HOST: 0}   # timeline -> component of the clocks
        for o in self.ops:
            if o.kind not in "HY":
                self.lines.setdefault(o.stream, len(self.lines))
        self.zero = (0,) * len(self.lines)
        self.tick = {}           # work operation -> (component, count): never changed by deleting an ordering operation
        self.clock, self.credited, self.waits, self.host_syncs, self.snap = {}, {}, {}, [], []
        state = ({}, self.zero, {})
        for i in range(len(self.ops)):
            state = self._step(i, state, self.clock, self.credited, True)
            self.snap.append(state)
        self.end = state
        self._pairs = None

    def pairs(self):
        if self._pairs is None:
            self._pairs = frontier_hazards(self.ops, self.before)
        return self._pairs

    def _step(self, i, state, clock, credited, base):
        """Operation i applied to (stream -> clock, the host's clock, event -> (clock, its record)) -> the state after it (new dicts where changed)."""
        streams, host, events = state
        o = self.ops[i]
        if o.kind == "H":
            host = host[:0] + (host[0] + 1,) + host[1:]
            clock[i] = host
            if base:
                self.tick[i] = (0, host[0])
            return streams, host, events
        if o.kind == "Y":
            got = events.get(o.event)
            credited[i] = got[1] if got else None
            if got:
                host = _join(host, got[0])
            if base:
                self.host_syncs.append((i, o.name, host))
            return streams, host, events
        s = streams.get(o.stream, self.zero)
        if o.kind == "S":
            host = _join(host, s)
            if base:
                self.host_syncs.append((i, o.name, host))
            return streams, host, events
        s = _join(s, host)
        if o.kind == "E":
            events = dict(events)
            events[o.event] = (s, i)
        elif o.kind == "W":
            got = events.get(o.event)
            credited[i] = got[1] if got else None
            if got:
                s = _join(s, got[0])
                if base:
                    self.waits.setdefault(o.stream, []).append((i, o.name, got[0]))
        else:
            c = self.lines[o.stream]
            s = s[:c] + (s[c] + 1,) + s[c + 1:]
            clock[i] = s
            if base:
                self.tick[i] = (c, s[c])
        if streams.get(o.stream) != s:
            streams = dict(streams)
            streams[o.stream] = s
        return streams, host, events

    def before(self, i, j, clock=None):
        c, n = self.tick[i]
        return (clock or self.clock)[j][c] >= n

    def covers(self, c, i):
        line, n = self.tick[i]
        return c[line] >= n

    def without(self, d):
        """The clocks that change when the ordering operation d is deleted: {work operation: clock}.  The walk stops where the state is the
        recorded schedule's again (a deleted record of count_ready matters until the next one has been waited for)."""
        assert self.ops[d].kind in "EWSY", "only ordering operations can be deleted"
        state = self.snap[d - 1] if d else ({}, self.zero, {})
        changed, scratch = {}, {}
        for i in range(d + 1, len(self.ops)):
            state = self._step(i, state, changed, scratch, False)
            if state == self.snap[i]:
                break
        return {i: c for i, c in changed.items() if c != self.clock[i]}


def check(ops, call_stream=0, idle_at_return=False, skip=(), exhaustive=False, schedule=None) -> Report:
    """ops: the operations of one frame in host order.  skip: indices of operations to leave out (a deleted wait or record).
    exhaustive: every hazard of the definition (hazards) instead of the ones that imply them (frontier_hazards).
    schedule: Schedule(ops) made before (check and mutate of one frame share its clocks and its list of hazards)."""
    skip = set(skip)
    if skip:   # the plain way: the same frame without them
        kept = [o for i, o in enumerate(ops) if i not in skip]
        assert all(ops[i].kind in "EWSY" for i in skip), "only ordering operations can be deleted"
        rep = check(kept, call_stream, idle_at_return, (), exhaustive)
        back = [i for i in range(len(ops)) if i not in skip]
        for o, i in zip(kept, back):
            o.index = i
        rep.ops = list(ops)
        rep.credited = {back[w]: (back[r] if r is not None else None) for w, r in rep.credited.items()}
        return rep
    sch = schedule or Schedule(ops)
    ops = sch.ops
    rep = Report(ops, credited=dict(sch.credited))

    def via(i, j):   # the first wait of j's stream (then: the first host synchronize) in front of j whose clock has reached i
        o = ops[j]
        if ops[i].kind == "H":
            return "host order"   # the host read first and enqueued afterwards
        if o.kind != "H":
            for w, tag, c in sch.waits.get(o.stream, ()):
                if w < j and sch.covers(c, i):
                    return tag
        for h, tag, c in sch.host_syncs:
            if h < j and sch.covers(c, i):
                return tag if o.kind == "H" else "host:" + tag
        return "?"

    pairs = hazards(ops) if exhaustive else sch.pairs()
    rep.n_hazards = len(pairs)
    for i, j, a, b in pairs:
        if not sch.before(i, j):
            rep.races.append((ops[i], ops[j], a, b))
        elif ops[i].timeline() != ops[j].timeline():
            rep.ordered.setdefault(via(i, j), []).append((ops[i], ops[j], a, b))
    streams, host, _ = sch.end
    end = host if idle_at_return else _join(host, streams.get(call_stream, sch.zero))
    rep.unjoined = [ops[i] for i in sorted(sch.clock) if not sch.covers(end, i)]
    return rep


def mutate(ops, schedule=None):
    """Delete every wait and record in turn -> [(op, the hazards that are unordered without it as (op a, op b, access a, access b))], in host
    order.  (A stream or event synchronize is the host's own waiting, not part of the schedule between the streams: those stay.)
    The hazards are the frontier's, listed once for the schedule as recorded (frontier_hazards: why that is enough); only the clocks
    that the deletion changes are looked at."""
    sch = schedule or Schedule(ops)
    ops = sch.ops
    into = {}   # later operation -> [(earlier operation, access, access)] of the hazards that cross timelines (one stream's own order cannot be deleted)
    for i, j, a, b in sch.pairs():
        if ops[i].timeline() != ops[j].timeline() and sch.before(i, j):
            into.setdefault(j, []).append((i, a, b))
    out = []
    for d, o in enumerate(ops):
        if o.kind in "EW":
            changed = sch.without(d)
            out.append((o, [(ops[i], ops[j], a, b) for j in sorted(changed) for i, a, b in into.get(j, ()) if not sch.before(i, j, changed)]))
    return out


def count(report: Report, first: str, second: str, tag: str) -> int:
    """Ordered cross-timeline hazards whose earlier operation's name starts with `first`, whose later one's with `second`, behind an event whose tag starts with `tag`."""
    return sum(1 for t, pairs in report.ordered.items() if t.startswith(tag) for a, b, _, _ in pairs if a.name.startswith(first) and b.name.startswith(second))
