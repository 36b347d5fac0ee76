"""Stream-ordering audit: a happens-before model of device work and a recorder that turns one pass of the Python orchestration
(hg_module.forward's forked branches, HostFrameFeed, CapturedStep.replay) into a trace the model can check.

MODEL.  A trace is a list of records:
    Access(stream, name, reads, writes, ors, where)   byte ranges [(lo, hi)) a launch on `stream` reads / writes / ORs a sticky bit into
    Wait(waiter, signaller)                           the waiter comes after everything enqueued on the signaller so far
    EventRecord(event, stream), EventWait(stream, event)    the same edge in two steps
    HostSync(stream | None)                           the host blocks until `stream` (None: every stream) has drained
    EventSync(event)                                  the host blocks until the event's record has been reached
    CaptureBegin(graph), CaptureEnd(graph)            the records in between were captured into `graph`, not executed
Every stream has a vector clock; records of one stream are totally ordered; NO ordering is assumed between two streams - the default
stream included - unless a wait, an event or a host sync makes it.  A HAZARD is a pair of accesses on different streams with overlapping
bytes, one of them a write, of which the earlier does not happen before the later.  check(trace) returns every hazard.

ONE exemption: the range-guard flag word (ops._MODE.range_flag, `Tensor(b!)? range_flag` of the launch entry points).  Kernels on any
stream OR a sticky bit into it; those accesses are `ors`, unordered among themselves by design.  An `or` still conflicts with every plain
read (the step's overflow check) and every plain write (the pass's zero_()).  It is recognised by the tensor's identity, not by op name.

RECORDER.  recording() patches, for its own duration only: ops._dispatch (every okp launch: tensors, write annotations and the stream come
from the dispatcher schema), a TorchDispatchMode (aten ops on device tensors, on the current raw stream), torch's stream / event calls, and
CUDAGraph capture / replay (a replay is ONE access on the current stream that reads and writes what the capture's own records touched).

What the model cannot see: races inside a kernel; memory reached through plan handles (weights, the flag pointer a plan holds); whether
the runtime honours the recorded edges; the caching allocator handing one stream's cached block to another after a device-wide free."""
import contextlib
import dataclasses
import os
import sys

HOST_ORDERED = "host-ordered"        # synchronous at the call (or no device access at all): nothing is enqueued that could race
CURRENT_STREAM = "current-stream"    # launches on torch's current stream

# okp entry points that take tensors but no `stream` argument, with their treatment (tests/test_stream_order.py holds this table against
# every schema of torch.ops.okp).  The *_create entry points take HOST tensors (okp_torch.cpp: host_f32 refuses device ones).
NO_STREAM_OPS = {
    # okp_api.hip:284-370: the packed weights, bias, slices and patch steps go up with hipMemcpy (synchronous) into buffers the plan just allocated
    "conv_create": HOST_ORDERED,
    "conv_bn_create": HOST_ORDERED,     # fold_bn on the host, then conv_create (okp_api.hip:284-370)
    "fold_bn": HOST_ORDERED,            # host tensors in, host tensors out (okp_torch.cpp: fold_bn); no device work
    # okp_stem.hip:433-435 and 466-467: hipMemcpy (synchronous) of the fragment-order weights, bias and output scales at plan creation
    "stem_create": HOST_ORDERED,
    # okp_api.hip:378-382 / okp_stem.hip:476-480: stores the flag's ADDRESS in the plan; the word itself is not touched
    "conv_set_range_flag": HOST_ORDERED,
    "stem_set_range_flag": HOST_ORDERED,
    # okp_api.hip:560-564: select_tile() decides on the host from shapes, strides and pointer values; no device memory is read
    "conv_select_tile": HOST_ORDERED,
}


# ---- model ------------------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass
class Access:
    stream: int
    name: str
    reads: list = dataclasses.field(default_factory=list)
    writes: list = dataclasses.field(default_factory=list)
    ors: list = dataclasses.field(default_factory=list)
    where: str = ""


@dataclasses.dataclass
class Wait:
    waiter: int
    signaller: int
    where: str = ""


@dataclasses.dataclass
class EventRecord:
    event: int
    stream: int


@dataclasses.dataclass
class EventWait:
    stream: int
    event: int


@dataclasses.dataclass
class HostSync:
    stream: object = None        # None: all streams


@dataclasses.dataclass
class EventSync:
    event: int


@dataclasses.dataclass
class CaptureBegin:
    graph: int


@dataclasses.dataclass
class CaptureEnd:
    graph: int


def access(stream, name, reads=(), writes=(), ors=(), where=""):
    return Access(stream, name, list(reads), list(writes), list(ors), where)


def wait(waiter, signaller):
    return Wait(waiter, signaller)


def event_record(ev, stream):
    return EventRecord(ev, stream)


def event_wait(stream, ev):
    return EventWait(stream, ev)


def host_sync(stream=None):
    return HostSync(stream)


@dataclasses.dataclass
class Hazard:
    kind: str            # "RAW" (the later access reads what the earlier wrote), "WAR", "WAW"
    first: int           # index of the earlier access in the trace
    second: int
    first_name: str
    second_name: str
    first_stream: int
    second_stream: int
    lo: int
    hi: int
    first_where: str = ""
    second_where: str = ""

    def __str__(self):
        return (f"{self.kind} on bytes [{self.lo:#x}, {self.hi:#x}): #{self.first} {self.first_name} (stream {self.first_stream:#x}, {self.first_where}) "
                f"is not ordered before #{self.second} {self.second_name} (stream {self.second_stream:#x}, {self.second_where})")


def _overlap(a, b):
    for lo0, hi0 in a:
        for lo1, hi1 in b:
            lo, hi = max(lo0, lo1), min(hi0, hi1)
            if lo < hi:
                yield lo, hi


def _merge(clock, other):
    for k, v in other.items():
        if clock.get(k, 0) < v:
            clock[k] = v


def check(trace):
    """Every hazard of `trace`, in trace order of the later access.  Records between CaptureBegin and CaptureEnd are skipped: they were
    captured, not executed (capture_body() returns them for a check of their own)."""
    clocks = {}           # stream -> {stream: tick}
    host = {}             # what the host has waited for: merged into a stream's clock when something is next enqueued on it
    events = {}
    per_stream = {}       # stream -> [(index, Access)] in enqueue order; the entry at position t - 1 has tick t
    hazards = []
    capturing = 0

    def clock(s):
        c = clocks.setdefault(s, {})
        _merge(c, host)
        return c

    for i, r in enumerate(trace):
        if isinstance(r, CaptureBegin):
            capturing += 1
            continue
        if isinstance(r, CaptureEnd):
            capturing -= 1
            continue
        if capturing:
            continue
        if isinstance(r, Wait):
            _merge(clock(r.waiter), clock(r.signaller))
        elif isinstance(r, EventRecord):
            events[r.event] = dict(clock(r.stream))
        elif isinstance(r, EventWait):
            _merge(clock(r.stream), events.get(r.event, {}))
        elif isinstance(r, HostSync):
            for s in (list(clocks) if r.stream is None else [r.stream]):
                _merge(host, clocks.get(s, {}))
        elif isinstance(r, EventSync):
            _merge(host, events.get(r.event, {}))
        elif isinstance(r, Access):
            c = clock(r.stream)
            c[r.stream] = c.get(r.stream, 0) + 1
            for s, earlier in per_stream.items():
                if s == r.stream:
                    continue
                for j, a in earlier[c.get(s, 0):]:         # the accesses of stream s this one does NOT come after
                    a_w, r_w = a.writes + a.ors, r.writes + r.ors
                    found = []
                    found += [("RAW", lo, hi) for lo, hi in _overlap(a_w, r.reads)]
                    found += [("WAR", lo, hi) for lo, hi in _overlap(a.reads, r_w)]
                    found += [("WAW", lo, hi) for lo, hi in _overlap(a.writes, r_w)]
                    found += [("WAW", lo, hi) for lo, hi in _overlap(a.ors, r.writes)]      # (or against or: the one exemption)
                    for kind, lo, hi in found:
                        hazards.append(Hazard(kind, j, i, a.name, r.name, a.stream, r.stream, lo, hi, a.where, r.where))
            per_stream.setdefault(r.stream, []).append((i, r))
        else:
            raise TypeError(f"not a trace record: {r!r}")
    return hazards


def capture_body(trace, graph=None):
    """The records captured into `graph` (default: the first capture of the trace), as a trace of their own: its waits are the graph's edges."""
    out, inside = [], False
    for r in trace:
        if isinstance(r, CaptureBegin) and (graph is None or r.graph == graph) and not out:
            inside = True
        elif isinstance(r, CaptureEnd) and inside:
            return out
        elif inside:
            out.append(r)
    return out


def _union(ranges):
    out = []
    for lo, hi in sorted(ranges):
        if out and lo <= out[-1][1]:
            out[-1] = (out[-1][0], max(out[-1][1], hi))
        else:
            out.append((lo, hi))
    return out


def waits_of(trace):
    """[(index, waiter, signaller)] of the executed Wait records and of record + wait event pairs (LIGHT_EVENTS = False), captures skipped."""
    out, recorded, capturing = [], {}, 0
    for i, r in enumerate(trace):
        if isinstance(r, (CaptureBegin, CaptureEnd)):
            capturing += 1 if isinstance(r, CaptureBegin) else -1
        elif capturing:
            continue
        elif isinstance(r, Wait):
            out.append((i, r.waiter, r.signaller))
        elif isinstance(r, EventRecord):
            recorded[r.event] = r.stream
        elif isinstance(r, EventWait) and r.event in recorded:
            out.append((i, r.stream, recorded[r.event]))
    return out


# ---- recorder ---------------------------------------------------------------------------------------------------------------------
def tensor_range(t):
    """[lo, hi) bytes of a strided tensor: from its first element to one past its last."""
    span = 1 + sum((n - 1) * s for n, s in zip(t.shape, t.stride()))
    lo = t.data_ptr()
    return lo, lo + span * t.element_size()


def schema_of(fn):
    """The dispatcher schema of a launch entry point: of the torch.ops.okp packet itself, or - for a function of the ctypes twin - of the
    packet of the same name."""
    import torch
    if hasattr(fn, "default"):
        return fn.default._schema
    return getattr(torch.ops.okp, fn.__name__).default._schema


def schema_tensor_args(schema):
    """[(position, name, is_write)] of the arguments that can hold tensors (Tensor, Tensor?, Tensor[], Tensor?[])."""
    out = []
    for i, a in enumerate(schema.arguments):
        if "Tensor" in str(a.type):
            out.append((i, a.name, bool(a.alias_info is not None and a.alias_info.is_write)))
    return out


def _tensors(v):
    import torch
    if isinstance(v, torch.Tensor):
        return [v]
    if isinstance(v, (list, tuple)):
        return [t for t in v if isinstance(t, torch.Tensor)]
    return []


_PKG = os.sep + "object_keypoints_amd" + os.sep


def _where():
    """file:line of the innermost frame inside perception/ (backbone.py, pipeline.py, models.py), else of the innermost package frame."""
    f, fallback = sys._getframe(2), ""
    while f is not None:
        name = f.f_code.co_filename
        if _PKG in name:
            here = f"{os.path.basename(name)}:{f.f_lineno} {f.f_code.co_name}"
            if os.sep + "perception" + os.sep in name:
                return here
            fallback = fallback or here
        f = f.f_back
    return fallback


class Recorder:
    def __init__(self, flags=()):
        self.trace = []
        self.flags = list(flags)       # range-flag tensors known up front (next to ops._MODE.range_flag at the time of a launch)
        self.graphs = {}               # id(graph) -> (reads, writes, ors) of its capture
        self._open = {}                # id(graph) -> index of its CaptureBegin
        self._keep = []                # events and graphs seen: kept alive so that their id() stays theirs
        self._quiet = 0

    def _is_flag(self, t):
        from object_keypoints_amd import ops
        flags = self.flags + [getattr(ops._MODE, "range_flag", None)]
        return any(f is not None and f.data_ptr() == t.data_ptr() for f in flags)

    # -- okp launches
    def dispatch(self, original):
        def _dispatch(fn, *args):
            out = original(fn, *args)
            self.okp(fn, args)
            return out
        return _dispatch

    def okp(self, fn, args):
        from object_keypoints_amd import ops
        schema = schema_of(fn)
        name = schema.name.split("::")[-1]
        if name == "stream_wait_stream":
            self.trace.append(Wait(int(args[0]), int(args[1]), _where()))
            return
        tensor_args = schema_tensor_args(schema)
        names = [a.name for a in schema.arguments]
        if "stream" in names:
            stream = int(args[names.index("stream")])
        elif not tensor_args:
            return
        elif NO_STREAM_OPS[name] == HOST_ORDERED:         # (KeyError: an entry point the table does not know - add it with its justification)
            return
        else:
            stream = ops.stream_int()
        acc = Access(stream, "okp." + name, where=_where())
        for i, _, is_write in tensor_args:
            for t in _tensors(args[i]) if i < len(args) else []:
                if not t.is_cuda or t.numel() == 0:
                    continue
                if is_write and self._is_flag(t):
                    acc.ors.append(tensor_range(t))
                else:
                    (acc.writes if is_write else acc.reads).append(tensor_range(t))
        self.trace.append(acc)

    # -- aten ops
    def aten(self, func, args, kwargs, out):
        import torch
        from torch.utils._pytree import tree_flatten
        schema = func._schema
        reads, writes, devices, host_in, inputs = [], [], [], False, set()
        bound = list(zip(schema.arguments, args)) + [(a, kwargs[a.name]) for a in schema.arguments if a.name in kwargs]
        for a, v in bound:
            is_write = a.alias_info is not None and a.alias_info.is_write
            for t in _tensors(v):
                if not t.is_cuda:
                    host_in = True
                    continue
                devices.append(t.device)
                inputs.add(t.untyped_storage().data_ptr())
                if t.numel():
                    (writes if is_write else reads).append(tensor_range(t))
        host_out = False
        for t in tree_flatten(out)[0]:
            if not isinstance(t, torch.Tensor):
                continue
            if not t.is_cuda:
                host_out = True
                continue
            devices.append(t.device)
            if t.untyped_storage().data_ptr() not in inputs and t.numel():       # owns fresh storage: this op wrote it
                writes.append(tensor_range(t))
        if not devices:
            return
        name = schema.name.split("::")[-1]
        to_host = (bool(reads) and host_out) or name == "_local_scalar_dense" or (name == "copy_" and host_in and not args[0].is_cuda)
        if not reads and not writes:
            return                                         # a view, or nothing but empty tensors
        stream = int(torch._C._cuda_getCurrentRawStream(devices[0].index))
        self.trace.append(Access(stream, "aten." + name, reads, writes, [], _where()))
        if to_host and not kwargs.get("non_blocking", False):
            self.trace.append(HostSync(stream))           # the host blocks on a device -> host copy

    # -- graphs
    def capture_begin(self, graph):
        self._keep.append(graph)
        self._open[id(graph)] = len(self.trace)
        self.trace.append(CaptureBegin(id(graph)))

    def capture_end(self, graph):
        body = self.trace[self._open.pop(id(graph)) + 1:]
        acc = [r for r in body if isinstance(r, Access)]
        self.graphs[id(graph)] = tuple(_union([x for a in acc for x in getattr(a, k)]) for k in ("reads", "writes", "ors"))
        self.trace.append(CaptureEnd(id(graph)))

    def replay(self, graph):
        import torch
        reads, writes, ors = self.graphs.get(id(graph), ([], [], []))
        stream = int(torch._C._cuda_getCurrentRawStream(torch.cuda.current_device()))
        self.trace.append(Access(stream, "graph.replay", list(reads), list(writes), list(ors), _where()))


@contextlib.contextmanager
def recording(flags=()):
    """with recording() as rec: ... ; rec.trace is the trace of everything launched inside.  Patches are undone on exit."""
    import torch
    from torch.utils._python_dispatch import TorchDispatchMode
    from object_keypoints_amd import ops
    rec = Recorder(flags)

    class Mode(TorchDispatchMode):
        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            kwargs = kwargs or {}
            out = func(*args, **kwargs)
            rec.aten(func, args, kwargs, out)
            return out

    S, E, G = torch.cuda.Stream, torch.cuda.Event, torch.cuda.CUDAGraph
    saved = [(ops, "_dispatch", ops._dispatch), (S, "wait_stream", S.wait_stream), (S, "wait_event", S.wait_event), (S, "synchronize", S.synchronize),
             (E, "record", E.record), (E, "wait", E.wait), (E, "synchronize", E.synchronize), (torch.cuda, "synchronize", torch.cuda.synchronize),
             (G, "capture_begin", G.capture_begin), (G, "capture_end", G.capture_end), (G, "replay", G.replay)]
    orig = {(o, n): f for o, n, f in saved}

    def outermost(owner, name, note):
        """Replace owner.name: `note(*args)` appends to the trace, unless the call is made from inside another patched call (torch's
        wait_stream is record_event + wait_event: one edge, not three)."""
        f = orig[(owner, name)]

        def patched(*a, **k):
            if rec._quiet == 0:
                note(*a, **k)
            rec._quiet += 1
            try:
                return f(*a, **k)
            finally:
                rec._quiet -= 1
        setattr(owner, name, patched)

    def current():
        return torch.cuda.current_stream()

    def ev(e):
        rec._keep.append(e)
        return id(e)

    ops._dispatch = rec.dispatch(ops._dispatch)
    outermost(S, "wait_stream", lambda self, stream: rec.trace.append(Wait(self.cuda_stream, stream.cuda_stream, _where())))
    outermost(S, "wait_event", lambda self, event: rec.trace.append(EventWait(self.cuda_stream, ev(event))))
    outermost(S, "synchronize", lambda self: rec.trace.append(HostSync(self.cuda_stream)))
    outermost(E, "record", lambda self, stream=None: rec.trace.append(EventRecord(ev(self), (stream if stream is not None else current()).cuda_stream)))
    outermost(E, "wait", lambda self, stream=None: rec.trace.append(EventWait((stream if stream is not None else current()).cuda_stream, ev(self))))
    outermost(E, "synchronize", lambda self: rec.trace.append(EventSync(ev(self))))
    outermost(torch.cuda, "synchronize", lambda device=None: rec.trace.append(HostSync(None)))
    outermost(G, "capture_begin", lambda self, *a, **k: rec.capture_begin(self))
    outermost(G, "capture_end", lambda self: rec.capture_end(self))
    outermost(G, "replay", lambda self: rec.replay(self))
    try:
        with Mode():
            yield rec
    finally:
        for owner, name, f in saved:
            setattr(owner, name, f)
