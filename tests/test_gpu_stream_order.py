"""Stream-ordering audit of the forked step on the device (tests/stream_order.py: model and recorder; tests/test_stream_order.py: the
model on hand-written traces).  Every scenario records ONE run of the real orchestration - hg_module.forward's forks and joins, its pinned
branch outputs, HostFrameFeed's copy stream and events, CapturedStep.replay - and asserts that no two conflicting accesses of the trace
are unordered, and that the trace is not vacuous.  Nothing here depends on the GPU's timing: a missing edge fails on the first run."""
import numpy as np
import pytest
import torch

import stream_order as so
from test_gpu_bench_shapes import CALIB, _frames, _net

pytestmark = pytest.mark.gpu

_NETS = {}
_TRACES = {}
# Waits of the eager bf16 trace that the model finds redundant, by position (stack, hg_module level n, "fork" | "join"): see
# test_every_recorded_wait_is_load_bearing and docs/EXPERIMENTS.md.
REDUNDANT_WAITS = set()


def net_of(dtype):
    from object_keypoints_amd import _lib
    assert _lib.torch_ops() is not None
    if dtype not in _NETS:
        _NETS[dtype] = _net(dtype)
    return _NETS[dtype]


class Levels:
    """Counts the hg_module levels that fork (one _side_stream call each) and the extent of every hg_module.forward in the trace."""

    def __init__(self, monkeypatch, rec):
        from object_keypoints_amd.perception import backbone as bb
        self.entries, self.extents, self.rec = [], [], rec         # (trace position, n, key, raw side stream), (begin, end, n)
        side_stream, forward = bb.hg_module._side_stream, bb.hg_module.forward

        def counted(mod, device):
            key, st = side_stream(mod, device)
            self.entries.append((len(rec.trace), mod.n, key, st.cuda_stream))
            return key, st

        def spanned(mod, x, out_pairs=False):
            begin = len(rec.trace)
            try:
                return forward(mod, x, out_pairs=out_pairs)
            finally:
                self.extents.append((begin, len(rec.trace), mod.n))

        monkeypatch.setattr(bb.hg_module, "_side_stream", counted)
        monkeypatch.setattr(bb.hg_module, "forward", spanned)

    def position(self, index):
        """(stack, level n, "fork" | "join") of the wait at trace index `index` (stack: counted over the executed outermost levels)."""
        forks = {e[0]: e for e in self.entries}
        inside = [x for x in self.extents if x[0] <= index < x[1]]
        begin, _, n = max(inside, key=lambda x: x[0])
        outer = sorted(x[0] for x in self.extents if x[2] == 4)
        stack = sum(1 for b in outer if b <= index) - 1
        return stack % 2, n, "fork" if index in forks else "join"


def captured_spans(trace):
    spans, begin = [], None
    for i, r in enumerate(trace):
        if isinstance(r, so.CaptureBegin):
            begin = i
        elif isinstance(r, so.CaptureEnd):
            spans.append((begin, i))
    return spans


def assert_not_vacuous(trace, entries, offset=0):
    """Forks = levels entered, at least one join per stack, work on every side stream.  `entries`: the Levels entries that belong to
    `trace` (offset: the position of trace[0] in the recording)."""
    assert entries and len(entries) % 8 == 0, len(entries)                      # two stacks of four levels per network pass
    sides, mains = {e[3] for e in entries}, {e[2][2] for e in entries}
    waits = so.waits_of(trace)
    forks = [w for w in waits if w[1] in sides and w[2] in mains]
    joins = [w for w in waits if w[1] in mains and w[2] in sides]
    assert len(forks) == len(entries), (len(forks), len(entries))
    assert sorted(w[0] + offset for w in forks) == sorted(e[0] for e in entries)      # each fork is the first record of its level
    assert len(joins) >= len(entries) // 4, (len(joins), len(entries))
    spans = captured_spans(trace)
    for s in sides:
        assert sum(1 for i, r in enumerate(trace) if isinstance(r, so.Access) and r.stream == s and not any(b < i < e for b, e in spans)) > 0, hex(s)
    return forks, joins


def executed(entries, trace):
    spans = captured_spans(trace)
    return [e for e in entries if not any(b < e[0] <= e_ for b, e_ in spans)]


def report(hazards):
    return "\n".join(str(h) for h in hazards[:20]) + (f"\n... {len(hazards)} hazards" if len(hazards) > 20 else "")


def eager_trace(dtype, light):
    """Two eager passes of 8 frames (ops.SIDE_MIN_BATCH: the smallest batch that forks) back to back, no host sync in between."""
    from object_keypoints_amd import ops
    if (dtype, light) not in _TRACES:
        net = net_of(dtype)
        x = _frames(8)
        assert ops.SIDE_STREAMS and x.shape[0] == ops.SIDE_MIN_BATCH
        with pytest.MonkeyPatch.context() as mp, torch.no_grad():
            mp.setattr(ops, "LIGHT_EVENTS", light)
            net.deployed(x, check_range=False)                                  # plans and allocator pools exist
            torch.cuda.synchronize()
            with so.recording() as rec:
                levels = Levels(mp, rec)
                a = [t.clone() for t in net.deployed(x, check_range=False)]
                b = net.deployed(x, check_range=False)
            torch.cuda.synchronize()
            assert all(torch.equal(u, v) for u, v in zip(a, b))
        _TRACES[(dtype, light)] = (rec.trace, levels)
    return _TRACES[(dtype, light)]


@pytest.mark.parametrize("light", [True, False], ids=["light_events", "torch_events"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, "float32x3", "float32mix", torch.float32], ids=str)
def test_eager_network_two_passes_back_to_back(dtype, light):
    """(a) The second pass reuses the side streams' pools and clears the pinned branch outputs of the first while its merges may still run."""
    trace, levels = eager_trace(dtype, light)
    hazards = so.check(trace)
    assert hazards == [], report(hazards)
    forks, joins = assert_not_vacuous(trace, levels.entries)
    assert len(forks) == 16
    assert not any(isinstance(r, so.HostSync) for r in trace[:forks[-1][0]])    # back to back: the host never waited
    assert len([r for r in trace if isinstance(r, so.Wait)]) == len(forks) + len(joins)      # okp_stream_wait_stream or torch's wait_stream: one edge each


def test_every_recorded_wait_is_load_bearing():
    """(f) Teeth on the real trace: the bf16 trace of (a) with each wait removed in turn (the trace is mutated, never the launches) has at
    least one hazard - except the waits listed by position in REDUNDANT_WAITS."""
    trace, levels = eager_trace(torch.bfloat16, True)
    assert so.check(trace) == []
    waits = so.waits_of(trace)
    assert len(waits) >= 16 + 4
    idle = set()
    for i, waiter, signaller in waits:
        found = so.check(trace[:i] + trace[i + 1:])
        print(levels.position(i), "waiter %#x signaller %#x:" % (waiter, signaller), len(found), "hazards without it;", str(found[0]) if found else "")
        if not found:
            idle.add(levels.position(i))
    assert idle == REDUNDANT_WAITS, f"waits that order nothing under the model: {sorted(idle)}; listed: {sorted(REDUNDANT_WAITS)}"


@pytest.mark.parametrize("dtype", [torch.bfloat16, "float32mix"], ids=str)
def test_captured_step_at_batch64_with_side_streams(dtype, monkeypatch):
    """(b) The configuration of the open failure: eager step, capture, eager step, two replays.  The capture's own records - its waits are
    the graph's edges - and the whole sequence, replays as one access over everything the capture touched."""
    from object_keypoints_amd.perception import pipeline as pp
    from object_keypoints_amd.perception.utils import camera_utils as cu
    from oracle import pipeline as op
    net = net_of(dtype)
    cam_o = op.eval_camera(CALIB)
    pipe = pp.BatchedKeypointPipeline(net, {"keypoint_config": [1, 3]}, cu.FisheyeCamera(cam_o.K, cam_o.D, cam_o.image_size), capacity=128)
    x0, x1 = _frames(64, seed=1), _frames(64, seed=2)
    monkeypatch.setattr(pp, "GRAPH_SIDE_STREAMS", True)
    torch.cuda.synchronize()
    with so.recording() as rec, torch.no_grad():
        levels = Levels(monkeypatch, rec)
        pipe.forward_device(x0)
        step = pipe.capture(x0)
        eager = pipe.forward_device(x1)
        step.replay(x1)
        out = step.replay(x1)
    torch.cuda.synchronize()
    for key in ("heat", "count", "xyc"):
        assert torch.equal(out[key], eager[key]), key
    trace = rec.trace
    (begin, end), = captured_spans(trace)
    body = so.capture_body(trace)
    assert body == trace[begin + 1:end] and not any(isinstance(r, (so.HostSync, so.EventSync)) for r in body)
    hazards = so.check(body)
    assert hazards == [], "inside the capture:\n" + report(hazards)
    assert_not_vacuous(body, [e for e in levels.entries if begin < e[0] <= end], offset=begin + 1)
    hazards = so.check(trace)
    assert hazards == [], report(hazards)
    assert_not_vacuous(trace, executed(levels.entries, trace))
    replays = [r for r in trace if isinstance(r, so.Access) and r.name == "graph.replay"]
    assert len(replays) == 2 and all(r.reads and r.writes for r in replays)
    lo, hi = so.tensor_range(step.static_in)
    assert any(a <= lo and hi <= b for a, b in replays[0].reads)                # the static input is part of the replay's footprint


@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
def test_host_fed_stream_over_four_ticks(use_graph, monkeypatch):
    """(c) StereoStreamPipeline.stream: the copy stream, ready / done events and release-before-overwrite on both slots of the feed."""
    from object_keypoints_amd.perception import pipeline as pp
    from object_keypoints_amd.perception.utils import camera_utils as cu
    from oracle import geometry as og
    p = og.load_calibration_params(CALIB)
    offset = np.array([(511 / 720 * 1280 - 511.0) / 2.0, 0.0])
    mk = lambda K, D: cu.FisheyeCamera(K, D, p["image_size"]).scale(511 / 720).cut(offset).scale(64 / 511)
    stereo = cu.StereoCamera(mk(p["K"], p["D"]), mk(p["Kp"], p["Dp"]), p["T_RL"])
    net = net_of(torch.float16)
    pipe = pp.StereoStreamPipeline(net, stereo, {"keypoint_config": [1, 3]}, capacity=4096, max_distance=1.5)
    rng = np.random.default_rng(12)
    hosts = [torch.from_numpy(rng.integers(0, 256, (8, 240, 320, 3), dtype=np.uint8)).pin_memory() for _ in range(4)]
    main = torch.cuda.current_stream().cuda_stream
    with so.recording() as rec:
        levels = Levels(monkeypatch, rec)
        if use_graph:
            pipe.capture(hosts[0].cuda())
        ticks = list(pipe.stream(iter(hosts), use_graph=use_graph))
    torch.cuda.synchronize()
    assert len(ticks) == 4
    trace = rec.trace
    hazards = so.check(trace)
    assert hazards == [], report(hazards)
    ran = executed(levels.entries, trace)
    assert len(ran) == (16 if use_graph else 32)                                 # the two warm-up passes of the capture, or four eager ticks
    assert_not_vacuous(trace, ran)
    sides = {e[3] for e in levels.entries}
    spans = captured_spans(trace)
    live = [r for i, r in enumerate(trace) if not any(b < i < e for b, e in spans)]
    uploads = [r for r in live if isinstance(r, so.Access) and r.stream not in sides | {main} and r.name == "aten.copy_"]
    assert len(uploads) == 4 and len({r.stream for r in uploads}) == 1 and len({r.writes[0] for r in uploads}) == 2      # two slots, each filled twice
    copy = uploads[0].stream
    assert sum(1 for r in trace if isinstance(r, so.EventWait) and r.stream == copy) == 2             # ticks 2 and 3 wait for `done`
    assert sum(1 for r in trace if isinstance(r, so.EventWait) and r.stream == main) == 4             # acquire
    assert sum(1 for r in trace if isinstance(r, so.EventRecord) and r.stream == main) == 4           # release
    if use_graph:
        assert sum(1 for r in trace if isinstance(r, so.Access) and r.name == "graph.replay" and r.reads) == 4
    # the copy stream starts behind the stream whose pool the buffers came from (HostFrameFeed.__init__): without that edge the first upload
    # into each slot is unordered against the previous owner of the block, which the model sees as the allocation itself
    first = next(i for i, r in enumerate(trace) if r is uploads[0])
    start = [i for i, w, s in so.waits_of(trace) if (w, s) == (copy, main) and i < first]
    assert len(start) == 1
    found = so.check(trace[:start[0]] + trace[start[0] + 1:])
    assert len(found) == 2 and {(h.kind, h.first_name, h.second_name) for h in found} == {("WAW", "aten.empty", "aten.copy_")}
    # teeth: without acquire's waits a tick reads frames that may still be crossing PCIe.  (tick() reads its results on the host, so under
    # the model the `done` waits of THIS loop order nothing the host has not ordered already: tests/test_stream_order.py plants that defect.)
    cut = [r for r in trace if not (isinstance(r, so.EventWait) and r.stream == main)]
    found = so.check(cut)
    assert {h.kind for h in found} >= {"RAW"} and {h.first_name for h in found if h.kind == "RAW"} == {"aten.copy_"}


def test_launch_that_raises_between_fork_and_join(monkeypatch):
    """(d) A Python exception (no GPU fault) in the low path of the outermost level: the finally clause joins, so the main stream waits for
    the branch before anything it does afterwards, and the next pass is clean."""
    from object_keypoints_amd import ops
    from object_keypoints_amd.perception import pipeline as pp
    net = net_of(torch.bfloat16)
    x = _frames(8)
    main = torch.cuda.current_stream().cuda_stream

    def planted(*a, **k):
        raise pp.OkpError("planted: raised before any launch")

    with torch.no_grad():
        net.deployed(x)
        torch.cuda.synchronize()
        with so.recording() as rec:
            levels = Levels(monkeypatch, rec)
            with monkeypatch.context() as mp:
                mp.setattr(net.backbone.hgs[0].low1[0], "forward", planted)
                with pytest.raises(pp.OkpError, match="planted"):
                    net.deployed(x)
            cut = len(rec.trace)
            net.deployed(x)
        torch.cuda.synchronize()
    trace = rec.trace
    assert len(levels.entries) == 1 + 8 and levels.entries[0][1] == 4            # the failing pass forked once, at the outermost level
    side = levels.entries[0][3]
    branch = [i for i, r in enumerate(trace[:cut]) if isinstance(r, so.Access) and r.stream == side]
    assert branch, "the branch was enqueued before the low path raised"
    after = next(i for i, r in enumerate(trace) if i > branch[-1] and isinstance(r, so.Access) and r.stream == main)
    assert after >= cut
    joins = [i for i, w, s in so.waits_of(trace) if branch[-1] < i < after and (w, s) == (main, side)]
    assert len(joins) == 1 and joins[0] < cut, "main must wait for the side stream before its next access"
    hazards = so.check(trace)
    assert hazards == [], report(hazards)
    # the join is what keeps it clean: the failing pass's input outlives the branch only through it
    assert so.check(trace[:joins[0]] + trace[joins[0] + 1:]) != []
    assert_not_vacuous(trace[cut:], levels.entries[1:], offset=cut)


def test_two_main_streams_interleaved():
    """(e) Passes on a user stream, their input produced on that stream, between passes on the default stream: no hazard, and the two
    main streams use disjoint side-stream entries (torch may hand out pooled handles that coincide)."""
    net = net_of(torch.bfloat16)
    x0 = _frames(8)
    user = torch.cuda.Stream()
    with torch.no_grad():
        net.deployed(x0)
        torch.cuda.synchronize()
        with pytest.MonkeyPatch.context() as mp, so.recording() as rec:
            levels = Levels(mp, rec)
            with torch.cuda.stream(user):
                x1 = torch.randn((8, 3, 511, 511), device="cuda", dtype=torch.float32)
                a1 = net.deployed(x1)
            b0 = net.deployed(x0)
            with torch.cuda.stream(user):
                a2 = net.deployed(x1)
            b1 = net.deployed(x0)
        torch.cuda.synchronize()
    assert all(torch.equal(u, v) for u, v in zip(a1, a2)) and all(torch.equal(u, v) for u, v in zip(b0, b1))
    trace = rec.trace
    hazards = so.check(trace)
    assert hazards == [], report(hazards)
    assert_not_vacuous(trace, levels.entries)
    default = torch.cuda.default_stream().cuda_stream
    keys = {m: {e[2] for e in levels.entries if e[2][2] == m} for m in (default, user.cuda_stream)}
    assert user.cuda_stream != default and len(keys[default]) == len(keys[user.cuda_stream]) == 3 and not keys[default] & keys[user.cuda_stream]
    assert len(levels.entries) == 32 and {e[2][2] for e in levels.entries} == {default, user.cuda_stream}
    assert sum(1 for r in trace if isinstance(r, so.Access) and r.stream == user.cuda_stream) > 100
