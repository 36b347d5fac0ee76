"""The stream-ordering model (tests/stream_order.py) on hand-written traces - the orderings hg_module.forward, HostFrameFeed and
CapturedStep.replay rely on are clean, each planted defect is reported as the right kind on the right pair -, the choke point the recorder
hooks (every launch of ops.py goes through _dispatch), and the recorder's reading of the dispatcher schemas.  No GPU needed."""
import ast
import glob
import os
import re

import pytest

import stream_order as so
from stream_order import access, check, event_record, event_wait, host_sync, wait

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M, S, C, U = 0, 0x51de, 0xc0b1, 0x05e2          # main, side, copy and a user stream
B = {name: (4096 * i, 4096 * i + 1000) for i, name in enumerate(
    ["x", "up1", "low", "out", "x_in", "up1_in", "low_in", "merged_in", "low_out", "b0", "b1", "static_in", "static_out", "flag", "maps"])}


def pairs(hazards):
    return sorted({(h.kind, h.first_name, h.second_name) for h in hazards})


def without(trace, name=None, index=None):
    """The trace with one record left out: the index-th (or only) wait / record named `name`."""
    hits = [i for i, r in enumerate(trace) if (getattr(r, "name", None) == name if name else isinstance(r, so.Wait))]
    drop = hits[index if index is not None else 0]
    assert index is not None or len(hits) == 1
    return trace[:drop] + trace[drop + 1:]


# ---- fork -> branch -> join -> merge ------------------------------------------------------------------------------------------------
def level():
    return [access(M, "produce x", writes=[B["x"]]),
            wait(S, M),                                                              # fork
            access(S, "up1", reads=[B["x"]], writes=[B["up1"]]),
            access(M, "low path", reads=[B["x"]], writes=[B["low"]]),
            wait(M, S),                                                              # join
            access(M, "merge", reads=[B["low"], B["up1"]], writes=[B["out"]])]


def test_fork_branch_join_merge_is_clean():
    assert check(level()) == []
    assert check(level() + [wait(S, M)] + level()[2:]) == []       # the next fork orders the branch's rewrite of up1 behind the merge


def test_no_fork_wait_is_a_raw_on_x():
    hz = check(without(level(), index=0))
    assert pairs(hz) == [("RAW", "produce x", "up1")]
    h = hz[0]
    assert (h.lo, h.hi) == B["x"] and (h.first, h.second) == (0, 1) and (h.first_stream, h.second_stream) == (M, S)
    assert "RAW" in str(h) and "produce x" in str(h) and "up1" in str(h) and "#0" in str(h) and "#1" in str(h)


def test_no_join_is_a_raw_on_up1():
    hz = check(without(level(), index=1))
    assert pairs(hz) == [("RAW", "up1", "merge")]
    assert (hz[0].lo, hz[0].hi) == B["up1"] and (hz[0].first, hz[0].second) == (2, 4)


def test_branch_output_rewritten_without_a_fork_wait_is_a_war_against_the_merge():
    nxt = access(S, "next up1", reads=[B["out"]], writes=[B["up1"]])           # the allocator hands the freed block to the next branch
    hz = check(level() + [nxt])
    assert ("WAR", "merge", "next up1") in pairs(hz)
    war = [h for h in hz if h.kind == "WAR"]
    assert len(war) == 1 and (war[0].lo, war[0].hi) == B["up1"] and (war[0].first, war[0].second) == (5, 6)
    assert check(level() + [wait(S, M), nxt]) == []


# ---- nested levels on one side stream, outer join skipped (_SIDE_SEQ / _JOINED_SEQ) -------------------------------------------------
def nested(inner_first=False):
    outer_branch = access(S, "outer up1", reads=[B["x"]], writes=[B["up1"]])
    inner = [wait(S, M),                                                             # inner fork
             access(S, "inner up1", reads=[B["x_in"]], writes=[B["up1_in"]]),
             access(M, "inner low path", reads=[B["x_in"]], writes=[B["low_in"]]),
             wait(M, S),                                                             # inner join: covers what the side stream holds so far
             access(M, "inner merge", reads=[B["low_in"], B["up1_in"]], writes=[B["merged_in"]])]
    return ([access(M, "produce x", writes=[B["x"]]), wait(S, M)]                    # outer fork
            + ([] if inner_first else [outer_branch])
            + [access(M, "low1", reads=[B["x"]], writes=[B["x_in"]])]
            + inner
            + ([outer_branch] if inner_first else [])                                # (defect: enqueued after the join that was to cover it)
            + [access(M, "low3", reads=[B["merged_in"]], writes=[B["low_out"]]),
               access(M, "outer merge", reads=[B["low_out"], B["up1"]], writes=[B["out"]])])     # outer join skipped


def test_nested_levels_sharing_a_side_stream_with_the_outer_join_skipped_are_clean():
    assert check(nested()) == []


def test_outer_join_skipped_although_the_inner_branch_came_first_is_a_raw():
    hz = check(nested(inner_first=True))
    assert pairs(hz) == [("RAW", "outer up1", "outer merge")]
    assert (hz[0].lo, hz[0].hi) == B["up1"]


def test_inner_fork_wait_is_needed_for_the_inner_input():
    assert pairs(check(without(nested(), index=1))) == [("RAW", "low1", "inner up1")]


# ---- two-slot feed over four ticks (HostFrameFeed) ------------------------------------------------------------------------------------
def feed(ticks=4, early_release=False):
    trace, done = [], {}
    ready = {0: "ready0", 1: "ready1"}

    def submit(t):
        slot = t % 2
        if slot in done:
            trace.append(event_wait(C, done[slot]))
        trace.append(access(C, f"upload {t}", writes=[B[f"b{slot}"]]))
        trace.append(event_record(ready[slot], C))

    submit(0)
    for t in range(ticks):
        slot = t % 2
        trace.append(event_wait(M, ready[slot]))                                      # acquire
        if t + 1 < ticks:
            submit(t + 1)
        compute = access(M, f"tick {t}", reads=[B[f"b{slot}"]], writes=[B["maps"]])
        release = event_record(f"done{t}", M)
        trace.extend([release, compute] if early_release else [compute, release])
        done[slot] = f"done{t}"
    return trace


def test_two_slot_feed_over_four_ticks_is_clean():
    assert check(feed()) == []


def test_release_before_the_ticks_last_reader_is_a_war_on_the_feed_buffer():
    hz = check(feed(early_release=True))
    assert pairs(hz) == [("WAR", "tick 0", "upload 2"), ("WAR", "tick 1", "upload 3")]
    assert {(h.lo, h.hi) for h in hz} == {B["b0"], B["b1"]}
    assert all((h.first_stream, h.second_stream) == (M, C) for h in hz)


def test_an_upload_without_acquire_is_a_raw():
    t = feed(ticks=2)
    first_acquire = next(i for i, r in enumerate(t) if isinstance(r, so.EventWait) and r.stream == M)
    assert pairs(check(t[:first_acquire] + t[first_acquire + 1:])) == [("RAW", "upload 0", "tick 0")]


# ---- replays ------------------------------------------------------------------------------------------------------------------------
def test_static_input_rewritten_on_another_stream_under_a_replay_is_a_war():
    replay = access(M, "graph.replay", reads=[B["static_in"]], writes=[B["static_out"]])
    trace = [access(M, "copy_ static_in", writes=[B["static_in"]]), replay, access(U, "copy_ static_in (next)", writes=[B["static_in"]])]
    hz = check(trace)
    assert ("WAR", "graph.replay", "copy_ static_in (next)") in pairs(hz) and ("WAW", "copy_ static_in", "copy_ static_in (next)") in pairs(hz)
    war = [h for h in hz if h.kind == "WAR"][0]
    assert (war.lo, war.hi) == B["static_in"] and (war.first, war.second) == (1, 2)
    assert check(trace[:2] + [wait(U, M)] + trace[2:]) == []
    assert check([trace[0], replay, access(M, "copy_ static_in (next)", writes=[B["static_in"]]), replay]) == []      # one stream: ordered


def test_captured_records_are_not_executed_and_make_the_replays_footprint():
    body = [wait(S, C), access(S, "up1", reads=[B["x"]], writes=[B["up1"]]), wait(C, S), access(C, "merge", reads=[B["up1"]], writes=[B["out"]])]
    trace = [access(M, "produce x", writes=[B["x"]]), host_sync(None), so.CaptureBegin(1)] + body + [so.CaptureEnd(1)]
    assert check(trace) == [] and so.capture_body(trace) == body and check(body) == []
    assert pairs(check([body[1], body[3]])) == [("RAW", "up1", "merge")]                          # the body without its edges
    assert pairs(check(trace[:1] + trace[2:] + [access(U, "reader", reads=[B["x"]])])) == [("RAW", "produce x", "reader")]     # (no host sync)
    assert so.waits_of(trace) == []


# ---- the one exemption: the range flag --------------------------------------------------------------------------------------------------
def flagged(join=True):
    return ([access(M, "zero_", writes=[B["flag"]]), wait(S, M),
             access(S, "cast", reads=[B["x"]], writes=[B["up1"]], ors=[B["flag"]]),
             access(M, "conv", reads=[B["x"]], writes=[B["low"]], ors=[B["flag"]])]
            + ([wait(M, S)] if join else [])
            + [access(M, "capacity_overflow", reads=[B["flag"]], writes=[B["out"]])])


def test_sticky_bit_writers_on_two_streams_are_exempt_among_themselves_only():
    assert check(flagged()) == []
    hz = check(flagged(join=False))
    assert pairs(hz) == [("RAW", "cast", "capacity_overflow")] and (hz[0].lo, hz[0].hi) == B["flag"]
    assert pairs(check(without(flagged(), index=0))) == [("WAW", "zero_", "cast")]                 # the pass's zero_() is no sticky-bit writer
    late_zero = flagged() + [wait(S, M), access(S, "cast", ors=[B["flag"]]), access(M, "zero_", writes=[B["flag"]])]
    assert pairs(check(late_zero)) == [("WAW", "cast", "zero_")]
    plain = [access(M, "a", writes=[B["flag"]]), access(S, "b", writes=[B["flag"]])]               # the same bytes without the `or` kind: a hazard
    assert pairs(check(plain)) == [("WAW", "a", "b")]


# ---- host syncs -----------------------------------------------------------------------------------------------------------------------
def test_host_syncs_order_what_follows_them_and_nothing_else():
    w, r = access(S, "w", writes=[B["x"]]), access(M, "r", reads=[B["x"]])
    assert pairs(check([w, r])) == [("RAW", "w", "r")]
    assert check([w, host_sync(S), r]) == [] and check([w, host_sync(None), r]) == []
    assert pairs(check([w, host_sync(M), r])) == [("RAW", "w", "r")]                               # the wrong stream drained
    assert pairs(check([host_sync(S), w, r])) == [("RAW", "w", "r")]                               # ... or too early
    assert check([w, event_record("e", S), so.EventSync("e"), r]) == []
    assert pairs(check([event_record("e", S), w, so.EventSync("e"), r])) == [("RAW", "w", "r")]
    assert pairs(check([w, event_record("e", S), access(S, "w2", writes=[B["x"]]), event_wait(M, "e"), r])) == [("RAW", "w2", "r")]
    with pytest.raises(TypeError):
        check([("not", "a", "record")])


# ---- the choke point: every launch goes through _dispatch ----------------------------------------------------------------------------
def _launch_sites(path):
    """(sites, stray): attribute reads on the binding - `_ops().x`, `B.x` for a B bound to `_ops()`, getattr(_ops(), ...) - that are the
    first argument of a _dispatch(...) call (through a conditional expression), and those that are anything else."""
    tree = ast.parse(open(path).read(), path)
    parent = {c: p for p in ast.walk(tree) for c in ast.iter_child_nodes(p)}
    is_ops_call = lambda n: isinstance(n, ast.Call) and ((isinstance(n.func, ast.Name) and n.func.id == "_ops")
                                                         or (isinstance(n.func, ast.Attribute) and n.func.attr == "_ops"))
    is_dispatch = lambda n: isinstance(n, ast.Call) and ((isinstance(n.func, ast.Name) and n.func.id == "_dispatch")
                                                         or (isinstance(n.func, ast.Attribute) and n.func.attr == "_dispatch"))

    def scope(n):
        while n in parent and not isinstance(n, (ast.FunctionDef, ast.Lambda, ast.Module)):
            n = parent[n]
        return n

    bound = set()                # (scope, name) of `name = _ops()`
    for n in ast.walk(tree):
        if isinstance(n, ast.Assign) and is_ops_call(n.value) and len(n.targets) == 1 and isinstance(n.targets[0], ast.Name):
            bound.add((scope(n), n.targets[0].id))
    sites, stray = [], []
    for n in ast.walk(tree):
        entry = None
        if isinstance(n, ast.Attribute) and (is_ops_call(n.value) or (isinstance(n.value, ast.Name) and (scope(n), n.value.id) in bound)):
            entry = n
        elif isinstance(n, ast.Call) and isinstance(n.func, ast.Name) and n.func.id == "getattr" and n.args and is_ops_call(n.args[0]):
            entry = n
        elif is_ops_call(n):     # the binding itself: only as the value of such an attribute, of such a getattr, or of `B = _ops()`
            p = parent[n]
            ok = ((isinstance(p, ast.Attribute) and p.value is n) or (isinstance(p, ast.Call) and isinstance(p.func, ast.Name) and p.func.id == "getattr" and p.args[0] is n)
                  or (isinstance(p, ast.Assign) and isinstance(p.targets[0], ast.Name)))
            if not ok:
                stray.append((path, n.lineno))
        elif isinstance(n, ast.Name) and isinstance(n.ctx, ast.Load) and (scope(n), n.id) in bound and not (isinstance(parent[n], ast.Attribute) and parent[n].value is n):
            stray.append((path, n.lineno))
        if entry is None:
            continue
        top = entry
        while isinstance(parent[top], ast.IfExp) and parent[top].test is not top:
            top = parent[top]
        p = parent[top]
        (sites if is_dispatch(p) and p.args and p.args[0] is top else stray).append((path, entry.lineno))
    return sites, stray


def test_every_launch_of_the_package_is_the_first_argument_of_a_dispatch_call():
    pkg = os.path.join(REPO, "object_keypoints_amd")
    files = [os.path.join(pkg, "ops.py")] + sorted(glob.glob(os.path.join(pkg, "perception", "*.py")))
    sites, stray = [], []
    for f in files:
        s, t = _launch_sites(f)
        sites += s
        stray += t
    assert stray == [], f"launches that bypass ops._dispatch (the stream-order recorder would not see them): {stray}"
    assert len(sites) >= 60
    # nothing outside ops.py reaches for the bindings at all
    for f in files[1:]:
        text = open(f).read()
        assert not re.search(r"torch\.ops\.okp|_ctypes_ops|_lib\.torch_ops", text), f


def test_the_choke_point_check_sees_a_bypass(tmp_path):
    bad = tmp_path / "bad.py"
    bad.write_text("def f(x):\n    _dispatch(_ops().good, x)\n    B = _ops()\n    _dispatch(B.good if x else B.good2, x)\n    B.direct(x)\n"
                   "    _ops().direct2(x)\n    g = getattr(_ops(), 'n')\n    _dispatch(getattr(_ops(), 'ok'), x)\n    h(_ops())\n    k(B)\n")
    sites, stray = _launch_sites(str(bad))
    assert sorted(l for _, l in sites) == [2, 4, 4, 8] and sorted(l for _, l in stray) == [5, 6, 7, 9, 10]


# ---- the recorder's reading of the schemas -----------------------------------------------------------------------------------------------
def _schemas():
    import torch
    from object_keypoints_amd import _lib, build
    build.build()
    assert _lib.torch_ops() is not None
    found = {s.name.split("::")[1]: s for s in torch._C._jit_get_all_schemas() if s.name.startswith("okp::")}
    source = open(os.path.join(REPO, "object_keypoints_amd", "csrc", "okp_torch.cpp")).read()
    assert sorted(found) == sorted(re.findall(r'm\.def\("(\w+)\(', source)) and len(found) >= 60       # every m.def(...) of the shim, nothing else
    return found


def test_every_entry_point_with_tensors_names_its_stream_or_is_in_the_table():
    schemas = _schemas()
    for name, s in schemas.items():
        if so.schema_tensor_args(s) and "stream" not in [a.name for a in s.arguments]:
            assert name in so.NO_STREAM_OPS, f"okp::{name} takes tensors but no stream: give it a treatment in stream_order.NO_STREAM_OPS"
    for name, treatment in so.NO_STREAM_OPS.items():                      # the table is not stale
        assert name in schemas and "stream" not in [a.name for a in schemas[name].arguments] and so.schema_tensor_args(schemas[name])
        assert treatment in (so.HOST_ORDERED, so.CURRENT_STREAM)
    args = [a for a in schemas["stream_wait_stream"].arguments]
    assert [a.name for a in args] == ["waiter", "signaller"]
    # the justifications cited in the table still describe the sources
    api = open(os.path.join(REPO, "object_keypoints_amd", "csrc", "okp_api.hip")).read().split("\n")
    stem = open(os.path.join(REPO, "object_keypoints_amd", "csrc", "okp_stem.hip")).read().split("\n")
    assert all("hipMemcpy(" in api[i - 1] for i in (284, 366, 367, 370)) and all("hipMemcpy(" in stem[i - 1] for i in (433, 434, 435, 466, 467))
    assert "plan->range_flag = flag_dev" in api[380 - 1] and "st->range_flag = flag_dev" in stem[478 - 1] and "select_tile(plan, a)" in api[563 - 1]
    torch_cpp = open(os.path.join(REPO, "object_keypoints_amd", "csrc", "okp_torch.cpp")).read()
    assert 'TORCH_CHECK(!t.is_cuda(), "okp: ", name, " is a HOST tensor' in torch_cpp


def test_every_write_annotation_parses_into_a_write():
    schemas = _schemas()
    total = 0
    for name, s in schemas.items():
        annotated = re.findall(r"Tensor\(\w+!\)\??(?:\[\])? (\w+)", str(s))
        parsed = [n for _, n, w in so.schema_tensor_args(s) if w]
        assert parsed == annotated, (name, parsed, annotated)
        plain = re.findall(r"Tensor\??(?:\[\])? (\w+)", str(s))            # ... and every unannotated tensor argument into a read
        assert [n for _, n, w in so.schema_tensor_args(s) if not w] == plain, (name, plain)
        total += len(annotated)
    assert total >= 150
    assert so.schema_tensor_args(schemas["cast"]) == [(0, "src", False), (1, "dst", True), (3, "range_flag", True)]
    assert so.schema_tensor_args(schemas["capacity_overflow"])[-1] == (6, "range_flag", False)
    assert (6, "outs", True) in so.schema_tensor_args(schemas["heads_forward"]) and (8, "set_index", False) in so.schema_tensor_args(schemas["score_objects"])


def test_recorder_resolves_both_bindings_patches_for_its_duration_only_and_reads_a_wait():
    import torch
    from object_keypoints_amd import _ctypes_ops, ops
    T = _schemas() and torch.ops.okp
    assert so.schema_of(T.cast) is so.schema_of(_ctypes_ops.cast) or str(so.schema_of(T.cast)) == str(so.schema_of(_ctypes_ops.cast))
    before = (ops._dispatch, torch.cuda.Stream.wait_stream, torch.cuda.Stream.wait_event, torch.cuda.Event.record, torch.cuda.synchronize,
              torch.cuda.CUDAGraph.replay)
    with pytest.raises(ZeroDivisionError):
        with so.recording() as rec:
            assert ops._dispatch is not before[0] and torch.cuda.Stream.wait_stream is not before[1]
            rec.okp(T.stream_wait_stream, (5, 7))
            rec.okp(_ctypes_ops.cast, (torch.zeros(4), torch.zeros(4), 9, None))             # host tensors: no device range
            rec.okp(T.conv_set_range_flag, (1, None))
            torch.zeros(3) + 1                                                                # host aten work: not recorded
            1 / 0
    after = (ops._dispatch, torch.cuda.Stream.wait_stream, torch.cuda.Stream.wait_event, torch.cuda.Event.record, torch.cuda.synchronize,
             torch.cuda.CUDAGraph.replay)
    assert after == before
    assert [type(r) for r in rec.trace] == [so.Wait, so.Access] and (rec.trace[0].waiter, rec.trace[0].signaller) == (5, 7)
    assert rec.trace[1].name == "okp.cast" and rec.trace[1].stream == 9 and rec.trace[1].reads == rec.trace[1].writes == []
    assert so.waits_of(rec.trace) == [(0, 5, 7)]


def test_tensor_range_spans_offset_sizes_and_strides():
    import torch
    t = torch.zeros(4, 6, 8, dtype=torch.float32)
    base = t.data_ptr()
    assert so.tensor_range(t) == (base, base + 4 * 6 * 8 * 4)
    v = t[1:3, :, 2:5]                                                    # first element (1,0,2), last (2,5,4)
    assert so.tensor_range(v) == (base + (48 + 2) * 4, base + (2 * 48 + 5 * 8 + 4 + 1) * 4)
    assert so.tensor_range(t[:, :, 0:1].expand(4, 6, 3)) == (base, base + (3 * 48 + 5 * 8 + 1) * 4)
