"""The refusals of the six sliding-window pushes, replayed: tests/golden/window_push_refusals.json holds, for every case of
tests/window_refusal_cases.py, the return code and okp_last_error() text of the C entry point, or the OkpError text of ops.window_state /
window_views_state / window_push / window_push_views, as scripts/record_window_refusals.py found them before the pushes came to share their
checks (csrc/okp_window_ring.h, the helpers of ops.py).  A call with two faults pins which of them is reported: the order of the checks is
part of the contract.  The file holds each distinct answer once and, per case, the index of its answer; a digest ties it to the module's list of
cases.  Equality of code and text, case by case, no case left out.  No GPU needed."""
import json
import os

import refusal_record
import window_refusal_cases as cases

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(REPO, "tests", "golden", "window_push_refusals.json")) as f:
    C, OPS = refusal_record.unpack(json.load(f), cases.c_cases(), cases.ops_cases())              # [(case, [rc, text])], [(case, text)]: the file holds the answers, the module the cases (tied by a digest)


def test_the_record_holds_every_case_and_only_refusals():
    assert [case for case, _ in C] == cases.c_cases() and [case for case, _ in OPS] == cases.ops_cases()
    assert {case["fn"] for case, _ in C} == set(cases.ENTRY_POINTS) and len(C) > 1000 and len(OPS) > 500
    for case, (rc, text) in C:
        assert rc == -1 and text.startswith(case["fn"] + ": "), case                                 # OKP_EINVAL, under the entry point's own name
        assert cases.CHECKED_LAST[case["fn"]] in case["null"]
    kinds = {(case["fn"], case.get("cfg"), tuple(map(tuple, case.get("faults", ())))) for case, _ in OPS}
    for fn in ("window_push", "window_push_views"):
        for cfg in cases.CONFIGS:
            for name in cases.tensors_of(fn, cfg):
                for kind in ("dtype", "shape", "host", "device"):
                    assert (fn, cfg, ((name, kind),)) in kinds
            for key in cases.TRACK_KEYS + ("win_obs", "win_views", "win_i"):
                assert (fn, cfg, ((key, "missing"),)) in kinds
        assert (fn, "confidence", (("win_prior", "missing"),)) in kinds and (fn, "motion", (("win_age", "missing"),)) in kinds   # a state made without prior= / timed=


def test_the_entry_points_refuse_what_they_refused_in_the_same_words():
    from object_keypoints_amd import _lib, build
    build.build()
    L = _lib.lib()
    differ = [(case, want, got) for case, want in C for got in [cases.run_c(L, case)] if got != want]
    assert not differ, f"{len(differ)} of {len(C)} differ; the first: {differ[0]}"


def test_the_wrappers_refuse_what_they_refused_in_the_same_words():
    differ = [(case, want, got) for case, want in OPS for got in [cases.run_ops(case)] if got != want]
    assert not differ, f"{len(differ)} of {len(OPS)} differ; the first: {differ[0]}"
