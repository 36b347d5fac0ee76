"""The refusals of the six refinements against views and the two bearing collectors, replayed: tests/golden/refine_views_refusals.json holds,
for every case of tests/refine_views_refusal_cases.py, the return code and okp_last_error() text of the C entry point, or the OkpError text of
the wrapper of ops.py, as scripts/record_refine_views_refusals.py found them before the family came to share one body per layer (the launcher
of csrc/okp_refine_views.hip, the helpers of ops.py).  A call with two faults pins which of them is reported: the order of the checks is part
of the contract.  The file holds each distinct answer once and, per case, the index of its answer; a digest ties it to the module's list of
cases.  Equality of code and text, case by case, no case left out.  No GPU needed."""
import json
import os

import refine_views_refusal_cases as cases
import refusal_record

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(REPO, "tests", "golden", "refine_views_refusals.json")) as f:
    C, OPS = refusal_record.unpack(json.load(f), cases.c_cases(), cases.ops_cases())      # [(case, [rc, text])], [(case, text)]


def test_the_record_holds_every_case_and_only_refusals():
    assert [case for case, _ in C] == cases.c_cases() and [case for case, _ in OPS] == cases.ops_cases()
    assert {case["fn"] for case, _ in C} == set(cases.ENTRY_POINTS) and len(cases.ENTRY_POINTS) == 8 and len(C) > 1000 and len(OPS) > 500
    for case, (rc, text) in C:
        assert rc == -1 and text.startswith(case["fn"] + ": "), case                                 # OKP_EINVAL, under the entry point's own name
    c_kinds = {(case["fn"], tuple(sorted(case["set"])), tuple(case["null"])) for case, _ in C}
    for fn in cases.ENTRY_POINTS:
        last = cases.ALWAYS_NULL[fn]
        assert (fn, (), (last,)) in c_kinds
        for p in cases.pointers_of(fn):
            assert p == last or (fn, (), (p, last)) in c_kinds, (fn, p)                               # every pointer null alone
        for group in cases.bad_scalars(fn):
            for fault in group:
                assert (fn, tuple(sorted(fault)), (last,)) in c_kinds, (fn, fault)                   # every scalar fault alone
    handed = [case for case, _ in C if case["fn"] == "okp_refine_pose_views_weighted" and case["set"].get("V") in (64, 65)]
    assert len(handed) > 40 and {case["set"]["V"] for case in handed} == {64, 65}                     # either side of the hand-off to the wide kernel
    kinds = {(case["fn"], tuple(sorted(case["kw"].items())), case["cfg"], tuple(map(tuple, case["faults"]))) for case, _ in OPS}
    for fn, kw in cases.OPS_FNS:
        for cfg in cases.configs_of(fn):
            at = (fn, tuple(sorted(kw.items())), cfg)
            for name in cases.tensors_of(fn):
                for kind in cases.KINDS:
                    assert at + (((name, kind),),) in kinds
            for fault in [("cfg", "class"), ("cfg", "resolve_views"), ("cfg", "motion"), ("pose", "missing"), ("assignment", "missing")] + [(w, "int") for w in kw]:
                assert at + ((fault,),) in kinds
            assert at + ((("cfg", "plain"),),) in kinds and at + ((("prior", "missing"),),) in kinds if "prior" in cases.tensors_of(fn) else at + ((("cfg", "confidence"),),) in kinds
    for fn in cases.COLLECTORS:
        for name in cases.tensors_of(fn):
            for kind in cases.kinds_of(name):
                assert (fn, (), None, ((name, kind),)) in kinds
        for key in cases.FUSED_KEYS:
            assert (fn, (), None, ((key, "missing"),)) in kinds


def test_the_entry_points_refuse_what_they_refused_in_the_same_words():
    from object_keypoints_amd import _lib, build
    build.build()
    L = _lib.lib()
    differ = [(case, want, got) for case, want in C for got in [cases.run_c(L, case)] if got != want]
    assert not differ, f"{len(differ)} of {len(C)} differ; the first: {differ[0]}"


def test_the_wrappers_refuse_what_they_refused_in_the_same_words():
    differ = [(case, want, got) for case, want in OPS for got in [cases.run_ops(case)] if got != want]
    assert not differ, f"{len(differ)} of {len(OPS)} differ; the first: {differ[0]}"
