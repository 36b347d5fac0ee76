#!/usr/bin/env python
"""Record what the six refinements against views and the two bearing collectors refuse, and in which words, into
tests/golden/refine_views_refusals.json:

    python scripts/record_refine_views_refusals.py [--out FILE]

The cases are those of tests/refine_views_refusal_cases.py (the eight C entry points with faulty scalars and null pointers, alone and in pairs,
and the wrappers of ops.py with one or two faulty arguments); every one is refused on the host, so no GPU is needed.  The file holds every
distinct answer once and, per case, which answer it got (tests/refusal_record.py); the cases themselves are the module's, tied to the file by a
digest.  tests/test_refine_views_refusals.py replays the file against the build, case by case: run this before a change of the family's checks,
not after it - the file is the record of what the code refused before."""
import argparse
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import refine_views_refusal_cases as cases                               # noqa: E402
import refusal_record                                                    # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden", "refine_views_refusals.json"))
    args = ap.parse_args()
    from object_keypoints_amd import _lib, build
    build.build()
    L = _lib.lib()
    c = [cases.run_c(L, case) for case in cases.c_cases()]
    o = [cases.run_ops(case) for case in cases.ops_cases()]
    with open(args.out, "w") as f:
        f.write(refusal_record.dumps(refusal_record.pack(cases.c_cases(), cases.ops_cases(), c, o)))
    print(f"{args.out}: {len(c)} C cases, {len(o)} ops cases, {os.path.getsize(args.out)} bytes")


if __name__ == "__main__":
    main()
