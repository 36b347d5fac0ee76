"""The record of a refusal suite (tests/window_refusal_cases.py, tests/refine_views_refusal_cases.py): what its recording script writes under
tests/golden/ and its test replays.  A suite has two lists of cases, in a fixed order - C cases {"fn": entry point, ..}, answered by
[return code, okp_last_error()], and ops cases, answered by the OkpError's text.  The file holds every distinct answer once (a C text without
the "<entry point>: " it begins with), per case the index of its answer, and a digest of each list: the cases are not in the file, their order
is."""
import hashlib
import json


def digest(cases):
    """What ties a record to the list of cases it was made from."""
    return hashlib.sha256(json.dumps(cases, sort_keys=True).encode()).hexdigest()


def pack(c_cases, ops_cases, c_results, ops_results):
    """[[rc, text]] of the C cases and [text] of the ops cases, in their order -> the record."""
    c = [[rc, text[len(case["fn"]) + 2:]] for case, (rc, text) in zip(c_cases, c_results) if text.startswith(case["fn"] + ": ")]
    assert len(c) == len(c_results) == len(c_cases) and len(ops_results) == len(ops_cases)
    answers = sorted({(rc, text) for rc, text in c}) + sorted({(None, text) for text in ops_results}, key=lambda a: a[1])
    index = {a: i for i, a in enumerate(answers)}
    return {"c_cases": digest(c_cases), "ops_cases": digest(ops_cases), "answers": [list(a) for a in answers],
            "c": [index[(rc, text)] for rc, text in c], "ops": [index[(None, text)] for text in ops_results]}


def unpack(record, c_cases, ops_cases):
    """The record -> ([(case, [rc, text])] of the C cases, [(case, text)] of the ops cases); refuses a record made from another list of cases."""
    assert record["c_cases"] == digest(c_cases) and record["ops_cases"] == digest(ops_cases), \
        "the record was made from another list of cases: record again at the commit before the change"
    assert len(record["c"]) == len(c_cases) and len(record["ops"]) == len(ops_cases)
    answer = record["answers"]
    return ([(case, [answer[i][0], case["fn"] + ": " + answer[i][1]]) for case, i in zip(c_cases, record["c"])],
            [(case, answer[i][1]) for case, i in zip(ops_cases, record["ops"])])


def dumps(record):
    """The record as text: an answer per line, the indices forty to a line."""
    rows = lambda v: ",\n".join("  " + ", ".join(map(str, v[i:i + 40])) for i in range(0, len(v), 40))
    return ('{"c_cases": "%s",\n"ops_cases": "%s",\n"answers": [\n' % (record["c_cases"], record["ops_cases"]) + ",\n".join("  " + json.dumps(a) for a in record["answers"])
            + '\n],\n"c": [\n' + rows(record["c"]) + '\n],\n"ops": [\n' + rows(record["ops"]) + "\n]}\n")
