"""The refusals of the six sliding-window pushes, as calls that can be made again: what scripts/record_window_refusals.py records into
tests/golden/window_push_refusals.json and tests/test_window_refusals.py replays.  Two layers:

  C     every okp_window_push* entry point with its scalars at the bad values of tests/test_window_args.py / test_window_views_args.py /
        test_refine_weighted_args.py - each alone, every pair of two faulty scalars (each at its first bad value), every required pointer
        null alone, every pair of a faulty scalar and a null pointer.  Every call also carries a null in the pointer its entry point checks
        last, so none can reach a launch; the other pointers are addresses the host never dereferences.
  ops   window_state / window_views_state at their bad sizes, and window_push / window_push_views under a plain, a confidence and a motion
        WindowConfig with one argument at fault: every tensor they name with a wrong dtype, a wrong shape, its key missing, in host memory, on
        another device than the rest, and the state made without prior= / timed=; then pairs of two faulty tensors, which pin the order of
        the walk.  The "device" tensors are host tensors that answer is_cuda with True (the stand-ins of tests/test_object_stage_wiring.py
        do the same job for the pipelines); the launch itself is replaced by a stub that fails the case, so none can reach the device.

A case is JSON: C cases {"fn", "set": {scalar: value}, "null": [pointer names]}; ops cases {"fn", "cfg", "faults": [[argument, kind], ..]} or
{"fn", "args": [..]} for the state constructors.  nan and the infinities are written as strings.  The record itself - digest, pack, unpack,
dumps - is tests/refusal_record.py's.  No GPU needed."""
import ctypes
import itertools

import numpy as np
import torch

FAKE = 64 * 4096         # a non-NULL "device" address the host never dereferences

_SINGLE_IN = ("tab", "assignment", "status", "meas_of", "track_i", "track_f", "track_pose", "T_WC", "cam", "B", "max_obj", "S", "T", "W", "min_views", "max_speed")
_RIG_IN = ("assignment", "status", "meas_of", "track_i", "track_f", "track_pose", "T_WB", "views", "B", "max_obj", "S", "T", "W", "V", "min_views", "max_speed")
ENTRY_POINTS = {          # the C parameter lists (include/okp.h), without the stream
    "okp_window_push": _SINGLE_IN + ("win_obs", "win_views", "win_i", "n_views", "start"),
    "okp_window_push_weighted": _SINGLE_IN + ("conf_ref", "conf_floor", "win_obs", "win_prior", "win_views", "win_i", "n_views", "start"),
    "okp_window_push_timed": _SINGLE_IN + ("win_obs", "win_age", "win_views", "win_i", "n_views", "start", "start_velocity"),
    "okp_window_push_views": ("obs",) + _RIG_IN + ("win_obs", "win_views", "win_i", "n_views", "start"),
    "okp_window_push_views_weighted": ("obs", "prior") + _RIG_IN + ("win_obs", "win_prior", "win_views", "win_i", "n_views", "start"),
    "okp_window_push_views_timed": ("obs",) + _RIG_IN + ("win_obs", "win_age", "win_views", "win_i", "n_views", "start", "start_velocity"),
}
CHECKED_LAST = {"okp_window_push": "start", "okp_window_push_weighted": "win_prior", "okp_window_push_timed": "start_velocity",
                "okp_window_push_views": "start", "okp_window_push_views_weighted": "win_prior", "okp_window_push_views_timed": "start_velocity"}
SINGLE_DEFAULTS = dict(B=2, max_obj=4, S=4, T=8, W=16, min_views=2, max_speed=0.5, fx=62.0, fy=62.0, cam=True, conf_ref=0.8, conf_floor=0.4)
RIG_DEFAULTS = dict(B=2, max_obj=4, S=4, T=8, W=8, V=8, min_views=2, max_speed=0.5)
_COMMON_BAD = [[dict(B=v) for v in (0, -1)], [dict(max_obj=v) for v in (0, -1)], [dict(S=v) for v in (0, 17, -3)], [dict(T=v) for v in (0, 65, -1)],
               [dict(W=v) for v in (0, 65, -1)], [dict(max_speed=v) for v in (0.0, -0.5, "nan", "-inf")]]
SINGLE_BAD = _COMMON_BAD + [[dict(min_views=v) for v in (0, 17, -1)], [dict(fx=v) for v in (0.0, -62.0, "nan", "inf")], [dict(fy=v) for v in (0.0, -62.0, "nan", "inf")],
                            [dict(cam=False)]]
WEIGHTED_BAD = [[dict(conf_ref=v) for v in (0.0, -1.0, "nan", "inf")], [dict(conf_floor=v) for v in (0.0, -0.5, "nan", 0.9, "inf")]]
RIG_BAD = _COMMON_BAD + [[dict(min_views=v) for v in (0, 9, -1)], [dict(V=v) for v in (0, 65, -1)], [dict(W=w, V=v) for w, v in ((9, 64), (64, 9), (64, 64), (33, 16))]]


def pointers_of(fn):
    return [n for n in ENTRY_POINTS[fn] if n != "cam" and n not in SINGLE_DEFAULTS and n not in RIG_DEFAULTS]


def c_cases():
    """Every C case, in a fixed order."""
    out = []
    for fn in ENTRY_POINTS:
        bad = RIG_BAD if "views" in fn else SINGLE_BAD + (WEIGHTED_BAD if fn.endswith("weighted") else [])
        last = CHECKED_LAST[fn]
        pointers = [p for p in pointers_of(fn) if p != last]
        case = lambda faults, null: {"fn": fn, "set": {k: v for f in faults for k, v in f.items()}, "null": list(null) + [last]}
        out.append(case((), ()))                                                    # good scalars: the pointer checked last is the one refused
        out += [case((f,), ()) for group in bad for f in group]
        out += [case((f[0], g[0]), ()) for f, g in itertools.combinations(bad, 2) if not set(f[0]) & set(g[0])]
        out += [case((), (p,)) for p in pointers]
        out += [case((group[0],), (p,)) for group in bad for p in pointers]
    return out


def run_c(L, case):
    """The call of a C case against the loaded library -> [return code, okp_last_error()]."""
    from object_keypoints_amd import _lib
    fn = case["fn"]
    v = dict(RIG_DEFAULTS if "views" in fn else SINGLE_DEFAULTS)
    v.update({k: float(x) if isinstance(x, str) else x for k, x in case["set"].items()})
    args = []
    for i, name in enumerate(ENTRY_POINTS[fn]):
        if name == "cam":
            args.append(ctypes.byref(_lib.okp_camera(v["fx"], v["fy"], 32.0, 32.0, (0.0, 0.0, 0.0, 0.0), 0)) if v["cam"] else None)
        elif name in v:
            args.append(v[name])
        else:
            args.append(None if name in case["null"] else FAKE * (1 + i))
    assert set(case["null"]) <= set(pointers_of(fn)) and CHECKED_LAST[fn] in case["null"]
    rc = getattr(L, fn)(*args, None)
    return [int(rc), L.okp_last_error().decode()]


# ---- ops ----------------------------------------------------------------------------------------------------------------------------------------

class Device(torch.Tensor):
    """A host tensor that says it is in device memory: what ops.window_push and window_push_views walk over before they launch."""
    is_cuda = True


class Elsewhere(Device):
    """One that says it is on another device than the rest."""
    device = torch.device("cuda", 1)


B, MAX_OBJ, S, T, W, V = 1, 2, 3, 5, 4, 2
CONFIGS = ("plain", "confidence", "motion")
KINDS = ("dtype", "shape", "missing", "host", "device")
STATE_ARGS = {"window_state": [(1, 2, 3, 4, "cpu"), (0, 2, 3, 4, "cuda"), (1, 65, 3, 4, "cuda"), (1, 2, 17, 4, "cuda"), (1, 2, 3, 65, "cuda")],
              "window_views_state": [(1, 2, 3, 4, 8, "cpu"), (0, 2, 3, 4, 8, "cuda"), (1, 65, 3, 4, 8, "cuda"), (1, 2, 17, 4, 8, "cuda"), (1, 2, 3, 65, 1, "cuda"),
                                     (1, 2, 3, 4, 0, "cuda"), (1, 2, 3, 4, 65, "cuda"), (1, 2, 3, 16, 64, "cuda")]}
TRACK_KEYS = ("meas_of", "track_i", "track_f", "track_pose")
STATE_KEYS = ("win_obs", "win_views", "win_i", "win_prior", "win_age")


def _shapes(rig):
    wv = W * V if rig else W
    sh = {"assignment": (torch.int32, (B, MAX_OBJ, S)), "status": (torch.int32, (B, MAX_OBJ)), "meas_of": (torch.int32, (B, T)), "track_i": (torch.int32, (B, T, 4)),
          "track_f": (torch.float64, (B, T, 16)), "track_pose": (torch.float64, (B, T, 12)), "win_obs": (torch.float64, (B, T, S, wv, 2)),
          "win_views": (torch.float64, (B, T, wv, 14)), "win_i": (torch.int32, (B, T, 4)), "win_prior": (torch.float64, (B, T, S, wv)), "win_age": (torch.int32, (B, T, wv))}
    if rig:
        sh.update(obs=(torch.float64, (B, MAX_OBJ, S, V, 2)), T_WB=(torch.float64, (B, 12)), views=(torch.float64, (V, 14)), prior=(torch.float64, (B, MAX_OBJ, S, V)))
    else:
        sh.update(tab=(torch.float64, (B, MAX_OBJ, S, 4)), T_WC=(torch.float64, (B, 12)))
    return sh


def tensors_of(fn, cfg):
    """The tensors a push under this config names, in the order of its parameters."""
    rig = fn == "window_push_views"
    names = (["obs"] if rig else ["tab"]) + ["assignment", "status", *TRACK_KEYS] + (["T_WB", "views"] if rig else ["T_WC"]) + ["win_obs", "win_views", "win_i"]
    names += {"plain": [], "confidence": ["win_prior"] + (["prior"] if rig else []), "motion": ["win_age"]}[cfg]
    return names


def ops_cases():
    out = [{"fn": fn, "args": list(a)} for fn, rows in STATE_ARGS.items() for a in rows]
    for fn in ("window_push", "window_push_views"):
        for cfg in CONFIGS:
            names = tensors_of(fn, cfg)
            keyed = lambda n: n in TRACK_KEYS or n in STATE_KEYS
            out += [{"fn": fn, "cfg": cfg, "faults": [[w, "other"]]} for w in ("cfg", "cam", "track", "state") if not (w == "cam" and fn == "window_push_views")]
            if fn == "window_push_views":
                out += [{"fn": fn, "cfg": cfg, "faults": [["prior", "given" if cfg != "confidence" else "missing"]]}, {"fn": fn, "cfg": cfg, "faults": [["obs", "wide"]]}]
            out += [{"fn": fn, "cfg": cfg, "faults": [[names[0], "rows"]]}]
            out += [{"fn": fn, "cfg": cfg, "faults": [[n, k]]} for n in names for k in KINDS if (k != "missing" or keyed(n)) and not (n == "prior" and k == "missing")]
            out += [{"fn": fn, "cfg": cfg, "faults": [[a, ka], [b, kb]]} for a, b in itertools.combinations(names, 2) for ka, kb in (("shape", "dtype"), ("dtype", "host"))]
    return out


def _fault(t, kind):
    if kind == "dtype":
        return t.to(torch.float32 if t.dtype == torch.float64 else torch.int64).as_subclass(Device)
    if kind == "shape":
        return torch.zeros(tuple(t.shape[:-1]) + (t.shape[-1] + 1,), dtype=t.dtype).as_subclass(Device)
    if kind == "device":
        return t.as_subclass(Elsewhere)
    assert kind == "host", kind
    return torch.zeros(tuple(t.shape), dtype=t.dtype)


def run_ops(case):
    """The call of an ops case -> the OkpError's text.  The launch is replaced: a case that gets that far fails."""
    from object_keypoints_amd import ops
    if "args" in case:
        try:
            getattr(ops, case["fn"])(*case["args"])
        except ops.OkpError as e:
            return str(e)
        raise AssertionError(f"{case}: not refused")
    rig = case["fn"] == "window_push_views"
    t = {n: torch.zeros(shape, dtype=dtype).as_subclass(Device) for n, (dtype, shape) in _shapes(rig).items()}
    cfg = {"plain": ops.WindowConfig(W), "confidence": ops.WindowConfig(W, confidence=ops.ConfidenceWeights(0.8, 0.4)),
           "motion": ops.WindowConfig(W, motion="constant_velocity")}[case["cfg"]]
    cam = ops.make_camera(np.array([[62.0, 0, 32], [0, 62.0, 32], [0, 0, 1]]), np.zeros(4))
    track = {k: t[k] for k in TRACK_KEYS}
    state = {k: t[k] for k in ("win_obs", "win_views", "win_i")}
    if case["cfg"] == "confidence":
        state["win_prior"] = t["win_prior"]
    if case["cfg"] == "motion":
        state["win_age"] = t["win_age"]
    prior = t["prior"] if rig and case["cfg"] == "confidence" else None
    for name, kind in case["faults"]:
        if kind == "other":
            cfg, cam, track, state = (ops.RefineConfig() if name == "cfg" else cfg), ([62.0, 62.0] if name == "cam" else cam), ([] if name == "track" else track), \
                (None if name == "state" else state)
            continue
        if name == "prior" and kind in ("given", "missing"):
            prior = t["prior"] if kind == "given" else None
            continue
        holder = track if name in TRACK_KEYS else state if name in STATE_KEYS else t
        if kind == "missing":
            del holder[name]
        elif kind == "rows":                                                          # more model rows than POSE_MAX_POINTS
            holder[name] = torch.zeros((B, MAX_OBJ, 17) + tuple(t[name].shape[3:]), dtype=torch.float64).as_subclass(Device)
        elif kind == "wide":                                                          # ticks x cameras beyond REFINE_WIDE_MAX_VIEWS
            cfg = ops.WindowConfig(64, **({"confidence": cfg.confidence} if cfg.confidence else {"motion": cfg.motion} if cfg.motion else {}))
            holder[name] = torch.zeros((B, MAX_OBJ, S, 16, 2), dtype=torch.float64).as_subclass(Device)
        else:
            holder[name] = _fault(holder[name], kind)
        if name == "prior":
            prior = holder[name]

    def launch(*a):
        raise AssertionError(f"{case}: reached the launch")
    real, ops._dispatch = ops._dispatch, launch
    try:
        if rig:
            ops.window_push_views(state, t["obs"], t["assignment"], t["status"], track, t["T_WB"], t["views"], cfg, **({"prior": prior} if prior is not None else {}))
        else:
            ops.window_push(state, t["tab"], t["assignment"], t["status"], track, t["T_WC"], cam, cfg)
    except ops.OkpError as e:
        return str(e)
    finally:
        ops._dispatch = real
    raise AssertionError(f"{case}: not refused")
