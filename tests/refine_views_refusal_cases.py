"""The refusals of the six refinements of a pose against bearings in many views and of the two collectors of those bearings, as calls that can
be made again: what scripts/record_refine_views_refusals.py records into tests/golden/refine_views_refusals.json and
tests/test_refine_views_refusals.py replays (the record's form is tests/refusal_record.py's, the manner tests/window_refusal_cases.py's).  Two layers:

  C     every entry point of ENTRY_POINTS with its scalars at the edges of the ranges refine_views_params / rig_bearings_launch check (the limits
        are include/okp.h's) - each alone, every pair of two faulty scalars in distinct parameters (each at its first bad value), every pointer
        null alone, every pair of a faulty scalar and a null pointer; okp_refine_pose_views_weighted also with V = 64 and V = 65, either side of
        its hand-off to the wide kernel, under every other fault.  No call can reach a launch: it carries a null in ALWAYS_NULL's pointer - one
        its entry point requires whatever the scalars are and checks after the others of that kind -, or a null in an output the Huber
        threshold it passes requires, or a pose_out that is the pose.  The other pointers are addresses the host never dereferences
        (type_count, which the host reads, is a host array).
  ops   refine_pose_views, refine_pose_views_each, refine_pose_views_wide (each = False / True) and refine_pose_views_weighted (each, wide)
        under every config they accept - a RefineConfig or a WindowConfig; plain, huber_px, confidence - and rig_bearings /
        rig_bearings_weighted, with one argument at fault: every tensor with a wrong dtype, a wrong shape, in host memory, on another device
        than the rest; the config of the wrong class, with resolve_views, with motion, with confidence but no prior and the reverse; each / wide
        that are no bool; the pose and fused dicts with a key missing; then pairs of two faulty tensors, which pin the order of the walk.
        The "device" tensors and the replaced launch are the window suite's.

A case is JSON: C cases {"fn", "set": {scalar: value}, "null": [pointer names]} (and "alias": true for pose_out = pose); ops cases
{"fn", "kw": {"each": .., "wide": ..}, "cfg", "faults": [[argument, kind], ..]}.  nan and the infinities are written as strings.  No GPU needed."""
import ctypes
import itertools

import torch

from window_refusal_cases import FAKE, Device, _fault

_TAIL = ("iters", "damping", "B", "max_obj", "S", "V", "pose_out", "fit", "n_obs")
_PLAIN = ("obs", "views", "pose", "assignment", "n_obj", "model", "sigma_px") + _TAIL + ("information", "status")
_HUBER = ("obs", "views", "views_each", "pose", "assignment", "n_obj", "model", "sigma_px", "huber_px") + _TAIL + ("n_inlier", "weight", "information", "status")
_BEARINGS = ("count", "xyc", "match", "member", "object", "n_fused", "table", "n_table", "n_pairs", "K", "cap", "cap_f", "type_count")
ENTRY_POINTS = {          # the C parameter lists (include/okp.h), without the stream
    "okp_refine_pose_views": _PLAIN, "okp_refine_pose_views_each": _PLAIN, "okp_refine_pose_views_robust": _HUBER, "okp_refine_pose_views_wide": _HUBER,
    "okp_refine_pose_views_weighted": _HUBER[:1] + ("prior",) + _HUBER[1:], "okp_refine_pose_views_weighted_wide": _HUBER[:1] + ("prior",) + _HUBER[1:],
    "okp_rig_bearings": _BEARINGS + ("obs",), "okp_rig_bearings_weighted": _BEARINGS + ("conf_ref", "conf_floor", "obs", "prior"),
}
ALWAYS_NULL = {"okp_refine_pose_views": "status", "okp_refine_pose_views_each": "status", "okp_refine_pose_views_robust": "weight", "okp_refine_pose_views_wide": "status",
               "okp_refine_pose_views_weighted": "prior", "okp_refine_pose_views_weighted_wide": "prior", "okp_rig_bearings": "obs", "okp_rig_bearings_weighted": "prior"}
V_MAX = {"okp_refine_pose_views": 64, "okp_refine_pose_views_each": 64, "okp_refine_pose_views_robust": 64, "okp_refine_pose_views_wide": 512,
         "okp_refine_pose_views_weighted": 512, "okp_refine_pose_views_weighted_wide": 512}
REFINE_DEFAULTS = dict(B=2, max_obj=4, S=4, V=8, sigma_px=1.0, huber_px=1.5, iters=4, damping=1e-3, views_each=0)
BEARINGS_DEFAULTS = dict(n_table=1, n_pairs=2, K=3, cap=8, cap_f=4, type_count=[2, 1], conf_ref=0.8, conf_floor=0.4)


def bad_scalars(fn):
    """The groups of faulty settings of an entry point: a group is one parameter's (or one combination's) bad values, the first of which stands for
    it in the pairs.  The `huber_px` groups of the entry points that take 0 as "the plain cost" end with that 0: no fault, the null is what is refused."""
    if fn in V_MAX:
        bad = [[dict(B=v) for v in (0, -1)], [dict(max_obj=v) for v in (0, -1)], [dict(B=65536, max_obj=65536)], [dict(S=v) for v in (0, 17, -3)],
               [dict(V=v) for v in (0, -1, V_MAX[fn] + 1)], [dict(iters=v) for v in (0, 17, -1)], [dict(sigma_px=v) for v in (0.0, -1.0, "nan", "inf")],
               [dict(damping=v) for v in (-1e-3, "nan", "inf")]]
        if "huber_px" in ENTRY_POINTS[fn]:
            zero = (0.0,) if fn == "okp_refine_pose_views_robust" else ()
            bad += [[dict(huber_px=v) for v in zero + (-1.0, "nan", "inf") + ((0.0,) if not zero else ())], [dict(views_each=v) for v in (2, -1)]]
        return bad
    bad = [[dict(n_pairs=v) for v in (0, 33, -1)], [dict(K=v) for v in (1, 9, -1)], [dict(type_count=v) for v in ([0, 1], [15, 1], None)],
           [dict(cap=v) for v in (0, 257, -1)], [dict(cap_f=v) for v in (0, 65, -1)], [dict(n_table=v) for v in (0, -1)], [dict(n_table=3, n_pairs=4)]]
    if fn.endswith("weighted"):
        bad += [[dict(conf_ref=v) for v in (0.0, -1.0, "nan", "inf")], [dict(conf_floor=v) for v in (0.0, -0.5, "nan", 0.9, "inf")]]
    return bad


def pointers_of(fn):
    return [n for n in ENTRY_POINTS[fn] if n not in REFINE_DEFAULTS and n not in BEARINGS_DEFAULTS]


def c_cases():
    """Every C case, in a fixed order."""
    out = []
    for fn in ENTRY_POINTS:
        bad, last = bad_scalars(fn), ALWAYS_NULL[fn]
        pointers = [p for p in pointers_of(fn) if p != last]
        case = lambda faults, null: {"fn": fn, "set": {k: v for f in faults for k, v in f.items()}, "null": list(null) + [last]}
        out.append(case((), ()))                                                    # good scalars: the pointer checked last is the one refused
        out += [case((f,), ()) for group in bad for f in group]
        out += [case((f[0], g[0]), ()) for f, g in itertools.combinations(bad, 2) if not set(f[0]) & set(g[0])]
        out += [case((), (p,)) for p in pointers]
        out += [case((group[0],), (p,)) for group in bad for p in pointers]
        if fn in V_MAX:
            out.append({"fn": fn, "set": {}, "null": [], "alias": True})           # every pointer there, pose_out the pose itself
        if fn == "okp_refine_pose_views_wide":                                      # its last two pointers, which only a Huber threshold requires
            out += [{"fn": fn, "set": {}, "null": [p]} for p in ("n_inlier", "weight")]
        if fn in V_MAX and "huber_px" in ENTRY_POINTS[fn] and fn != "okp_refine_pose_views_robust":      # 0, the plain cost, does not require them
            out.append(case((dict(huber_px=0.0),), ("n_inlier", "weight")))
        if fn == "okp_refine_pose_views_weighted":                                  # one wave (64) and the hand-off to the wide kernel (65): the caller's name on both
            for v in (64, 65):
                out.append(case((dict(V=v),), ()))
                out += [case((dict(V=v), group[0]), ()) for group in bad if "V" not in group[0]]
                out += [case((dict(V=v),), (p,)) for p in pointers]
    return out


def run_c(L, case):
    """The call of a C case against the loaded library -> [return code, okp_last_error()]."""
    fn = case["fn"]
    v = dict(REFINE_DEFAULTS if fn in V_MAX else BEARINGS_DEFAULTS)
    v.update({k: float(x) if isinstance(x, str) else x for k, x in case["set"].items()})
    huber_needs = v.get("huber_px") == REFINE_DEFAULTS["huber_px"] and {"n_inlier", "weight"} & set(case["null"])
    assert set(case["null"]) <= set(pointers_of(fn)) and (ALWAYS_NULL[fn] in case["null"] or huber_needs or case.get("alias")), f"{case} could reach a launch"
    args, at = [], {}
    for i, name in enumerate(ENTRY_POINTS[fn]):
        if name == "type_count":
            args.append(None if v[name] is None else (ctypes.c_int32 * 8)(*v[name]))
        elif name in v:
            args.append(v[name])
        else:
            at[name] = None if name in case["null"] else FAKE * (1 + i)
            args.append(at["pose"] if name == "pose_out" and case.get("alias") else at[name])
    rc = getattr(L, fn)(*args, None)
    return [int(rc), L.okp_last_error().decode()]


# ---- ops ----------------------------------------------------------------------------------------------------------------------------------------

B, MAX_OBJ, S, V = 1, 2, 3, 2
PAIRS, K, CAP, CAP_F = 2, 3, 4, 3
KINDS = ("dtype", "shape", "host", "device")
OPS_FNS = [("refine_pose_views", {}), ("refine_pose_views_each", {}), ("refine_pose_views_wide", {"each": False}), ("refine_pose_views_wide", {"each": True}),
           ("refine_pose_views_weighted", {"each": False, "wide": False}), ("refine_pose_views_weighted", {"each": True, "wide": False}),
           ("refine_pose_views_weighted", {"each": False, "wide": True}), ("refine_pose_views_weighted", {"each": True, "wide": True})]
COLLECTORS = ("rig_bearings", "rig_bearings_weighted")
POSE_KEYS = ("pose", "assignment")
FUSED_KEYS = ("member", "object", "n_fused")


def configs_of(fn):
    """The configs a refinement accepts, by name (see _config)."""
    if fn == "refine_pose_views_weighted":
        return ("refine_conf", "window_conf", "refine_conf_huber", "window_conf_huber")
    return ("refine", "refine_huber") + (("window", "window_huber") if fn != "refine_pose_views" else ())


def tensors_of(fn):
    """The tensors a call names, in the order of its parameters."""
    if fn in COLLECTORS:
        return ["table", "count", "xyc", "match", *FUSED_KEYS]
    return ["obs"] + (["prior"] if fn == "refine_pose_views_weighted" else []) + ["views", *POSE_KEYS, "n_obj", "model"]


def kinds_of(name):
    """The faults a tensor is given alone: every kind, but for a collector's count, whose device the wrapper leaves to the binding."""
    return tuple(k for k in KINDS if (name, k) != ("count", "device"))


def ops_cases():
    out = []
    pairs = lambda names: [[[a, ka], [b, kb]] for a, b in itertools.combinations(names, 2) for ka, kb in (("shape", "dtype"), ("dtype", "host"))]
    for fn, kw in OPS_FNS:
        names, weighted = tensors_of(fn), fn == "refine_pose_views_weighted"
        for cfg in configs_of(fn):
            case = lambda *faults: {"fn": fn, "kw": kw, "cfg": cfg, "faults": [list(f) for f in faults]}
            out += [case(("cfg", k)) for k in ("class", "resolve_views", "motion", "plain" if weighted else "confidence")]
            if fn == "refine_pose_views":
                out.append(case(("cfg", "window")))
            if weighted:
                out.append(case(("prior", "missing")))
            out += [case((w, "int")) for w in kw]
            out += [case(("pose", "other"))] + [case((k, "missing")) for k in POSE_KEYS]
            out += [case(("obs", "rows")), case(("obs", "wide"))]
            out += [case((n, k)) for n in names for k in KINDS]
            out += [case(*p) for p in pairs(names)]
    for fn in COLLECTORS:
        names = tensors_of(fn)
        case = lambda *faults: {"fn": fn, "kw": {}, "cfg": None, "faults": [list(f) for f in faults]}
        out += [case(("fused", "other"))] + [case((k, "missing")) for k in FUSED_KEYS]
        out += [case(("type_count", k)) for k in ("short", "zero", "rows")] + [case(("xyc", "odd")), case(("xyc", "pairs")), case(("table", "few"))]
        if fn == "rig_bearings_weighted":
            out.append(case(("confidence", "other")))
        out += [case((n, k)) for n in names for k in kinds_of(n)]
        out += [case(*p) for p in pairs(names)]
    return out


def _config(ops, name):
    kw = {}
    if "huber" in name:
        kw["huber_px"] = 1.5
    if "conf" in name:
        kw["confidence"] = ops.ConfidenceWeights(0.8, 0.4)
    return ops.WindowConfig(4, **kw) if name.startswith("window") else ops.RefineConfig(**kw)


def _config_fault(ops, name, kind):
    if kind == "class":
        return ops.ConfidenceWeights(0.8, 0.4)
    if kind == "window":
        return ops.WindowConfig(4)
    if kind == "resolve_views":
        return ops.RefineConfig(resolve_views=True, **({"confidence": ops.ConfidenceWeights(0.8, 0.4)} if "conf" in name else {}))
    if kind == "motion":
        return ops.WindowConfig(4, motion="constant_velocity")
    return _config(ops, {"plain": name.replace("_conf", ""), "confidence": name.split("_")[0] + "_conf"}[kind])


def _refine_tensors(each):
    sh = {"obs": (torch.float64, (B, MAX_OBJ, S, V, 2)), "prior": (torch.float64, (B, MAX_OBJ, S, V)), "views": (torch.float64, (B, MAX_OBJ, V, 14) if each else (V, 14)),
          "pose": (torch.float64, (B, MAX_OBJ, 12)), "assignment": (torch.int32, (B, MAX_OBJ, S)), "n_obj": (torch.int32, (B,)), "model": (torch.float64, (S, 3))}
    return {n: torch.zeros(shape, dtype=dtype).as_subclass(Device) for n, (dtype, shape) in sh.items()}


def _collector_tensors(ops):
    sh = {"table": (torch.uint8, (1, ops.STEREO_PAIR_BYTES)), "count": (torch.int32, (2 * PAIRS, K)), "xyc": (torch.float32, (2 * PAIRS, K, CAP, 3)),
          "match": (torch.int32, (PAIRS, K, CAP)), "member": (torch.int32, (PAIRS, K, CAP)), "object": (torch.int32, (K, CAP_F)), "n_fused": (torch.int32, (K,))}
    return {n: torch.zeros(shape, dtype=dtype).as_subclass(Device) for n, (dtype, shape) in sh.items()}


def run_ops(case):
    """The call of an ops case -> the OkpError's text.  The launch is replaced: a case that gets that far fails."""
    from object_keypoints_amd import ops
    fn, kw = case["fn"], dict(case["kw"])
    if fn in COLLECTORS:
        t = _collector_tensors(ops)
        fused, type_count, confidence = {k: t[k] for k in FUSED_KEYS}, [2, 1], ops.ConfidenceWeights(0.8, 0.4)
        for name, kind in case["faults"]:
            holder = fused if name in FUSED_KEYS else t
            if name == "fused":
                fused = None
            elif name == "confidence":
                confidence = (0.8, 0.4)
            elif name == "type_count":
                type_count = {"short": [2], "zero": [0, 1], "rows": [15, 1]}[kind]
            elif kind == "missing":
                del holder[name]
            elif (name, kind) == ("object", "shape"):                                 # (a column more is another cap_f: a row more is no [K,cap_f])
                holder[name] = torch.zeros((K + 1, CAP_F), dtype=torch.int32).as_subclass(Device)
            elif kind == "odd":                                                       # a tick with a left map and no right one
                t["count"], t["xyc"] = t["count"][:3], t["xyc"][:3]
            elif kind == "pairs":                                                     # more pairs than RIG_MAX_PAIRS
                t["count"], t["xyc"] = (torch.zeros((66,) + tuple(t[n].shape[1:]), dtype=t[n].dtype).as_subclass(Device) for n in ("count", "xyc"))
            elif kind == "few":                                                       # two calibrations for three pairs
                t["table"] = torch.zeros((2, ops.STEREO_PAIR_BYTES), dtype=torch.uint8).as_subclass(Device)
                t["count"], t["xyc"] = (torch.zeros((6,) + tuple(t[n].shape[1:]), dtype=t[n].dtype).as_subclass(Device) for n in ("count", "xyc"))
            else:
                holder[name] = _fault(holder[name], kind)
        args = (t["table"], t["count"], t["xyc"], t["match"], fused, type_count) + ((confidence,) if fn == "rig_bearings_weighted" else ())
    else:
        t = _refine_tensors(kw.get("each", fn == "refine_pose_views_each"))
        cfg, pose = _config(ops, case["cfg"]), {k: t[k] for k in POSE_KEYS}
        prior = t["prior"] if fn == "refine_pose_views_weighted" else None
        for name, kind in case["faults"]:
            holder = pose if name in POSE_KEYS else t
            if name == "cfg":
                cfg = _config_fault(ops, case["cfg"], kind)
            elif name in ("each", "wide"):
                kw[name] = 1
            elif name == "pose" and kind == "other":
                pose = None
            elif name == "prior" and kind == "missing":
                prior = None
            elif kind == "missing":
                del holder[name]
            elif kind == "rows":                                                      # more model rows than POSE_MAX_POINTS
                t["obs"] = torch.zeros((B, MAX_OBJ, 17, V, 2), dtype=torch.float64).as_subclass(Device)
            elif kind == "wide":                                                      # one view more than the entry point takes
                t["obs"] = torch.zeros((B, MAX_OBJ, S, (ops.REFINE_MAX_VIEWS if fn in ("refine_pose_views", "refine_pose_views_each") else ops.REFINE_WIDE_MAX_VIEWS) + 1, 2),
                                       dtype=torch.float64).as_subclass(Device)
            else:
                holder[name] = _fault(holder[name], kind)
                if name == "prior":
                    prior = holder[name]
        args = (t["obs"],) + ((prior,) if fn == "refine_pose_views_weighted" else ()) + (t["views"], pose, t["n_obj"], t["model"], cfg)

    def launch(*a):
        raise AssertionError(f"{case}: reached the launch")
    real, ops._dispatch = ops._dispatch, launch
    try:
        getattr(ops, fn)(*args, **kw)
    except ops.OkpError as e:
        return str(e)
    finally:
        ops._dispatch = real
    raise AssertionError(f"{case}: not refused")
