"""CPU-side checks of the views refinements weighted by the peaks' confidences (okp_refine_pose_views_weighted, okp_rig_bearings_weighted,
okp_window_push_weighted, okp_window_push_views_weighted; ops.ConfidenceWeights and the confidence keyword of ops.RefineConfig and
ops.WindowConfig): the names exist in the header, the ctypes table and the op registry; every refusal is raised by the C entry point, with its
argument and function named, before any device pointer is touched; the configs, the wrappers and the pipelines name what they refuse; with the
keyword a step makes the weighted launches, as many as before, and without it the launches it made before (recording stubs, as
tests/test_refine_robust_args.py); the NumPy specification with all priors 1.0 IS the two unweighted specifications; the cases of the GPU
test (tests/refine_weighted_cases.py) are away from every decision; the two accuracy statements of the stage; the rig's window and the sharded
tick; and the build's report that no instance of the weighted kernels uses scratch memory.  No GPU needed."""
import os
import re

import numpy as np
import pytest
import torch

import refine_robust_cases as robust_cases
import refine_robust_spec as robust_spec
import refine_views_cases as views_cases
import refine_views_spec as views_spec
import refine_weighted_cases as cases
import refine_weighted_spec as spec
import test_object_stage_wiring as wiring
import test_refine_robust_args as rra
import window_cases
import window_spec
import window_views_cases
import window_views_spec

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 64                # a non-NULL "device" address the host never dereferences: the checks that follow must stop at the NULL buffers
NAMES = ("okp_refine_pose_views_weighted", "okp_refine_pose_views_weighted_wide", "okp_rig_bearings_weighted", "okp_window_push_weighted", "okp_window_push_views_weighted")
CASES = cases.all_cases()


def _lib():
    from object_keypoints_amd import _lib, build
    build.build()
    return _lib


def test_header_ctypes_table_and_op_registry_agree_on_the_names():
    lib = _lib()
    text = open(os.path.join(REPO, "include", "okp.h")).read()
    declared = set(re.findall(r"\b(okp_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S)))
    additions = text[text.index("additions at 7"):text.index("*/", text.index("additions at 7"))]
    from object_keypoints_amd import _ctypes_ops
    T = lib.torch_ops()
    assert T is not None
    for name in NAMES:
        assert name in declared and name in {n for n, _, _ in lib.SIGNATURES} and hasattr(lib.lib(), name) and name in additions, name
        assert callable(getattr(_ctypes_ops, name[4:])) and hasattr(T, name[4:]), name
    assert lib.lib().okp_abi_version() == 7 and re.search(r"#define OKP_ABI_VERSION 7\b", text)
    schema = str(T.refine_pose_views_weighted.default._schema)
    assert schema.startswith("okp::refine_pose_views_weighted(Tensor obs, Tensor prior, Tensor views, int views_each, ")
    for arg, mark in zip(("pose_out", "fit", "n_obs", "information", "status"), "abcfg"):
        assert f"Tensor({mark}!) {arg}" in schema, (arg, schema)
    assert "Tensor(d!)? n_inlier" in schema and "Tensor(e!)? weight" in schema
    for op, outs in (("rig_bearings_weighted", ("obs", "prior")), ("window_push_weighted", ("win_obs", "win_prior", "win_views", "win_i", "n_views", "start")),
                     ("window_push_views_weighted", ("win_obs", "win_prior", "win_views", "win_i", "n_views", "start"))):
        schema = str(getattr(T, op).default._schema)
        for arg, mark in zip(outs, "abcdef"):
            assert f"Tensor({mark}!) {arg}" in schema, (op, arg, schema)
    flat = " ".join(text.replace("\n *", " ").split())
    for word in ("s' = a * (e_u*e_u + e_v*e_v)", "sigma_px / sqrt(a)", "H = sum a j^T j", "H = sum (a w_h) j^T j", "s' <= c2", "c / sqrt(s')", "stays w_h alone",
                 "c >= conf_ref ? 1.0 : ((c > conf_floor ? c : conf_floor) / conf_ref)", "a NaN c falls to the floor", "BIT FOR BIT those of the unweighted entry point",
                 "NaN, infinite or <= 0 makes the object OKP_REFINE_SKIPPED", "ASSUMED", "not measured on real data", "about 15.8", "Priors do not detect outliers"):
        assert word in flat, word
    # the four "Limits" sentences say what is now true, and the statements the earlier tests read are still there
    for word in ("the peaks' confidences are not used unless the weighted entry points are called", "do not use the peaks' confidences unless okp_refine_pose_views_weighted",
                 "unless the ring is kept by okp_window_push_weighted", "or the ring is kept by okp_window_push_views_weighted"):
        assert word in flat, word


# ---- the argument checks of the four entry points -----------------------------------------------------------------------------------------------

REFINE_POINTERS = ("obs", "prior", "views", "pose", "assignment", "n_obj", "model", "pose_out", "fit", "n_obs", "n_inlier", "weight", "information", "status")


def _refine_call(L, views_each=0, sigma_px=0.25, huber_px=0.5, iters=6, damping=1e-9, B=2, max_obj=4, S=4, V=8, null=None, overlap=False, wide=False):
    p = {name: (None if name == null else FAKE * (1 + i) * 4096) for i, name in enumerate(REFINE_POINTERS)}
    if overlap:
        p["pose_out"] = p["pose"] + 8
    entry = L.okp_refine_pose_views_weighted_wide if wide else L.okp_refine_pose_views_weighted
    return entry(p["obs"], p["prior"], p["views"], views_each, p["pose"], p["assignment"], p["n_obj"], p["model"], sigma_px, huber_px, iters,
                                            damping, B, max_obj, S, V, p["pose_out"], p["fit"], p["n_obs"], p["n_inlier"], p["weight"], p["information"], p["status"], None)


def test_the_refinement_checks_its_arguments_before_any_device_call():
    """Every call here carries a null required pointer or an overlap, so none can reach the launch - on either side of V = 64."""
    L = _lib().lib()
    err = L.okp_last_error
    fn = b"okp_refine_pose_views_weighted"
    nan, inf = float("nan"), float("inf")
    for V in (8, 200):
        bad = lambda **kw: _refine_call(L, null="status", **dict(dict(V=V), **kw))
        assert bad() == -1 and b"null status" in err() and fn in err()
        assert bad(views_each=1, iters=1, damping=0.0, S=16, B=1, max_obj=1, huber_px=0.0) == -1 and b"null status" in err()      # the edges are allowed
        for v in (0, -1):
            assert bad(B=v) == -1 and f"B = {v}".encode() in err() and fn in err()
            assert bad(max_obj=v) == -1 and f"max_obj = {v}".encode() in err()
        for v in (0, 17, -3):
            assert bad(S=v) == -1 and f"S = {v} ".encode() in err()
            assert bad(iters=v) == -1 and f"iters = {v} ".encode() in err()
        for v in (0.0, -0.25, nan, inf):
            assert bad(sigma_px=v) == -1 and b"sigma_px = " in err() and fn in err()
        for v in (-0.5, nan, inf, -inf):
            assert bad(huber_px=v) == -1 and b"huber_px = " in err() and fn in err()
        for v in (-1e-12, nan, inf):
            assert bad(damping=v) == -1 and b"damping = " in err()
        for v in (2, -1, 7):
            assert bad(views_each=v) == -1 and f"views_each = {v};".encode() in err()
        for name in REFINE_POINTERS:
            assert _refine_call(L, V=V, null=name) == -1 and f"null {name}".encode() in err() and fn in err(), name
        assert _refine_call(L, V=V, overlap=True) == -1 and b"pose_out overlaps pose" in err() and fn in err()
    for v in (0, 513, -2):
        assert _refine_call(L, V=v, null="status") == -1 and f"V = {v} outside [1, 512]".encode() in err() and fn in err()
    assert _refine_call(L, V=512, null="prior") == -1 and b"null prior" in err()
    fn = b"okp_refine_pose_views_weighted_wide"                          # the wide kernel whatever V is: the same refusals under its own name
    for V in (8, 200):
        for name in REFINE_POINTERS:
            assert _refine_call(L, V=V, null=name, wide=True) == -1 and f"null {name}".encode() in err() and fn in err(), name
        for kw, word in ((dict(B=0), b"B = 0"), (dict(S=17), b"S = 17 "), (dict(iters=0), b"iters = 0 "), (dict(sigma_px=0.0), b"sigma_px = "), (dict(huber_px=-1.0), b"huber_px = "),
                         (dict(damping=-1.0), b"damping = "), (dict(views_each=2), b"views_each = 2;"), (dict(V=513), b"V = 513 outside [1, 512]")):
            assert _refine_call(L, null="status", wide=True, **dict(dict(V=V), **kw)) == -1 and word in err() and fn in err(), kw
        assert _refine_call(L, V=V, overlap=True, wide=True) == -1 and b"pose_out overlaps pose" in err() and fn in err()
    assert _refine_call(L, V=65, huber_px=0.0, null="prior") == -1 and b"null prior" in err()


BEARINGS_POINTERS = ("count", "xyc", "match", "member", "object", "n_fused", "table", "obs", "prior")


def _bearings_call(L, n_table=1, n_pairs=4, K=3, cap=8, cap_f=12, type_count=(1, 3), conf_ref=8.0, conf_floor=0.5, null=None):
    import ctypes
    p = {name: (None if name == null else FAKE * (1 + i) * 4096) for i, name in enumerate(BEARINGS_POINTERS)}
    tc = (ctypes.c_int32 * max(1, len(type_count)))(*type_count) if type_count is not None else None
    return L.okp_rig_bearings_weighted(p["count"], p["xyc"], p["match"], p["member"], p["object"], p["n_fused"], p["table"], n_table, n_pairs, K, cap, cap_f, tc, conf_ref,
                                       conf_floor, p["obs"], p["prior"], None)


def test_the_bearings_check_their_arguments_before_any_device_call():
    L = _lib().lib()
    err = L.okp_last_error
    fn = b"okp_rig_bearings_weighted"
    nan, inf = float("nan"), float("inf")
    bad = lambda **kw: _bearings_call(L, null="prior", **kw)
    assert bad() == -1 and b"null prior" in err() and fn in err()
    assert bad(conf_floor=8.0) == -1 and b"null prior" in err()                                  # floor == ref is allowed
    for v in (0.0, -1.0, nan, inf):
        assert bad(conf_ref=v) == -1 and b"conf_ref = " in err() and fn in err()
    for v in (0.0, -0.5, nan, 8.5, inf):
        assert bad(conf_floor=v) == -1 and b"conf_floor = " in err() and fn in err()
    for v in (0, 33):
        assert bad(n_pairs=v) == -1 and f"n_pairs = {v}".encode() in err() and fn in err()
    assert bad(K=1) == -1 and b"K = 1" in err()
    assert bad(type_count=None) == -1 and b"null type_count" in err()
    assert bad(type_count=(1, 0)) == -1 and b"type_count[1] = 0" in err()
    assert bad(cap=0) == -1 and b"cap = 0" in err() and bad(cap=257) == -1 and b"cap = 257" in err()
    assert bad(cap_f=0) == -1 and b"cap_f = 0" in err()
    assert bad(n_table=0) == -1 and b"n_table = 0" in err() and bad(n_table=2) == -1 and b"n_table = 2" in err()
    for name in BEARINGS_POINTERS:
        assert _bearings_call(L, null=name) == -1 and f"null {name}".encode() in err() and fn in err(), name


PUSH_POINTERS = ("tab", "assignment", "status", "meas_of", "track_i", "track_f", "track_pose", "T_WC", "win_obs", "win_prior", "win_views", "win_i", "n_views", "start")


def _push_call(L, B=2, max_obj=4, S=4, T=3, W=4, min_views=2, max_speed=0.5, conf_ref=0.8, conf_floor=0.4, fx=62.0, fy=62.0, cam=True, null=None):
    import ctypes
    from object_keypoints_amd import _lib
    p = {name: (None if name == null else FAKE * (1 + i) * 4096) for i, name in enumerate(PUSH_POINTERS)}
    c = ctypes.byref(_lib.okp_camera(fx, fy, 32.0, 32.0, (0.0, 0.0, 0.0, 0.0), 0)) if cam else None
    return L.okp_window_push_weighted(p["tab"], p["assignment"], p["status"], p["meas_of"], p["track_i"], p["track_f"], p["track_pose"], p["T_WC"], c, B, max_obj, S, T, W,
                                      min_views, max_speed, conf_ref, conf_floor, p["win_obs"], p["win_prior"], p["win_views"], p["win_i"], p["n_views"], p["start"], None)


def test_the_push_checks_its_arguments_before_any_device_call():
    L = _lib().lib()
    err = L.okp_last_error
    fn = b"okp_window_push_weighted"
    nan, inf = float("nan"), float("inf")
    bad = lambda **kw: _push_call(L, null="win_prior", **kw)
    assert bad() == -1 and b"null win_prior" in err() and fn in err()
    for v in (0.0, -1.0, nan, inf):
        assert bad(conf_ref=v) == -1 and b"conf_ref = " in err() and fn in err()
    for v in (0.0, -0.5, nan, 0.9, inf):
        assert bad(conf_floor=v) == -1 and b"conf_floor = " in err() and fn in err()
    for kw, word in ((dict(B=0), b"B = 0"), (dict(max_obj=0), b"max_obj = 0"), (dict(S=17), b"S = 17"), (dict(T=65), b"T = 65"), (dict(W=65), b"W = 65"),
                     (dict(min_views=5), b"min_views = 5"), (dict(max_speed=0.0), b"max_speed = 0"), (dict(max_speed=nan), b"max_speed = "), (dict(cam=False), b"null cam"),
                     (dict(fx=0.0), b"cam fx = 0")):
        assert bad(**kw) == -1 and word in err() and fn in err(), kw
    for name in PUSH_POINTERS:
        assert _push_call(L, null=name) == -1 and f"null {name}".encode() in err() and fn in err(), name


PUSH_VIEWS_POINTERS = ("obs", "prior", "assignment", "status", "meas_of", "track_i", "track_f", "track_pose", "T_WB", "views", "win_obs", "win_prior", "win_views", "win_i",
                       "n_views", "start")


def _push_views_call(L, B=1, max_obj=4, S=4, T=3, W=4, V=8, min_views=2, max_speed=0.5, null=None):
    p = {name: (None if name == null else FAKE * (1 + i) * 4096) for i, name in enumerate(PUSH_VIEWS_POINTERS)}
    return L.okp_window_push_views_weighted(p["obs"], p["prior"], p["assignment"], p["status"], p["meas_of"], p["track_i"], p["track_f"], p["track_pose"], p["T_WB"], p["views"],
                                            B, max_obj, S, T, W, V, min_views, max_speed, p["win_obs"], p["win_prior"], p["win_views"], p["win_i"], p["n_views"], p["start"], None)


def test_the_push_of_a_rig_checks_its_arguments_before_any_device_call():
    L = _lib().lib()
    err = L.okp_last_error
    fn = b"okp_window_push_views_weighted"
    bad = lambda **kw: _push_views_call(L, null="win_prior", **kw)
    assert bad() == -1 and b"null win_prior" in err() and fn in err()
    for kw, word in ((dict(B=0), b"B = 0"), (dict(max_obj=0), b"max_obj = 0"), (dict(S=0), b"S = 0"), (dict(T=0), b"T = 0"), (dict(V=65), b"V = 65"), (dict(W=0), b"W = 0"),
                     (dict(W=64, V=16), b"W * V = 64 x 16 = 1024"), (dict(min_views=0), b"min_views = 0"), (dict(max_speed=-1.0), b"max_speed = -1")):
        assert bad(**kw) == -1 and word in err() and fn in err(), kw
    for name in PUSH_VIEWS_POINTERS:
        assert _push_views_call(L, null=name) == -1 and f"null {name}".encode() in err() and fn in err(), name


# ---- ops and the pipelines ----------------------------------------------------------------------------------------------------------------------

def test_the_configs_take_confidence_and_name_what_they_refuse():
    from object_keypoints_amd import ops
    cw = ops.ConfidenceWeights(8, 0.5)
    assert (cw.ref, cw.floor) == (8.0, 0.5) and isinstance(cw.ref, float) and repr(cw) == "ConfidenceWeights(ref=8.0, floor=0.5)"
    assert ops.ConfidenceWeights(2.0, 2.0).floor == 2.0 and ops.ConfidenceWeights(np.float32(4), np.float64(1)).ref == 4.0
    for v in (True, "high", None, [8.0], 0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ops.OkpError, match="ConfidenceWeights: ref = "):
            ops.ConfidenceWeights(v, 0.5)
    for v in (False, "low", None, 0.0, -0.5, float("nan"), 8.5, float("inf")):
        with pytest.raises(ops.OkpError, match="ConfidenceWeights: floor = "):
            ops.ConfidenceWeights(8.0, v)
    assert ops.RefineConfig().confidence is None and ops.WindowConfig(8).confidence is None
    assert repr(ops.RefineConfig()) == "RefineConfig(sigma_px=0.25, sigma_z=0.05, iters=6, damping=1e-09)"                       # unchanged without the keyword
    assert repr(ops.WindowConfig(8, 3, 0.2)) == "WindowConfig(ticks=8, min_views=3, max_speed=0.2, sigma_px=0.25, iters=6, damping=1e-09)"
    assert ops.RefineConfig(confidence=cw).confidence is cw and ops.WindowConfig(8, confidence=cw, huber_px=0.5).confidence is cw
    assert repr(ops.RefineConfig(confidence=cw)).endswith(", confidence=ConfidenceWeights(ref=8.0, floor=0.5))")
    assert repr(ops.WindowConfig(8, huber_px=1.5, confidence=cw)).endswith(", huber_px=1.5, confidence=ConfidenceWeights(ref=8.0, floor=0.5))")
    for v in (True, 8.0, (8.0, 0.5), "on"):
        with pytest.raises(ops.OkpError, match="RefineConfig: confidence = "):
            ops.RefineConfig(confidence=v)
        with pytest.raises(ops.OkpError, match="WindowConfig: confidence = "):
            ops.WindowConfig(8, confidence=v)
    with pytest.raises(TypeError):
        ops.WindowConfig(8, 2, 0.5, 0.25, 6, 1e-9, None, cw)              # a keyword, like huber_px


def test_the_wrappers_refuse_before_the_launch():
    from object_keypoints_amd import ops
    cw = ops.ConfidenceWeights(8.0, 0.5)
    obs, prior = torch.zeros(1, 2, 4, 6, 2, dtype=torch.float64), torch.ones(1, 2, 4, 6, dtype=torch.float64)
    views = torch.zeros(6, 14, dtype=torch.float64)
    pose = {"pose": torch.zeros(1, 2, 12, dtype=torch.float64), "assignment": torch.zeros(1, 2, 4, dtype=torch.int32)}
    n_obj, model = torch.zeros(1, dtype=torch.int32), torch.zeros(4, 3, dtype=torch.float64)
    with pytest.raises(ops.OkpError, match="obs must be a device tensor"):
        ops.refine_pose_views_weighted(obs, prior, views, pose, n_obj, model, ops.RefineConfig(confidence=cw))
    with pytest.raises(ops.OkpNotOffered, match="cfg.confidence: refine_pose_views_weighted takes it"):      # a config without the keyword: not uniform weights quietly
        ops.refine_pose_views_weighted(obs, prior, views, pose, n_obj, model, ops.RefineConfig())
    for fn, table in ((ops.refine_pose_views, views), (ops.refine_pose_views_each, torch.zeros(1, 2, 6, 14, dtype=torch.float64)), (ops.refine_pose_views_wide, views)):
        with pytest.raises(ops.OkpNotOffered, match="cfg.confidence: refine_pose_views_weighted takes it"):  # ... and the keyword is not dropped quietly either
            fn(obs, table, pose, n_obj, model, ops.RefineConfig(confidence=cw))
    with pytest.raises(ops.OkpError, match="cfg must be an ops.RefineConfig or an ops.WindowConfig"):
        ops.refine_pose_views_weighted(obs, prior, views, pose, n_obj, model, cw)
    with pytest.raises(ops.OkpError, match="wide = 1 must be True"):
        ops.refine_pose_views_weighted(obs, prior, views, pose, n_obj, model, ops.RefineConfig(confidence=cw), wide=1)
    tab = torch.zeros(1, 2, 4, 4, dtype=torch.float64)
    cam = ops.make_camera(np.array([[62.0, 0, 32], [0, 62.0, 32], [0, 0, 1]]), np.zeros(4))
    with pytest.raises(ops.OkpNotOffered, match="confidence: not offered for the single-camera refinement .*refine_pose_views_weighted takes it"):
        ops.refine_pose(tab, pose, n_obj, model, cam, ops.RefineConfig(confidence=cw))
    with pytest.raises(ops.OkpNotOffered, match="confidence: not offered for the single-camera refinement"):
        ops.refine_assignments(tab, pose, n_obj, model, [1, 1, 1], cam, ops.RefineConfig(confidence=cw, resolve_assignment=True))
    with pytest.raises(ops.OkpError, match="confidence must be an ops.ConfidenceWeights"):
        ops.rig_bearings_weighted(None, None, None, None, None, [1, 1], (8.0, 0.5))
    with pytest.raises(ops.OkpError, match="prior: the bearings' priors .* go with a WindowConfig whose confidence is set"):
        ops.window_push_views({}, obs, None, None, {}, None, None, ops.WindowConfig(4), prior=prior)
    with pytest.raises(ops.OkpError, match="prior: the bearings' priors"):
        ops.window_push_views({}, obs, None, None, {}, None, None, ops.WindowConfig(4, confidence=cw))
    T = _lib().torch_ops()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        T.refine_pose_views_weighted(obs, prior, views, 0, pose["pose"], pose["assignment"], n_obj, model, 0.25, 0.0, 6, 1e-9, torch.zeros(1, 2, 12, dtype=torch.float64),
                                     torch.zeros(1, 2, 2, dtype=torch.float64), torch.zeros(1, 2, dtype=torch.int32), None, None, torch.zeros(1, 2, 36, dtype=torch.float64),
                                     torch.zeros(1, 2, dtype=torch.int32), 0)


def test_the_pipelines_offer_the_keyword_where_there_is_a_weighted_form():
    from object_keypoints_amd import ops
    cw = ops.ConfidenceWeights(8.0, 0.5)
    with pytest.raises(ops.OkpNotOffered, match="refine with confidence: not offered for one camera .*window=ops.WindowConfig") as refusal:
        rra._camera_pipeline(refine=ops.RefineConfig(confidence=cw))
    assert isinstance(refusal.value, ops.OkpError) and isinstance(refusal.value, TypeError)
    pipe = rra._camera_pipeline(refine=ops.RefineConfig(), window=ops.WindowConfig(4, confidence=cw))
    assert pipe.window.confidence is cw and pipe.refine.confidence is None
    assert rra._camera_pipeline(window=ops.WindowConfig(4, confidence=cw, huber_px=0.5)).window.huber_px == 0.5            # with or without huber_px
    rig = rra._rig_pipeline(None, ops.RefineConfig(confidence=cw, huber_px=0.75))
    assert rig.refine.confidence is cw and rig._stage.bearings_confidence is cw
    assert rra._rig_pipeline(None, ops.RefineConfig())._stage.bearings_confidence is None


# ---- the wiring ------------------------------------------------------------------------------------------------------------------------------------

class Recorder(rra.Recorder):
    """tests/test_refine_robust_args.py's recorder plus the weighted stubs: the state with its ring of priors, the bearings with their priors,
    and the weighted entry point of the binding."""

    def __init__(self, monkeypatch):
        super().__init__(monkeypatch)
        from object_keypoints_amd import ops
        monkeypatch.setattr(ops, "rig_bearings_weighted", self.rig_bearings_weighted)

    def label(self, v):
        from object_keypoints_amd import ops
        return "ConfidenceWeights" if isinstance(v, ops.ConfidenceWeights) else super().label(v)

    def window_state(self, B, max_tracks, S, ticks, device, **kw):
        st = super().window_state(B, max_tracks, S, ticks, device)
        if kw:
            assert kw == {"prior": True}
            self.trace[-1] = self.trace[-1][:-1] + ", prior=True)"
            st["win_prior"] = self.new("win_prior", (B, max_tracks, S, ticks))
        return st

    def window_push(self, state, tab, assignment, status, track, T_WC, cam, cfg):
        out = super().window_push(state, tab, assignment, status, track, T_WC, cam, cfg)
        if "win_prior" in state:
            self.trace[-1] = self.trace[-1][:-1] + f", win_prior={self.label(state['win_prior'])}, confidence={cfg.confidence})"
        return out

    def rig_bearings_weighted(self, table, count, xyc, match, fused, type_count, confidence):
        self.call("rig_bearings_weighted", table=table, count=count, xyc=xyc, match=match, member=fused["member"], type_count=type_count, confidence=confidence)
        shape = (1, fused["fused"].shape[1], 1 + sum(type_count), xyc.shape[0])
        return self.new("obs", shape + (2,)), self.new("prior", shape)

    def refine_pose_views_weighted(self, obs, prior, views, views_each, pose, assignment, n_obj, model, sigma_px, huber_px, iters, damping, pose_out, fit, n_obs, n_inlier,
                                   weight, information, status, stream):
        outputs = dict(pose=pose_out, fit=fit, n_obs=n_obs, information=information, status=status)
        if n_inlier is not None:
            outputs.update(n_inlier=n_inlier, weight=weight)
        self._launch("refine_pose_views_weighted", outputs, obs=obs, prior=prior, views=views, views_each=views_each, pose=pose, assignment=assignment, n_obj=n_obj,
                     model=model, sigma_px=sigma_px, huber_px=huber_px, iters=iters, damping=damping)


def test_the_window_step_makes_the_weighted_launches_with_the_keyword_and_the_plain_ones_without(monkeypatch):
    from object_keypoints_amd import ops
    rec = Recorder(monkeypatch)
    cw = ops.ConfidenceWeights(0.8, 0.4)
    T, S, W = wiring.TRACKS, 1 + sum(wiring.CFG), 4
    traces = {}
    plain_keys = ["pose", "fit", "n_obs", "n_views", "information", "status", "pose_C", "win_obs", "win_views", "win_i"]
    for key, window in (("off", ops.WindowConfig(W)), ("on", ops.WindowConfig(W, confidence=cw)), ("huber", ops.WindowConfig(W, confidence=cw, huber_px=0.5))):
        pipe = rra._camera_pipeline(window=window)
        rec.name("model", pipe._model_host)
        maps = [rec.new("heat", (wiring.N, 1 + len(wiring.CFG), wiring.HW, wiring.HW), torch.float32), rec.new("depth", (wiring.N, 1 + len(wiring.CFG), wiring.HW, wiring.HW), torch.float32),
                rec.new("centers", (wiring.N, len(wiring.CFG), 2, wiring.HW, wiring.HW), torch.float32)]
        del rec.trace[:]
        out = pipe.postprocess_device(*maps, range_flag=rec.new("range_flag", (1,), torch.int32), camera_pose=rec.new("camera_pose", (wiring.N, 12)))
        traces[key] = list(rec.trace)
        w = out["window"]
        state = pipe._stage.window.state(torch.device("cpu"), wiring.N, S)
        tensors = "views=win_views, {}pose=window.start, assignment=win_assignment, n_obj=win_n, model=model, sigma_px=0.25, "
        if key == "off":                                                  # exactly the parent's launch, keys and state
            assert rra._launches(rec) == ["launch refine_pose_views_each(obs=win_obs, " + tensors.format("") + "iters=6, damping=1e-09)"]
            assert list(w) == plain_keys and sorted(state) == ["win_assignment", "win_i", "win_n", "win_obs", "win_views"]
            assert not [line for line in rec.trace if "prior" in line or "confidence" in line]
        else:
            huber = 0.5 if key == "huber" else 0.0
            assert rra._launches(rec) == ["launch refine_pose_views_weighted(obs=win_obs, prior=win_prior, " + tensors.format("views_each=1, ") + f"huber_px={huber}, iters=6, damping=1e-09)"]
            assert list(w) == plain_keys + (["n_inlier", "weight"] if huber else []) + ["prior"] and rec.label(w["prior"]) == "win_prior"
            assert sorted(state) == ["win_assignment", "win_i", "win_n", "win_obs", "win_prior", "win_views"]
            assert tuple(w["fit"].shape) == (wiring.N, T, 4 if huber else 2)
            push = [line for line in rec.trace if line.startswith("window_push(")]
            assert len(push) == 1 and push[0].endswith("win_prior=win_prior, confidence=ConfidenceWeights(ref=0.8, floor=0.4))")
        assert w["pose"] is rec.outputs["pose"] and w["status"] is rec.outputs["status"]
    assert len(traces["on"]) == len(traces["off"]) == len(traces["huber"])                     # the same number of launches
    # ... in the same order, and nothing else differs (by op: a stub labels a tensor by its storage address, which a later, unnamed one may reuse)
    ops_of = lambda lines: [line.split("(")[0].replace("refine_pose_views_weighted", "refine_pose_views_each") for line in lines]
    assert ops_of(traces["on"]) == ops_of(traces["off"]) == ops_of(traces["huber"])


def test_the_rig_tick_makes_the_weighted_launches_with_the_keyword_and_the_plain_ones_without(monkeypatch):
    from object_keypoints_amd import ops
    rec = Recorder(monkeypatch)
    cw = ops.ConfidenceWeights(8.0, 0.5)
    traces = {}
    S, V = 1 + sum(wiring.RIG_CFG), 2 * wiring.PAIRS
    for key, refine in (("off", ops.RefineConfig()), ("on", ops.RefineConfig(confidence=cw)), ("huber", ops.RefineConfig(confidence=cw, huber_px=0.75))):
        pipe = rra._rig_pipeline(rec, refine)
        for label, t in (("table", pipe._table_host), ("rig_poses", pipe._poses_host), ("model", pipe._model_host), ("rig_views", pipe._views.host)):
            rec.name(label, t)
        del rec.trace[:]
        out = pipe.tick_device(torch.zeros((2 * wiring.PAIRS, 3, 16, 16)))
        traces[key] = list(rec.trace)
        r = out["refine"]
        tensors = "views=rig_views, {}pose=pose.pose, assignment=pose.assignment, n_obj=fused.n_obj, model=model, sigma_px=0.25, "
        before = rec.trace[rec.trace.index(rra._launches(rec)[0]) - 1]
        if key == "off":
            assert rra._launches(rec) == ["launch refine_pose_views(obs=obs, " + tensors.format("") + "iters=6, damping=1e-09)"]
            assert list(r) == ["pose", "fit", "n_obs", "information", "status", "obs"] and before.startswith("rig_bearings(")
        else:
            huber = 0.75 if key == "huber" else 0.0
            assert rra._launches(rec) == ["launch refine_pose_views_weighted(obs=obs, prior=prior, " + tensors.format("views_each=0, ") + f"huber_px={huber}, iters=6, damping=1e-09)"]
            assert list(r) == ["pose", "fit", "n_obs", "information", "status"] + (["n_inlier", "weight"] if huber else []) + ["obs", "prior"]
            assert before.startswith("rig_bearings_weighted(") and before.endswith("confidence=ConfidenceWeights)") and rec.label(r["prior"]) == "prior"
            assert tuple(r["prior"].shape) == (1, wiring.CAP_F, S, V) and tuple(r["fit"].shape) == (1, wiring.CAP_F, 4 if huber else 2)
        assert list(out)[-2:] == ["pose", "refine"] and r["pose"] is rec.outputs["pose"]
    assert len(traces["on"]) == len(traces["off"]) == len(traces["huber"])                     # still two launches
    ops_of = lambda lines: [line.split("(")[0].replace("_weighted", "") for line in lines]     # (by op: see the window's test)
    assert ops_of(traces["on"]) == ops_of(traces["off"]) == ops_of(traces["huber"])


def test_the_readers_list_the_priors_of_the_bearings():
    from object_keypoints_amd.perception import pipeline as pp
    nan = np.nan
    prior = np.full((2, 3, 4), nan)
    prior[1, 0, :3] = 1.0, 0.25, 0.0625
    prior[1, 2, 1] = 0.5
    rec = {"refine": np.zeros((2, 12)), "refine_fit": np.array([[nan] * 2, [2.0, 2.5]]), "refine_n_obs": np.array([0, 4]), "information": np.zeros((2, 36)),
           "refine_status": np.array([1, 0]), "refine_prior": prior}
    e = pp._rig_refine_entries(rec, 1, np.eye(4))
    assert e["refine_priors"] == [(0, 0, 1.0), (0, 1, 0.25), (0, 2, 0.0625), (2, 1, 0.5)] and pp._rig_refine_entries(rec, 0, None)["refine_priors"] == []
    assert "refine_priors" not in pp._rig_refine_entries({k: v for k, v in rec.items() if k != "refine_prior"}, 1, np.eye(4))
    win = {"window_status": np.array([0, 1]), "window_fit": np.array([[2.0, 2.5], [nan] * 2]), "window_pose": np.zeros((2, 12)), "window_pose_C": np.zeros((2, 12)),
           "window_n_views": np.array([4, 1]), "window_information": np.zeros((2, 36)), "window_prior": prior[::-1]}
    assert pp._window_entries(win, 0)["window_priors"] == e["refine_priors"] and pp._window_entries(win, 1)["window_priors"] == []
    assert pp._window_entries(win, 0, cameras=2)["window_priors"] == [(0, 0, 0, 1.0), (0, 0, 1, 0.25), (0, 1, 0, 0.0625), (2, 0, 1, 0.5)]     # (row, column, camera, prior)
    assert "window_priors" not in pp._window_entries({k: v for k, v in win.items() if k != "window_prior"}, 0)


# ---- the specification with all priors 1.0 is the unweighted specifications ---------------------------------------------------------------------------

def _equal(a, b):
    assert sorted(a) == sorted(b)
    for k in a:
        assert a[k].dtype == b[k].dtype and np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), k


def test_with_all_priors_one_the_specification_is_the_unweighted_ones_bit_for_bit():
    by = {c["name"]: c for c in robust_cases.all_cases()}
    for name in ("s5_v6", "s5_v14", "b3_obj64_n_0_5_64", "each_s5_v6", "crafted_statuses", "crafted_outliers"):
        c = by[name]
        ones = np.ones(c["obs"].shape[:-1])
        args = (c["views"], c["pose"], c["assignment"], c["n_obj"], c["model"])
        _equal(spec.refine_pose_views_weighted(c["obs"], ones, *args, **c["params"]), robust_spec.refine_pose_views_robust(c["obs"], *args, **c["params"]))
        plain = {k: v for k, v in c["params"].items() if k != "huber_px"}
        want = window_views_spec.refine_pose_views_wide(c["obs"], *args, **plain)
        _equal(spec.refine_pose_views_weighted(c["obs"], ones, *args, huber_px=0.0, **plain), want)
        assert (want["status"] == 0).any()
    c = views_cases.crafted_case()
    _equal(spec.refine_pose_views_weighted(c["obs"], np.ones(c["obs"].shape[:-1]), c["views"], c["pose"], c["assignment"], c["n_obj"], c["model"], huber_px=0.0, **c["params"]),
           views_spec.refine_pose_views(c["obs"], c["views"], c["pose"], c["assignment"], c["n_obj"], c["model"], **c["params"]))


def test_the_mapping_is_comparisons_and_one_division():
    f = lambda c: spec.prior_of(c, 8.0, 0.5)
    assert f(8.0) == 1.0 and f(16.0) == 1.0 and f(np.inf) == 1.0 and f(0.5) == 0.0625 and f(0.25) == 0.0625 and f(-3.0) == 0.0625 and f(np.nan) == 0.0625 and f(-np.inf) == 0.0625
    assert f(3.0) == 3.0 / 8.0 and f(np.float32(0.7)) == np.float64(np.float32(0.7)) / 8.0 and f(np.nextafter(8.0, 0.0)) < 1.0
    assert spec.prior_of(5.0, 1e-30, 1e-30) == 1.0 and spec.prior_of(0.0, 1e-30, 1e-30) == 1.0 and spec.prior_of(np.nan, 1e-30, 1e-30) == 1.0     # every prior exactly 1.0


# ---- the conditions of the GPU cases --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_the_cases_are_away_from_every_decision(case):
    out, diags = cases.reference(case["name"])
    robust = case["params"]["huber_px"] > 0.0
    compared = 0
    for (b, o), d in diags.items():
        status = int(out["status"][b, o])
        assert out["n_obs"][b, o] == d["n_obs"]
        if status == spec.SKIPPED:
            assert "pivot" not in d
            continue
        if status != 0:
            # a status of a scene: far from its decision as well (the crafted statuses are asserted below)
            if status == spec.REJECTED:
                slack = spec.SLACK * d["n_obs"]
                assert d["J_final"] - d["J_initial"] - slack > 1e-6 * (d["J_initial"] + slack), (b, o, d)
            else:
                assert case["kind"] == "crafted", (b, o, status)
            continue
        assert d["rows"] >= 3 and d["pivot"] > 1e-6 and d["min_qz"] >= 1e-3, (b, o, d)
        slack = spec.SLACK * d["n_obs"]
        assert abs(d["J_final"] - d["J_initial"] - slack) > 1e-6 * (d["J_initial"] + slack), (b, o, d)
        assert d["cond"] <= 1e8, (b, o, d["cond"])                    # the premise of the 1e-9 bar of tests/test_gpu_refine_weighted.py
        if robust:
            assert d["margin"] > 1e-6, (b, o, d["margin"])            # |s' - c2| > 1e-6 c2 at the final iterate
            assert out["n_inlier"][b, o] == d["n_obs"] - d["outliers_final"]
        compared += 1
    assert compared >= 1
    # the priors: every observation's is a positive finite number (but for the crafted bad ones), and garbage lies on entries that are not observations
    S = case["obs"].shape[2]
    row = (case["assignment"] >= 0) & (case["assignment"] < S)
    seen = np.isfinite(case["obs"]).all(axis=-1) & row[..., None]
    live = np.arange(case["obs"].shape[1])[None, :] < case["n_obj"][:, None]
    with np.errstate(invalid="ignore"):
        good = (case["prior"] > 0.0) & (case["prior"] < np.inf)
    if case["kind"] != "crafted_priors":
        assert good[seen & live[..., None, None]].all()
    if case["kind"] == "scene":
        assert ((~good[~seen]).any() or (~seen).sum() < 4) and len(np.unique(case["prior"][seen])) > 3
    ok = out["status"] == 0
    assert np.isnan(out["fit"][~ok]).all() and np.isfinite(out["fit"][ok]).all()
    if robust:
        w = out["weight"]
        assert np.isnan(w[~ok]).all() and not out["n_inlier"][~ok].any()
        assert (np.isfinite(w).sum(axis=(2, 3))[ok] == out["n_obs"][ok]).all() and ((w == 1.0).sum(axis=(2, 3))[ok] == out["n_inlier"][ok]).all()
        with np.errstate(invalid="ignore"):
            assert not (w > 1.0).any() and (w[np.isfinite(w)] > 0.0).all()


def test_the_cases_cover_the_shapes_the_kernels_can_go_wrong_at():
    by = {c["name"]: c for c in CASES}
    for loss in ("_plain", "_huber"):
        for prefix in ("", "each_"):
            assert [by[prefix + n + loss]["obs"].shape[2:4] for n in ("s4_v2", "s5_v6", "s5_v14", "s16_v64_iters16")] == [(4, 2), (5, 6), (5, 14), (16, 64)]
            assert by[prefix + "s16_v64_iters16" + loss]["params"]["iters"] == 16 and by[prefix + "s4_v2" + loss]["each"] == bool(prefix)
        c = by["b3_obj64_n_0_5_64" + loss]
        assert c["obs"].shape[:2] == (3, 64) and c["n_obj"].tolist() == [0, 5, 64] and (c["assignment"] < 0).any() and np.isnan(c["obs"]).any()
        for V in (65, 200, 512):
            for each in ("", "_each"):
                c = by[f"v{V}_s5{each}{loss}"]
                assert c["obs"].shape[2:4] == (5, V) and c["each"] == bool(each) and c["views"].ndim == (4 if each else 2) and (c["params"]["huber_px"] > 0) == (loss == "_huber")
    assert len({c["name"] for c in CASES}) == len(CASES)


def test_the_crafted_objects_are_what_their_lines_say():
    by = {c["name"]: c for c in CASES}
    for loss in ("_plain", "_huber"):
        c = by["crafted_statuses" + loss]
        out, _ = cases.reference(c["name"])
        assert out["status"][0].tolist() == c["want"] == [0, 1, 1, 1, 1, 2, 4, 8, 1]                    # one object per non-zero status
        assert np.isfinite(c["pose"][0, 8]).all() and np.isfinite(c["obs"][0, 8]).all() and out["n_obs"][0, 8] == 0      # past n_obj: finite garbage that is not read
        for V in (8, 65):
            c = by[f"crafted_priors_v{V}{loss}"]
            out, _ = cases.reference(c["name"])
            assert out["status"][0].tolist() == c["want"] == [0, 1, 1, 1, 1, 0, 1]
            seen = np.isfinite(c["obs"][0, 0]).all(axis=-1)
            assert (~seen).sum() >= 5 and not np.isfinite(c["prior"][0, 0][~seen]).all() and (c["prior"][0, 5][~seen] == 1.0).all()
            for o in (1, 2, 3, 4):                                        # ONE bad prior on a filled observation, nothing else differs from object 0
                differs = ~((c["prior"][0, o] == c["prior"][0, 0]) | (np.isnan(c["prior"][0, o]) & np.isnan(c["prior"][0, 0])))
                assert differs.sum() == 1 and seen[differs].all() and np.array_equal(out["pose"][0, o], c["pose"][0, o]) and out["n_obs"][0, o] == out["n_obs"][0, 0]
            for k in ("pose", "fit", "information"):                      # garbage on unfilled entries: no effect
                assert np.array_equal(out[k][0, 0], out[k][0, 5]), k
            assert np.isfinite(c["prior"][0, 6]).all() and np.isnan(out["pose"][0, 6]).all()


def test_the_confidences_are_away_from_the_thresholds_or_exactly_on_them():
    kinds = set()
    for c in cases.bearings_cases():
        conf = c["xyc"][..., 2].astype(np.float64)
        for bound in (c["conf_ref"], c["conf_floor"]):
            near = np.abs(conf - bound) <= 1e-6 * bound
            assert (conf[near] == bound).all()
        with np.errstate(invalid="ignore"):
            for kind, hit in (("at_ref", conf == c["conf_ref"]), ("at_floor", conf == c["conf_floor"]), ("nan", np.isnan(conf)), ("above", conf > c["conf_ref"]),
                              ("below", conf < c["conf_floor"]), ("between", (conf > c["conf_floor"]) & (conf < c["conf_ref"]))):
                if hit.any():
                    kinds.add(kind)
    assert kinds == {"at_ref", "at_floor", "nan", "above", "below", "between"}
    kinds = set()
    for seq in cases.push_sequences():
        conf = np.concatenate([t["tab"][..., 3].reshape(-1) for t in seq["ticks"]])
        conf = conf[np.isfinite(conf)]
        for bound in (seq["conf_ref"], seq["conf_floor"]):
            near = np.abs(conf - bound) <= 1e-6 * bound
            assert (conf[near] == bound).all()
        for kind, hit in (("at_ref", conf == seq["conf_ref"]), ("at_floor", conf == seq["conf_floor"]), ("above", conf > seq["conf_ref"]), ("below", conf < seq["conf_floor"])):
            if hit.any():
                kinds.add(kind)
    assert kinds == {"at_ref", "at_floor", "above", "below"}
    for make in (cases.rig_scene, cases.window_scene):                      # the accuracy scenes: 16, 4 and 1 against ref 16 and floor 0.5
        s = make()
        assert set(np.unique(s["prior"][np.isfinite(s["prior"])])) == {1.0, 0.25, 0.0625}


def test_the_pushes_write_a_prior_wherever_they_write_a_bearing():
    wraps = {cases.run_push_spec: 0, cases.run_push_views_spec: 0}
    for seq, run in [(s, cases.run_push_spec) for s in cases.push_sequences()] + [(s, cases.run_push_views_spec) for s in cases.push_views_sequences()]:
        snaps = run(seq)
        bare = dict(seq, ticks=[{k: v for k, v in tick.items() if k != "prior"} for tick in seq["ticks"]])
        plain = (window_cases.run_spec if run is cases.run_push_spec else window_views_cases.run_spec)(bare)
        wrapped, written = False, []
        for (state, out), (want, want_out) in zip(snaps, plain):
            for k in want:                                                # the unweighted state, bit for bit
                assert np.array_equal(state[k].view(np.uint8), want[k].view(np.uint8)), (seq["name"], k)
            assert np.array_equal(out["n_views"], want_out["n_views"])
            empty = np.isnan(state["win_obs"]).all(axis=-1)
            if run is cases.run_push_spec:                                # NaN exactly where win_obs is (NaN, NaN); in [floor / ref, 1] elsewhere
                assert np.array_equal(np.isnan(state["win_prior"]), empty), seq["name"]
                p = state["win_prior"][~empty]
                assert ((p >= seq["conf_floor"] / seq["conf_ref"]) & (p <= 1.0)).all()
                written.append(p)
            wrapped = wrapped or bool((state["win_i"][..., 2] == state["win_obs"].shape[3] // (seq["shape"][4] if len(seq["shape"]) == 6 else 1)).any())
        wraps[run] += wrapped
        if written and seq["shape"][0] > 1:                               # (the sequences of more than one stream: enough pushes for every kind of confidence)
            p = np.concatenate(written)
            assert (p == 1.0).any() and (p == seq["conf_floor"] / seq["conf_ref"]).any() and ((p > seq["conf_floor"] / seq["conf_ref"]) & (p < 1.0)).any(), seq["name"]
    assert min(wraps.values()) >= 2                                         # rings that fill, of both kinds
    events = set()
    for seq in cases.push_views_sequences():
        cases.run_push_views_spec(seq, events)
    assert {"freed", "new_id", "speed_reset", "missing_T_WB", "duplicate_row", "ring_wrap"} <= events
    events = set()
    for seq in window_cases.sequences():
        window_cases.run_spec(seq, events)
    assert {"freed", "new_owner", "speed_reset", "nan_T", "same_row_twice", "wrapped"} <= events


# ---- the accuracy statements ----------------------------------------------------------------------------------------------------------------------

def _statement(name, s, plain_fn, pick):
    p = dict(sigma_px=0.25, iters=6, damping=1e-9)
    uniform = plain_fn(s["obs"], s["views"], s["pose"], s["assignment"], s["n_obj"], s["model"], **p)
    weighted = spec.refine_pose_views_weighted(s["obs"], s["prior"], s["views"], s["pose"], s["assignment"], s["n_obj"], s["model"], huber_px=0.0, **p)
    assert (uniform["status"] == 0).all() and (weighted["status"] == 0).all()                  # every status is 0
    r0, p0 = cases.errors(pick(uniform["pose"]), s["truth"], s["model"])
    r1, p1 = cases.errors(pick(weighted["pose"]), s["truth"], s["model"])
    print(f"{name}, every bearing noised with 0.1 px / sqrt(a), a from {{1, 1/4, 1/16}} (median / worst):")
    print(f"  uniform least squares       rotation {np.median(r0):.2f} / {r0.max():.2f} deg, centre {1e3 * np.median(p0):.1f} / {1e3 * p0.max():.1f} mm")
    print(f"  each term weighted by a     rotation {np.median(r1):.2f} / {r1.max():.2f} deg, centre {1e3 * np.median(p1):.1f} / {1e3 * p1.max():.1f} mm")
    print(f"  objects that end worse in rotation under the weights: {int((r1 > r0).sum())} of {len(r0)} (expected: nothing is asserted per object)")
    assert np.median(r1) < np.median(r0) and r1.max() < r0.max() and np.median(p1) < np.median(p0)


def test_the_weights_improve_a_rig_tick_under_heteroscedastic_noise():
    """The figures printed here are the ones README.md and DESIGN.md quote (seed 90, 128 five-point objects in front of a rig of four pairs, exact
    bearings noised with 0.1 px / sqrt(a); the confidences are a x 16 against ConfidenceWeights(16, 0.5); 6 steps, sigma_px 0.25)."""
    _statement(f"rig of {robust_cases.RIG_PAIRS} pairs, {robust_cases.RIG_OBJECTS} objects, seed {robust_cases.RIG_SEED}", cases.rig_scene(), views_spec.refine_pose_views,
               lambda pose: pose[0])


def test_the_weights_improve_the_window_under_heteroscedastic_noise():
    """The same for the sliding window (seed 7, 64 valve-like objects, the camera 2 cm and 0.01 rad further every tick, 16 ticks)."""
    _statement(f"window of {robust_cases.WINDOW_TICKS} ticks, {robust_cases.WINDOW_OBJECTS} objects, seed {robust_cases.WINDOW_SEED}", cases.window_scene(),
               window_spec.refine_pose_views_each, lambda pose: pose[:, 0])


# ---- the rig's window and the sharded tick ------------------------------------------------------------------------------------------------------------

def _rig_window_recorder(monkeypatch):
    """tests/test_window_views_args.py's recorder plus the weighted stubs at the level of ops: the bearings with their priors, the state and the
    push with the ring of priors, and the weighted refinement (which records whether the wide instance was asked for)."""
    import test_window_views_args as wva
    from object_keypoints_amd import ops
    base = wva._recorder(monkeypatch)

    class Weighted(type(base)):
        def label(self, v):
            return "ConfidenceWeights" if isinstance(v, ops.ConfidenceWeights) else super().label(v)

        def rig_bearings_weighted(self, table, count, xyc, match, fused, type_count, confidence):
            self.call("rig_bearings_weighted", table=table, count=count, xyc=xyc, match=match, member=fused["member"], type_count=type_count, confidence=confidence)
            shape = (1, fused["fused"].shape[1], 1 + sum(type_count), xyc.shape[0])
            return self.new("obs", shape + (2,)), self.new("prior", shape)

        def window_views_state(self, B, max_tracks, S, ticks, n_views, device, **kw):
            st = super().window_views_state(B, max_tracks, S, ticks, n_views, device)
            if kw:
                assert kw == {"prior": True}
                self.trace[-1] = self.trace[-1][:-1] + ", prior=True)"
                st["win_prior"] = self.new("win_prior", (B, max_tracks, S, ticks * n_views))
            return st

        def window_push_views(self, state, obs, assignment, status, track, T_WB, views, cfg, **kw):
            out = super().window_push_views(state, obs, assignment, status, track, T_WB, views, cfg)
            if kw:
                assert list(kw) == ["prior"]
                self.trace[-1] = self.trace[-1][:-1] + f", prior={self.label(kw['prior'])}, win_prior={self.label(state['win_prior'])})"
            return out

        def refine_pose_views_weighted(self, obs, prior, views, pose, n_obj, model, cfg, each=False, wide=False):
            self.call("refine_pose_views_weighted", obs=obs, prior=prior, views=views, pose=pose["pose"], assignment=pose["assignment"], n_obj=n_obj, model=model, cfg=cfg,
                      each=each, wide=wide)
            b, t = obs.shape[:2]
            where = "window" if each else "refine"
            return {"pose": self.new(where + ".pose", (b, t, 12)), "fit": self.new(where + ".fit", (b, t, 2)), "n_obs": self.new(where + ".n_obs", (b, t), torch.int32),
                    "information": self.new(where + ".information", (b, t, 36)), "status": self.new(where + ".status", (b, t), torch.int32)}

    rec = Weighted(monkeypatch)
    for name in ("rig_bearings_weighted", "window_views_state", "window_push_views", "refine_pose_views_weighted"):
        monkeypatch.setattr(ops, name, getattr(rec, name))
    return rec


@pytest.mark.parametrize("refine", (False, True), ids=("window_alone", "with_refine"))
def test_the_rig_window_makes_the_weighted_launches_with_the_keyword_and_the_plain_ones_without(monkeypatch, refine):
    import test_window_views_args as wva
    from object_keypoints_amd import ops
    cw = ops.ConfidenceWeights(15.8, 1.0)
    traces, outs, states = {}, {}, {}
    for key in ("off", "on"):
        rec = _rig_window_recorder(monkeypatch)                       # (a recorder of its own: no label of an earlier tick's tensor is left to be reused)
        kw = {"confidence": cw} if key == "on" else {}
        pipe = wva._rig_pipeline(rec, refine=ops.RefineConfig(**kw) if refine else None, rig_window=ops.WindowConfig(4, **kw))
        for label, t in (("table", pipe._table_host), ("rig_poses", pipe._poses_host), ("model", pipe._model_host), ("rig_views", pipe._views.host)):
            rec.name(label, t)
        outs[key] = pipe.tick_device(torch.zeros((2 * wiring.PAIRS, 3, 16, 16)), rig_pose=rec.new("rig_pose", (1, 12)))
        traces[key] = list(rec.trace)
        states[key] = sorted(pipe._stage.window.state(torch.device("cpu"), 1, 1 + sum(wiring.RIG_CFG)))
        labels = {k: rec.label(v) for k, v in outs[key]["window"].items()}
        if key == "on":
            assert labels["prior"] == "win_prior" and labels["tick_prior"] == "prior" and labels["tick_obs"] == "obs"
    off, on = traces["off"], traces["on"]
    # without the keyword: the parent's launches, keys and state, to the letter
    tail = wva.RIG_WINDOW_TAIL if refine else [wva.BEARINGS] + wva.RIG_WINDOW_TAIL
    assert off[-len(tail):] == tail and ([wva.BEARINGS, wva.RIG_REFINE] == [l for l in off if l.startswith(("rig_bearings", "refine_pose_views("))][:2] if refine else True)
    assert list(outs["off"]["window"]) == ["pose", "fit", "n_obs", "n_views", "information", "status", "pose_B", "tick_obs", "win_obs", "win_views", "win_i"]
    assert states["off"] == ["win_assignment", "win_i", "win_n", "win_obs", "win_views"] and not [l for l in off if "prior" in l or "weighted" in l or "confidence" in l]
    # with it: as many launches, in the same order, each the weighted one; ONE launch of the bearings, shared with the refinement where there is one
    assert len(on) == len(off)
    ops_of = lambda lines: [line.split("(")[0] for line in lines]
    renamed = {"rig_bearings": "rig_bearings_weighted", "refine_pose_views": "refine_pose_views_weighted", "refine_pose_views_wide": "refine_pose_views_weighted"}
    assert ops_of(on) == [renamed.get(op, op) for op in ops_of(off)]
    assert sum(l.startswith("rig_bearings") for l in on) == 1 and [l for l in on if l.startswith("rig_bearings")][0].endswith("confidence=ConfidenceWeights)")
    push = [l for l in on if l.startswith("window_push_views(")]
    assert len(push) == 1 and "obs=obs, " in push[0] and push[0].endswith("prior=prior, win_prior=win_prior)")
    assert "state=['win_obs', 'win_views', 'win_i', 'win_assignment', 'win_n', 'win_prior']" in push[0]
    refined = [l for l in on if l.startswith("refine_pose_views_weighted(")]
    assert refined[-1] == ("refine_pose_views_weighted(obs=win_obs, prior=win_prior, views=win_views, pose=window.start, assignment=win_assignment, n_obj=win_n, model=model, "
                           "cfg=WindowConfig, each=True, wide=True)")           # the wide instance whatever V is: the unweighted window's kernel
    if refine:
        assert len(refined) == 2 and refined[0] == ("refine_pose_views_weighted(obs=obs, prior=prior, views=rig_views, pose=pose.pose, assignment=pose.assignment, "
                                                    "n_obj=fused.n_obj, model=model, cfg=RefineConfig, each=False, wide=False)")
        assert outs["on"]["window"]["tick_obs"] is outs["on"]["refine"]["obs"] and outs["on"]["window"]["tick_prior"] is outs["on"]["refine"]["prior"]
    assert list(outs["on"]["window"]) == list(outs["off"]["window"]) + ["prior", "tick_prior"] and list(outs["on"]) == list(outs["off"])
    assert states["on"] == ["win_assignment", "win_i", "win_n", "win_obs", "win_prior", "win_views"]
    assert [l for l in on if l.startswith("window_views_state(")] == ["window_views_state(B=1, max_tracks=7, S=4, ticks=4, n_views=4, prior=True)"]


def test_the_rig_window_and_the_refinement_share_one_mapping():
    import test_window_views_args as wva
    from object_keypoints_amd import ops
    cw = ops.ConfidenceWeights(15.8, 1.0)
    with pytest.raises(ops.OkpError, match="refine has confidence = .* and rig_window confidence = .*the two must agree"):
        wva._rig_pipeline(refine=ops.RefineConfig(confidence=cw), rig_window=ops.WindowConfig(4, confidence=ops.ConfidenceWeights(8.0, 1.0)))
    both = wva._rig_pipeline(refine=ops.RefineConfig(confidence=cw), rig_window=ops.WindowConfig(4, confidence=ops.ConfidenceWeights(15.8, 1.0)))
    assert both._stage.bearings_confidence is cw
    one = wva._rig_pipeline(refine=ops.RefineConfig(), rig_window=ops.WindowConfig(4, confidence=cw))       # either may carry it alone
    assert one._stage.bearings_confidence is cw and one.refine.confidence is None


def test_tick_sharded_refuses_the_keyword_under_a_process_group(monkeypatch):
    """Under an initialised process group tick_sharded refuses refine and rig_window as it always did (OkpError, the parent's words); with the
    keyword on either it refuses with OkpNotOffered and names where the keyword is accepted."""
    import torch.distributed as dist
    import test_window_views_args as wva
    from object_keypoints_amd import ops
    cw = ops.ConfidenceWeights(15.8, 1.0)
    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    frames, rig_pose = torch.zeros((4, 3, 16, 16)), torch.zeros((1, 12), dtype=torch.float64)
    accepted = "tick_device and capture_device of a pipeline built with refine / rig_window take the keyword"
    for name, kw in (("refine", dict(refine=ops.RefineConfig(confidence=cw), rig_window=None)), ("rig_window", dict(rig_window=ops.WindowConfig(4, confidence=cw))),
                     ("refine", dict(refine=ops.RefineConfig(confidence=cw, huber_px=0.5), rig_window=ops.WindowConfig(4, confidence=cw)))):
        pipe = wva._rig_pipeline(**kw)
        with pytest.raises(ops.OkpNotOffered, match=f"tick_sharded with {name} and its confidence under a process group: not offered .*{accepted}") as refusal:
            pipe.tick_sharded(frames, 2, rig_pose=rig_pose)
        assert isinstance(refusal.value, ops.OkpError) and isinstance(refusal.value, TypeError)
    # without the keyword: the refusals and the words they had
    for kw, words in ((dict(refine=ops.RefineConfig(), rig_window=None), "tick_sharded with refine under a process group: the refinement reads every pair's peaks"),
                      (dict(refine=ops.RefineConfig(huber_px=0.5)), "tick_sharded with refine under a process group"),
                      (dict(), "tick_sharded with rig_window under a process group: the window reads every pair's peaks")):
        with pytest.raises(ops.OkpError, match=words) as refusal:
            wva._rig_pipeline(**kw).tick_sharded(frames, 2, rig_pose=rig_pose)
        assert not isinstance(refusal.value, ops.OkpNotOffered)
    # without a process group the sharded tick is the device tick: the keyword is accepted
    monkeypatch.setattr(dist, "is_initialized", lambda: False)
    rec = _rig_window_recorder(monkeypatch)
    pipe = wva._rig_pipeline(rec, rig_window=ops.WindowConfig(4, confidence=cw))
    out = pipe.tick_sharded(torch.zeros((2 * wiring.PAIRS, 3, 16, 16)), wiring.PAIRS, rig_pose=rec.new("rig_pose", (1, 12)))
    assert "prior" in out["window"] and out["window"] is out["local"]["window"]


def test_no_instance_of_the_weighted_kernels_uses_scratch_memory():
    """The done-criterion of the register budget, held by the build's own report (-Rpass-analysis=kernel-resource-usage, gfx950): the wide
    PRIOR instances sit at the 256 registers a lane has at 512 threads, so a toolchain that allocates differently would spill - loudly, here.
    The instances without the flag keep what they had: no scratch either."""
    from object_keypoints_amd import build
    build.build()
    res = build.kernel_resources()
    families = {"okp_refine_pose_views_kernel": 4, "okp_refine_pose_views_robust_kernel": 4, "okp_refine_pose_views_wide_kernel": 4, "okp_rig_bearings_kernel": 2,
                "okp_window_push_kernel": 2, "okp_window_push_views_kernel": 2}
    seen = {name: 0 for name in families}
    for symbol, r in res.items():
        for name in families:
            if re.search(rf"\d+{name}I", symbol):
                seen[name] += 1
                assert r["scratch"] == 0, (symbol, r)
                prior = re.search(r"I(?:Lb[01]E)*Lb1EEEv", symbol) is not None            # the last template argument: PRIOR
                if name == "okp_refine_pose_views_wide_kernel":
                    assert r["vgprs"] <= 256 and r["agprs"] == 0 and r["vgpr_spill"] == 0, (symbol, r)
                print(f"{symbol}: PRIOR {prior}, {r['vgprs']} VGPRs, {r['agprs']} AGPRs, scratch {r['scratch']}")
    assert seen == families, seen                                     # every instance, with and without the flag, was found in the report
