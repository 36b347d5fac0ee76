"""The dispatcher shim's own refusals for the six refinements against views and the two bearing collectors (csrc/okp_torch.cpp: refine_views_any,
rig_bearings_any), in the manner of test_the_shim_names_the_state_it_refuses of tests/test_gpu_window.py: torch.ops.okp called directly at
B = 1, max_obj = 2, S = 3 and V = 2 (V = 65 for refine_pose_views_wide and refine_pose_views_weighted_wide).  The sentences are written out
as the source held them, op by op, before the ops came to share one body: (a) every tensor of every op with one element too many, (b) a fit
of the other width, (c) n_inlier / weight given as None - accepted, and run, by the ops that take huber_px = 0 as the plain cost, a schema
error under refine_pose_views_robust.  No kernel is launched but in (c), on zeroed buffers with no live object."""
import re

import pytest
import torch

pytestmark = pytest.mark.gpu

B, MAX_OBJ, S = 1, 2, 3
PAIRS, K, CAP, CAP_F = 2, 3, 4, 3

OBS = "okp: obs is [B,max_obj,S,V,2] float64"
PRIOR = "okp: prior is [B,max_obj,S,V] float64, one value per entry of obs"
PLAIN_IN = "okp: refine_pose_views inputs are views [V,14], pose [B,max_obj,12], assignment [B,max_obj,S], n_obj [B] and model [S,3]"
PLAIN_OUT = "okp: refine_pose_views outputs are pose_out [B,max_obj,12], fit [B,max_obj,2], n_obs [B,max_obj], information [B,max_obj,36] and status [B,max_obj]"
SENTENCES = {             # op -> (views, the other inputs, the outputs, n_inlier and weight)
    "refine_pose_views": (PLAIN_IN, PLAIN_IN, PLAIN_OUT, None),
    "refine_pose_views_each": ("okp: refine_pose_views_each takes views [B,max_obj,V,14]: one table per object", PLAIN_IN, PLAIN_OUT, None),
    "refine_pose_views_robust": (
        "okp: refine_pose_views_robust takes views [V,14] (views_each = 0) or [B,max_obj,V,14] (views_each = 1)",
        "okp: refine_pose_views_robust inputs are pose [B,max_obj,12], assignment [B,max_obj,S], n_obj [B] and model [S,3]",
        "okp: refine_pose_views_robust outputs are pose_out [B,max_obj,12], fit [B,max_obj,4], n_obs and n_inlier [B,max_obj], weight [B,max_obj,S,V], "
        "information [B,max_obj,36] and status [B,max_obj]", None),
    "refine_pose_views_wide": (
        "okp: refine_pose_views_wide takes views [V,14] (views_each = 0) or [B,max_obj,V,14] (views_each = 1)",
        "okp: refine_pose_views_wide inputs are pose [B,max_obj,12], assignment [B,max_obj,S], n_obj [B] and model [S,3]",
        "okp: refine_pose_views_wide outputs are pose_out [B,max_obj,12], fit [B,max_obj,2] ([B,max_obj,4] with huber_px > 0), n_obs [B,max_obj], "
        "information [B,max_obj,36] and status [B,max_obj]",
        "okp: refine_pose_views_wide writes n_inlier [B,max_obj] and weight [B,max_obj,S,V] when huber_px > 0"),
}
SENTENCES["refine_pose_views_weighted"] = SENTENCES["refine_pose_views_weighted_wide"] = (                  # both speak as refine_pose_views_weighted
    "okp: refine_pose_views_weighted takes views [V,14] (views_each = 0) or [B,max_obj,V,14] (views_each = 1)",
    "okp: refine_pose_views_weighted inputs are pose [B,max_obj,12], assignment [B,max_obj,S], n_obj [B] and model [S,3]",
    "okp: refine_pose_views_weighted outputs are pose_out [B,max_obj,12], fit [B,max_obj,2] ([B,max_obj,4] with huber_px > 0), n_obs [B,max_obj], "
    "information [B,max_obj,36] and status [B,max_obj]",
    "okp: refine_pose_views_weighted writes n_inlier [B,max_obj] and weight [B,max_obj,S,V] when huber_px > 0")
ONE_WAVE = ("refine_pose_views", "refine_pose_views_each")
ZERO_IS_PLAIN = ("refine_pose_views_wide", "refine_pose_views_weighted", "refine_pose_views_weighted_wide")
INPUTS = ("pose", "assignment", "n_obj", "model")
OUTPUTS = ("pose_out", "fit", "n_obs", "information", "status")

TICK = "okp: a tick's peaks are count [2P,K] int32 and xyc [2P,K,cap,3] float32"
COLLECTORS = {            # op -> the sentence of its buffers
    "rig_bearings": "okp: rig_bearings buffers are match and member [P,K,cap], n_fused [K] int32 and obs [cap_f,S,2P,2] float64",
    "rig_bearings_weighted": "okp: rig_bearings_weighted buffers are match and member [P,K,cap], n_fused [K] int32, obs [cap_f,S,2P,2] and prior [cap_f,S,2P] float64"}


def _zeros(shape, dtype=torch.float64):
    return torch.zeros(shape, dtype=dtype, device="cuda")


def _longer(t):
    """The tensor with one element too many (and so of no shape the op knows)."""
    return _zeros((t.numel() + 1,), t.dtype)


def _refine_tensors(op, huber_px):
    v = 65 if op in ("refine_pose_views_wide", "refine_pose_views_weighted_wide") else 2
    i32 = torch.int32
    t = {"obs": _zeros((B, MAX_OBJ, S, v, 2)), "prior": _zeros((B, MAX_OBJ, S, v)), "views": _zeros((B, MAX_OBJ, v, 14) if op == "refine_pose_views_each" else (v, 14)),
         "pose": _zeros((B, MAX_OBJ, 12)), "assignment": _zeros((B, MAX_OBJ, S), i32), "n_obj": _zeros((B,), i32), "model": _zeros((S, 3)),
         "pose_out": _zeros((B, MAX_OBJ, 12)), "fit": _zeros((B, MAX_OBJ, 4 if huber_px > 0.0 else 2)), "n_obs": _zeros((B, MAX_OBJ), i32),
         "n_inlier": _zeros((B, MAX_OBJ), i32), "weight": _zeros((B, MAX_OBJ, S, v)), "information": _zeros((B, MAX_OBJ, 36)), "status": _zeros((B, MAX_OBJ), i32)}
    return t


def _refine(op, t, huber_px):
    from object_keypoints_amd import _lib
    stream = torch.cuda.current_stream().cuda_stream
    if op in ONE_WAVE:
        args = (t["obs"], t["views"], t["pose"], t["assignment"], t["n_obj"], t["model"], 0.25, 6, 1e-9, t["pose_out"], t["fit"], t["n_obs"], t["information"], t["status"])
    else:
        args = (t["obs"],) + ((t["prior"],) if "weighted" in op else ()) + (t["views"], 0, t["pose"], t["assignment"], t["n_obj"], t["model"], 0.25, huber_px, 6, 1e-9,
                                                                            t["pose_out"], t["fit"], t["n_obs"], t["n_inlier"], t["weight"], t["information"], t["status"])
    getattr(_lib.torch_ops(), op)(*args, stream)


def _refused(op, t, huber_px, sentence):
    with pytest.raises(RuntimeError, match=re.escape(sentence)):
        _refine(op, t, huber_px)


@pytest.mark.parametrize("op", list(SENTENCES))
def test_the_shim_names_the_tensors_it_refuses(op):
    views, inputs, outputs, robust = SENTENCES[op]
    huber_px = 0.0 if op in ONE_WAVE else 0.5
    wanted = [("obs", OBS), ("views", views)] + [(n, inputs) for n in INPUTS] + [(n, outputs) for n in OUTPUTS]
    if "weighted" in op:
        wanted.append(("prior", PRIOR))
    if op not in ONE_WAVE:
        wanted += [(n, robust or outputs) for n in ("n_inlier", "weight")]
    for name, sentence in wanted:                                           # (a) one tensor with one element too many
        t = _refine_tensors(op, huber_px)
        t[name] = _longer(t[name])
        _refused(op, t, huber_px, sentence)
    if op not in ONE_WAVE:                                                  # (b) a fit of the other width
        t = _refine_tensors(op, huber_px)
        t["fit"] = _zeros((B, MAX_OBJ, 2))
        _refused(op, t, huber_px, outputs)
    if op in ZERO_IS_PLAIN:
        t = _refine_tensors(op, 0.0)
        t["fit"] = _zeros((B, MAX_OBJ, 4))
        _refused(op, t, 0.0, outputs)
        t = dict(_refine_tensors(op, 0.0), n_inlier=None, weight=None)      # (c) the plain cost writes neither: None is accepted, and the op runs
        t["status"].fill_(-1)
        _refine(op, t, 0.0)
        torch.cuda.synchronize()
        assert (t["status"] == 1).all() and (t["n_obs"] == 0).all() and torch.isnan(t["fit"]).all()      # n_obj = 0: every object REFINE_SKIPPED, every word written
    if op == "refine_pose_views_robust":
        for name in ("n_inlier", "weight"):
            with pytest.raises(RuntimeError, match=name):                   # the schema's own refusal: a Tensor, not an optional one
                _refine(op, dict(_refine_tensors(op, huber_px), **{name: None}), huber_px)
    torch.cuda.synchronize()


@pytest.mark.parametrize("op", list(COLLECTORS))
def test_the_shim_names_the_collectors_buffers(op):
    from object_keypoints_amd import _lib, ops
    i32 = torch.int32
    table = "okp: a rig's calibration table is uint8 [n_table, %d] (ops.stereo_rig)" % ops.STEREO_PAIR_BYTES
    wanted = [("table", table), ("count", TICK), ("xyc", TICK), ("object", "okp: object is [K,cap_f] int32 (rig_fuse)")]
    wanted += [(n, COLLECTORS[op]) for n in ("match", "member", "n_fused", "obs") + (("prior",) if op == "rig_bearings_weighted" else ())]
    for name, sentence in wanted:
        t = {"table": _zeros((1, ops.STEREO_PAIR_BYTES), torch.uint8), "count": _zeros((2 * PAIRS, K), i32), "xyc": _zeros((2 * PAIRS, K, CAP, 3), torch.float32),
             "match": _zeros((PAIRS, K, CAP), i32), "member": _zeros((PAIRS, K, CAP), i32), "object": _zeros((K, CAP_F), i32), "n_fused": _zeros((K,), i32),
             "obs": _zeros((CAP_F, S + 1, 2 * PAIRS, 2)), "prior": _zeros((CAP_F, S + 1, 2 * PAIRS))}
        t[name] = _longer(t[name])
        args = (t["table"], t["count"], t["xyc"], t["match"], t["member"], t["object"], t["n_fused"], [2, 1])
        args += (0.8, 0.4, t["obs"], t["prior"]) if op == "rig_bearings_weighted" else (t["obs"],)
        with pytest.raises(RuntimeError, match=re.escape(sentence)):
            getattr(_lib.torch_ops(), op)(*args, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
