"""What both device pipelines launch after the network, and which tensor feeds which launch, against recording stubs: every ops function
they call is replaced by one that returns CPU tensors of the right shapes and writes one line to a trace - its name, a label for each tensor
argument (the name of the launch that made it, found by its storage, so a view counts as its base) and its scalar arguments.  The expected
traces are literals: with nothing enabled they are the plain tick's; the pose, refine, world and track segments follow in that order, and
the world-frame change and the tracker take the refined pose where there is one.  No GPU needed."""
import os

import numpy as np
import pytest
import torch

from object_keypoints_amd import ops, synth
from object_keypoints_amd.perception import pipeline as pp
from object_keypoints_amd.perception.utils import camera_utils as cu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, CFG, CAP, MAX_OBJ, MAX_SEL, TRACKS, HW = 2, [1, 2, 1], 5, 3, 2, 7, 8
RIG_CFG, RIG_CAP, CAP_F, PAIRS = [1, 2], 6, 5, 2
MODEL = [[0.1, 0.0, 0.0], [0.0, 0.1, 0.0], [0.0, 0.0, 0.1], [0.1, 0.1, 0.1]]
BATCHED = [dict(pose=p, refine=r, track=t, world=w) for p in (0, 1) for r in (0, 1) for t in (0, 1) for w in (0, 1) if p or not (r or t)]
RIG = [dict(pose=p, track=t, world=w) for p in (0, 1) for t in (0, 1) for w in (0, 1) if p or not t]
ident = lambda c: "-".join(k for k, v in c.items() if v) or "plain"


class Recorder:
    """The stubs: self.trace collects one line per call, self.names maps a tensor's storage to its label."""

    def __init__(self, monkeypatch):
        self.trace, self.names = [], {}
        for name in ("peak_nms", "lift_peaks", "group_objects", "capacity_overflow", "stereo_match_rig", "stereo_triangulate_rig", "rig_fuse", "object_points",
                     "rig_object_points", "object_pose", "refine_pose", "change_frame", "track_state", "track_objects"):
            monkeypatch.setattr(ops, name, getattr(self, name))

    def new(self, label, shape, dtype=torch.float64):
        t = torch.zeros(shape, dtype=dtype)
        return self.name(label, t)

    def name(self, label, t):
        self.names[t.untyped_storage().data_ptr()] = label
        return t

    def label(self, v):
        if isinstance(v, torch.Tensor):
            return self.names.get(v.untyped_storage().data_ptr(), "?")
        if isinstance(v, (ops.TrackConfig, ops.RefineConfig)):
            return type(v).__name__
        return "cam" if type(v).__name__ == "okp_camera" else repr(v)

    def call(self, op, **args):
        self.trace.append(f"{op}({', '.join(f'{k}={self.label(v)}' for k, v in args.items())})")

    # -- the plain ticks
    def peak_nms(self, heat, cap=64):
        self.call("peak_nms", heat=heat, cap=cap)
        n, k = heat.shape[:2]
        return self.new("count", (n, k), torch.int32), self.new("yx", (n, k, cap, 2), torch.int32), self.new("xyc", (n, k, cap, 3), torch.float32)

    def lift_peaks(self, cam, count, xyc, depth, max_x, max_y):
        self.call("lift_peaks", cam=cam, count=count, xyc=xyc, depth=depth, max_x=max_x, max_y=max_y)
        return self.new("points", tuple(xyc.shape[:3]) + (4,))

    def group_objects(self, count, xyc, centers, type_count, max_obj=16, max_sel=4, max_dist=20.0):
        self.call("group_objects", count=count, xyc=xyc, centers=centers, type_count=type_count, max_obj=max_obj, max_sel=max_sel)
        n, k, cap = xyc.shape[:3]
        return {"n_obj": self.new("n_obj", (n,), torch.int32), "sel": self.new("sel", (n, max_obj, k - 1, max_sel), torch.int32),
                "n_votes": self.new("n_votes", (n, max_obj, k - 1), torch.int32), "assign": self.new("assign", (n, k, cap), torch.int32),
                "pred": self.new("pred", (n, k, cap, 2)), "reduced": self.new("reduced", (n, max_obj, k - 1, max_sel, 2), torch.float32)}

    def capacity_overflow(self, count, cap, max_obj, range_flag=None):
        self.call("capacity_overflow", count=count, cap=cap, max_obj=max_obj, range_flag=range_flag)
        return self.new("overflow", (1,), torch.int32)[0]

    def stereo_match_rig(self, table, count, xyc, max_distance, first_pair=0, range_flag=None):
        self.call("stereo_match_rig", table=table, count=count, xyc=xyc, max_distance=max_distance, first_pair=first_pair, range_flag=range_flag)
        n, k, cap = xyc.shape[:3]
        return self.new("match", (n // 2, k, cap), torch.int32), self.new("overflow", (1,), torch.int32)[0]

    def stereo_triangulate_rig(self, table, count, xyc, match, first_pair=0, correct_matches=True):
        self.call("stereo_triangulate_rig", table=table, count=count, xyc=xyc, match=match, first_pair=first_pair)
        return self.new("points", tuple(match.shape) + (4,))

    def rig_fuse(self, points, poses, type_count, merge_radius, object_radius, cap_f, overflow=None):
        self.call("rig_fuse", points=points, poses=poses, type_count=type_count, merge_radius=merge_radius, object_radius=object_radius, cap_f=cap_f, overflow=overflow)
        p, k, cap = points.shape[:3]
        return {"fused": self.new("fused", (k, cap_f, 4)), "n_fused": self.new("n_fused", (k,), torch.int32), "views": self.new("views", (k, cap_f), torch.int32),
                "object": self.new("object", (k, cap_f), torch.int32), "member": self.new("member", (p, k, cap), torch.int32),
                "n_obj": self.new("fused.n_obj", (1,), torch.int32)[0], "overflow": self.new("fused.overflow", (1,), torch.int32)[0]}

    # -- the object stage
    def object_points(self, cam, out, type_count, max_x, max_y):
        self.call("object_points", cam=cam, type_count=type_count, max_x=max_x, max_y=max_y, **{k: out[k] for k in ("points", "sel", "n_obj", "n_votes", "reduced", "depth")})
        n, max_obj = out["sel"].shape[:2]
        return self.new("tab", (n, max_obj, 1 + sum(type_count), 4))

    def rig_object_points(self, fused, type_count):
        self.call("rig_object_points", type_count=type_count, **{k: fused[k] for k in ("fused", "n_fused", "object")})
        return self.new("tab", (1, fused["fused"].shape[1], 1 + sum(type_count), 4))

    def object_pose(self, tab, n_obj, model, type_count, max_rmse=None):
        self.call("object_pose", tab=tab, n_obj=n_obj, model=model, type_count=type_count, max_rmse=max_rmse)
        b, max_obj, s = tab.shape[:3]
        return {"pose": self.new("pose.pose", (b, max_obj, 12)), "fit": self.new("pose.fit", (b, max_obj, 2)), "assignment": self.new("pose.assignment", (b, max_obj, s), torch.int32),
                "used": self.new("pose.used", (b, max_obj), torch.int32), "status": self.new("pose.status", (b, max_obj), torch.int32)}

    def refine_pose(self, tab, pose, n_obj, model, cam, cfg):
        self.call("refine_pose", tab=tab, pose=pose["pose"], assignment=pose["assignment"], n_obj=n_obj, model=model, cam=cam, cfg=cfg)
        b, max_obj = tab.shape[:2]
        return {"pose": self.new("refine.pose", (b, max_obj, 12)), "fit": self.new("refine.fit", (b, max_obj, 4)), "information": self.new("refine.information", (b, max_obj, 36)),
                "status": self.new("refine.status", (b, max_obj), torch.int32)}

    def change_frame(self, T, points=None, poses=None, inverse=False, overflow=None, out_points=None, out_poses=None):
        self.call("change_frame", T=T, points=points, poses=poses, inverse=inverse, overflow=overflow)
        assert out_points is None and out_poses is None
        tag = "local" if inverse else "world"
        return {"points": self.new(f"{tag}({self.label(points)})", tuple(points.shape)) if points is not None else None,
                "poses": self.new(f"{tag}({self.label(poses)})", tuple(poses.shape)) if poses is not None else None,
                "overflow": self.new(f"{tag}.overflow", (1,), torch.int32)[0]}

    def track_state(self, B, max_tracks, device):
        self.call("track_state", B=B, max_tracks=max_tracks)
        return {"track_f": self.new("track_f", (B, max_tracks, 16)), "track_i": self.new("track_i", (B, max_tracks, 4), torch.int32), "next_id": self.new("next_id", (B,), torch.int32)}

    def track_objects(self, state, tab, pose, status, n_obj, model, cfg, overflow=None):
        self.call("track_objects", state=list(state), track_f=state["track_f"], tab=tab, pose=pose, status=status, n_obj=n_obj, model=model, cfg=cfg, overflow=overflow)
        b, max_obj = tab.shape[:2]
        return {"track_pose": self.new("track_pose", (b, cfg.max_tracks, 12)), "track_of": self.new("track_of", (b, max_obj), torch.int32),
                "meas_of": self.new("meas_of", (b, cfg.max_tracks), torch.int32), "n_tracks": self.new("n_tracks", (b,), torch.int32),
                "overflow": self.new("track.overflow", (1,), torch.int32)[0]}


# ---- the expected traces, written out ----------------------------------------------------------------------------------------------------

BATCHED_PLAIN = [
    "peak_nms(heat=heat, cap=5)",
    "lift_peaks(cam=cam, count=count, xyc=xyc, depth=depth, max_x=63, max_y=63)",
    "group_objects(count=count, xyc=xyc, centers=centers, type_count=[1, 2, 1], max_obj=3, max_sel=2)",
    "capacity_overflow(count=count, cap=5, max_obj=3, range_flag=range_flag)",
]
BATCHED_POSE = [
    "object_points(cam=cam, type_count=[1, 2, 1], max_x=63, max_y=63, points=points, sel=sel, n_obj=n_obj, n_votes=n_votes, reduced=reduced, depth=depth)",
    "object_pose(tab=tab, n_obj=n_obj, model=model, type_count=[1, 2, 1], max_rmse=0.25)",
]
BATCHED_REFINE = ["refine_pose(tab=tab, pose=pose.pose, assignment=pose.assignment, n_obj=n_obj, model=model, cam=cam, cfg=RefineConfig)"]
RIG_PLAIN = [
    "peak_nms(heat=heat, cap=6)",
    "stereo_match_rig(table=table, count=count, xyc=xyc, max_distance=3.0, first_pair=0, range_flag=range_flag)",
    "stereo_triangulate_rig(table=table, count=count, xyc=xyc, match=match, first_pair=0)",
]
RIG_FUSE = ["rig_fuse(points=points, poses=rig_poses, type_count=[1, 2], merge_radius=0.08, object_radius=0.18, cap_f=5, overflow=overflow)"]
RIG_POSE = [
    "rig_object_points(type_count=[1, 2], fused=fused, n_fused=n_fused, object=object)",
    "object_pose(tab=tab, n_obj=fused.n_obj, model=model, type_count=[1, 2], max_rmse=inf)",
]


def stage_tail(c, frame_pose, points, n_obj, overflow, streams):
    """The launches behind the pose (and the refinement): the world-frame change of the points, then of the table and the pose that is fed on
    - the refined one where there is a refinement -, then the tracker on what that gave, and its poses back through the inverse change."""
    fed = "refine.pose" if c.get("refine") else "pose.pose"
    tail = []
    if c["world"]:
        tail.append(f"change_frame(T={frame_pose}, points={points}, poses=None, inverse=False, overflow={overflow})")
        if c["pose"]:
            tail.append(f"change_frame(T={frame_pose}, points=tab, poses={fed}, inverse=False, overflow={overflow})")
    if c["track"]:
        tail.append(f"track_state(B={streams}, max_tracks=7)")
        state = "state=['track_f', 'track_i', 'next_id'], track_f=track_f"
        if c["world"]:
            tail.append(f"track_objects({state}, tab=world(tab), pose=world({fed}), status=pose.status, n_obj={n_obj}, model=model, cfg=TrackConfig, overflow=world.overflow)")
            tail.append(f"change_frame(T={frame_pose}, points=None, poses=track_pose, inverse=True, overflow=None)")
        else:
            tail.append(f"track_objects({state}, tab=tab, pose={fed}, status=pose.status, n_obj={n_obj}, model=model, cfg=TrackConfig, overflow={overflow})")
    return tail


def stage_keys(c):
    return [k for k in ("pose", "refine", "world", "track") if c.get(k)]


def check_stage_values(rec, c, out, frame_pose, points_label):
    """Which tensor sits under which key of the entries the stage adds."""
    lab = lambda t: rec.label(t)
    fed = "refine.pose" if c.get("refine") else "pose.pose"
    if c["pose"]:
        assert list(out["pose"]) == ["pose", "fit", "assignment", "used", "status", "tab"]
        assert [lab(out["pose"][k]) for k in out["pose"]] == ["pose.pose", "pose.fit", "pose.assignment", "pose.used", "pose.status", "tab"]
    if c.get("refine"):
        assert [(k, lab(v)) for k, v in out["refine"].items()] == [("pose", "refine.pose"), ("fit", "refine.fit"), ("information", "refine.information"), ("status", "refine.status")]
    if c["world"]:
        w = out["world"]
        assert list(w) == ["T", "points", "overflow"] + (["tab", "pose"] if c["pose"] else [])
        assert w["T"] is frame_pose and lab(w["points"]) == f"world({points_label})" and lab(w["overflow"]) == "world.overflow"
        assert tuple(w["points"].shape) == tuple(out["fused"]["fused"].shape if "fused" in out else out["points"].shape)
        if c["pose"]:
            assert lab(w["tab"]) == "world(tab)" and lab(w["pose"]) == f"world({fed})"
    if c["track"]:
        t = out["track"]
        assert list(t) == ["track_pose", "track_of", "meas_of", "n_tracks", "overflow", "track_f", "track_i", "next_id"] + (["track_pose_C"] if c["world"] else [])
        assert lab(t["overflow"]) == "track.overflow" and lab(t["track_f"]) == "track_f" and lab(t["next_id"]) == "next_id"
        if c["world"]:
            assert lab(t["track_pose_C"]) == "local(track_pose)"


# ---- the batched pipeline -----------------------------------------------------------------------------------------------------------------

def batched(rec, c):
    cam = cu.FisheyeCamera(np.array([[300.0, 0, 32], [0, 300.0, 32], [0, 0, 1]]), np.zeros(4), np.array([64, 64]))
    pipe = pp.BatchedKeypointPipeline(None, {"keypoint_config": CFG}, cam, capacity=CAP, max_objects=MAX_OBJ, max_per_type=MAX_SEL,
                                      points_3d=MODEL if c["pose"] else None, max_rmse=0.25 if c["pose"] else None, world_frame=bool(c["world"]),
                                      track=ops.TrackConfig(0.5, 0.1, max_tracks=TRACKS) if c["track"] else None, refine=ops.RefineConfig() if c["refine"] else None)
    if c["pose"]:
        rec.name("model", pipe._model_host)
    maps = [rec.new("heat", (N, 1 + len(CFG), HW, HW), torch.float32), rec.new("depth", (N, 1 + len(CFG), HW, HW), torch.float32),
            rec.new("centers", (N, len(CFG), 2, HW, HW), torch.float32)]
    return pipe, maps, rec.new("range_flag", (1,), torch.int32), rec.new("camera_pose", (N, 12)) if c["world"] else None


@pytest.mark.parametrize("c", BATCHED, ids=ident)
def test_the_batched_step_launches_the_stage_in_order_on_the_right_tensors(monkeypatch, c):
    rec = Recorder(monkeypatch)
    pipe, maps, flag, camera_pose = batched(rec, c)
    out = pipe.postprocess_device(*maps, range_flag=flag, camera_pose=camera_pose)
    want = BATCHED_PLAIN + (BATCHED_POSE if c["pose"] else []) + (BATCHED_REFINE if c["refine"] else []) + stage_tail(c, "camera_pose", "points", "n_obj", "overflow", N)
    assert rec.trace == want, "\n" + "\n".join(rec.trace)
    assert list(out) == ["heat", "depth", "centers", "count", "yx", "xyc", "points", "n_obj", "sel", "n_votes", "assign", "pred", "reduced", "overflow"] + stage_keys(c)
    assert out["heat"] is maps[0] and rec.label(out["overflow"]) == "overflow" and rec.label(out["points"]) == "points"
    check_stage_values(rec, c, out, camera_pose, "points")
    if c["track"]:                                                                     # the second step finds the tracker's state where the first left it
        again = pipe.postprocess_device(*maps, range_flag=flag, camera_pose=camera_pose)
        assert rec.trace[len(want):] == [line for line in want if not line.startswith("track_state(")]
        assert all(again["track"][k] is out["track"][k] for k in ("track_f", "track_i", "next_id"))


# ---- the stereo pipeline ------------------------------------------------------------------------------------------------------------------

class StubNet:
    def __init__(self, rec):
        self.rec = rec
        self.flag = rec.new("range_flag", (1,), torch.int32)

    def deployed(self, frames, check_range=True):
        assert check_range is False
        k = 1 + len(RIG_CFG)
        return self.rec.new("heat", (frames.shape[0], k, HW, HW), torch.float32), self.rec.new("depth", (frames.shape[0], k, HW, HW), torch.float32), None

    def range_flag(self, device):
        return self.flag


def rig(rec, c, fused=True):
    calib = cu.load_calibration_params(os.path.join(REPO, "config", "calibration.yaml"))
    fusion = dict(rig_poses=synth.rig_poses(PAIRS), merge_radius=0.08, object_radius=0.18, fuse_capacity=CAP_F) if fused else {}
    pipe = pp.StereoStreamPipeline(StubNet(rec), synth.stereo_rig(calib, n_pairs=PAIRS), {"keypoint_config": RIG_CFG}, capacity=RIG_CAP,
                                   points_3d=MODEL[:3] if c["pose"] else None, track=ops.TrackConfig(0.5, 0.1, max_tracks=TRACKS) if c["track"] else None,
                                   world_frame=bool(c["world"]), **fusion)
    rec.name("table", pipe._table_host)
    if fused:
        rec.name("rig_poses", pipe._poses_host)
    if c["pose"]:
        rec.name("model", pipe._model_host)
    return pipe, torch.zeros((2 * PAIRS, 3, 16, 16)), rec.new("rig_pose", (1, 12)) if c["world"] else None


RIG_KEYS = ["heat", "depth", "count", "xyc", "match", "points", "overflow"]


@pytest.mark.parametrize("c", RIG, ids=ident)
def test_the_fused_tick_launches_the_stage_in_order_on_the_right_tensors(monkeypatch, c):
    rec = Recorder(monkeypatch)
    pipe, frames, rig_pose = rig(rec, c)
    out = pipe.tick_device(frames, rig_pose=rig_pose)
    want = RIG_PLAIN + RIG_FUSE + (RIG_POSE if c["pose"] else []) + stage_tail(c, "rig_pose", "fused", "fused.n_obj", "fused.overflow", 1)
    assert rec.trace == want, "\n" + "\n".join(rec.trace)
    assert list(out) == RIG_KEYS + ["fused"] + stage_keys(c)
    assert rec.label(out["overflow"]) == "fused.overflow" and out["overflow"] is out["fused"]["overflow"]
    check_stage_values(rec, c, out, rig_pose, "fused")
    # without a process group the sharded tick is this tick, its stage entries handed up next to the payload
    del rec.trace[:]
    whole = pipe.tick_sharded(frames, PAIRS, rig_pose=rig_pose)
    assert rec.trace == [line for line in want if not line.startswith("track_state(")]
    assert list(whole) == ["points", "overflow", "local", "fused"] + stage_keys(c) and list(whole["local"]) == list(out)
    assert all(whole[k] is whole["local"][k] for k in ["points", "overflow", "fused"] + stage_keys(c))
    # the local tick of a shard runs none of the stage and fuses nothing: that follows the gather
    del rec.trace[:]
    local = pipe.tick_device(frames, _fuse=False)
    assert rec.trace == RIG_PLAIN and list(local) == RIG_KEYS and rec.label(local["overflow"]) == "overflow"


def test_with_nothing_enabled_both_ticks_are_the_plain_ones(monkeypatch):
    rec = Recorder(monkeypatch)
    pipe, frames, _ = rig(rec, dict(pose=0, track=0, world=0), fused=False)
    out = pipe.tick_device(frames)
    assert rec.trace == RIG_PLAIN and list(out) == RIG_KEYS
    del rec.trace[:]
    pipe, maps, flag, _ = batched(rec, dict(pose=0, refine=0, track=0, world=0))
    out = pipe.postprocess_device(*maps, range_flag=flag)
    assert rec.trace == BATCHED_PLAIN and list(out)[-1] == "overflow"
