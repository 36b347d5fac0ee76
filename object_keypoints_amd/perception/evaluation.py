"""Accuracy bookkeeping for evaluation runs: what the reference's harness tabulates (scripts/eval_model.py:129-232).

Per frame, every detected object is matched to the ground-truth object whose centre is nearest in the camera's x/y plane
(depth is the least certain coordinate), every lifted keypoint to the nearest ground-truth keypoint of that object, and
the Euclidean errors are collected; keypoints that were not lifted count as missing.  `summary()` returns the columns of
the reference's table (centimetres; "< 3cm" and "missing" as the reference prints them).  `Results` is host NumPy: a handful
of points per frame, fed through objects(out, n).  `DeviceResults` keeps the same table - and pose errors and detection recall
next to it - on the device, behind the step, without a copy or a host loop per frame (okp_score_objects).
"""
import numpy as np

from .utils import linalg

_MAX_RANGE = 2.0          # predictions with a coordinate beyond 2 m are treated as not lifted (eval_model.py:170)
_SMALL = 0.03             # the "< 3cm" column


class Results:
    COLUMNS = ("mean", "mean xy", "std", "< 3cm", "25th percentile", "75th percentile", "missing", "points")

    def __init__(self):
        self._err = []            # metres, one entry per matched keypoint
        self._err_xy = []
        self._missing = 0
        self._points = 0
        self.camera = None

    def set_calibration(self, camera):
        self.camera = camera

    # -- helpers -------------------------------------------------------------------------------------------------
    def _visible(self, points_C):
        px = self.camera.project(np.atleast_2d(points_C))
        return self.camera.in_frame(px)

    def _match_object(self, detection, truth_C):
        centre_xy = np.asarray(detection["p_C"][0][0])[:2]
        return truth_C[np.linalg.norm(truth_C[:, 0, :2] - centre_xy, axis=1).argmin()]

    # -- API of the reference's class ---------------------------------------------------------------------------------
    def add(self, T_WC, objects, scene_points):
        """T_WC: camera-to-world transform (4x4); objects: the keypoint pipeline's output for one frame (dicts with 'p_C':
        per keypoint type an (n,3) array, a list with None entries, or None); scene_points: (n_objects, n_keypoints, 3)
        ground truth in the world frame, index 0 = object centre."""
        truth_C = linalg.transform_points(linalg.inv_transform(np.asarray(T_WC)), np.asarray(scene_points, dtype=np.float64))
        for det in objects:
            target = self._match_object(det, truth_C)
            if not self._visible(target[0])[0]:
                continue                                           # the object's centre is outside the frame: skipped
            for group in det["p_C"]:
                if group is None:
                    continue
                for p in group:
                    if p is None or not (np.asarray(p) < _MAX_RANGE).all():
                        self._points += 1
                        self._missing += 1
                        continue
                    p = np.asarray(p, dtype=np.float64)
                    nearest = target[np.linalg.norm(target - p, axis=1).argmin()]
                    if not self._visible(nearest)[0]:
                        continue                                   # its ground truth is out of view: not scored
                    self._points += 1
                    self._err.append(float(np.linalg.norm(nearest - p)))
                    self._err_xy.append(float(np.linalg.norm(nearest[:2] - p[:2])))

    def summary(self):
        n = self._points
        if n == 0 or not self._err:
            return {"points": n, "missing": 100.0 if n else 0.0}
        cm, cm_xy = np.array(self._err) * 100.0, np.array(self._err_xy) * 100.0
        q25, q75 = np.percentile(cm, [25, 75])
        return {"mean": float(cm.mean()), "mean xy": float(cm_xy.mean()), "std": float(cm.std()),
                "< 3cm": float((np.array(self._err) < _SMALL).sum()) / n, "25th percentile": float(q25),
                "75th percentile": float(q75), "missing": 100.0 * self._missing / n, "points": n}

    def print_results(self):
        s = self.summary()
        print(" | ".join(self.COLUMNS))
        print(" | ".join(f"{s[c]:.4g}" if isinstance(s.get(c), float) else str(s.get(c, "-")) for c in self.COLUMNS))


def keypoint_summary(err, err_xy, points, missing):
    """Results.summary() from the collected errors (metres) and the two counts: the same keys from the same NumPy calls."""
    n = int(points)
    if n == 0 or len(err) == 0:
        return {"points": n, "missing": 100.0 if n else 0.0}
    cm, cm_xy = np.array(err) * 100.0, np.array(err_xy) * 100.0
    q25, q75 = np.percentile(cm, [25, 75])
    return {"mean": float(cm.mean()), "mean xy": float(cm_xy.mean()), "std": float(cm.std()),
            "< 3cm": float((np.array(err) < _SMALL).sum()) / n, "25th percentile": float(q25),
            "75th percentile": float(q75), "missing": 100.0 * int(missing) / n, "points": n}


class DeviceResults:
    """The table of `Results`, the pose errors of up to four stages and the detection recall of labelled steps, tabulated on the device
    (ops.score_objects -> okp_score_objects; the specification is include/okp.h): add() is three launches behind the step - the labels into
    the step's frame (ops.change_frame, inverse), then the two of okp_score_objects - without a host synchronisation and, after the first call
    of a batch size, without an allocation beyond change_frame's one word, so it can be captured with the step; the log lives in device memory
    and summary() reads it in ONE device -> host copy.

    pipeline: a BatchedKeypointPipeline (the reference's view test through its camera) or a StereoStreamPipeline with rig_poses (a rig's
    table: no view test).  world_points [G, S, 3]: the labelled key points in the world frame, row 0 of every object its centre, the other
    rows in the table's slot order (SceneTargets.truth_points()).  Where the pipeline has points_3d the labelled objects' world poses T_WO
    are fitted once, here, by ops.object_pose on the labels; `label_rmse` [G] is that fit's rmse, and a label the fit refuses is refused.

    What the table does not say: without config.match_radius a false detection is scored against its nearest label, as in the reference;
    the rotation error has no symmetry allowance (a pose 120 degrees off on a nearly symmetric object reads 120); a rig's table is not
    tested for visibility."""
    POSE_SETS = ("fit", "refined", "track", "window")

    def __init__(self, pipeline, world_points, capacity_points=1 << 16, capacity_poses=1 << 14, config=None, device="cuda"):
        import torch
        from .. import ops
        self._torch, self._ops = torch, ops
        self.config = config if config is not None else ops.ScoreConfig()
        if not isinstance(self.config, ops.ScoreConfig):
            raise ops.OkpError("config must be an ops.ScoreConfig")
        pts = np.asarray(world_points, dtype=np.float64)
        if pts.ndim != 3 or pts.shape[2] != 3 or pts.shape[0] < 1 or not np.isfinite(pts).all():
            raise ops.OkpError(f"world_points must be finite [G, S, 3] with row 0 of every object its centre, not {pts.shape}")
        self.pipeline, self.device = pipeline, torch.device(device)
        rig = hasattr(pipeline, "stereo_cameras")
        if rig and pipeline._poses_host is None:
            raise ops.OkpError("DeviceResults serves a StereoStreamPipeline with rig_poses: the fused tick is what has one object table")
        self.rig = rig
        self.type_count = list(pipeline.config[1:]) if rig else list(pipeline.config['keypoint_config'])
        s = 1 + sum(self.type_count)
        if pts.shape[1] != s or not 1 <= pts.shape[0] <= ops.SCORE_MAX_OBJECTS:
            raise ops.OkpError(f"world_points is {list(pts.shape)}: the table has S = {s} rows per object, and at most {ops.SCORE_MAX_OBJECTS} labelled objects are scored")
        self.cam = None if rig else pipeline.cam
        self.size = None if rig else tuple(float(v) for v in pipeline.camera.image_size)
        self.G, self.S = int(pts.shape[0]), s
        self.log = ops.score_log(capacity_points, capacity_poses, self.device)
        self._truth_W = torch.from_numpy(np.concatenate([pts, np.ones(pts.shape[:2] + (1,))], axis=2)).to(self.device)      # [G,S,4]
        self._model = pipeline._model(self.device) if pipeline._model_host is not None else None
        self._pose_W, self.label_rmse = None, None
        if self._model is not None:
            n = torch.full((1,), self.G, dtype=torch.int32, device=self.device)
            fit = ops.object_pose(self._truth_W[None].contiguous(), n, self._model, self.type_count)
            status = fit["status"][0].cpu().numpy()
            if status.any():
                g = int(np.flatnonzero(status)[0])
                raise ops.OkpError(f"world_points: labelled object {g} is refused by the pose fit (status {int(status[g])}): its key points do not fit the object model")
            self._pose_W = fit["pose"][0].contiguous()                                                                    # [G,12]
            self.label_rmse = fit["fit"][0, :, 0].cpu().numpy()
        self._per_batch = {}

    def _buffers(self, b, max_obj):
        """What add() reads and writes besides the step, made once per batch size."""
        torch = self._torch
        buf = self._per_batch.get((b, max_obj))
        if buf is None:
            buf = {"truth_W": self._truth_W[None].expand(b, -1, -1, -1).contiguous(), "truth": torch.empty((b, self.G, self.S, 4), dtype=torch.float64, device=self.device),
                   "n_truth": torch.full((b,), self.G, dtype=torch.int32, device=self.device)}
            if self._pose_W is not None:
                buf["pose_W"] = self._pose_W[None].expand(b, -1, -1).contiguous()
                buf["pose"] = torch.empty((b, self.G, 12), dtype=torch.float64, device=self.device)
                buf["none"] = torch.full((b, max_obj, 12), float("nan"), dtype=torch.float64, device=self.device)       # a stage the step does not have
            self._per_batch[(b, max_obj)] = buf
        return buf

    def _frame(self, T):
        torch, ops = self._torch, self._ops
        if isinstance(T, torch.Tensor) and T.dim() == 2 and T.shape[1] == 12 and T.dtype == torch.float64 and T.is_cuda:
            return T.contiguous()
        return ops.frame_poses(T).to(self.device)

    def add(self, out, T_WC):
        """Score one step: out = the step's dict (forward_device / postprocess_device, a rig's fused device tick); T_WC [B,4,4], or the [B,12]
        device tensor of ops.frame_poses - for a rig tick the rig pose [1,12].  Returns ops.score_objects' {"match", "nearest"}."""
        ops = self._ops
        T = self._frame(T_WC)
        if "pose" in out:
            tab = out["pose"]["tab"]
        elif self.rig:
            tab = ops.rig_object_points(out["fused"], self.type_count)
        else:
            tab = ops.object_points(self.cam, out, self.type_count, int(self.pipeline.max_index[0]), int(self.pipeline.max_index[1]))
        n_obj = out["fused"]["n_obj"] if self.rig else out["n_obj"]
        b, max_obj = int(tab.shape[0]), int(tab.shape[1])
        if T.shape[0] != b:
            raise ops.OkpError(f"T_WC holds {T.shape[0]} poses, the step {b} frames")
        buf = self._buffers(b, max_obj)
        with_poses = "pose" in out and self._pose_W is not None
        ops.change_frame(T, points=buf["truth_W"], poses=buf["pose_W"] if with_poses else None, inverse=True, out_points=buf["truth"],
                         out_poses=buf["pose"] if with_poses else None)
        sets = []
        if with_poses:
            none = (buf["none"], None)
            track, window = out.get("track"), out.get("window")
            sets = [(out["pose"]["pose"], None), (out["refine"]["pose"], None) if "refine" in out else none, none, none]
            if track is not None:
                sets[2] = (track["track_pose_C"] if "track_pose_C" in track else track["track_pose"], track["track_of"])
                if window is not None:
                    sets[3] = (window["pose_B"] if self.rig else window["pose_C"], track["track_of"])
        return ops.score_objects(tab, n_obj.reshape(b), buf["truth"], buf["n_truth"], self.log, self.config, cam=self.cam, size=self.size, pose_sets=sets,
                                 truth_pose=buf["pose"] if with_poses else None, model=self._model if with_poses else None)

    def reset(self):
        """Empty the log in place (on the current stream): a captured add() keeps working."""
        self.log["buffer"].zero_()

    def _host(self):
        return self._ops.score_log_host(self.log)

    def summary(self):
        """{"keypoints": the keys of Results.summary() from the same NumPy calls; "detection": every counter by name and recall =
        truth_detected / truth_visible; "poses": per stage the step had, n and rotation_deg, centre_mm, model_rmse_mm as {median, p75, max}
        over the records that have it; "overflow": a record was dropped}.  ONE device -> host copy."""
        ops = self._ops
        host = self._host()
        c = host["counts"]
        nk, npose = int(c[ops.SCORE_KP_WRITTEN]), int(c[ops.SCORE_POSE_WRITTEN])
        detection = {name: int(c[i]) for i, name in enumerate(ops.SCORE_COUNTERS) if name != "overflow"}
        seen = detection["truth_visible"]
        detection["recall"] = detection["truth_detected"] / seen if seen else float("nan")
        poses = {}
        for p, name in enumerate(self.POSE_SETS):
            rec = host["pose_err"][:npose, p]
            rec = rec[~np.isnan(rec[:, 0])]
            if len(rec) == 0:
                continue
            cols = {"rotation_deg": rec[:, 0], "centre_mm": rec[:, 1] * 1000.0, "model_rmse_mm": rec[:, 2] * 1000.0}
            poses[name] = dict({"n": int(len(rec))}, **{k: {"median": float(np.median(v)), "p75": float(np.percentile(v, 75)), "max": float(v.max())}
                                                        for k, v in cols.items()})
        return {"keypoints": keypoint_summary(host["kp_err"][:nk, 0], host["kp_err"][:nk, 1], c[ops.SCORE_POINTS], c[ops.SCORE_MISSING]),
                "detection": detection, "poses": poses, "overflow": bool(int(c[ops.SCORE_OVERFLOW_WORD]) & ops.SCORE_OVERFLOW)}

    def worst(self, k, by="rotation_deg", pose="refined"):
        """The k worst pose records of one stage by one error -> [{"step", "frame", "object", "truth", by: value}], worst first."""
        ops = self._ops
        columns = {"rotation_deg": (0, 1.0), "centre_mm": (1, 1000.0), "model_rmse_mm": (2, 1000.0)}
        if by not in columns or pose not in self.POSE_SETS:
            raise ops.OkpError(f"worst: by is one of {sorted(columns)} and pose one of {list(self.POSE_SETS)}, not {by!r} / {pose!r}")
        host = self._host()
        npose = int(host["counts"][ops.SCORE_POSE_WRITTEN])
        col, unit = columns[by]
        v = host["pose_err"][:npose, self.POSE_SETS.index(pose), col] * unit
        order = [i for i in np.argsort(-np.nan_to_num(v, nan=-np.inf), kind="stable") if not np.isnan(v[i])][:int(k)]
        return [dict(zip(("step", "frame", "object", "truth"), (int(x) for x in host["pose_id"][i])), **{by: float(v[i])}) for i in order]
