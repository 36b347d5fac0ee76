"""Drop-in for the reference's perception/pipeline.py on the HIP path.

Same classes, constructor / __call__ signatures and return nesting as the reference
(perception/pipeline.py:13-209): InferenceComponent, KeypointExtractionComponent, ObjectExtraction,
DetectionToPoint, ObjectKeypointPipeline, LearnedKeypointTrackingPipeline, plus the
TriangulationComponent the reference's test expects (test/test_pipeline.py:171-177).

Device work (network, peak extraction, undistort + depth lifting, DLT) goes through libokp_hip.so;
the object-grouping glue (ObjectExtraction) is host logic as in the reference.  BatchedKeypointPipeline
is the data-parallel form of the same path: a whole batch of frames stays on the device from the
packed input to the per-peak 3D points (one D2H copy at the end).
"""
import numpy as np
import torch

from .. import ops
from ..ops import OkpError, OkpNotOffered
from . import models
from .utils import camera_utils  # noqa: F401  (re-exported like the reference module does)

DEFAULT_PEAK_CAPACITY = 64


def _device():
    if not torch.cuda.is_available():
        raise OkpError("the keypoint pipeline runs on the HIP device; no GPU is visible and there is no CPU fallback")
    return torch.device("cuda", torch.cuda.current_device())


def _is_torchscript_archive(path):
    """A TorchScript file is a zip archive with a `<name>/constants.pkl` and `<name>/code/` entries; a torch.save'd
    checkpoint is a zip without them (or a legacy pickle)."""
    import zipfile
    if not zipfile.is_zipfile(path):
        return False
    with zipfile.ZipFile(path) as z:
        names = z.namelist()
    return any(n.endswith("/constants.pkl") for n in names) and any("/code/" in n for n in names)


class _OpaqueGlobal:
    """Stand-in for a pickled global that is not a tensor-building function: callable, constructible, stateless.  Nothing of
    the module the pickle names is imported or run."""

    def __init__(self, *args, **kwargs):
        pass

    def __call__(self, *args, **kwargs):
        return _OpaqueGlobal()

    def __setstate__(self, state):
        pass


MAX_OPAQUE_GLOBALS = 256        # a training checkpoint names a handful of foreign classes; a file that names more is not one
# torch.serialization.safe_globals is PROCESS-global, not thread-local: while the stubs of one checkpoint are registered, a concurrent
# torch.load(weights_only=True) on another thread would resolve those foreign names to inert stubs instead of refusing them.  The
# loads of this module take the lock; other threads' own torch.load calls cannot be held off from here - load model files before
# starting threads that unpickle untrusted data.
import threading
_OPAQUE_LOAD_LOCK = threading.Lock()


def _load_with_opaque_globals(path):
    """torch.load(weights_only=True) - torch's own restricted unpickling VM, with its limits on what REDUCE / BUILD / NEWOBJ may touch -
    for a checkpoint that names globals the VM does not allow: each such global (torch.serialization.get_unsafe_globals_in_checkpoint
    lists them without unpickling anything) is registered as a SAFE global under its pickled name, bound to an inert stub class
    (_OpaqueGlobal: constructible, callable, stateless), for the duration of this one load.  Nothing the pickle names is imported or
    run; what a stub 'constructs' is another stub.  Needed for the reference's training checkpoints: pytorch-lightning 1.2.1
    (requirements.txt) keys the `callbacks` dict of a checkpoint by the callback CLASS (ModelCheckpoint, scripts/train.py:170) and
    stores hyper-parameter objects.  Residual trust: torch's VM itself and the tensor / storage rebuilders on its default allow-list
    (tests/test_host_logic.py pins that the allow-list names nothing outside torch, collections and builtins' containers).
    Zip-format files only (torch.save's format since 1.6; get_unsafe_globals_in_checkpoint reads nothing else): a legacy-format
    checkpoint that names foreign globals is refused with that explanation - re-save it with a current torch."""
    try:
        names = list(torch.serialization.get_unsafe_globals_in_checkpoint(path))
    except Exception as e:
        raise OkpError(f"{path}: cannot list the globals of this file ({type(e).__name__}: {e}); checkpoints that name classes outside torch "
                       "must be in torch.save's zip format (re-save a legacy-format file with a current torch)") from e
    if len(names) > MAX_OPAQUE_GLOBALS:
        raise OkpError(f"{path}: names {len(names)} globals outside torch's weights-only allow-list; not a training checkpoint")
    stubs = []
    for full in names:
        module, _, name = full.rpartition(".")
        stubs.append((type(name or "opaque", (_OpaqueGlobal,), {"__module__": "okp_opaque." + module}), full))
    with _OPAQUE_LOAD_LOCK, torch.serialization.safe_globals(stubs):
        return torch.load(path, map_location="cpu", weights_only=True)


def read_checkpoint_state_dict(path):
    """Tensors of a model file: TorchScript archive (scripts/package_model.py:40-42), torch.save'd state_dict, or a
    (pytorch-lightning) training checkpoint {"state_dict": ..., "callbacks": ..., ...}.  Never executes pickled code and never leaves
    torch's weights-only unpickler: a checkpoint that carries other globals is re-read with those bound to inert stubs
    (_load_with_opaque_globals) and only its tensors are kept.  Returns {name: tensor} with the module prefixes stripped."""
    import pickle
    if _is_torchscript_archive(path):
        sd = torch.jit.load(path, map_location="cpu").state_dict()
    else:
        try:
            sd = torch.load(path, map_location="cpu", weights_only=True)
        except pickle.UnpicklingError:
            try:
                sd = _load_with_opaque_globals(path)
            except Exception as e:
                raise OkpError(f"{path}: not a state_dict, Lightning checkpoint or TorchScript archive this loader can read ({e})") from e
        if isinstance(sd, dict) and isinstance(sd.get("state_dict"), dict):
            sd = sd["state_dict"]
    if not isinstance(sd, dict):
        raise OkpError(f"{path}: no state_dict found in the file")
    return strip_module_prefixes({k: v for k, v in sd.items() if isinstance(k, str) and isinstance(v, torch.Tensor)})


def strip_module_prefixes(sd):
    clean = {}
    for k, v in sd.items():
        for prefix in ("model.model.", "model."):          # TorchScript wrapper / Lightning module prefixes
            if k.startswith(prefix):
                k = k[len(prefix):]
                break
        clean[k] = v
    return clean


HEAT_BAR = 1e-3          # north_star: heat maps within 1e-3 of the fp32 reference


AUDIT_AUTO = "auto"      # load_keypoint_net(audit_frames=...): audit a mixed plan on two synthetic frames when the caller gives none


AUDIT_BATCH = 16         # the synthetic audit runs at a batch that takes the kernels a deployment takes (patch-resident kernel, pair tensors, fused heads)


def _audited(net, audit_frames, heat_bar, _source=None):
    """float32mix is a plan derived on ONE weight family: its single-term fp16 branches are cheap because BatchNorm
    gains attenuate them there.  With `audit_frames` the loaded network is priced on the device against float32x3 (fp32-grade, 2e-6)
    on the caller's frames (KeypointNet.precision_audit: two passes, no CPU reference) and, where the heat maps are further than
    `heat_bar` apart - or a value left the fp16 range: fp16 operands overflow above 65504 - the network falls back to float32x3 with a
    warning.  float32x3 itself is audited for that range (its one failure mode, KeypointNet.on_overflow): where the audit frames leave
    it, the network falls back to exact float32, again with a warning.
    The default (AUDIT_AUTO) audits a split-product configuration on synthetic frames - two N(0,1) frames repeated to a batch of
    AUDIT_BATCH, so that the launch heuristics pick the kernels a deployment runs - so that no such plan ships unverified on the weights it
    was loaded with; `net.audit` records the source of the frames and the batch.  Synthetic frames say nothing about activations on REAL
    frames: the per-pass guard (on_overflow) stays on.  16-bit configurations are the caller's explicit choice of a precision outside the
    bar and are audited only on request.  audit_frames=None skips the audit; for a mixed configuration that is said with a RuntimeWarning."""
    import warnings
    if audit_frames is None:
        if getattr(net, "mixed", False):
            warnings.warn(f"{net.configuration()}: loaded without an audit - this mixed-precision plan was derived on one weight family and is "
                          "UNVERIFIED on these weights (pass audit_frames, or leave the default, to price it against float32x3)", RuntimeWarning, stacklevel=3)
        return net
    source = _source or "caller"
    if isinstance(audit_frames, str):
        if audit_frames != AUDIT_AUTO:
            raise OkpError(f"audit_frames: a [n,3,H,W] tensor, None or '{AUDIT_AUTO}'")
        if not net.mfma_split:
            return net
        from .. import synth
        audit_frames = torch.from_numpy(synth.frames(2, seed=20251)).repeat(AUDIT_BATCH // 2, 1, 1, 1)
        source = "synthetic"
    if not (net.mfma_split or net.compute_dtype in ops.HALF_DTYPES):
        net.audit = {"configuration": net.configuration(), "checked": False, "reason": "exact float32: nothing to audit"}
        return net
    frames = audit_frames.to(next(net.parameters()).device, torch.float32)
    requested = net.configuration()
    base = {"configuration": requested, "checked": True, "frames": int(frames.shape[0]), "batch": int(frames.shape[0]), "frames_source": source, "heat_bar": heat_bar}
    if net.mfma_split and not net.mixed:
        # float32x3: one pass; its only failure mode is the fp16 range of its operands
        with torch.no_grad():
            outs = net.deployed(frames, check_range=False)
        ok = not net.range_overflow() and all(bool(torch.isfinite(t).all()) for t in outs)
        net.audit = dict(base, report={"range_ok": ok}, fell_back=not ok, fell_back_to=None if ok else "float32")
        if not ok:
            warnings.warn(f"{requested}: an activation leaves the fp16 range on the audit frames ({source}); falling back to exact float32", RuntimeWarning, stacklevel=3)
            net.set_compute_dtype(torch.float32)
        return net
    report = net.precision_audit(frames)
    ok = report["heat"]["finite"] and report["heat"]["max"] <= heat_bar
    net.audit = dict(base, report=report, fell_back=not ok, fell_back_to=None if ok else ops.F32X3)
    if not ok:
        warnings.warn(f"{requested}: heat maps differ from float32x3 by {report['heat']['max']:.2e} on the audit frames ({source}, batch {frames.shape[0]}; "
                      f"bar {heat_bar:.0e}, in range and finite: {report['heat']['finite']}); falling back to float32x3", RuntimeWarning, stacklevel=3)
        net.set_compute_dtype(ops.F32X3)
        if net.mixed is False and not report["heat"]["finite"]:
            return _audited(net, audit_frames, heat_bar, _source=source)          # the range may be the reason: float32x3 is audited for it in turn
    return net


def load_keypoint_net(model, compute_dtype=torch.float32, device=None, audit_frames=AUDIT_AUTO, heat_bar=HEAT_BAR, on_overflow="raise", range_guard=None,
                      frame_format=None):
    """Accepts a KeypointNet, a state_dict, or a path to a torch.save'd state_dict / Lightning checkpoint /
    TorchScript file produced by the reference's scripts/package_model.py, and returns an eval KeypointNet.
    Entries of the file that are not KeypointNet parameters (loss buffers, metrics of the Lightning module) are ignored;
    a missing network tensor is an error.
    audit_frames ([n,3,H,W] float32, a handful of representative frames): price a mixed / 16-bit `compute_dtype` on these weights and
    fall back to float32x3 when it misses `heat_bar` (see _audited; the result is in `net.audit`).  Default: a split-product configuration
    ("float32x3", "float32mix") is audited on synthetic frames; None skips the audit (with a RuntimeWarning for a mixed configuration).
    on_overflow ("raise" | "float32" | "defer"): what a pass of a split-product configuration does when an activation leaves the fp16
    range (KeypointNet.on_overflow): raise OkpError, re-run the pass with the exact float32 kernels, or leave the flag to the caller.
    range_guard (KeypointNet.range_guard): True runs a torch.float16 network under the same guard (on_overflow then applies to it); None
    keeps each configuration's default (a KeypointNet passed in keeps its own).
    frame_format (KeypointNet.frame_format): an ops.YUV420Format takes 3-D uint8 tensors as 4:2:0 decoder output (NV12 / I420); an
    ops.BayerFormat or ops.Mono8Format takes them as a camera's 8-bit Bayer mosaic / mono8 frames [N, H, W]; None keeps a KeypointNet's
    own (a new one refuses them)."""
    device = device or _device()
    if on_overflow not in ("raise", "float32", "defer"):
        raise OkpError("on_overflow is 'raise', 'float32' or 'defer'")
    if isinstance(model, models.KeypointNet):
        model.on_overflow = on_overflow
        if range_guard is not None:
            model.range_guard = range_guard
        if frame_format is not None:
            model.frame_format = frame_format
        return _audited(model.to(device).eval(), audit_frames, heat_bar)
    if isinstance(model, (str, bytes)) or hasattr(model, "__fspath__"):
        clean = read_checkpoint_state_dict(model)
    elif isinstance(model, dict):
        clean = strip_module_prefixes(model)
    else:
        raise OkpError("cannot interpret model argument")
    for need in ("heatmap_head.output_head2.2.weight", "heatmap_head.output_head2.0.conv.weight"):
        if need not in clean:
            raise OkpError(f"model file holds no KeypointNet: '{need}' is missing")
    heat_out = clean["heatmap_head.output_head2.2.weight"].shape[0]
    features = clean["heatmap_head.output_head2.0.conv.weight"].shape[0]
    net = models.KeypointNet(features=features, heatmaps_out=heat_out, compute_dtype=compute_dtype, range_guard=range_guard, frame_format=frame_format)
    own = net.state_dict()
    missing = [k for k in own if k not in clean]
    if missing:
        raise OkpError(f"model file lacks {len(missing)} KeypointNet tensors, e.g. '{missing[0]}'")
    net.load_state_dict({k: clean[k] for k in own})
    net.on_overflow = on_overflow
    return _audited(net.to(device).eval(), audit_frames, heat_bar)


def load_cornernet_backbone(net, pretrained):
    """Copies the hourglass of a CornerNet-Squeeze checkpoint into `net.backbone`, as the reference's
    KeypointNet._build_hourglass does with ./models/corner_net.pkl (perception/models.py:69-78: the pickle holds the
    DataParallel-wrapped detector, keys `module.hg.*`, loaded by core/nnet/py_factory.py:119-123); the detector's own
    corner heads (`module.tl_*`, `module.br_*`, ...) are not part of KeypointNet and are skipped.
    `pretrained`: a state_dict or a path to a torch.save'd one.  Returns the number of tensors copied."""
    if isinstance(pretrained, (str, bytes)) or hasattr(pretrained, "__fspath__"):
        pretrained = torch.load(pretrained, map_location="cpu", weights_only=True)      # tensors only: never runs pickled code
    own = net.backbone.state_dict()
    picked = {}
    for k, v in pretrained.items():
        for prefix in ("module.hg.", "hg."):
            if k.startswith(prefix):
                picked[k[len(prefix):]] = v
                break
    missing = [k for k in own if k not in picked]
    if missing:
        raise OkpError(f"CornerNet checkpoint lacks {len(missing)} hourglass tensors, e.g. {missing[0]}")
    bad = [k for k in own if tuple(picked[k].shape) != tuple(own[k].shape)]
    if bad:
        raise OkpError(f"CornerNet checkpoint: shape mismatch at {bad[0]}")
    net.backbone.load_state_dict({k: picked[k] for k in own})
    return len(own)


class InferenceComponent:
    name = "inference"

    def __init__(self, model, cuda=True, compute_dtype=torch.float32, on_overflow="float32", range_guard=None, frame_format=None):
        """on_overflow (split-product compute dtypes only): the reference's fp32 model returns numbers for any input; the drop-in does too -
        a pass whose activations leave the fp16 range is re-run with the exact float32 kernels ("float32", with a RuntimeWarning the first
        time) - unless the caller prefers an OkpError ("raise").  range_guard=True extends that to torch.float16 (KeypointNet.range_guard).
        frame_format (KeypointNet.frame_format): an ops.YUV420Format - frames may be 4:2:0 decoder output [N, 3H/2, W] uint8; an
        ops.BayerFormat or ops.Mono8Format - frames may be 8-bit Bayer mosaics / mono8 frames [N, H, W] uint8."""
        if not cuda:
            raise OkpError("InferenceComponent(cuda=False): this build has no CPU path (the CPU restatement is oracle/, test-only)")
        self.cuda = cuda
        self.model = load_keypoint_net(model, compute_dtype, on_overflow=on_overflow, range_guard=range_guard, frame_format=frame_format)

    def __call__(self, frames):
        frames = frames.to(_device())
        with torch.no_grad():
            heatmaps, depth, centers = [t.cpu() for t in self.model.deployed(frames)]
        return heatmaps, depth, centers


class KeypointExtractionComponent:
    name = "keypoints"
    PROBABILITY_CUTOFF = 0.1

    def __init__(self, keypoint_config, prediction_size, bandwidth=1.0, capacity=None):
        """capacity: peak slots per map; None (default) = one per pixel, i.e. no cap, like the reference
        (pipeline.py:73 keeps every peak).  The batched pipeline passes its fixed capacity explicitly."""
        self.keypoint_config = [1] + keypoint_config['keypoint_config']     # centre map first
        self.n_keypoints = sum(self.keypoint_config)
        self.prediction_size = prediction_size
        self.capacity = capacity

    def extract_device(self, frames):
        """frames N x K x H x W (device or host) -> device tensors (count, yx, xyc)."""
        if isinstance(frames, np.ndarray):
            frames = torch.from_numpy(np.ascontiguousarray(frames.astype(np.float32)))
        frames = frames.to(_device(), torch.float32)
        assert frames.shape[1] == len(self.keypoint_config)
        return ops.peak_nms(frames, cap=self.capacity or frames.shape[2] * frames.shape[3])

    def __call__(self, frames):
        count, _, xyc = self.extract_device(frames)
        count, xyc = count.cpu().numpy(), xyc.cpu().numpy()
        if self.capacity is not None and int(count.max(initial=0)) > self.capacity:
            raise OkpError(f"a heat map has {int(count.max())} peaks, above the capacity {self.capacity}; "
                           "raise `capacity` or leave it None (the reference has no cap)")
        keypoints, confidence = [], []
        for n in range(count.shape[0]):
            kp, cf = [], []
            for k in range(count.shape[1]):
                c = int(count[n, k])
                kp.append([xyc[n, k, j, :2].copy() for j in range(c)])          # (x, y) float32
                cf.append([xyc[n, k, j, 2] for j in range(c)])
            keypoints.append(kp)
            confidence.append(cf)
        return keypoints, confidence


class ObjectExtraction:
    """Centre-vector voting (interface and results of the reference's pipeline.py:93-153): the peaks of map 0 are object centres; every
    other peak votes with `pixel centre + predicted offset` at its rounded position for the nearest centre, votes further than
    VOTE_RADIUS pixels are dropped; per object and keypoint type the surplus over the configured count is reduced (most confident
    detection for a single-instance type, k-means centres for a multi-instance one).  Returns one dict per centre peak:
    {'center', 'heatmap_points': per type (n, 2) or empty, 'confidence': per type list, 'p_centers': the votes received}."""

    VOTE_RADIUS = 20.0

    def __init__(self, keypoint_config, prediction_size):
        self.keypoint_config = keypoint_config['keypoint_config']
        self.prediction_size = prediction_size
        h, w = prediction_size
        self.min = np.zeros(2, dtype=np.int32)
        self.max = np.array([w - 1, h - 1], dtype=np.int32)                      # (x, y) bounds of a rounded peak
        cols, rows = np.arange(w) + 0.5, np.arange(h) + 0.5
        self.image_indices = np.stack([np.broadcast_to(cols[None, :], (h, w)), np.broadcast_to(rows[:, None], (h, w))])   # (2, h, w): x, y of pixel centres

    def _votes(self, keypoints, centers, center_points):
        """All non-centre peaks of the frame at once -> (type index, index within its type, predicted centre (fp64), voted object or -1),
        in the reference's visiting order (type by type, peak by peak)."""
        types = [np.full(len(pts), i, dtype=np.int64) for i, pts in enumerate(keypoints[1:])]
        flat = [p for pts in keypoints[1:] for p in pts]
        if not flat:
            return np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros((0, 2)), np.zeros(0, np.int64)
        type_of = np.concatenate(types)
        within = np.concatenate([np.arange(len(pts)) for pts in keypoints[1:]])
        pts = np.stack(flat)
        cell = np.clip(np.round(pts).astype(np.int32), self.min, self.max)      # (x, y), half to even like ndarray.round
        predicted = (self.image_indices[:, cell[:, 1], cell[:, 0]] + centers[type_of, :, cell[:, 1], cell[:, 0]].T).T          # (n, 2) fp64
        delta = center_points[None, :, :] - predicted[:, None, :]
        dist = np.sqrt(delta[..., 0] * delta[..., 0] + delta[..., 1] * delta[..., 1])                                            # (n, n_centres)
        nearest = dist.argmin(axis=1)
        voted = np.where(dist[np.arange(len(pts)), nearest] > self.VOTE_RADIUS, -1, nearest)
        return type_of, within, predicted, voted

    def _reduce(self, points, confidences, wanted):
        if points.shape[0] <= wanted:
            return points
        if wanted == 1:
            return points[np.argmax(confidences)][None]
        from sklearn import cluster
        # the reference passes no n_init (pipeline.py:146) under its pinned scikit-learn 0.24.1, whose default is 10 restarts; newer
        # releases changed the default ('auto' -> 1 for init='random' from 1.4), so it is spelled out
        return cluster.KMeans(init='random', n_clusters=wanted, n_init=10).fit(points).cluster_centers_

    def __call__(self, keypoints, confidence, centers):
        if len(keypoints[0]) == 0:
            return []
        center_points = np.stack(keypoints[0])
        n_types = len(keypoints) - 1
        type_of, within, predicted, voted = self._votes(keypoints, np.asarray(centers), center_points)
        objects = []
        for o, c in enumerate(center_points):
            mine = voted == o
            obj = {'center': c, 'heatmap_points': [], 'p_centers': [p for p in predicted[mine]], 'confidence': []}
            for i in range(n_types):
                picked = within[mine & (type_of == i)]
                conf = [confidence[i + 1][j] for j in picked]
                obj['confidence'].append(conf)
                if len(picked) == 0:
                    obj['heatmap_points'].append(np.array([]))
                else:
                    obj['heatmap_points'].append(self._reduce(np.stack([keypoints[i + 1][j] for j in picked]), np.stack(conf), self.keypoint_config[i]))
            objects.append(obj)
        return objects


class DetectionToPoint:
    def reset(self, camera):
        self.camera = camera
        self.min_index = np.zeros(2, dtype=int)
        self.max_index = camera.image_size.astype(int) - 1

    def __call__(self, xy, p_depth):
        """xy (n,2) pixels + one depth map (H,W) -> (n,3) float64 camera-frame points (device kernel)."""
        if xy.shape[0] == 0:
            return None
        dev = _device()
        depth = torch.from_numpy(np.ascontiguousarray(p_depth, dtype=np.float32))[None].to(dev)
        pts = torch.from_numpy(np.ascontiguousarray(xy, dtype=np.float32)).to(dev)
        ids = torch.zeros(xy.shape[0], dtype=torch.int32, device=dev)
        # the reference clips x against image_size[0]-1 and y against image_size[1]-1 (pipeline.py:161-169)
        out = ops.unproject_depth(self.camera.okp(), pts, ids, depth, int(self.max_index[0]), int(self.max_index[1]))
        return out.cpu().numpy()

    def lift_groups(self, groups, p_depth):
        """Every keypoint group of a frame in ONE launch: groups = [(xy (n_i, 2), depth-map index k_i), ...], p_depth (K, H, W) ->
        [(n_i, 3) float64 or None, ...], each exactly what __call__(xy, p_depth[k_i]) returns (the kernel treats points one by one;
        one upload, one launch and one read-back per frame instead of three tiny transfers and a launch per group)."""
        sizes = [int(np.asarray(xy).shape[0]) for xy, _ in groups]
        if sum(sizes) == 0:
            return [None] * len(groups)
        dev = _device()
        xy_all = np.concatenate([np.asarray(xy, dtype=np.float32).reshape(-1, 2) for xy, _ in groups if np.asarray(xy).shape[0]], axis=0)
        ids_all = np.concatenate([np.full(n, k, dtype=np.int32) for n, (_, k) in zip(sizes, groups) if n])
        depth = torch.from_numpy(np.ascontiguousarray(p_depth, dtype=np.float32)).to(dev)
        out = ops.unproject_depth(self.camera.okp(), torch.from_numpy(np.ascontiguousarray(xy_all)).to(dev), torch.from_numpy(ids_all).to(dev),
                                  depth, int(self.max_index[0]), int(self.max_index[1])).cpu().numpy()
        res, at = [], 0
        for n in sizes:
            res.append(out[at:at + n] if n else None)
            at += n
        return res


class ObjectKeypointPipeline:
    def __init__(self, prediction_size, points_3d, keypoint_config):
        self.keypoint_extraction = KeypointExtractionComponent(keypoint_config, prediction_size)
        self.object_extraction = ObjectExtraction(keypoint_config, prediction_size)
        self.detection_to_point = DetectionToPoint()

    def reset(self, camera):
        self.detection_to_point.reset(camera)

    def __call__(self, heatmap, p_depth, p_centers):
        assert heatmap.shape[0] == 1, "One at the time, please."
        heatmap = heatmap.numpy() if isinstance(heatmap, torch.Tensor) else np.asarray(heatmap)
        p_centers = (p_centers[0].numpy() if isinstance(p_centers, torch.Tensor) else np.asarray(p_centers)[0])
        p_depth = (p_depth[0].numpy() if isinstance(p_depth, torch.Tensor) else np.asarray(p_depth)[0])
        points, confidence = self.keypoint_extraction(heatmap)
        detected_objects = self.object_extraction(points[0], confidence[0], p_centers)
        # the reference lifts group by group (pipeline.py:190-200); here all groups of the frame go through one launch
        groups = []
        for obj in detected_objects:
            groups.append((obj['center'][None], 0))
            for i in range(len(obj['heatmap_points'])):
                groups.append((obj['heatmap_points'][i], 1 + i))
        lifted = self.detection_to_point.lift_groups(groups, p_depth) if groups else []
        objects, at = [], 0
        for obj in detected_objects:
            n_groups = 1 + len(obj['heatmap_points'])
            objects.append({'p_centers': obj['p_centers'],
                            'keypoints': [obj['center'][None]] + obj['heatmap_points'],
                            'p_C': lifted[at:at + n_groups]})
            at += n_groups
        return objects


class LearnedKeypointTrackingPipeline(ObjectKeypointPipeline):
    def __init__(self, model, cuda=True, *args, **kwargs):
        """Keywords of its own, handed to InferenceComponent: compute_dtype, on_overflow, range_guard and frame_format (an ops.YUV420Format,
        ops.BayerFormat or ops.Mono8Format: the frames of __call__ may then be 4:2:0 [N, 3H/2, W] or Bayer / mono8 [N, H, W] uint8)."""
        compute_dtype = kwargs.pop("compute_dtype", torch.float32)
        on_overflow = kwargs.pop("on_overflow", "float32")
        range_guard = kwargs.pop("range_guard", None)
        frame_format = kwargs.pop("frame_format", None)
        super().__init__(*args, **kwargs)
        self.inference = InferenceComponent(model, cuda, compute_dtype=compute_dtype, on_overflow=on_overflow, range_guard=range_guard,
                                            frame_format=frame_format)

    def __call__(self, frame):
        heatmap, depth, centers = self.inference(frame)
        return super().__call__(heatmap, depth, centers), heatmap


class TriangulationComponent:
    """reset(stereo_camera); __call__(left (n,2), right (n,2)) -> (n,3) in the left camera frame."""

    def reset(self, stereo_camera):
        self.stereo_camera = stereo_camera

    def __call__(self, left_keypoints, right_keypoints):
        return self.stereo_camera.triangulate(left_keypoints, right_keypoints)


class AssociationComponent:
    """Left/right keypoint matching before triangulation: reset(stereo_camera); __call__(points_left (n,2),
    points_right (m,2)) -> int array (n,), -1 = unmatched.  The reference tree has no implementation; the contract is
    its test (test/test_pipeline.py:208-261).  Minimum-cost one-to-one assignment on the symmetric epipolar distance
    of the (device-)undistorted points; matches beyond `max_distance` pixels are dropped."""

    def __init__(self, max_distance=20.0):
        self.max_distance = float(max_distance)

    def reset(self, stereo_camera):
        self.stereo_camera = stereo_camera

    def cost(self, points_left, points_right):
        cam = self.stereo_camera
        ul = cam.left_camera.undistort(np.asarray(points_left, dtype=np.float64))
        ur = cam.right_camera.undistort(np.asarray(points_right, dtype=np.float64))
        hl = np.concatenate([ul, np.ones((ul.shape[0], 1))], axis=1)
        hr = np.concatenate([ur, np.ones((ur.shape[0], 1))], axis=1)
        lines_r, lines_l = hl @ cam.F.T, hr @ cam.F
        num = np.abs(lines_r @ hr.T)
        d_r = num / np.maximum(np.linalg.norm(lines_r[:, :2], axis=1), 1e-300)[:, None]
        d_l = num / np.maximum(np.linalg.norm(lines_l[:, :2], axis=1), 1e-300)[None, :]
        return 0.5 * (d_r + d_l)

    def __call__(self, points_left, points_right):
        from scipy.optimize import linear_sum_assignment
        points_left, points_right = np.asarray(points_left), np.asarray(points_right)
        out = np.full(points_left.shape[0], -1, dtype=np.int64)
        if points_left.shape[0] == 0 or points_right.shape[0] == 0:
            return out
        cost = self.cost(points_left, points_right)
        # gate first: a point without any admissible partner must not steal one (all its pairs cost the same)
        rows, cols = linear_sum_assignment(np.where(cost <= self.max_distance, cost, 1e6))
        keep = cost[rows, cols] <= self.max_distance
        out[rows[keep]] = cols[keep]
        return out


# Graph capture keeps the hourglass' forked side streams (fork / join by events captures as graph edges).  Round 1 captured
# without them because replays differed from the eager step at batch 64; the cause was a WAR race inside okp_fire2_kernel
# (fixed in round 2, see its phase-1 comment), not the graph: replays are bit-equal to the eager step either way
# (tests/test_gpu_bench_shapes.py::test_graph_replay_equals_eager_at_batch64).  False = capture the branches serially.
GRAPH_SIDE_STREAMS = True


def _capture(step):
    """`step` (a callable without arguments, reading static device tensors) as a hipGraph -> (graph, the static outputs of the captured call)."""
    for _ in range(2):                                       # warm-up: plans, allocator pools, kernel attributes, calibration tables
        step()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    keep, ops.SIDE_STREAMS = ops.SIDE_STREAMS, ops.SIDE_STREAMS and GRAPH_SIDE_STREAMS
    try:
        with torch.cuda.graph(graph):
            static_out = step()
    finally:
        ops.SIDE_STREAMS = keep
    return graph, static_out


def _raise_on_overflow(flag, fused=False):
    """A tick's overflow word (host int) as the OkpError it stands for; fused: the word of a fused tick, ops.FUSE_OVERFLOW read as well."""
    if flag & 1:
        raise OkpError("peak capacity exceeded in a tick; raise `capacity`")
    if flag & ops.RANGE_OVERFLOW:
        raise OkpError("an activation of the split-product network left the fp16 range in this tick: its maps are not fp32-grade "
                       "(load the network with on_overflow='float32', or run it in torch.float32)")
    if fused and flag & ops.FUSE_OVERFLOW:
        raise OkpError("a key-point type had more fused clusters than fit in a tick; raise `fuse_capacity`")


def _live_plans(net):
    """Every device plan object currently cached by the modules of `net` (ConvPlan / StemPlan / tuples of them)."""
    found = []

    def walk(v):
        if isinstance(v, (tuple, list)):
            for e in v:
                walk(e)
        elif isinstance(v, (ops.ConvPlan, ops.StemPlan)) or isinstance(v, torch.Tensor):
            found.append(v)

    for m in net.modules():
        for v in getattr(m, "_plans", {}).values():
            walk(v)
    return found


def _to_host(fields):
    """The one unpacker of the host readers: an ordered {name: device tensor} (float64, float32 or int32, all on one device) -> {name: ndarray of
    the same shape}, through ONE device -> host copy of their concatenation as float64 (int32 and float32 are exact in it); integer fields come
    back as int32."""
    flat = torch.cat([t.reshape(-1).to(torch.float64) for t in fields.values()]).cpu().numpy()
    host, at = {}, 0
    for name, t in fields.items():
        a = flat[at:at + t.numel()].reshape(tuple(t.shape))
        host[name] = a if t.dtype.is_floating_point else a.astype(np.int32)
        at += t.numel()
    return host


def _pose_fields(pose, n, refine=None):
    """What the readers take of frame n of an ops.object_pose dict: "pose" [max_obj,12], "fit" [max_obj,2], "status" [max_obj]; with an
    ops.refine_pose dict also "refine" (the refined pose [max_obj,12]), "refine_fit" [max_obj,4], "information" [max_obj,36], "refine_status";
    with an ops.refine_assignments dict also "refine_assignment" [max_obj,S], "refine_hypothesis" [max_obj,2] and "refine_cost" [max_obj,2]."""
    fields = {"pose": pose["pose"][n], "fit": pose["fit"][n], "status": pose["status"][n]}
    if refine is not None:
        fields.update(refine=refine["pose"][n], refine_fit=refine["fit"][n], information=refine["information"][n], refine_status=refine["status"][n])
        if "n_obs" in refine:                    # an ops.refine_pose_views dict (a rig): "refine_fit" is [max_obj,2], and "refine_n_obs" [max_obj]
            fields.update(refine_n_obs=refine["n_obs"][n])
        if "n_inlier" in refine:                 # under a Huber loss (RefineConfig.huber_px): "refine_fit" is [max_obj,4], "refine_weight" [max_obj,S,V]
            fields.update(refine_n_inlier=refine["n_inlier"][n], refine_weight=refine["weight"][n])
        if "prior" in refine:                    # weighted by the peaks' confidences (RefineConfig.confidence): "refine_prior" [max_obj,S,V]
            fields.update(refine_prior=refine["prior"][n])
        if "hypothesis" in refine:
            fields.update(refine_assignment=refine["assignment"][n], refine_hypothesis=refine["hypothesis"][n], refine_cost=refine["cost"][n])
        if "resolve_status" in refine:           # a rig's resolve_views: the resolver's own status next to the refinement's
            fields.update(resolve_status=refine["resolve_status"][n])
    return fields


def _track_fields(track, n, window=None):
    """What the readers take of stream n of a tick's "track" dict: "track_pose" [T,12], "track_f" [T,16], "track_i" [T,4], "track_of" [max_obj],
    "meas_of" [T] and, of a world-frame tick, "track_pose_C" [T,12] - the track poses back in the camera / rig frame; with the step's "window"
    dict also "window_pose" and "window_pose_C" [T,12], "window_fit" [T,2], "window_n_views" [T], "window_information" [T,36], "window_status" [T]."""
    fields = {k: track[k][n] for k in ("track_pose", "track_f", "track_i", "track_of", "meas_of", "track_pose_C") if k in track}
    if window is not None:
        fields.update({"window_" + k: window[k][n] for k in ("pose", "fit", "n_views", "information", "status")})
        fields["window_pose_C"] = window["pose_C" if "pose_C" in window else "pose_B"][n]       # (a rig's window: the rig frame, [T,S,W*V] weights)
        if "n_inlier" in window:                 # under a Huber loss (WindowConfig.huber_px): "window_fit" is [T,4], "window_weight" [T,S,W]
            fields.update(window_n_inlier=window["n_inlier"][n], window_weight=window["weight"][n])
        if "prior" in window:                    # weighted by the confidences (WindowConfig.confidence): "window_prior" [T,S,W] ([T,S,W*V] for a rig)
            fields.update(window_prior=window["prior"][n])
        if "velocity" in window:                 # a moving object (WindowConfig.motion): "window_velocity" [T,3], and "window_information" is [T,81]
            fields.update(window_velocity=window["velocity"][n])
    return fields


def _host_poses(pose, n, refine=None):
    """_pose_fields on the host, in ONE device -> host copy."""
    return _to_host(_pose_fields(pose, n, refine))


def _host_tracks(track, n, window=None):
    """_track_fields on the host, in ONE device -> host copy."""
    return _to_host(_track_fields(track, n, window))


def _window_entries(rec, slot, key='T_CO_window', cameras=None):
    """A track slot's windowed pose as the entries tracks() adds: 'T_WO_window' and `key`, 'T_CO_window' or a rig's 'T_BO_window' (4 x 4; None where 'window_status' is not 0 -
    a short window, a free slot, a refused refinement - or, for 'T_CO_window', the camera pose is missing: the caller falls back to the
    track pose), 'window_views' (filled ring columns), 'window_rmse' (reprojection rmse before, after; map pixels), 'window_information'
    (6 x 6) and 'window_status'; under a Huber loss also 'window_inliers', 'window_robust_rmse' (the rmse of the robust cost before, after; map
    pixels) and 'window_outliers', the (model row, ring column) entries the final iterate down-weighted - of a rig's window, whose ring
    column holds `cameras` views, (model row, ring column, camera)."""
    ok = int(rec["window_status"][slot]) == 0
    fit = rec["window_fit"][slot]
    entries = {'T_WO_window': _track_transform(rec["window_pose"][slot]) if ok else None, key: _track_transform(rec["window_pose_C"][slot]) if ok else None,
               'window_views': int(rec["window_n_views"][slot]), 'window_rmse': (float(fit[0]), float(fit[1])),
               'window_information': rec["window_information"][slot].reshape(*((9, 9) if "window_velocity" in rec else (6, 6))).copy(),
               'window_status': int(rec["window_status"][slot])}
    if "window_velocity" in rec:             # WindowConfig.motion: the object's linear velocity in the world frame, metres per second; the information is 9 x 9
        entries.update(window_velocity=rec["window_velocity"][slot].copy() if ok else None)
    if "window_n_inlier" in rec:
        outliers = _outliers(rec["window_weight"][slot])
        if cameras is not None:
            outliers = [(s, v // cameras, v % cameras) for s, v in outliers]
        entries.update(window_inliers=int(rec["window_n_inlier"][slot]), window_robust_rmse=(float(fit[2]), float(fit[3])), window_outliers=outliers)
    if "window_prior" in rec:                # WindowConfig.confidence: 'window_priors', indexed as 'window_outliers' is, with the prior as the last value
        priors = _priors(rec["window_prior"][slot])
        if cameras is not None:
            priors = [(s, v // cameras, v % cameras, a) for s, v, a in priors]
        entries.update(window_priors=priors)
    return entries


def _priors(prior):
    """The (row, column, prior) entries of one object's table of priors [S,V] that hold one: the bearings it has (NaN: no bearing)."""
    return [(int(s), int(v), float(prior[s, v])) for s, v in zip(*np.nonzero(~np.isnan(prior)))]


def _outliers(weight):
    """The (row, column) entries of one object's weight table [S,V] with weight < 1: what the Huber loss down-weighted (NaN: no observation)."""
    with np.errstate(invalid="ignore"):
        return [(int(s), int(v)) for s, v in zip(*np.nonzero(weight < 1.0))]


def _refine_entries(rec, o, T_CO):
    """Object o's refined pose as the entries objects() adds: 'T_CO_refined' (None where 'T_CO' is; the fitted pose where the refinement's
    status is not 0), 'reprojection_rmse' and 'depth_rmse' (before, after), 'pose_information' (6 x 6) and 'refine_status'."""
    fit = rec["refine_fit"]
    T = None
    if T_CO is not None:
        T = np.eye(4)
        T[:3] = rec["refine"][o].reshape(3, 4)
    entries = {'T_CO_refined': T, 'reprojection_rmse': (float(fit[o, 0]), float(fit[o, 1])), 'depth_rmse': (float(fit[o, 2]), float(fit[o, 3])),
               'pose_information': rec["information"][o].reshape(6, 6).copy(), 'refine_status': int(rec["refine_status"][o])}
    if "refine_hypothesis" in rec:           # resolve_assignment: the winning assignment (model row per slot), (winner, runner-up) indices and costs
        entries.update(assignment_refined=rec["refine_assignment"][o].copy(), refine_hypothesis=tuple(int(h) for h in rec["refine_hypothesis"][o]),
                       refine_cost=tuple(float(c) for c in rec["refine_cost"][o]))
    return entries


def _rig_refine_entries(rec, o, T_BO):
    """Object o's refined pose as the entries rig_objects() adds: 'T_BO_refined' (None where 'T_BO' is; the fitted pose where the refinement's
    status is not 0), 'reprojection_rmse' (before, after), 'refine_observations', 'pose_information' (6 x 6) and 'refine_status'; under a
    Huber loss also 'refine_inliers', 'robust_rmse' (the rmse of the robust cost before, after; map pixels) and 'refine_outliers', the
    (table slot, camera) entries the final iterate down-weighted."""
    fit = rec["refine_fit"]
    T = None
    if T_BO is not None:
        T = np.eye(4)
        T[:3] = rec["refine"][o].reshape(3, 4)
    entries = {'T_BO_refined': T, 'reprojection_rmse': (float(fit[o, 0]), float(fit[o, 1])), 'refine_observations': int(rec["refine_n_obs"][o]),
               'pose_information': rec["information"][o].reshape(6, 6).copy(), 'refine_status': int(rec["refine_status"][o])}
    if "refine_n_inlier" in rec:
        entries.update(refine_inliers=int(rec["refine_n_inlier"][o]), robust_rmse=(float(fit[o, 2]), float(fit[o, 3])), refine_outliers=_outliers(rec["refine_weight"][o]))
    if "refine_prior" in rec:                # RefineConfig.confidence: 'refine_priors', (table slot, camera, prior) of every bearing the object has
        entries.update(refine_priors=_priors(rec["refine_prior"][o]))
    if "refine_hypothesis" in rec:           # resolve_views: the winning assignment (model row per slot), (winner, runner-up) indices and costs, the resolver's status
        entries.update(assignment_refined=rec["refine_assignment"][o].copy(), refine_hypothesis=tuple(int(h) for h in rec["refine_hypothesis"][o]),
                       refine_cost=tuple(float(c) for c in rec["refine_cost"][o]), resolve_status=int(rec["resolve_status"][o]))
    return entries


def _pose_entries(rec, o, key):
    """Object o's pose as the entries objects() / rig_objects() add: the 4 x 4 transform under `key` (None where the status refuses a pose)."""
    fit, status = rec["fit"], int(rec["status"][o])
    T = None
    if not status & (ops.POSE_FEW | ops.POSE_DEGENERATE):
        T = np.eye(4)
        T[:3] = rec["pose"][o].reshape(3, 4)
    return {key: T, 'rmse': float(fit[o, 0]), 'ambiguity': float(fit[o, 1]), 'pose_status': status}


def _track_transform(row):
    if not np.isfinite(row).all():           # (a world-frame track seen from a tick whose camera pose is missing)
        return None
    T = np.eye(4)
    T[:3] = row.reshape(3, 4)
    return T


def _track_poses(rec, slot, key, world_key):
    """The filtered pose of a track slot under `key` (the camera or rig frame) and, for a world-frame tick, under `world_key` as well: the
    tracker's own pose is then the world one and `key` is read from the inverse transform."""
    if "track_pose_C" not in rec:
        return {key: _track_transform(rec["track_pose"][slot])}
    return {world_key: _track_transform(rec["track_pose"][slot]), key: _track_transform(rec["track_pose_C"][slot])}


def _track_entries(rec, o, key, min_hits, world_key=None, cameras=None):
    """Object o's track as the entries objects() / rig_objects() add: 'track_id' (None: the object went to no track - a position-only or
    dropped measurement), the filtered pose under `key`, 'velocity', 'track_hits', 'confirmed'."""
    slot = int(rec["track_of"][o])
    windowed = "window_status" in rec        # the window segment: 'T_CO_window' / 'T_BO_window' and 'window_views' of the object's track
    window_key = key.replace("_track", "_window")
    if slot < 0:
        none = {key: None} if "track_pose_C" not in rec else {world_key: None, key: None}
        if windowed:
            none.update({window_key: None, 'window_views': 0})
        return dict({'track_id': None, 'velocity': None, 'track_hits': 0, 'confirmed': False}, **none)
    hits = int(rec["track_i"][slot, 1])
    entries = dict({'track_id': int(rec["track_i"][slot, 0]), 'velocity': rec["track_f"][slot, 3:6].copy(), 'track_hits': hits, 'confirmed': hits >= min_hits},
                   **_track_poses(rec, slot, key, world_key))
    if windowed:
        w = _window_entries(rec, slot, window_key, cameras)
        entries.update({window_key: w[window_key], 'window_views': w['window_views']})
    return entries


def _track_list(rec, key, min_hits, world_key=None, cameras=None):
    """Every live track, coasting ones included, in slot order."""
    track_f, track_i, meas_of = rec["track_f"], rec["track_i"], rec["meas_of"]
    return [dict({'track_id': int(track_i[i, 0]), 'velocity': track_f[i, 3:6].copy(), 'hits': int(track_i[i, 1]),
                  'misses': int(track_i[i, 2]), 'age': int(track_i[i, 3]), 'confirmed': int(track_i[i, 1]) >= min_hits,
                  'object': int(meas_of[i]) if meas_of[i] >= 0 else None}, **_track_poses(rec, i, key, world_key),
                 **(_window_entries(rec, i, key.replace("_track", "_window"), cameras) if "window_status" in rec else {}))
            for i in range(track_i.shape[0]) if track_i[i, 0] != 0]


class _PerDevice:
    """A host tensor, uploaded once per device and kept for the pipeline's life - captured steps read the device copy on every replay:
    cache(device) -> that copy; cache.host: the host tensor (None: the feature it serves is off); cache.on: {device: copy}."""

    def __init__(self, host):
        self.host, self.on = host, {}

    def __call__(self, device):
        t = self.on.get(device)
        if t is None:
            t = self.on[device] = self.host.to(device)
        return t


class _Tracker:
    """The device state of a pipeline's tracker, one ops.track_state per (device, streams), created on first use and kept for the pipeline's
    life: captured steps hold these very tensors, so reset() zeroes them in place."""

    def __init__(self, cfg):
        self.cfg, self.states = cfg, {}

    def state(self, device, streams):
        st = self.states.get((device, streams))
        if st is None:
            st = self.states[(device, streams)] = ops.track_state(streams, self.cfg.max_tracks, device)
        return st

    def step(self, tab, pose, status, n_obj, model, overflow):
        """ops.track_objects on the state of the table's device and streams -> its outputs plus the state tensors."""
        st = self.state(tab.device, int(tab.shape[0]))
        return dict(ops.track_objects(st, tab, pose, status, n_obj, model, self.cfg, overflow=overflow), **st)

    def reset(self):
        for st in self.states.values():
            for t in st.values():
                t.zero_()


def _refine_static(cfg, each, wide, obs, prior, views, start, n_obj, model):
    """The one launch that refines static objects against views under cfg -> its dict: with cfg.confidence the weighted refinement, on the bearings'
    priors (a push under it kept the ring of them); otherwise the plain one of the same shape (each: a views table per object; wide: beyond one wave)."""
    if cfg.confidence is not None:
        return ops.refine_pose_views_weighted(obs, prior, views, start, n_obj, model, cfg, each=each, wide=wide)
    if wide:
        return ops.refine_pose_views_wide(obs, views, start, n_obj, model, cfg, each=each)
    return (ops.refine_pose_views_each if each else ops.refine_pose_views)(obs, views, start, n_obj, model, cfg)


class _Window:
    """The device state of a pipeline's sliding window, one ops.window_state per (device, streams), created on first use and kept for the
    pipeline's life like the tracker's: captured steps hold these very tensors, so reset() empties them in place."""

    def __init__(self, cfg, max_tracks, dt=None):
        self.cfg, self.max_tracks, self.states, self.dt = cfg, max_tracks, {}, dt      # dt: the tracker's seconds per tick, what an age is counted in

    def state(self, device, streams, rows):
        st = self.states.get((device, streams))
        if st is None:
            st = self.states[(device, streams)] = ops.window_state(streams, self.max_tracks, rows, self.cfg.ticks, device, **self._prior())
        return st

    def _prior(self):
        """The keyword that gives the state its ring of priors - only under cfg.confidence - or the ages of its columns - only under cfg.motion:
        without either the call is the one it was."""
        return {"prior": True} if self.cfg.confidence is not None else {"timed": True} if self.cfg.motion is not None else {}

    def _moving(self, st, pushed, model, T, pose_key):
        """cfg.motion: ops.refine_motion_views on the timed state from the pushed start and start velocity, and the refined poses back in the
        frame of T -> the entries of the step's "window" dict: "velocity" and "win_age" more, "information" [.., 81]."""
        start = {"pose": pushed["start"], "velocity": pushed["start_velocity"], "assignment": st["win_assignment"]}
        refined = ops.refine_motion_views(st["win_obs"], st["win_views"], st["win_age"], start, st["win_n"], model, self.cfg, self.dt)
        local = ops.change_frame(T, poses=refined["pose"], inverse=True)["poses"]
        return {"pose": refined["pose"], "fit": refined["fit"], "n_obs": refined["n_obs"], "n_views": pushed["n_views"], "information": refined["information"],
                "status": refined["status"], pose_key: local, "velocity": refined["velocity"], "win_obs": st["win_obs"], "win_views": st["win_views"],
                "win_i": st["win_i"], "win_age": st["win_age"]}

    def _static(self, st, pushed, refined, T, pose_key, **tick):
        """The entries of the step's "window" dict for a static object, from the state, the pushed dict and the refined dict: the refined poses
        also back in the frame of T, under pose_key; `tick`: what a rig's tick puts right after them (its "tick_obs")."""
        local = ops.change_frame(T, poses=refined["pose"], inverse=True)["poses"]
        out = {"pose": refined["pose"], "fit": refined["fit"], "n_obs": refined["n_obs"], "n_views": pushed["n_views"], "information": refined["information"],
               "status": refined["status"], pose_key: local, **tick, "win_obs": st["win_obs"], "win_views": st["win_views"], "win_i": st["win_i"]}
        if "n_inlier" in refined:                # cfg.huber_px: the refinement was the Huber instance
            out.update(n_inlier=refined["n_inlier"], weight=refined["weight"])
        if "win_prior" in st:                    # cfg.confidence: the ring of priors, a state tensor like win_obs
            out.update(prior=st["win_prior"])
        return out

    def step(self, tab, assignment, status, track, T_WC, cam, model):
        """ops.window_push on the state of the table's device and streams, ops.refine_pose_views_each on that state from the pushed start, and
        the refined poses back in the camera frame -> the entries of the step's "window" dict."""
        st = self.state(tab.device, int(tab.shape[0]), int(tab.shape[2]))
        pushed = ops.window_push(st, tab, assignment, status, track, T_WC, cam, self.cfg)
        if self.cfg.motion is not None:
            return self._moving(st, pushed, model, T_WC, "pose_C")
        start = {"pose": pushed["start"], "assignment": st["win_assignment"]}
        refined = _refine_static(self.cfg, True, False, st["win_obs"], st.get("win_prior"), st["win_views"], start, st["win_n"], model)
        return self._static(st, pushed, refined, T_WC, "pose_C")

    def reset(self):
        for st in self.states.values():
            st["win_obs"].fill_(float("nan"))
            st["win_views"].zero_()
            st["win_i"].zero_()
            if "win_prior" in st:
                st["win_prior"].fill_(float("nan"))
            if "win_age" in st:
                st["win_age"].zero_()


class _RigWindow(_Window):
    """_Window for a rig: a ring column holds the tick's bearings in all `cameras` cameras (ops.window_views_state, ops.window_push_views) and
    the refinement is the one beyond one wave (ops.refine_pose_views_wide, a views table per track)."""

    def __init__(self, cfg, max_tracks, cameras, dt=None):
        super().__init__(cfg, max_tracks, dt)
        self.cameras = cameras

    def state(self, device, streams, rows):
        st = self.states.get((device, streams))
        if st is None:
            st = self.states[(device, streams)] = ops.window_views_state(streams, self.max_tracks, rows, self.cfg.ticks, self.cameras, device, **self._prior())
        return st

    def step(self, obs, assignment, status, track, T_WB, views, model, prior=None):
        """ops.window_push_views on the state of the bearings' device and streams, ops.refine_pose_views_wide on that state from the pushed
        start, and the refined poses back in the rig frame -> the entries of the tick's "window" dict."""
        st = self.state(obs.device, int(obs.shape[0]), int(obs.shape[2]))
        pushed = ops.window_push_views(st, obs, assignment, status, track, T_WB, views, self.cfg, **({"prior": prior} if prior is not None else {}))
        if self.cfg.motion is not None:
            out = self._moving(st, pushed, model, T_WB, "pose_B")
            out["tick_obs"] = obs
            return out
        start = {"pose": pushed["start"], "assignment": st["win_assignment"]}
        refined = _refine_static(self.cfg, True, True, st["win_obs"], st.get("win_prior"), st["win_views"], start, st["win_n"], model)
        out = self._static(st, pushed, refined, T_WB, "pose_B", tick_obs=obs)
        if "win_prior" in st:                    # cfg.confidence: next to the ring of priors, the tick's
            out.update(tick_prior=prior)
        return out


def _check_frame_pose(pose, world_frame, streams, device, name, what):
    """The per-tick pose argument of both device pipelines against their world_frame switch: both or neither."""
    if not world_frame:
        if pose is not None:
            raise OkpError(f"{name} given to a pipeline built without world_frame")
        return None
    if pose is None:
        raise OkpError(f"{name} is required by a pipeline built with world_frame: ops.frame_poses(...).to(device), {what}")
    if not isinstance(pose, torch.Tensor) or pose.dtype != torch.float64 or tuple(pose.shape) != (streams, 12) or pose.device != device or not pose.is_contiguous():
        raise OkpError(f"{name} must be a float64 [{streams},12] tensor on the frames' device ({device}): ops.frame_poses(...).to(device), {what}")
    return pose


class _ObjectStage:
    """Everything that follows the object point table in a device step, for both device pipelines - each makes its table its own way
    (okp_object_points from a camera's lifted peaks, okp_rig_object_points from a rig's fused clusters) and names the frame ('T_CO' / 'T_BO'):

    Pose (points_3d, the object model: [sum(type_count), 3] key points in model coordinates in type order, validated here by ops.object_model
    and uploaded once per device): okp_object_pose -> "pose", ops.object_pose's dict plus "tab".  max_rmse (metres, optional): objects that
    fit worse carry ops.POSE_POOR.
    Refinement (refine = ops.RefineConfig(...), needs the pose and the camera the table was lifted through): okp_refine_pose -> "refine",
    ops.refine_pose's dict.  "pose" keeps its bits; the world-frame change and the tracker are fed the refined pose from here on.  With
    RefineConfig(..., resolve_assignment=True) the one launch is okp_refine_assignments instead - every assignment of the interchangeable key
    points refined, the one of least final cost kept - and "refine" is ops.refine_assignments' dict ("assignment", "hypothesis", "cost" too);
    a model with more than ops.REFINE_MAX_HYPOTHESES assignments is refused at construction.  A rig's table holds fused points, not one camera's
    bearings: its step hands run() `rig` - the tick's peaks, matches, fusion, calibration table and views table - and the refinement is
    okp_rig_bearings, then okp_refine_pose_views against the bearings of every camera; "refine" is ops.refine_pose_views' dict plus "obs".
    With RefineConfig(..., huber_px=h) that second launch is okp_refine_pose_views_robust - the same refinement under a Huber loss - and
    "refine" gains "n_inlier" and "weight" (WindowConfig(..., huber_px=h) does the same to the window's refinement and "window").
    World frame (world_frame=True; the step's frame_pose [B,12] takes the table's frame to the world, an all-NaN row = missing in this tick):
    okp_change_frame on the step's points and, with the pose, on the table and the poses -> "world": {"T", "points", "overflow" (the
    step's word | ops.FRAME_MISSING)} and "tab", "pose".
    Tracking (track = ops.TrackConfig(...), needs the pose): okp_track_objects - in the world frame where there is one, on "world"'s table,
    poses and overflow word - -> "track": ops.track_objects' outputs plus the state tensors "track_f", "track_i", "next_id" (one state per
    device and number of streams, kept for the pipeline's life) and, in the world frame, "track_pose_C": the filtered poses back in the table's
    frame (okp_change_frame, inverse).  "track"["overflow"] is the word it was given | ops.TRACK_OVERFLOW.
    Window (window = ops.WindowConfig(...), the camera pipeline's; needs the pose, the tracker and the world frame): okp_window_push keeps a
    ring of the last `ticks` measured ticks per track slot - the CAMERA-frame table's bearings by model row (under the refined assignment where
    resolve_assignment produced one) and each tick's camera-from-world pose -, okp_refine_pose_views_each refines every track's world pose
    against its ring, and okp_change_frame (inverse) takes the result back into the camera frame -> "window": {"pose" (T_WO [B,T,12]), "fit",
    "n_obs", "n_views", "information", "status", "pose_C", and the state "win_obs", "win_views", "win_i"} (one state per device and number of
    streams, kept for the pipeline's life; reset_tracks() empties it too).  Static objects only: the ring does not model motion.

    A rig's window (rig_cameras = 2 P, the rig pipeline's rig_window): a ring column holds one TICK of all 2 P cameras - okp_window_push_views
    takes the tick's table of bearings (okp_rig_bearings: the refinement's where there is one, otherwise launched here) and composes every
    camera's row of the views table with the tick's rig pose -, okp_refine_pose_views_wide refines every track's world pose against its
    ticks x 2 P views, and okp_change_frame (inverse) takes the result back into the rig frame -> "window" with "pose_B" where the camera
    window has "pose_C", plus "tick_obs", the tick's bearings.

    Every launch is captured with the step it ends.  Without any of the five no launch, key or value of the step differs."""

    def __init__(self, type_count, points_3d, max_rmse, track, max_obj, what, world_frame, refine=None, window=None, rig_cameras=0):
        self.type_count, self.world_frame = type_count, bool(world_frame)
        if points_3d is None and max_rmse is not None:
            raise OkpError("max_rmse without points_3d: the pose needs the object model")
        self.model = _PerDevice(ops.object_model(points_3d, type_count) if points_3d is not None else None)       # (.host None: pose off)
        self.max_rmse = ops.check_max_rmse(max_rmse) if points_3d is not None else None
        if track is not None:
            if not isinstance(track, ops.TrackConfig):
                raise OkpError("track must be an ops.TrackConfig")
            if points_3d is None:
                raise OkpError("track without points_3d: the tracker follows the poses of the object model")
            if max_obj > ops.TRACK_MAX_OBJECTS:
                raise OkpError(f"{what} = {max_obj}: the tracker takes at most {ops.TRACK_MAX_OBJECTS} objects per stream")
        self.tracker = _Tracker(track) if track is not None else None
        if refine is not None:
            if not isinstance(refine, ops.RefineConfig):
                raise OkpError("refine must be an ops.RefineConfig")
            if points_3d is None:
                raise OkpError("refine without points_3d: the refinement starts from the pose of the object model")
            if refine.resolve_assignment or refine.resolve_views:
                ops.check_refine_hypotheses(type_count)
        self.refine = refine
        # a rig's resolve_views: the resolver reads sigma_px, iters and damping; the configured refinement that follows it is called without the keyword
        self.resolver = ops.RefineConfig(refine.sigma_px, refine.sigma_z, refine.iters, refine.damping) if getattr(refine, "resolve_views", False) else None
        self.refine_after = ops.without_resolve_views(refine) if self.resolver is not None else refine
        if window is not None:
            name, pose = ("rig_window", "rig_pose") if rig_cameras else ("window", "camera_pose")      # (a rig's keyword: its ring holds rig_cameras views per tick)
            if not isinstance(window, ops.WindowConfig):
                raise OkpError(f"{name} must be an ops.WindowConfig")
            for missing, why in ((points_3d is None, "points_3d: the window refines the pose of the object model"), (track is None, "track: a window belongs to a track"),
                                 (not world_frame, f"world_frame=True: the ticks of a window share the world frame, through each tick's {pose}")):
                if missing:
                    raise OkpError(f"{name} without {why}")
        self.window = None
        if window is not None:
            if window.motion is not None and rig_cameras * window.ticks > ops.REFINE_MAX_VIEWS:
                raise OkpNotOffered(f"{name}: motion with 2 x {rig_cameras // 2} pairs x {window.ticks} ticks = {rig_cameras * window.ticks} views exceeds the "
                                        f"{ops.REFINE_MAX_VIEWS} of okp_refine_motion_views (the wide motion kernel is a follow-up)")
            moving = {"dt": track.dt} if window.motion is not None else {}
            self.window = _RigWindow(window, track.max_tracks, rig_cameras, **moving) if rig_cameras else _Window(window, track.max_tracks, **moving)
        # a rig's one launch of the bearings serves the refinement and the window: the priors it writes follow one ConfidenceWeights
        given = [c for c in (getattr(refine, "confidence", None), getattr(window, "confidence", None) if rig_cameras else None) if c is not None]
        if len(given) == 2 and (given[0].ref, given[0].floor) != (given[1].ref, given[1].floor):
            raise OkpError(f"refine has confidence = {given[0]} and rig_window confidence = {given[1]}: the tick's bearings are collected, and their priors "
                           "formed, in one launch for both, so the two must agree")
        self.bearings_confidence = given[0] if given else None

    def run(self, tab, n_obj, points, overflow, frame_pose, cam=None, rig=None):
        """The stage behind a step: tab = the object point table (None without a model), n_obj, points (what the world frame shows besides the
        objects) and overflow = the step's own; frame_pose: the checked per-step pose, or None; cam: the camera of a refined table; rig: what
        a refined rig tick observes with - {"table", "count", "xyc", "match", "fused", "views"}
        -> the entries the step's dict gains, in order: "pose", "refine", "world", "track", "window"."""
        out, fed, obs, prior = {}, None, None, None
        if self.model.host is not None:
            model = self.model(tab.device)
            fed = out["pose"] = dict(ops.object_pose(tab, n_obj, model, self.type_count, self.max_rmse), tab=tab)
            if self.refine is not None:
                if rig is not None:
                    obs, prior = self._bearings(rig)
                    start, resolved = fed, None
                    if self.resolver is not None:                # every assignment against all cameras' bearings: the pose and assignment of the least cost
                        resolved = ops.refine_assignments_views(obs, rig["views"], tab, fed, n_obj, model, self.type_count, self.resolver)
                        start = dict(fed, pose=resolved["pose"], assignment=resolved["assignment"])      # (the fit's where the resolver's status is not 0)
                    weighted = self.refine.confidence is not None
                    if weighted or resolved is None or self.refine.huber_px is not None:
                        out["refine"] = dict(_refine_static(self.refine_after, False, False, obs, prior, rig["views"], start, n_obj, model), obs=obs)
                        if weighted:
                            out["refine"]["prior"] = prior
                    else:                                        # neither a Huber loss nor priors: the resolver is the whole refinement
                        out["refine"] = dict(resolved, obs=obs)
                    if resolved is not None:
                        out["refine"].update(assignment=resolved["assignment"], hypothesis=resolved["hypothesis"], cost=resolved["cost"], resolve_status=resolved["status"])
                elif self.refine.resolve_assignment:
                    out["refine"] = ops.refine_assignments(tab, fed, n_obj, model, self.type_count, cam, self.refine)
                else:
                    out["refine"] = ops.refine_pose(tab, fed, n_obj, model, cam, self.refine)
                fed = dict(fed, pose=out["refine"]["pose"])          # what the world-frame change and the tracker take
        if frame_pose is not None:
            first = ops.change_frame(frame_pose, points=points.reshape((frame_pose.shape[0], -1, 4)), overflow=overflow)
            out["world"] = {"T": frame_pose, "points": first["points"].view(points.shape), "overflow": first["overflow"]}
            if fed is not None:
                second = ops.change_frame(frame_pose, points=tab, poses=fed["pose"], overflow=overflow)
                out["world"].update(tab=second["points"], pose=second["poses"])
                fed, overflow = dict(fed, tab=second["points"], pose=second["poses"]), first["overflow"]
        if self.tracker is not None:
            out["track"] = self.tracker.step(fed["tab"], fed["pose"], fed["status"], n_obj, model, overflow)
            if frame_pose is not None:
                out["track"]["track_pose_C"] = ops.change_frame(frame_pose, poses=out["track"]["track_pose"], inverse=True)["poses"]
        if isinstance(self.window, _RigWindow):
            if obs is None:                      # (no refinement: the one launch of the bearings is the window's)
                obs, prior = self._bearings(rig)
            weighted = {"prior": prior} if self.window.cfg.confidence is not None else {}
            resolved = out.get("refine", {}).get("assignment")       # the resolved assignment where resolve_views produced one
            out["window"] = self.window.step(obs, resolved if resolved is not None else out["pose"]["assignment"], out["pose"]["status"], out["track"], frame_pose,
                                             rig["views"], model, **weighted)
        elif self.window is not None:
            resolved = out.get("refine", {}).get("assignment")       # the refined assignment where resolve_assignment produced one
            out["window"] = self.window.step(tab, resolved if resolved is not None else out["pose"]["assignment"], out["pose"]["status"], out["track"], frame_pose, cam, model)
        return out

    def _bearings(self, rig):
        """The one launch that collects a rig tick's bearings -> (obs, prior): okp_rig_bearings_weighted where the refinement or the window
        weights them by the peaks' confidences, otherwise okp_rig_bearings and no priors."""
        if self.bearings_confidence is None:
            return ops.rig_bearings(rig["table"], rig["count"], rig["xyc"], rig["match"], rig["fused"], self.type_count), None
        return ops.rig_bearings_weighted(rig["table"], rig["count"], rig["xyc"], rig["match"], rig["fused"], self.type_count, self.bearings_confidence)

    def reset_tracks(self):
        if self.tracker is None:
            raise OkpError("this pipeline was built without track")
        self.tracker.reset()
        if self.window is not None:
            self.window.reset()

    def tracks(self, track, n, key, window=None):
        """Every live track of stream n of a step's "track" dict, `key` naming its pose in the table's frame, with the entries of the step's
        "window" dict where there is one - ONE device -> host copy."""
        return _track_list(_host_tracks(track, n, window), key, self.tracker.cfg.min_hits, 'T_WO_track', getattr(self.window, "cameras", None))

    def pin(self, step, static_out):
        """What a captured graph reads on every replay besides its inputs, kept on `step`: the object model - the very tensor the captured launch
        took, looked up by the device that launch ran on - and the tracker's state, which the graph also writes.  The warm-up passes and the
        capture advanced that state: it is reset."""
        if "pose" in static_out:
            step._model = self.model(static_out["pose"]["tab"].device)
        if "track" in static_out:
            step._track_state = [static_out["track"][k] for k in ("track_f", "track_i", "next_id")]
            if "window" in static_out:
                step._window_state = [static_out["window"][k] for k in ("win_obs", "win_views", "win_i", "prior", "win_age") if k in static_out["window"]]
            self.reset_tracks()


class _ObjectStagePipeline:
    """What both device pipelines show of their _ObjectStage (self._stage)."""
    world_frame = property(lambda self: self._stage.world_frame)
    max_rmse = property(lambda self: self._stage.max_rmse)
    refine = property(lambda self: self._stage.refine)
    window = property(lambda self: self._stage.window.cfg if self._stage.window is not None else None)
    _tracker = property(lambda self: self._stage.tracker)
    _model_host = property(lambda self: self._stage.model.host)
    _models = property(lambda self: self._stage.model.on)

    def _model(self, device):
        return self._stage.model(device)

    def reset_tracks(self):
        """Empty the tracker: its state tensors are zeroed in place on the current stream, so a captured step keeps working."""
        self._stage.reset_tracks()


def _frame_point(T, p, missing):
    """One host-lifted point [3] into the world frame by the formula of okp_change_frame (a row of T [3,4]: ((a + b) + c) + t)."""
    if missing:
        return None
    return np.array([((T[i, 0] * p[0] + T[i, 1] * p[1]) + T[i, 2] * p[2]) + T[i, 3] for i in range(3)])


class CapturedStep:
    """A captured hipGraph of BatchedKeypointPipeline.forward_device plus everything its kernel nodes point at.

    The graph holds raw device pointers to the plans' packed weights: this object keeps those plan objects alive (a
    load_state_dict() or .to() on the network clears the modules' plan caches, which would otherwise free them under
    the graph), and replay() refuses to run once the network's plans are no longer the captured ones - the graph would
    silently compute with the old weights."""

    def __init__(self, net, graph, static_in, static_out):
        self.net, self.graph, self.static_in, self.static_out = net, graph, static_in, static_out
        self.static_pose = None                  # world_frame: the static camera / rig pose tensor next to static_in
        self._pinned = _live_plans(net)
        # every module that caches plans, with its plan epoch at capture time: the per-replay staleness test is ~150 integer
        # compares (walking and comparing the plan objects themselves cost a replay ~0.4 ms of host time)
        self._epochs = [(m, m._plan_epoch) for m in net.modules() if hasattr(m, "_plan_epoch")]

    def stale(self):
        return any(m._plan_epoch != e for m, e in self._epochs)

    def replay(self, frames=None, camera_pose=None):
        if self.stale():
            raise OkpError("the network's weights / plans changed after capture(): capture the step again")
        if camera_pose is not None:
            if self.static_pose is None:
                raise OkpError("this step was captured without a pose (a pipeline built without world_frame): it has no pose input")
            self.static_pose.copy_(camera_pose)
        if frames is not None:
            self.static_in.copy_(frames)
        self.graph.replay()
        return self.static_out

    def __iter__(self):                      # graph, static_in, static_out = pipe.capture(x)
        return iter((self, self.static_in, self.static_out))


class CapturedTick(CapturedStep):
    """StereoStreamPipeline.capture_device: the whole device tick as one hipGraph.  heat_override, when captured, is the static input
    `static_heat` next to `static_in` (the frames)."""

    def __init__(self, net, graph, static_in, static_out, static_heat=None):
        super().__init__(net, graph, static_in, static_out)
        self.static_heat = static_heat

    def replay(self, frames=None, heat_override=None, rig_pose=None):
        if heat_override is not None:
            if self.static_heat is None:
                raise OkpError("this tick was captured without heat_override: it has no heat input")
            self.static_heat.copy_(heat_override)
        return super().replay(frames, camera_pose=rig_pose)


class BatchedKeypointPipeline(_ObjectStagePipeline):
    """Frames -> heat/depth/centre maps -> peaks -> per-peak 3D points for a whole batch, device-resident.

    forward_device(frames) returns device tensors
        heat [N,K,H,W], depth [N,K,H,W], centers [N,K-1,2,H,W],
        count [N,K] int32, xyc [N,K,cap,3] fp32 (x, y, confidence), points [N,K,cap,4] fp64 (X, Y, Z, confidence),
        overflow (0-d int32, non-zero: some map exceeded `capacity` peaks or `max_objects` centres - results are truncated)
    `points` is the fixed-capacity payload that is all-gathered across ranks (object_keypoints_amd.distributed).
    objects(...) groups one frame's peaks exactly as ObjectKeypointPipeline does, reusing the lifted points (surplus votes of a
    multi-instance type reduced by the device k-means of okp_group_objects).
    `frames` are whatever the network takes: fp32 NCHW crops, raw RGB uint8 [N,H,W,3] or, with the network's frame_format set, 4:2:0
    decoder output [N,3H/2,W] or 8-bit Bayer mosaics / mono8 frames [N,H,W] (KeypointNet.frame_format); eager and captured steps alike.

    Pose, refinement, world frame and tracking (all optional) end the device step, inside a captured step too: _ObjectStage describes the
    launches and the keys "pose", "refine", "world" and "track" they add to the step's dict, in the CAMERA frame of each frame.  Here:
    points_3d is the argument ObjectKeypointPipeline takes and ignores; the table is okp_object_points' [N,max_objects,S,4].  objects() adds to
    every object 'T_CO' (4 x 4 float64, model -> camera coordinates; None where the status is ops.POSE_FEW or ops.POSE_DEGENERATE), 'rmse',
    'ambiguity' (the runner-up assignment's rmse: close to 'rmse' = the data cannot tell the two apart) and 'pose_status'.
    refine: the fitted pose rests on key points lifted through the depth head, the weakest measurement of the step; okp_refine_pose minimises
    the reprojection error of the same key points' bearings with the depth as a weak prior.  'T_WO', 'T_CO_track', 'T_WO_track' and 'velocity'
    then come from the refined pose - the fitted one where the refinement's status is not 0.  objects() adds 'T_CO_refined' (None where 'T_CO'
    is), 'reprojection_rmse' and 'depth_rmse' ((before, after): map pixels, metres), 'pose_information' (6 x 6, the inverse covariance over
    (rotation, translation)) and 'refine_status', still in one device -> host copy.  With resolve_assignment=True the refinement also resolves
    which interchangeable key point is which (okp_refine_assignments): objects() further adds 'assignment_refined' (the model row of each table
    slot, -1 = empty), 'refine_hypothesis' (winner, runner-up; -1 = none) and 'refine_cost' (their final costs; NaN = none).
    world_frame=True, for a camera that moves: every step takes camera_pose, a float64 [N,12] tensor on the frames' device
    (ops.frame_poses(T_WC).to(device): camera coordinates -> world, one pose per stream and tick; an all-NaN row = the pose of that stream
    is missing in this tick); "world"["points"] is out["points"] in the world frame.  objects() adds 'p_W' next to 'p_C', 'T_WO' and
    'T_WO_track' ('T_CO_track' then comes from track_pose_C; all None where the pose is missing); tracks() lists both.  Without world_frame a
    camera_pose is refused.
    track: batch index = stream - frame n of every step is the next tick of stream n.  objects() adds 'track_id' (None where the object went
    to no track), 'T_CO_track' (the filtered pose), 'velocity', 'track_hits' and 'confirmed'; tracks(out, n) lists every live track of stream
    n, coasting ones included; reset_tracks() empties the tracker.  The step's own "overflow" word is unchanged.
    window = ops.WindowConfig(ticks, ...) (needs points_3d, track and world_frame=True; each is refused by name when missing): every track's
    world pose refined against the bearings of its last `ticks` measured ticks, each seen from that tick's camera pose - a multi-view
    triangulation that does not use the depth head, whose gain comes from the baseline the camera travels (a standing camera gains nothing in
    depth).  tracks() adds 'T_WO_window', 'T_CO_window' (None where 'window_status' is not 0 - a short window, a refused refinement -: fall back
    to the track pose), 'window_views', 'window_rmse', 'window_information' and 'window_status'; objects() adds 'T_CO_window' and
    'window_views' of the object's track - still one device -> host copy each.  Static objects only, and the error of camera_pose goes
    straight into the result.  StereoStreamPipeline has no `window` (2 P cameras x ticks exceed this kernel's 64 views): it takes rig_window.
    window = ops.WindowConfig(..., huber_px=h): the ring is refined under a Huber loss (okp_refine_pose_views_robust, one launch in place of
    okp_refine_pose_views_each), so one wrong peak in one tick no longer pulls the pose by its full residual; "window" gains "n_inlier" and
    "weight", "fit" has four values, and tracks() adds 'window_inliers', 'window_robust_rmse' and 'window_outliers', the (model row, ring
    column) entries that were down-weighted.  The weights do not use the peaks' confidences, and an outlier's pull is bounded, not removed.
    refine = ops.RefineConfig(..., huber_px=h) is refused here (ops.OkpNotOffered): one camera's five points leave no redundancy to vote with.
    """

    def __init__(self, net, keypoint_config, camera, prediction_size=(64, 64), capacity=DEFAULT_PEAK_CAPACITY,
                 max_objects=16, max_per_type=4, points_3d=None, max_rmse=None, track=None, world_frame=False, refine=None, window=None):
        self.net = net
        if isinstance(refine, ops.RefineConfig) and refine.huber_px is not None:
            raise OkpNotOffered("refine with huber_px: not offered for one camera (five points against six unknowns and a depth prior leave a Huber loss "
                                "nothing to vote with); window=ops.WindowConfig(..., huber_px=...) and a rig's refine take it")
        if isinstance(refine, ops.RefineConfig) and refine.confidence is not None:
            raise OkpNotOffered("refine with confidence: not offered for one camera (the single-camera refinement has no weighted form); "
                                "window=ops.WindowConfig(..., confidence=...) and StereoStreamPipeline's refine and rig_window take it")
        if isinstance(refine, ops.RefineConfig) and refine.resolve_views:
            raise OkpNotOffered("refine with resolve_views=True: not offered for one camera (it resolves a rig's key points against every camera's bearings: "
                                "StereoStreamPipeline's refine takes it); resolve_assignment=True resolves one camera's")
        self.max_objects = max_objects
        self.max_per_type = max_per_type
        self.config = keypoint_config
        self.capacity = capacity
        self.prediction_size = list(prediction_size)
        self.object_extraction = ObjectExtraction(keypoint_config, self.prediction_size)
        self.camera = camera
        self.cam = camera.okp()
        self.max_index = camera.image_size.astype(int) - 1
        cfg = keypoint_config['keypoint_config']
        self._stage = _ObjectStage(cfg, points_3d, max_rmse, track, max_objects, "max_objects", world_frame, refine, window)
        if points_3d is not None and max(cfg) > max_per_type:
            raise OkpError(f"a keypoint type has {max(cfg)} instances, above max_per_type = {max_per_type}")

    def tracks(self, out, n):
        """Every live track of stream n after the step `out`, coasting ones included, in slot order: a list of {'track_id', 'T_CO_track'
        (4 x 4, model -> camera coordinates, filtered), 'velocity' (m/s), 'hits', 'misses', 'age', 'confirmed' (hits >= min_hits), 'object'
        (the index into objects(out, n) that updated or founded it in this step, or None)} - ONE device -> host copy."""
        if "track" not in out:
            raise OkpError("tracks reads the step of a pipeline built with track")
        return self._stage.tracks(out["track"], n, 'T_CO_track', out.get("window"))

    def forward_device(self, frames, camera_pose=None):
        """Split-product configurations: the network's fp16-range flag is not read here (no host sync in the batch loop) but folded into
        `overflow` on the device (bit ops.RANGE_OVERFLOW), which objects() checks - except with on_overflow = "float32", where the pass has
        to be judged on the host before it can be re-run."""
        _check_frame_pose(camera_pose, self.world_frame, frames.shape[0], frames.device, "camera_pose", "one T_WC per frame")
        defer = getattr(self.net, "on_overflow", "raise") != "float32"
        heat, depth, centers = self.net.deployed(frames, check_range=not defer)
        return self.postprocess_device(heat, depth, centers, range_flag=self.net.range_flag(frames.device) if defer else None, camera_pose=camera_pose)

    def capture(self, frames, camera_pose=None):
        """Capture forward_device for this frame shape into a hipGraph (HIP stream capture through torch): the ~75
        launches of a step become one graph launch, which removes the host launch cost that dominates small
        batches (batch 8: 2.7 -> 2.2 ms per step).  Returns a CapturedStep; it also unpacks as
        (step, static_input, static_outputs): replay with step.replay(new_frames) or static_input.copy_(...); step.replay().
        With track: the graph steps the tracker's state of this batch size in place, the state eager steps of the same batch size use; the
        warm-up passes and the capture advance it, so capture() ends with reset_tracks() - every track alive before it is gone.
        With world_frame: camera_pose is a static input of the graph like the frames - step.replay(frames, camera_pose=...) copies a new one
        into step.static_pose before the replay."""
        _check_frame_pose(camera_pose, self.world_frame, frames.shape[0], frames.device, "camera_pose", "one T_WC per frame")
        static_in = frames.clone()
        static_pose = camera_pose.clone() if camera_pose is not None else None
        graph, static_out = _capture(lambda: self.forward_device(static_in, static_pose))
        step = CapturedStep(self.net, graph, static_in, static_out)
        step.static_pose = static_pose
        self._stage.pin(step, static_out)
        return step

    def postprocess_device(self, heat, depth, centers, range_flag=None, camera_pose=None):
        """Peaks, per-peak 3D points and the object grouping from (post-sigmoid) heat, depth and centre maps, all on
        the device: three small launches, nothing crosses PCIe."""
        camera_pose = _check_frame_pose(camera_pose, self.world_frame, heat.shape[0], heat.device, "camera_pose", "one T_WC per frame")
        count, yx, xyc = ops.peak_nms(heat, cap=self.capacity)
        points = ops.lift_peaks(self.cam, count, xyc, depth, int(self.max_index[0]), int(self.max_index[1]))
        out = {"heat": heat, "depth": depth, "centers": centers, "count": count, "yx": yx, "xyc": xyc, "points": points}
        out.update(ops.group_objects(count, xyc, centers, self.config['keypoint_config'], max_obj=self.max_objects,
                                     max_sel=self.max_per_type))
        # The reference has no capacity (pipeline.py:73 keeps every peak); the fixed-capacity tensors do.  `overflow` is a
        # device-side flag (no sync here): a map with more peaks than `capacity`, or more centre peaks than `max_objects`,
        # means `points` / the grouping are truncated - callers check it (objects() raises, bench.py asserts).
        out["overflow"] = ops.capacity_overflow(count, self.capacity, self.max_objects, range_flag=range_flag)
        tab = ops.object_points(self.cam, out, self.config['keypoint_config'], int(self.max_index[0]), int(self.max_index[1])) if self._model_host is not None else None
        out.update(self._stage.run(tab, out["n_obj"], points, out["overflow"], camera_pose, self.cam))
        return out

    def objects(self, out, n):
        """Frame n of a forward_device() result as the reference's list of object dicts
        ({'p_centers', 'keypoints', 'p_C'}, pipeline.py:190-200), assembled from the device-side grouping.  A multi-instance type that
        received more votes than it has instances comes back as the cluster centres of the device k-means reduction (`reduced`,
        okp_group_objects; the reference: an unseeded sklearn KMeans, pipeline.py:143-148), lifted to 3D by one okp_unproject_depth
        launch for the frame - no scikit-learn, no host clustering."""
        cfg = self.config['keypoint_config']
        count = out["count"][n].cpu().numpy()
        xyc = out["xyc"][n].cpu().numpy()
        pts3 = out["points"][n].cpu().numpy()
        n_obj = int(out["n_obj"][n])
        votes = out["n_votes"][n].cpu().numpy()
        if int(count.max(initial=0)) > self.capacity or int(count[0]) > self.max_objects:
            raise OkpError("peak / object capacity exceeded; raise `capacity` / `max_objects`")
        if int(out["overflow"]) & ops.RANGE_OVERFLOW:
            raise OkpError("an activation of the split-product network left the fp16 range in this batch: its maps are not fp32-grade "
                           "(load the network with on_overflow='float32', or run it in torch.float32; a guarded float16 network sets the same bit)")
        if any(c > self.max_per_type for c in cfg):
            raise OkpError(f"a keypoint type has {max(cfg)} instances, above max_per_type = {self.max_per_type}")
        sel = out["sel"][n].cpu().numpy()
        assign = out["assign"][n].cpu().numpy()
        pred = out["pred"][n].cpu().numpy()
        surplus = [(o, i) for o in range(n_obj) for i in range(len(cfg)) if cfg[i] > 1 and votes[o, i] > cfg[i]]
        centres, lifted = {}, {}
        if surplus:
            reduced = out["reduced"][n].cpu().numpy()
            for o, i in surplus:
                centres[(o, i)] = reduced[o, i, :cfg[i]].copy()
            xy = np.concatenate([centres[key] for key in surplus])
            ids = np.concatenate([np.full(cfg[i], i + 1, dtype=np.int32) for _, i in surplus])
            dev = out["depth"].device
            world = ops.unproject_depth(self.cam, torch.from_numpy(xy).to(dev), torch.from_numpy(ids).to(dev), out["depth"][n],
                                        int(self.max_index[0]), int(self.max_index[1])).cpu().numpy()
            at = 0
            for o, i in surplus:
                lifted[(o, i)] = world[at:at + cfg[i]]
                at += cfg[i]
        poses = _host_poses(out["pose"], n, out.get("refine")) if "pose" in out else None
        tracked = _host_tracks(out["track"], n, out.get("window")) if "track" in out else None
        in_world = "world" in out
        if in_world:                                               # 'p_W' parallel to 'p_C': the device's world points, row for row
            T_WC = out["world"]["T"][n].cpu().numpy().reshape(3, 4)
            missing = not np.isfinite(T_WC).all()
            pts3_w = out["world"]["points"][n].cpu().numpy()
            poses_w = _host_poses(dict(out["pose"], pose=out["world"]["pose"]), n) if poses is not None else None
        objects = []
        for o in range(n_obj):
            keypoints = [xyc[0, o, :2].copy()[None]]
            world = [pts3[0, o, :3][None]]
            p_W = [None if missing else pts3_w[0, o, :3][None]] if in_world else None
            for i in range(len(cfg)):
                if (o, i) in centres:
                    keypoints.append(centres[(o, i)])
                    world.append(lifted[(o, i)])
                    if in_world:                                   # lifted on the host just above: transformed here, by the same formula
                        p_W.append(None if missing else np.stack([_frame_point(T_WC, p, False) for p in lifted[(o, i)]]))
                    continue
                idx = [int(j) for j in sel[o, i] if j >= 0][:max(cfg[i], 1)]
                if idx:
                    keypoints.append(xyc[i + 1, idx, :2].copy())
                    world.append(pts3[i + 1, idx, :3])
                    if in_world:
                        p_W.append(None if missing else pts3_w[i + 1, idx, :3])
                else:
                    keypoints.append(np.array([]))
                    world.append(None)
                    if in_world:
                        p_W.append(None)
            p_centers = [pred[k, j] for k in range(1, count.shape[0]) for j in range(int(count[k])) if assign[k, j] == o]
            objects.append({'p_centers': p_centers, 'keypoints': keypoints, 'p_C': world})
            if in_world:
                objects[-1]['p_W'] = p_W
            if poses is not None:
                objects[-1].update(_pose_entries(poses, o, 'T_CO'))
                if "refine" in poses:
                    objects[-1].update(_refine_entries(poses, o, objects[-1]['T_CO']))
                if in_world:
                    objects[-1]['T_WO'] = None if missing else _pose_entries(poses_w, o, 'T_WO')['T_WO']
            if tracked is not None:
                objects[-1].update(_track_entries(tracked, o, 'T_CO_track', self._tracker.cfg.min_hits, 'T_WO_track'))
        return objects

    def objects_reference(self, out, n):
        """The same frame through the host ObjectExtraction (the reference's loop with scikit-learn's k-means): for comparisons only -
        objects() never comes here."""
        return self._objects_host(out, n, out["count"][n].cpu().numpy(), out["xyc"][n].cpu().numpy(), out["points"][n].cpu().numpy())

    def _objects_host(self, out, n, count, xyc, pts3):
        centers = out["centers"][n].cpu().numpy()
        keypoints = [[xyc[k, j, :2].copy() for j in range(int(count[k]))] for k in range(count.shape[0])]
        confidence = [[xyc[k, j, 2] for j in range(int(count[k]))] for k in range(count.shape[0])]
        lifted = {}
        for k in range(count.shape[0]):
            for j in range(int(count[k])):
                lifted[(k, xyc[k, j, 0].tobytes(), xyc[k, j, 1].tobytes())] = pts3[k, j, :3]
        detected = self.object_extraction(keypoints, confidence, centers)
        d2p = None
        objects = []
        for obj in detected:
            groups = [obj['center'][None]] + obj['heatmap_points']
            world = []
            for k, pts in enumerate(groups):
                if pts.shape[0] == 0:
                    world.append(None)
                    continue
                rows = []
                for p in pts:
                    key = (k, np.float32(p[0]).tobytes(), np.float32(p[1]).tobytes())
                    if key in lifted:
                        rows.append(lifted[key])
                    else:                      # k-means centre: not a detected peak, lift it on demand
                        if d2p is None:
                            d2p = DetectionToPoint(); d2p.reset(self.camera)
                        rows.append(d2p(np.asarray(p, dtype=np.float32)[None], out["depth"][n, k].cpu().numpy())[0])
                world.append(np.stack(rows))
            objects.append({'p_centers': obj['p_centers'], 'keypoints': groups, 'p_C': world})
        return objects


class SceneScorer:
    """Score labelled frames on the device: net.forward (raw logits of both stacks) plus the fused KeypointLoss against targets rendered
    from the labels in registers (ops.keypoint_loss).  Nothing synchronises with the host, so a step can be captured.

    score(frames, labels) -> {"loss" [], "heat" [S], "depth" [S], "center" [S] (the reference's 4-tuple, perception/loss.py:48, fp64),
    "terms" [N,S,3] fp64 per-frame sums, "mask_count" [N,K] int32, "range_overflow" 0-d int32 (non-zero: a guarded configuration left
    the fp16 range in this pass - the score is not to be trusted; always 0 for float32 / bfloat16)}.  labels: SceneTargets.labels.
    frames: whatever net.forward takes, 4:2:0, Bayer and mono8 frames of a network with a frame_format (KeypointNet.frame_format) included."""

    def __init__(self, net, keypoint_config, depth_weight=10.0, center_weight=1.0):
        from .loss import KeypointLoss
        cfg = keypoint_config['keypoint_config'] if isinstance(keypoint_config, dict) else keypoint_config
        self.net = net
        self.loss = KeypointLoss(cfg, depth_weight=depth_weight, center_weight=center_weight)

    def score(self, frames, labels):
        heat, depth, centers = self.net.forward(frames, check_range=False)      # the flag is folded in below, not read here
        self.loss.from_labels(list(heat), list(depth), list(centers), labels)
        r = self.loss.last
        flag = self.net.range_flag(frames.device)
        overflow = (flag != 0).to(torch.int32).reshape(()) if flag is not None else torch.zeros((), dtype=torch.int32, device=frames.device)
        return {"loss": r["loss"], "heat": r["heat"], "depth": r["depth"], "center": r["center"], "terms": r["terms"],
                "mask_count": r["mask_count"], "range_overflow": overflow}

    def capture(self, frames, labels):
        """score() for this frame and label shape as one hipGraph -> CapturedStep (static_in: the frames; static_labels: the labels, to be
        overwritten in place with .copy_()); replay(frames) returns the static result dict."""
        static_in = frames.clone()
        static_labels = {"points": labels["points"].clone(), "n_obj": labels["n_obj"].clone()}
        graph, static_out = _capture(lambda: self.score(static_in, static_labels))
        step = CapturedStep(self.net, graph, static_in, static_out)
        step.static_labels = static_labels
        return step

    def compare(self, frames, labels, configurations):
        """{configuration name: score} of several compute configurations on the same weights, frames and labels (set_compute_dtype);
        the network is left in the configuration it had."""
        mine = (self.net.compute_dtype, self.net.mfma_split, self.net.mixed)
        out = {}
        try:
            for c in configurations:
                self.net.set_compute_dtype(c)
                r = self.score(frames, labels)
                out[self.net.configuration()] = {k: v.clone() for k, v in r.items()}
        finally:
            self.net.compute_dtype, self.net.mfma_split, self.net.mixed = mine
        return out


class HostFrameFeed:
    """Host -> HBM upload of camera frames on a COPY stream, double-buffered, so that the frames of tick t + 1 cross PCIe while tick t is
    computed (the reference feeds its model from a DataLoader on the host, one frame per call: scripts/eval_model.py:274-293; raw frames
    are 1280 x 720 uint8, perception/datasets/video.py:83-100).  Frames come as a pinned host tensor of the shape / dtype given at
    construction (pin_memory() once, reuse it: the copy is only asynchronous from pinned memory): RGB [n, H, W, 3], 4:2:0 decoder output
    [n, 3H/2, W], or a camera's 8-bit Bayer mosaic / mono8 frames [n, H, W] - a third of the RGB bytes - for a network whose
    frame_format names them.

        feed = HostFrameFeed(host.shape, host.dtype)
        slot = feed.submit(host)                 # async H2D on the copy stream into the next free device buffer
        frames = feed.acquire(slot)              # the compute stream waits for that copy (device-side wait, no host sync)
        ...                                      # launches that read `frames`
        feed.release(slot)                       # the buffer may be overwritten once the work enqueued so far has run

    The ordering of the copy stream against the compute stream (ready / done, release before overwrite, the buffers' first use) is
    checked by tests/test_gpu_stream_order.py.
    """

    def __init__(self, shape, dtype=torch.uint8, device=None, depth=2):
        self.device = device or _device()
        self.buffers = [torch.empty(tuple(shape), dtype=dtype, device=self.device) for _ in range(depth)]
        self.copy_stream = torch.cuda.Stream(device=self.device)
        # The buffers come from the CURRENT stream's pool: the allocator may hand out a block whose previous owner's kernels are still in
        # that stream's queue, safe for work enqueued on that stream only.  Their first writer is the copy stream, which therefore starts
        # behind the current stream, once (found by the stream-order audit: the first upload into each slot was unordered against it).
        self.copy_stream.wait_stream(torch.cuda.current_stream(self.device))
        self.ready = [torch.cuda.Event() for _ in range(depth)]
        self.done = [None] * depth
        self.next = 0

    def submit(self, host_frames):
        if host_frames.is_cuda or tuple(host_frames.shape) != tuple(self.buffers[0].shape) or host_frames.dtype != self.buffers[0].dtype:
            raise OkpError("HostFrameFeed.submit: a host tensor of the shape / dtype the feed was built for")
        slot = self.next
        self.next = (self.next + 1) % len(self.buffers)
        with torch.cuda.stream(self.copy_stream):
            if self.done[slot] is not None:
                self.copy_stream.wait_event(self.done[slot])          # the buffer's previous tick has been consumed
            self.buffers[slot].copy_(host_frames, non_blocking=True)
            self.ready[slot].record(self.copy_stream)
        return slot

    def acquire(self, slot):
        torch.cuda.current_stream().wait_event(self.ready[slot])
        return self.buffers[slot]

    def release(self, slot):
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream())
        self.done[slot] = ev


class StereoStreamPipeline(_ObjectStagePipeline):
    """BASELINE configs[4] / SURVEY 8(d) config 5: a rig of stereo cameras streamed frame-synchronously.  One TICK takes the 2P
    frames of P stereo pairs (left frame of pair p at index 2p, right at 2p + 1) through the network as ONE batch, finds the heat-map
    peaks of all 2P x K maps in one launch, matches left and right peaks per pair and key-point type (AssociationComponent's
    epipolar assignment, test/test_pipeline.py:208-261), and triangulates every matched pair of the tick in ONE
    okp_triangulate_dlt launch (StereoCamera.triangulate, camera_utils.py:92-110).  The reference's harness processes one frame
    of one camera per call at a 30 Hz cap (scripts/eval_model.py:274-293).  Geometry is fp32 / fp64 whatever the network's
    compute dtype.

    tick(frames) -> list over pairs of {type k: (n_k, 3) float64 points in the left camera frame}, plus timing-free device work:
    three small device -> host copies per tick (peaks, undistorted peaks, 3D points).
    `frames`: fp32 NCHW crops [2P, 3, 511, 511] in HBM, or raw camera frames uint8 [2P, H, W, 3] (resized, cropped and normalised on the
    device, okp_preprocess_u8), or - for a network whose frame_format names them - 4:2:0 decoder output [2P, 3H/2, W] or the cameras' 8-bit
    Bayer mosaics / mono8 frames [2P, H, W] (okp_preprocess_yuv420, okp_preprocess_raw8); tick, tick_device, capture_device and stream take
    all of them.  Host-fed operation: stream(host_ticks) uploads the raw frames of tick t + 1 on a copy stream while tick t
    is computed (HostFrameFeed) and yields the same results, bit for bit, as tick() on resident frames.

    stereo_camera: one StereoCamera, used for every pair of a tick of any size, or a RIG - a sequence of P StereoCameras, each pair
    calibrated on its own (pair p = frames 2p and 2p + 1, its points in its own left camera frame); a rig's ticks hold exactly its 2P
    frames (tick_device / tick_sharded: a shard of them, first_pair = the shard's first pair).  The calibration is validated and packed
    at construction (ops.stereo_rig: a bad one fails here, before any device work) and uploaded to the frames' device on the first
    device tick; the device copy lives as long as the pipeline, since captured ticks read it on every replay.

    Fusion (optional): rig_poses = one 4 x 4 transform T_BL per pair (the pair's left-camera coordinates -> rig coordinates) with
    merge_radius and object_radius in metres - the three are given together or not at all.  A rig needs one pose per StereoCamera; with
    a single StereoCamera the number of poses fixes the number of pairs of a tick.  The device ticks (tick_device, capture_device - inside
    the graph -, tick_sharded - after the gather, on every rank) then end with okp_rig_fuse and carry the key "fused" (ops.rig_fuse's dict:
    one list of clusters per type in the rig frame, grouped into objects), and their "overflow" word carries ops.FUSE_OVERFLOW;
    rig_objects(out) reads it.  fuse_capacity: fused clusters kept per type (default: the kernel's limit, ops.RIG_MAX_FUSED).  Poses and
    radii are validated at construction (ops.rig_poses).  tick(), the host tick, is unchanged and does not fuse.

    Pose, world frame and tracking (all optional, all need the fusion - the fused tick is what has ONE frame) end the fused device ticks, inside
    the captured graph and after the gather on every rank with no further collective (every rank keeps the same tracker): _ObjectStage describes
    the launches and the keys "pose", "world" and "track" they add to the tick's dict, for ONE stream in the RIG frame.  Here: the table is
    okp_rig_object_points' [1,fuse_capacity,S,4]; "world"["points"] is the fused clusters [K,cap_f,4] in the world frame.
    refine = ops.RefineConfig(...) (needs points_3d): the fitted pose rests on fused points, means of two-view triangulations with the depth
    noise of a short baseline; the peaks they came from do not carry it.  okp_rig_bearings collects them as one bearing per object, table slot
    and camera, and okp_refine_pose_views minimises their reprojection error in all 2P cameras at once, from the fitted pose (sigma_px, iters
    and damping of the config; no depth term, so sigma_z is not used; resolve_assignment=True is refused with ops.OkpNotOffered, an OkpError that is also the TypeError
    the call raised while the rig took no `refine`: not offered for a rig).  The tick's
    dict gains "refine" - ops.refine_pose_views' dict plus "obs" -, "pose" keeps its bits, and the world-frame change and the tracker take the
    refined pose (the fitted one where the refinement's status is not 0).  The views table (ops.rig_views) is built at construction and
    uploaded once per device, like the calibration and the poses.  rig_objects(out) then adds 'T_BO_refined' (None where 'T_BO' is),
    'reprojection_rmse' (before, after; map pixels), 'refine_observations', 'pose_information' (6 x 6) and 'refine_status'.  Under an
    initialised process group tick_sharded refuses a refinement: the other ranks' peaks are not in the gathered payload.
    refine = ops.RefineConfig(..., huber_px=h): the second launch is okp_refine_pose_views_robust, the same refinement under a Huber loss, so a
    false peak or a wrong match among the 10 P bearings of an object no longer pulls the pose by its full residual (bounded, not removed; the
    weights do not use the peaks' confidences).  "refine" gains "n_inlier" and "weight", its "fit" has four values, and rig_objects(out) adds
    'refine_inliers', 'robust_rmse' (the rmse of the robust cost before, after) and 'refine_outliers', the (table slot, camera) entries that
    were down-weighted; 'reprojection_rmse' stays the plain one.  The tracker and the world frame take the refined pose as before.
    rig_objects(out) adds 'T_BO' (4 x 4, model -> rig coordinates, or None), 'rmse', 'ambiguity' and 'pose_status' to every object; with track
    'track_id', 'T_BO_track', 'velocity', 'track_hits' and 'confirmed'; with world_frame 'T_WO' and 'T_WO_track' next to them.  rig_tracks(out)
    lists the live tracks, reset_tracks() empties the tracker.
    rig_window = ops.WindowConfig(ticks, ...) (needs points_3d, track and world_frame=True - hence the fusion; each is refused by name when
    missing; 2 x pairs x ticks above ops.REFINE_WIDE_MAX_VIEWS is refused with the numbers; it does not need refine): every track's world pose
    refined against the last `ticks` measured ticks of ALL 2 P cameras.  The fused device tick ends, after the tracker, with
    okp_window_push_views (a ring column = one tick: the bearings of okp_rig_bearings by model row - the refinement's table where there is one,
    otherwise launched for the window alone - and every camera's camera-from-world view, its row of the views table composed with rig_pose),
    okp_refine_pose_views_wide (one workgroup of up to eight waves per track, an identity assignment, from the track pose) and one
    okp_change_frame (inverse) -> "window": the keys of the camera window with "pose_B" where that has "pose_C", plus "tick_obs"; under
    huber_px also "n_inlier", "weight" and a four-value "fit".  rig_tracks(out) adds 'T_WO_window', 'T_BO_window' (None where 'window_status' is
    not 0: fall back to the track pose), 'window_views' (filled TICKS), 'window_rmse', 'window_information' and 'window_status' - under huber_px
    also 'window_inliers', 'window_robust_rmse' and 'window_outliers' as (model row, ring column, camera) -, rig_objects(out) 'T_BO_window' and
    'window_views' of the object's track; one device -> host copy each as before.  capture_device pins the state, reset_tracks() empties it.
    Under an initialised process group tick_sharded refuses rig_window as it refuses refine.  Static objects only; the error of rig_pose and of
    the calibration goes straight into the result; uniform weights unless huber_px.
    world_frame=True, for a rig that moves: tick_device, capture_device / CapturedTick.replay and tick_sharded take rig_pose, a float64 [1,12]
    tensor on the frames' device (ops.frame_poses(T_WB).to(device): rig coordinates -> world; the same on every rank of a sharded tick; all NaN
    = missing in this tick).  Without world_frame a rig_pose is refused."""

    def __init__(self, net, stereo_camera, keypoint_config, capacity=16, max_distance=3.0, rig_poses=None, merge_radius=None, object_radius=None,
                 fuse_capacity=None, points_3d=None, max_rmse=None, track=None, world_frame=False, refine=None, rig_window=None):
        self.net = net
        if isinstance(refine, ops.RefineConfig) and refine.resolve_assignment:
            raise OkpNotOffered("refine with resolve_assignment=True: not offered for a rig (its refinement keeps the assignment of the fit; "
                                "resolve_views=True resolves a rig's key points against every camera's bearings)")
        if world_frame and rig_poses is None:
            raise OkpError("world_frame without rig_poses, merge_radius and object_radius: the fused tick is what has one frame to pose")
        self.rig = None if hasattr(stereo_camera, "left_camera") else list(stereo_camera)       # one StereoCamera, or a sequence of them
        self.stereo_cameras = self.rig if self.rig is not None else [stereo_camera]
        self._table = _PerDevice(ops.stereo_rig(self.stereo_cameras))  # (refuses an empty rig)
        self.stereo = self.stereo_cameras[0]
        self.config = [1] + list(keypoint_config["keypoint_config"])
        self.capacity = capacity
        self.assoc = AssociationComponent(max_distance=max_distance)
        self.assoc.reset(self.stereo)
        # fisheye model, as the reference; one (left, right) pair per calibration
        self._cams = [(ops.make_camera(st.left_camera.K, st.left_camera.D), ops.make_camera(st.right_camera.K, st.right_camera.D))
                      for st in self.stereo_cameras]
        self.cam_l, self.cam_r = self._cams[0]
        self._graph = None
        given = [n for n, v in (("rig_poses", rig_poses), ("merge_radius", merge_radius), ("object_radius", object_radius)) if v is not None]
        if given and len(given) != 3:
            raise OkpError(f"fusion takes rig_poses, merge_radius and object_radius together: only {', '.join(given)} given")
        if not given and fuse_capacity is not None:
            raise OkpError("fuse_capacity without rig_poses, merge_radius and object_radius")
        self._poses = _PerDevice(ops.rig_poses(rig_poses) if given else None)          # (.host None: fusion off)
        if given:
            self.n_fused_pairs = int(self._poses_host.shape[0])
            if self.rig is not None and self.n_fused_pairs != len(self.rig):
                raise OkpError(f"{self.n_fused_pairs} rig poses for a rig of {len(self.rig)} stereo pairs: one pose per pair")
            self.merge_radius, self.object_radius = ops.check_fuse_radii(merge_radius, object_radius)
            self.fuse_capacity = ops.RIG_MAX_FUSED if fuse_capacity is None else int(fuse_capacity)
            if not 1 <= self.fuse_capacity <= ops.RIG_MAX_FUSED:
                raise OkpError(f"fuse_capacity = {fuse_capacity} outside [1, {ops.RIG_MAX_FUSED}]")
            if len(self.config) > ops.RIG_MAX_TYPES or self.n_fused_pairs * self.capacity > ops.RIG_MAX_ROWS:
                raise OkpError(f"fusion holds at most {ops.RIG_MAX_TYPES} key-point types and {ops.RIG_MAX_ROWS} rows (pairs x capacity) per type: "
                               f"{len(self.config)} types, {self.n_fused_pairs} x {self.capacity} rows asked for")
        if points_3d is not None and not given:
            raise OkpError("points_3d without rig_poses, merge_radius and object_radius: the pose is fitted to the fused objects of the rig")
        cameras = 2 * self.n_fused_pairs if given else 2 * len(self.stereo_cameras)
        if isinstance(rig_window, ops.WindowConfig) and cameras * rig_window.ticks > ops.REFINE_WIDE_MAX_VIEWS:
            raise OkpError(f"rig_window: 2 x {cameras // 2} pairs x {rig_window.ticks} ticks = {cameras * rig_window.ticks} views exceed the "
                           f"{ops.REFINE_WIDE_MAX_VIEWS} of okp_refine_pose_views_wide")
        self._stage = _ObjectStage(self.config[1:], points_3d, max_rmse, track, self.fuse_capacity if given else 0, "fuse_capacity", world_frame, refine,
                                   window=rig_window, rig_cameras=cameras if rig_window is not None else 0)
        on = refine is not None or rig_window is not None       # (_ObjectStage refused either without points_3d, and points_3d without the fusion)
        self._views = _PerDevice(ops.rig_views(stereo_camera if self.rig is None else self.rig, rig_poses) if on else None)      # (.host None: refinement off)

    _table_host = property(lambda self: self._table.host)
    window = None                                   # (the camera pipeline's keyword; a rig's is rig_window)
    rig_window = property(lambda self: self._stage.window.cfg if self._stage.window is not None else None)
    _poses_host = property(lambda self: self._poses.host)

    def _finish(self, out, rig_pose):
        """What follows okp_rig_fuse in a fused device tick: the table of the fused objects (with a model), then the object stage."""
        fused = out["fused"]
        tab = ops.rig_object_points(fused, self.config[1:]) if self._model_host is not None else None
        rig = None
        if self._views.host is not None:        # what the refinement and the window observe with: this tick's own peaks (the whole rig's)
            dev = fused["fused"].device
            rig = {"table": self._table(dev), "views": self._views(dev), "fused": fused, **{k: out[k] for k in ("count", "xyc", "match")}}
        out.update(self._stage.run(tab, fused["n_obj"], fused["fused"], fused["overflow"], rig_pose, rig=rig))

    def rig_tracks(self, out):
        """Every live track after the fused tick `out`, coasting ones included, in slot order: a list of {'track_id', 'T_BO_track' (4 x 4,
        model -> rig coordinates, filtered), 'velocity' (m/s), 'hits', 'misses', 'age', 'confirmed', 'object' (the index into
        rig_objects(out), or None)}, with rig_window also 'T_WO_window', 'T_BO_window', 'window_views', 'window_rmse', 'window_information' and
        'window_status' (see the class) - ONE device -> host copy."""
        if not isinstance(out, dict) or "track" not in out:
            raise OkpError("rig_tracks reads the fused device tick of a pipeline built with track")
        return self._stage.tracks(out["track"], 0, 'T_BO_track', out.get("window"))

    def _check_fused_tick(self, n_pairs, first_pair=0):
        """A fused tick holds every pair of the rig: the clusters are formed across all of them."""
        if self._poses_host is not None and (n_pairs != self.n_fused_pairs or first_pair != 0):
            raise OkpError(f"a fused tick holds the {2 * self.n_fused_pairs} frames of all {self.n_fused_pairs} posed stereo pairs, from pair 0 on "
                           f"({2 * n_pairs} frames from pair {first_pair} on given; a shard of the rig goes through tick_sharded)")

    def _fuse(self, points, overflow):
        return ops.rig_fuse(points, self._poses(points.device), self.config[1:], self.merge_radius, self.object_radius, self.fuse_capacity, overflow=overflow)

    def _check_rig_frames(self, frames, first_pair=0):
        """A rig's tick holds 2 frames for each of its pairs first_pair .. first_pair + P - 1 (a single calibration: any P)."""
        if frames.shape[0] % 2:
            raise OkpError("a tick holds the left and right frame of every stereo pair: an even number of frames")
        first_pair = int(first_pair)
        if self.rig is not None and (first_pair < 0 or first_pair + frames.shape[0] // 2 > len(self.rig)):
            raise OkpError(f"{frames.shape[0]} frames from pair {first_pair} on: the rig has {len(self.rig)} stereo pairs "
                           f"(pairs {first_pair} .. {first_pair + frames.shape[0] // 2 - 1} asked for)")
        return first_pair

    def capture(self, frames):
        """Capture the network pass of a tick for this frame shape into a hipGraph (one graph launch instead of ~66)."""
        static_in = frames.clone()
        graph, static_out = _capture(lambda: self.net.deployed(static_in))
        self._graph = CapturedStep(self.net, graph, static_in, static_out)
        return self._graph

    def stream(self, host_ticks, heat_override=None, use_graph=False):
        """host_ticks: an iterable of pinned host tensors, one per tick (all of one shape / dtype: raw uint8 [2P, H, W, 3] frames, fp32
        [2P, 3, 511, 511] crops or, with the network's frame_format set, 4:2:0 [2P, 3H/2, W] or Bayer / mono8 [2P, H, W] frames).  Generator of tick() results; the upload of the next tick overlaps the current one."""
        it = iter(host_ticks)
        try:
            first = next(it)
        except StopIteration:
            return
        feed = HostFrameFeed(first.shape, first.dtype, device=next(self.net.parameters()).device)
        slot = feed.submit(first)
        while slot is not None:
            frames = feed.acquire(slot)
            upcoming = next(it, None)
            nxt = feed.submit(upcoming) if upcoming is not None else None      # crosses PCIe under this tick's kernels
            result = self.tick(frames, heat_override=heat_override, use_graph=use_graph)
            feed.release(slot)
            yield result
            slot = nxt

    def tick(self, frames, heat_override=None, use_graph=False):
        self._check_rig_frames(frames)
        if self.rig is not None and frames.shape[0] != 2 * len(self.rig):
            raise OkpError(f"{frames.shape[0]} frames for a rig of {len(self.rig)} stereo pairs: a tick holds {2 * len(self.rig)}")
        with torch.no_grad():
            if use_graph:
                if self._graph is None:
                    raise OkpError("capture() the tick first")
                heat, depth, centers = self._graph.replay(frames)
            else:
                heat, depth, centers = self.net.deployed(frames)
            if heat_override is not None:
                heat = heat_override
            count, _, xyc = ops.peak_nms(heat, cap=self.capacity)
            count_h = count.cpu().numpy()                                   # D2H 1 (tiny)
            if int(count_h.max(initial=0)) > self.capacity:
                raise OkpError("peak capacity exceeded in a tick; raise `capacity`")
            n_pairs, K = frames.shape[0] // 2, heat.shape[1]
            # undistort every left and every right peak of the tick, two launches per calibration (the cost of the assignment needs them)
            xy = xyc[..., :2].reshape(n_pairs, 2, K, self.capacity, 2)
            groups = [slice(None)] if self.rig is None else [slice(p, p + 1) for p in range(n_pairs)]      # the pairs of calibration c
            und = []
            for c, pairs in enumerate(groups):
                cam_l, cam_r = self._cams[c]
                ul = ops.camera_undistort(cam_l, xy[pairs, 0].reshape(-1, 2))
                ur = ops.camera_undistort(cam_r, xy[pairs, 1].reshape(-1, 2))
                und.append(torch.stack([ul, ur]).reshape(2, -1, K, self.capacity, 2))
            und = (und[0] if len(und) == 1 else torch.cat(und, dim=1)).cpu().numpy()                # D2H 2
            raw = xy.cpu().numpy()
        left_sel, right_sel, owner = [[] for _ in groups], [[] for _ in groups], [[] for _ in groups]
        from scipy.optimize import linear_sum_assignment
        for p in range(n_pairs):
            c = 0 if self.rig is None else p
            F = self.stereo_cameras[c].F
            for k in range(K):
                cl, cr = int(count_h[2 * p, k]), int(count_h[2 * p + 1, k])
                if cl == 0 or cr == 0:
                    continue
                hl = np.concatenate([und[0, p, k, :cl], np.ones((cl, 1))], axis=1)
                hr = np.concatenate([und[1, p, k, :cr], np.ones((cr, 1))], axis=1)
                lines_r, lines_l = hl @ F.T, hr @ F
                num = np.abs(lines_r @ hr.T)
                cost = 0.5 * (num / np.maximum(np.linalg.norm(lines_r[:, :2], axis=1), 1e-300)[:, None]
                              + num / np.maximum(np.linalg.norm(lines_l[:, :2], axis=1), 1e-300)[None, :])
                rows, cols = linear_sum_assignment(np.where(cost <= self.assoc.max_distance, cost, 1e6))
                keep = cost[rows, cols] <= self.assoc.max_distance
                for i, j in zip(rows[keep], cols[keep]):
                    left_sel[c].append(raw[p, 0, k, i]); right_sel[c].append(raw[p, 1, k, j]); owner[c].append((p, k))
        result = [{k: np.zeros((0, 3)) for k in range(K)} for _ in range(n_pairs)]
        dev = frames.device
        for c in range(len(groups)):                                   # one triangulation launch per calibration
            if not left_sel[c]:
                continue
            st = self.stereo_cameras[c]
            pts = ops.triangulate_dlt(*self._cams[c], st.T_RL, torch.from_numpy(np.stack(left_sel[c])).to(dev),
                                      torch.from_numpy(np.stack(right_sel[c])).to(dev), F=st.F).cpu().numpy()          # D2H 3
            for (p, k), X in zip(owner[c], pts):
                result[p][k] = np.concatenate([result[p][k], X[None]])
        return result

    # ---- the device-resident tick (no host wait between the frames and the 3D points) ------------------------------------------------
    def _check_device_tick(self, frames, first_pair=0):
        if self.capacity > ops.STEREO_MAX_CAPACITY:
            raise OkpError(f"capacity = {self.capacity}: the device association holds at most {ops.STEREO_MAX_CAPACITY} peaks per map")
        return self._check_rig_frames(frames, first_pair)

    def tick_device(self, frames, heat_override=None, first_pair=0, _fuse=True, rig_pose=None):
        """The whole tick on the device, with no host wait anywhere: network -> peak-NMS -> left/right association (okp_stereo_match) ->
        triangulation of every matched slot (okp_stereo_triangulate).  Same frames as tick().  Returns a dict of device tensors
            heat, depth [2P,K,H,W], count [2P,K] int32, xyc [2P,K,cap,3] fp32, match [P,K,cap] int32,
            points [P,K,cap,4] fp64 (X, Y, Z, left confidence; NaN rows = unmatched slots), overflow (0-d int32: bit 0 some map of the tick
            holds more than `capacity` peaks, bit 1 ops.RANGE_OVERFLOW the split-product network's fp16-range flag)
        results(out) turns it into tick()'s return value.  `points` is the fixed-capacity payload all_gather_keypoints carries
        (tick_sharded).  first_pair: the rig-wide index of the frames' first pair (a rig: pair p of the frames is calibrated as the
        rig's pair first_pair + p; a single calibration: no effect).  With rig_poses (see the class) the tick ends with okp_rig_fuse: the
        dict gains "fused" and its overflow word the bit ops.FUSE_OVERFLOW; such a tick holds all the posed pairs."""
        first_pair = self._check_device_tick(frames, first_pair)
        fuse = _fuse and self._poses_host is not None           # (tick_sharded fuses after the gather instead)
        if fuse:
            self._check_fused_tick(frames.shape[0] // 2, first_pair)
        if _fuse:
            rig_pose = _check_frame_pose(rig_pose, self.world_frame, 1, frames.device, "rig_pose", "the one T_WB of the tick")
        with torch.no_grad():
            # split-product networks: the fp16-range flag is folded into `overflow` on the device instead of being read here (as
            # BatchedKeypointPipeline.forward_device does), except with on_overflow = "float32", where the pass is judged on the host
            defer = getattr(self.net, "on_overflow", "raise") != "float32"
            heat, depth, _ = self.net.deployed(frames, check_range=not defer)
            range_flag = self.net.range_flag(frames.device) if defer and hasattr(self.net, "range_flag") else None
            if heat_override is not None:
                heat = heat_override
            count, _, xyc = ops.peak_nms(heat, cap=self.capacity)
            table = self._table(frames.device)                 # (a single calibration: the one-entry table, broadcast to every pair)
            match, overflow = ops.stereo_match_rig(table, count, xyc, self.assoc.max_distance, first_pair=first_pair, range_flag=range_flag)
            points = ops.stereo_triangulate_rig(table, count, xyc, match, first_pair=first_pair)
            out = {"heat": heat, "depth": depth, "count": count, "xyc": xyc, "match": match, "points": points, "overflow": overflow}
            if fuse:
                out["fused"] = self._fuse(points, overflow)
                out["overflow"] = out["fused"]["overflow"]
                self._finish(out, rig_pose)
        return out

    def capture_device(self, frames, heat_override=None, first_pair=0, rig_pose=None):
        """Capture the WHOLE tick_device (network, NMS, association, triangulation, overflow word) for this frame shape into one hipGraph;
        that the capture succeeds is itself the check that nothing in the tick waits on the host.  Returns a CapturedTick: replay with
        step.replay(new_frames[, new_heat]) or by copying into step.static_in / step.static_heat (heat_override, when given, is a static
        input of the graph like the frames) and step.replay(); the outputs are step.static_out (tick_device's dict).  first_pair: as for
        tick_device; the warm-up ticks upload the calibration table before the capture begins.  With track: the graph steps the tracker's
        state in place, the state eager ticks use; the warm-up ticks and the capture advance it, so capture_device() ends with
        reset_tracks() - every track alive before it is gone.  With world_frame: rig_pose is a static input of the graph as well -
        step.replay(frames, rig_pose=...) copies a new one into step.static_pose before the replay."""
        first_pair = self._check_device_tick(frames, first_pair)
        self._check_fused_tick(frames.shape[0] // 2, first_pair)
        _check_frame_pose(rig_pose, self.world_frame, 1, frames.device, "rig_pose", "the one T_WB of the tick")
        static_in = frames.clone()
        static_heat = heat_override.clone() if heat_override is not None else None
        static_pose = rig_pose.clone() if rig_pose is not None else None
        graph, static_out = _capture(lambda: self.tick_device(static_in, heat_override=static_heat, first_pair=first_pair, rig_pose=static_pose))
        step = CapturedTick(self.net, graph, static_in, static_out, static_heat)
        step.static_pose = static_pose
        step._table = self._table(frames.device)               # (the graph reads it on every replay)
        step._poses = self._poses.on.get(frames.device)        # (and the pose table)
        step._views = self._views.on.get(frames.device)        # (and, with refine, the views table)
        self._stage.pin(step, static_out)
        return step

    def results(self, out):
        """A device tick (tick_device, a CapturedTick's outputs, or tick_sharded's gathered payload) as tick() returns it: a list over
        pairs of {type k: (n_k, 3) float64 points in the left camera frame}, in ascending left-peak order.  Reads `points` (a NaN row =
        unmatched slot) and `overflow` only, in ONE device -> host copy; raises OkpError like tick() when the overflow word is set."""
        host = _to_host({"overflow": out["overflow"], "points": out["points"]})        # the one D2H copy
        _raise_on_overflow(int(host["overflow"]))
        pts = host["points"]
        result = []
        for p in range(pts.shape[0]):
            per = {}
            for k in range(pts.shape[1]):
                rows = pts[p, k]
                per[k] = np.ascontiguousarray(rows[~np.isnan(rows[:, 3]), :3])       # (column 3, the confidence, is NaN exactly in unused slots)
            result.append(per)
        return result

    def tick_sharded(self, frames_local, n_pairs_total, heat_override=None, rig_pose=None):
        """The rig's pairs sharded over the ranks of the process group (both views of a pair on one GPU): this rank holds the frames of
        pairs distributed.shard(n_pairs_total, rank, world) (2 per pair, left first).  Runs tick_device on them and returns
            {"points": [n_pairs_total, K, cap, 4] fp64 - ONE all_gather_keypoints of the per-rank payloads, ordered by pair,
             "overflow": 0-d int32 - the overflow words folded over the ranks on the device (one all_reduce, MAX: set on one rank = set
                         on every rank), "local": this rank's tick_device dict (None for a rank without pairs)}
        which results() reads; with rig_poses also "fused": okp_rig_fuse of the gathered payload, run on every rank (the same bits on each),
        and "overflow" then carries ops.FUSE_OVERFLOW as well.  A rank without pairs (world > n_pairs_total) joins both collectives with an empty block.  Without a
        process group it is tick_device on the whole rig.  A rig of individually calibrated pairs: n_pairs_total == len(rig), and each
        rank's pairs are calibrated by their rig-wide index (first_pair = the shard's start)."""
        import torch.distributed as dist
        from .. import distributed
        if int(n_pairs_total) < 1:
            raise OkpError(f"n_pairs_total = {n_pairs_total}: a rig has at least one stereo pair")
        if self.rig is not None and int(n_pairs_total) != len(self.rig):
            raise OkpError(f"n_pairs_total = {n_pairs_total}, but the rig has {len(self.rig)} stereo pairs")
        self._check_device_tick(frames_local)
        if self._poses_host is not None and int(n_pairs_total) != self.n_fused_pairs:
            raise OkpError(f"n_pairs_total = {n_pairs_total}, but {self.n_fused_pairs} rig poses were given")
        rig_pose = _check_frame_pose(rig_pose, self.world_frame, 1, frames_local.device, "rig_pose", "the one T_WB of the tick, the same on every rank")
        if not dist.is_initialized():
            if frames_local.shape[0] != 2 * n_pairs_total:
                raise OkpError(f"{frames_local.shape[0]} frames for {n_pairs_total} stereo pairs")
            out = self.tick_device(frames_local, heat_override=heat_override, rig_pose=rig_pose)
            whole = {"points": out["points"], "overflow": out["overflow"], "local": out}
            for key in ("fused", "pose", "refine", "world", "track", "window"):
                if key in out:
                    whole[key] = out[key]
            return whole
        for name, cfg in (("refine", self.refine), ("rig_window", self.rig_window)):
            if cfg is not None and cfg.confidence is not None:
                raise OkpNotOffered(f"tick_sharded with {name} and its confidence under a process group: not offered (the weighted refinement reads every "
                                    "pair's peaks); tick_device and capture_device of a pipeline built with refine / rig_window take the keyword")
        if self.refine is not None:
            raise OkpError("tick_sharded with refine under a process group: the refinement reads every pair's peaks and matches, and the gathered "
                           "payload holds the other ranks' 3D points only")
        if self.rig_window is not None:
            raise OkpError("tick_sharded with rig_window under a process group: the window reads every pair's peaks and matches, and the gathered "
                           "payload holds the other ranks' 3D points only")
        start, n_local = distributed.shard(int(n_pairs_total), dist.get_rank(), dist.get_world_size())
        if frames_local.shape[0] != 2 * n_local:
            raise OkpError(f"rank {dist.get_rank()} holds {frames_local.shape[0]} frames; shard({n_pairs_total}, {dist.get_rank()}, "
                           f"{dist.get_world_size()}) gives it {n_local} stereo pairs = {2 * n_local} frames")
        if n_local:
            local = self.tick_device(frames_local, heat_override=heat_override, first_pair=start, _fuse=False)
            points, flag = local["points"], local["overflow"].reshape(1).clone()
        else:
            local, dev = None, frames_local.device
            points = torch.empty((0, len(self.config), self.capacity, 4), dtype=torch.float64, device=dev)
            flag = torch.zeros((1,), dtype=torch.int32, device=dev)
        gathered = distributed.all_gather_keypoints(points, total_frames=int(n_pairs_total))
        dist.all_reduce(flag, op=dist.ReduceOp.MAX)
        out = {"points": gathered, "overflow": flag[0], "local": local}
        if self._poses_host is not None:
            with torch.no_grad():
                out["fused"] = self._fuse(gathered, flag)
                self._finish(out, rig_pose)
            out["overflow"] = out["fused"]["overflow"]
        return out

    def rig_objects(self, out):
        """The objects of a fused device tick (tick_device, a CapturedTick's outputs or tick_sharded's dict, of a pipeline built with
        rig_poses) in the rig frame: a list over objects of
            {"p_B": [(1, 3) centre, (n_1, 3), ..., (n_{K-1}, 3)] float64 points in rig coordinates - the nesting of
                    ObjectKeypointPipeline's 'p_C', one array per key-point type, n_k <= the type's count, in cluster order,
             "confidence": [(1,), (n_1,), ...] float64, "views": [(1,), (n_1,), ...] int32 bit masks of the contributing pairs}
        plus, for a pipeline built with points_3d, 'T_BO' (4 x 4 float64: model -> rig coordinates; None where the status is ops.POSE_FEW or
        ops.POSE_DEGENERATE), 'rmse', 'ambiguity' (the runner-up assignment's rmse) and 'pose_status', and, for one built with track,
        'track_id' (None where the object went to no track), 'T_BO_track' (the filtered pose), 'velocity', 'track_hits' and 'confirmed', and,
        for one built with refine, 'T_BO_refined' (None where 'T_BO' is; the fitted pose where 'refine_status' is not 0), 'reprojection_rmse'
        (before, after), 'refine_observations', 'pose_information' (6 x 6) and 'refine_status'; with world_frame 'T_WO' then comes from the
        refined pose; with rig_window 'T_BO_window' (None where the window's status is not 0) and 'window_views' of the object's track - read
        in ONE device -> host copy.  Raises OkpError when the tick's overflow word is set, as results() does (bit ops.FUSE_OVERFLOW:
        a type had more than fuse_capacity clusters).  tick(), the host tick, does not fuse: its return value is not accepted here."""
        if not isinstance(out, dict) or "fused" not in out:
            raise OkpError("rig_objects reads a fused device tick: the dict of tick_device / capture_device / tick_sharded of a pipeline "
                           "built with rig_poses (the host tick() does not fuse)")
        f = out["fused"]
        fields = {"overflow": out["overflow"], "n_obj": f["n_obj"], "n_fused": f["n_fused"], "views": f["views"], "object": f["object"], "fused": f["fused"]}
        if "pose" in out:
            fields.update(_pose_fields(out["pose"], 0, out.get("refine")))
        if "track" in out:
            fields.update(_track_fields(out["track"], 0, out.get("window")))
        in_world = "world" in out
        if in_world:
            fields["T_WB"] = out["world"]["T"]
            if "pose" in out:
                fields["world_pose"] = out["world"]["pose"][0]
        host = _to_host(fields)                                    # the one D2H copy
        _raise_on_overflow(int(host["overflow"]), fused=True)
        n_obj, n_fused, views, obj, rows = int(host["n_obj"]), host["n_fused"], host["views"], host["object"], host["fused"]
        missing = in_world and not np.isfinite(host["T_WB"]).all()
        objects = []
        for o in range(n_obj):
            p_B, conf, seen = [], [], []
            for k in range(views.shape[0]):
                sel = np.nonzero(obj[k, :n_fused[k]] == o)[0]
                p_B.append(np.ascontiguousarray(rows[k, sel, :3]))
                conf.append(np.ascontiguousarray(rows[k, sel, 3]))
                seen.append(views[k, sel])
            objects.append({"p_B": p_B, "confidence": conf, "views": seen})
            if "pose" in out:
                objects[-1].update(_pose_entries(host, o, "T_BO"))
                if "refine" in out:
                    objects[-1].update(_rig_refine_entries(host, o, objects[-1]["T_BO"]))
                if in_world:
                    objects[-1]["T_WO"] = None if missing else _pose_entries(dict(host, pose=host["world_pose"]), o, "T_WO")["T_WO"]
            if "track" in out:
                objects[-1].update(_track_entries(host, o, "T_BO_track", self._tracker.cfg.min_hits, "T_WO_track", getattr(self._stage.window, "cameras", None)))
        return objects
