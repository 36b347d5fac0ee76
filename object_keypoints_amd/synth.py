"""Procedural (counter-based) weights, frames and heat/depth/centre maps.

There is no network access for checkpoints or datasets, so every test, golden
vector and benchmark uses values generated here from an integer seed.  The
generator is a pure-NumPy splitmix64 hash of (seed, crc32(name), element index):
no torch RNG, no NumPy distribution code, so the same (seed, name, shape) gives
the same bits in the build container, on the GPU box and in the golden-vector
generator that runs the reference (tests/golden/make_goldens.py).

Weight scales are chosen so activations stay O(1) through the ~60-layer
stacked hourglass (the reference's default init leaves the logits in
[0.005, 0.013], useless as a parity signal — SURVEY.md §8(c)).
"""
import zlib

import numpy as np

_M64 = np.uint64(0xFFFFFFFFFFFFFFFF)


def _splitmix64(x):
    x = (x + np.uint64(0x9E3779B97F4A7C15)) & _M64
    z = x
    z = ((z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)) & _M64
    z = ((z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)) & _M64
    return z ^ (z >> np.uint64(31))


def unit_uniform(name, shape, seed):
    """float32 array in [0, 1), a pure function of (name, shape, seed)."""
    n = int(np.prod(shape)) if len(shape) else 1
    tag = np.uint64(zlib.crc32(name.encode("utf-8")))
    base = (np.uint64(seed & 0xFFFFFFFF) << np.uint64(32)) | tag
    with np.errstate(over="ignore"):
        h = _splitmix64(_splitmix64(np.full(n, base, dtype=np.uint64))
                        + np.arange(n, dtype=np.uint64))
    u = (h >> np.uint64(40)).astype(np.float32) * np.float32(1.0 / (1 << 24))
    return u.reshape(shape)


def uniform(name, shape, seed, lo, hi):
    return (np.float32(lo) + np.float32(hi - lo) * unit_uniform(name, shape, seed)).astype(np.float32)


def normal_like(name, shape, seed):
    """Approximately N(0,1) float32 (sum of 4 uniforms, variance-corrected)."""
    acc = np.zeros(shape, dtype=np.float32)
    for i in range(4):
        acc += unit_uniform(f"{name}#{i}", shape, seed)
    return ((acc - np.float32(2.0)) * np.float32(np.sqrt(3.0))).astype(np.float32)


# ----------------------------------------------------------------------------
# state_dict filling
# ----------------------------------------------------------------------------

def _is_bn_group(prefix, keys):
    return (prefix + ".running_mean") in keys


def _is_head_output(prefix):
    parts = prefix.split(".")
    return len(parts) >= 2 and parts[-1] == "2" and parts[-2].startswith("output_head")


def fill_state_dict(shapes, seed=0, branch_gain=0.3, head_gain=0.45):
    """shapes: {state_dict key: shape tuple} -> {key: np.ndarray}.

    Conv / conv-transpose weights: uniform with variance gain^2/fan_in.
    BatchNorm: gamma in [0.8,1.2] (x branch_gain for the last BN of a residual
    branch, so `relu(branch + skip)` keeps O(1) scale through both hourglasses), beta in [-0.2,0.2],
    running_mean in [-0.2,0.2], running_var in [0.6,1.4].
    """
    keys = set(shapes)
    out = {}
    for key, shape in shapes.items():
        shape = tuple(shape)
        prefix, _, leaf = key.rpartition(".")
        if leaf == "num_batches_tracked":
            out[key] = np.array(100, dtype=np.int64)
        elif leaf == "running_mean":
            out[key] = uniform(key, shape, seed, -0.2, 0.2)
        elif leaf == "running_var":
            out[key] = uniform(key, shape, seed, 0.6, 1.4)
        elif _is_bn_group(prefix, keys):
            if leaf == "weight":
                g = uniform(key, shape, seed, 0.8, 1.2)
                last = prefix.rsplit(".", 1)[-1]
                # bn2 closes fire/residual branches; skip.1 is the projected skip
                if last == "bn2":
                    g = g * np.float32(branch_gain)
                out[key] = g.astype(np.float32)
            else:
                out[key] = uniform(key, shape, seed, -0.2, 0.2)
        elif leaf == "weight":
            if len(shape) != 4:
                raise ValueError(f"unexpected weight {key} {shape}")
            if prefix.endswith("up2"):           # ConvTranspose2d (Cin, Cout, 4, 4), stride 2
                fan_in = shape[0] * 4            # 2x2 taps reach each output pixel
                gain = 1.0
            else:
                fan_in = shape[1] * shape[2] * shape[3]
                gain = np.sqrt(2.0)
                if _is_head_output(prefix):      # last 1x1 of a head: keeps logits ~N(0, 1.5^2)
                    gain = head_gain
            b = gain * np.sqrt(3.0 / fan_in)
            out[key] = uniform(key, shape, seed, -b, b)
        elif leaf == "bias":
            out[key] = uniform(key, shape, seed, -0.1, 0.1)
        else:
            raise ValueError(f"unexpected state_dict entry {key}")
    return out


def frames(n, seed=1, start=0, size=511):
    """(n,3,size,size) float32 ~N(0,1): stands in for the normalised RGB crop
    (reference perception/datasets/video.py:215)."""
    return np.stack([normal_like(f"frame{start + i}", (3, size, size), seed) for i in range(n)])


# ----------------------------------------------------------------------------
# synthetic heat / depth / centre maps (SURVEY.md §8(d) "Heatmaps for NMS/3D stages")
# ----------------------------------------------------------------------------

def bump_scene(keypoint_config, n_objects=1, seed=0, index=0, size=64, length_scale=2.0,
               margin=6.0, max_radius=9.0):
    """One frame of post-network maps for `n_objects` objects.

    Returns dict with heat (K,size,size), depth (K,size,size), centers (K-1,2,size,size),
    and the generating 2D points/depths.  Gaussian bumps exp(-|d|^2/l^2) as in the
    reference's target rendering (perception/datasets/video.py:22-25,44-53), clipped to [0,1].
    """
    config = [1] + list(keypoint_config)
    K = len(config)
    heat = np.zeros((K, size, size), dtype=np.float32)
    depth = np.zeros((K, size, size), dtype=np.float32)
    centers = np.zeros((K - 1, 2, size, size), dtype=np.float32)
    ys, xs = np.meshgrid(np.arange(size, dtype=np.float32), np.arange(size, dtype=np.float32), indexing="ij")
    objects = []
    tag = f"scene{index}"
    # object centres on a jittered grid so objects stay > 20 px apart when possible
    g = int(np.ceil(np.sqrt(n_objects)))
    cell = (size - 2 * margin) / g
    for o in range(n_objects):
        gy, gx = divmod(o, g)
        j = unit_uniform(f"{tag}/o{o}/c", (2,), seed)
        cx = margin + (gx + 0.3 + 0.4 * j[0]) * cell
        cy = margin + (gy + 0.3 + 0.4 * j[1]) * cell
        obj = {"center": np.array([cx, cy], dtype=np.float32), "points": [], "depths": []}
        radius = min(0.35 * cell, max_radius)
        for k, count in enumerate(config):
            pts = []
            for i in range(count):
                if k == 0:
                    p = np.array([cx, cy], dtype=np.float32)
                else:
                    a = unit_uniform(f"{tag}/o{o}/k{k}/{i}", (2,), seed)
                    ang = 2 * np.pi * (a[0] + (i + 0.37 * k) / max(count, 1))
                    r = radius * (0.55 + 0.45 * a[1])
                    p = np.array([cx + r * np.cos(ang), cy + r * np.sin(ang)], dtype=np.float32)
                    p = np.clip(p, 2.0, size - 3.0).astype(np.float32)
                z = np.float32(0.3 + 1.2 * unit_uniform(f"{tag}/o{o}/k{k}/{i}/z", (1,), seed)[0])
                d2 = (xs - p[0]) ** 2 + (ys - p[1]) ** 2
                heat[k] += np.exp(-d2 / np.float32(length_scale ** 2)).astype(np.float32)
                near = d2 < np.float32(16.0)
                depth[k][near] = z
                if k > 0:
                    centers[k - 1, 0][near] = (cx - (xs + 0.5))[near]
                    centers[k - 1, 1][near] = (cy - (ys + 0.5))[near]
                pts.append((p, z))
            obj["points"].append([p for p, _ in pts])
            obj["depths"].append([z for _, z in pts])
        objects.append(obj)
    heat = np.clip(heat, 0.0, 1.0).astype(np.float32)
    return {"heat": heat, "depth": depth, "centers": centers, "objects": objects}


def add_double_detections(scene, k, offset=(4.0, 3.0), size=64, length_scale=2.0):
    """Every keypoint of map `k` (>= 1) of a bump_scene gets a second bump at `offset` pixels from it, with the same depth and a centre
    vector that points at the same object: each instance is detected twice, so the object receives twice as many votes for that type as it
    has instances - the case the reference reduces with k-means (perception/pipeline.py:143-148).  Returns a new scene dict."""
    heat, depth, centers = scene["heat"].copy(), scene["depth"].copy(), scene["centers"].copy()
    ys, xs = np.meshgrid(np.arange(size, dtype=np.float32), np.arange(size, dtype=np.float32), indexing="ij")
    extra = np.zeros((size, size), dtype=np.float32)
    for obj in scene["objects"]:
        cx, cy = obj["center"]
        for p, z in zip(obj["points"][k], obj["depths"][k]):
            q = np.clip(p + np.array(offset, dtype=np.float32), 2.0, size - 3.0).astype(np.float32)
            d2 = (xs - q[0]) ** 2 + (ys - q[1]) ** 2
            extra += np.exp(-d2 / np.float32(length_scale ** 2)).astype(np.float32)
            near = d2 < np.float32(16.0)
            depth[k][near] = z
            centers[k - 1, 0][near] = (cx - (xs + 0.5))[near]
            centers[k - 1, 1][near] = (cy - (ys + 0.5))[near]
    heat[k] = np.clip(heat[k] + extra, 0.0, 1.0).astype(np.float32)
    return {"heat": heat, "depth": depth, "centers": centers, "objects": scene["objects"]}


# ----------------------------------------------------------------------------
# a synthetic rig of individually calibrated stereo pairs (StereoStreamPipeline with a sequence of StereoCameras)
# ----------------------------------------------------------------------------

RIG_BASELINES = (0.06, 0.12, 0.20, 0.30)          # metres, pair by pair
# per pair: (fx, fy, cx, cy) factors of the left and of the right camera (cx only 1.5-2 %: PinholeCamera's centring check of the crop),
# a factor on the distortion coefficients, and a relative rotation of the right camera (axis, degrees)
_RIG_PAIRS = (
    ((1.00, 1.00, 1.00, 1.00), (1.00, 1.00, 1.00, 1.00), 1.00, (1, 0.0)),
    ((1.08, 1.10, 1.02, 1.06), (0.93, 0.92, 0.98, 0.94), 0.70, (1, 2.5)),
    ((0.90, 0.88, 0.985, 0.91), (1.12, 1.14, 1.02, 1.10), 1.25, (0, -3.0)),
    ((1.15, 1.13, 1.015, 1.12), (0.87, 0.86, 0.98, 0.89), 0.50, (2, 4.0)),
)
# per pair of a rig scene: 1 centre (type 0), 1 point of type 1, 3 points of type 2 (bench.py run_stream8's scene), pushed back and
# shifted by half the baseline as the pair's baseline grows, so that every point stays inside both views' 64 x 64 maps
RIG_SCENE = {0: [[0.00, 0.00, 0.55]], 1: [[0.12, -0.10, 0.60]], 2: [[-0.16, 0.12, 0.50], [0.14, 0.04, 0.65], [-0.12, -0.16, 0.70]]}


def stereo_rig(params, n_pairs=4, size=64):
    """n_pairs (<= 4) clearly different StereoCameras derived from one calibration (camera_utils.load_calibration_params): baselines
    RIG_BASELINES, focal lengths and principal points 5-15 % apart (cx 1.5-2 %), distortion scaled by 0.5-1.25, a few degrees of relative
    rotation; every camera resampled to the size x size prediction space of a 720 x 1280 camera (resize to 511 rows, centre crop 511,
    scale), as the stereo tests and bench.py do."""
    from .perception.utils import camera_utils as cu
    offset = np.array([(511 / 720 * 1280 - 511.0) / 2.0, 0.0])
    T0 = np.asarray(params["T_RL"], dtype=np.float64)
    rig = []
    for q in range(n_pairs):
        fl, fr, dscale, (axis, deg) = _RIG_PAIRS[q]
        cams = []
        for K, D, f in ((params["K"], params["D"], fl), (params["Kp"], params["Dp"], fr)):
            K = np.array(K, dtype=np.float64)
            K[0, 0] *= f[0]; K[1, 1] *= f[1]; K[0, 2] *= f[2]; K[1, 2] *= f[3]
            cam = cu.FisheyeCamera(K, np.asarray(D, dtype=np.float64) * dscale, params["image_size"])
            cams.append(cam.scale(511 / 720).cut(offset).scale(size / 511))
        a = np.deg2rad(deg)
        c, s = np.cos(a), np.sin(a)
        i, j = [(1, 2), (0, 2), (0, 1)][axis]
        R = np.eye(3)
        R[i, i], R[i, j], R[j, i], R[j, j] = c, -s, s, c
        T = np.eye(4)
        T[:3, :3] = R @ T0[:3, :3]
        T[:3, 3] = T0[:3, 3] / np.linalg.norm(T0[:3, 3]) * RIG_BASELINES[q]
        rig.append(cu.StereoCamera(cams[0], cams[1], T))
    return rig


def rig_scene_points(q, shift=0.0):
    """{type: (n, 3) points in pair q's left camera frame} of the rig scene."""
    b = RIG_BASELINES[q]
    depth = max(1.0, b / RIG_BASELINES[0]) ** 0.5
    return {k: np.array(pts) * depth + np.array([b / 2 + shift, 0.0, 0.0]) for k, pts in RIG_SCENE.items()}


def render_rig_heat(rig, pairs=None, shift=0.0, crowd=None, size=64):
    """Heat maps [2 len(pairs), K, size, size] float32 (NumPy) of the rig scene: pair q's points rendered through pair q's OWN left and
    right camera (Gaussian bumps exp(-d^2 / 4), clipped to [0, 1]).  crowd = (pair q, side, type): twelve extra bumps in that map."""
    pairs = list(range(len(rig))) if pairs is None else list(pairs)
    ys, xs = np.meshgrid(np.arange(size, dtype=np.float32), np.arange(size, dtype=np.float32), indexing="ij")
    heat = np.zeros((2 * len(pairs), len(RIG_SCENE), size, size), np.float32)
    for i, q in enumerate(pairs):
        st = rig[q]
        for k, X in rig_scene_points(q, shift).items():
            for side, (cam, T) in enumerate(((st.left_camera, np.eye(4)), (st.right_camera, st.T_RL))):
                for px, py in cam.project(X, T):
                    heat[2 * i + side, k] += np.exp(-((xs - px) ** 2 + (ys - py) ** 2) / 4.0)
        if crowd is not None and crowd[0] == q:
            for a in range(4):
                for c in range(3):
                    heat[2 * i + crowd[1], crowd[2]] += np.exp(-((xs - 8 - 12 * a) ** 2 + (ys - 50 - 5 * c) ** 2) / 2.0)
    return np.clip(heat, 0.0, 1.0)


# ----------------------------------------------------------------------------
# the same rig with a pose per pair, and one scene in rig coordinates (StereoStreamPipeline with rig_poses: okp_rig_fuse)
# ----------------------------------------------------------------------------

# two objects in the rig (body) frame: per object 1 centre (type 0), 1 point of type 1, 3 points of type 2 - RIG_SCENE's object and a
# second one beside and behind it, far enough apart that every key point is nearer to its own centre than to the other
RIG_FUSE_SCENE = (
    {0: [[-0.12, -0.03, 0.00]], 1: [[-0.06, -0.10, 0.03]], 2: [[-0.12, 0.09, -0.03], [-0.224, -0.08, 0.04], [-0.05, -0.135, 0.03]]},
    {0: [[0.14, 0.05, 0.16]], 1: [[0.20, -0.02, 0.19]], 2: [[0.14, -0.03, 0.13], [0.22, 0.14, 0.18], [0.036, 0.03, 0.21]]},
)
# metres.  Points of one type are at least 0.14 m apart - and 0.05 m apart in height, more than the epipolar gate of the stereo tests in
# every pair's maps, so that each pair's left / right association is unambiguous -; with views that miss the truth by e < 0.03 a merge
# radius between 2 e and 0.14 - 2 e joins the views of one point and nothing else; a key point lies within 0.13 m of its own centre and at
# least 0.13 m farther from the other one, so the object radius holds the former plus 2 e.  (The tests assert these conditions on the
# tick's own payload.)
RIG_FUSE_MERGE_RADIUS = 0.08
RIG_FUSE_OBJECT_RADIUS = 0.18
# per pair: the yaw (about the rig's y axis, degrees) from which it looks at the rig frame's origin, its height above it and its distance
# to it - growing with the baseline, so that each pair works in a depth range its baseline resolves on 64 x 64 maps
_RIG_FUSE_YAW = (0.0, 9.0, -8.0, 14.0)
_RIG_FUSE_HEIGHT = (0.0, 0.03, -0.02, 0.04)
_RIG_FUSE_DISTANCE = (0.50, 0.62, 0.75, 0.90)


def rig_poses(n_pairs=4):
    """T_BL (4 x 4: pair q's left-camera coordinates -> rig coordinates) of stereo_rig's pairs: pair q looks at the rig frame's origin
    - where RIG_FUSE_SCENE lies - from a yaw of its own, at the distance rig_scene_points gives its baseline, offset by half the baseline
    so that the scene sits between its two cameras."""
    poses = []
    for q in range(n_pairs):
        b = RIG_BASELINES[q]
        a = np.deg2rad(_RIG_FUSE_YAW[q])
        c, s = np.cos(a), np.sin(a)
        R = np.array([[c, 0.0, s], [0.0, 1.0, 0.0], [-s, 0.0, c]])                 # camera axes in rig coordinates
        in_camera = np.array([b / 2, _RIG_FUSE_HEIGHT[q], _RIG_FUSE_DISTANCE[q]])     # the rig's origin, seen by the left camera
        T = np.eye(4)
        T[:3, :3] = R
        T[:3, 3] = -R @ in_camera
        poses.append(T)
    return poses


def rig_fuse_scene(shift=0.0):
    """[{type: (n, 3) points in rig coordinates}] per object of the fused rig scene (shift: metres along the rig's x axis)."""
    return [{k: np.array(pts) + np.array([shift, 0.0, 0.0]) for k, pts in obj.items()} for obj in RIG_FUSE_SCENE]


def render_rig_fuse_heat(rig, poses, shift=0.0, size=64):
    """Heat maps [2 len(rig), K, size, size] float32 (NumPy) of rig_fuse_scene: every object's points taken into pair q's left-camera
    frame by inv(poses[q]) and rendered through pair q's OWN left and right camera, as render_rig_heat does."""
    ys, xs = np.meshgrid(np.arange(size, dtype=np.float32), np.arange(size, dtype=np.float32), indexing="ij")
    heat = np.zeros((2 * len(rig), len(RIG_FUSE_SCENE[0]), size, size), np.float32)
    for q, st in enumerate(rig):
        T_LB = np.linalg.inv(np.asarray(poses[q], dtype=np.float64))
        for obj in rig_fuse_scene(shift):
            for k, X_B in obj.items():
                X = X_B @ T_LB[:3, :3].T + T_LB[:3, 3]
                for side, (cam, T) in enumerate(((st.left_camera, np.eye(4)), (st.right_camera, st.T_RL))):
                    for px, py in cam.project(X, T):
                        heat[2 * q + side, k] += np.exp(-((xs - px) ** 2 + (ys - py) ** 2) / 4.0)
    return np.clip(heat, 0.0, 1.0)
