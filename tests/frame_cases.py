"""Seeded cases for okp_change_frame (tests/test_frame_args.py on the CPU, tests/test_gpu_world_frame.py on the device).

A case: {"name", "T" [B,12], "points" [B,n_points,4] or None, "poses" [B,n_pose,12] or None}.  Coordinates up to 10 m, rotations by any
angle about any axis.  Except in the two one-row cases, point row 1 and pose row 0 of stream 0 are EMPTY (all NaN) and the last point row of
the last stream holds one infinite value: neither is special-cased by the specification.  The shapes (B, n_points, n_pose) put the total
row count B * (n_points + n_pose) one below, at and one above the kernel's block of 256 lanes and above two blocks, with several streams
inside a block and streams that straddle two."""
import numpy as np

BLOCK = 256           # csrc/okp_frame.hip OKP_FRAME_THREADS
REACH = 10.0          # metres

SHAPES = [("one_point", 1, 1, 0), ("one_pose", 1, 0, 1), ("small", 3, 5, 2), ("block_minus_1", 5, 40, 11), ("block", 4, 40, 24),
          ("block_plus_1", 1, 200, 57), ("three_blocks", 7, 50, 30)]


def rot(axis, angle):
    """Rodrigues' rotation about `axis` by `angle` (radians)."""
    u = np.asarray(axis, dtype=np.float64)
    u = u / np.linalg.norm(u)
    K = np.array([[0.0, -u[2], u[1]], [u[2], 0.0, -u[0]], [-u[1], u[0], 0.0]])
    return np.eye(3) + np.sin(angle) * K + (1.0 - np.cos(angle)) * (K @ K)


def transforms(rng, n):
    """n rigid transforms [n,12], row-major [R | t], |t_i| <= REACH."""
    out = np.empty((n, 3, 4))
    for k in range(n):
        out[k, :, :3] = rot(rng.normal(size=3), rng.uniform(-np.pi, np.pi))
        out[k, :, 3] = rng.uniform(-REACH, REACH, size=3)
    return out.reshape(n, 12)


def _case(name, B, n_points, n_pose, seed):
    rng = np.random.default_rng(seed)
    case = {"name": name, "T": transforms(rng, B), "points": None, "poses": None}
    if n_points:
        case["points"] = np.concatenate([rng.uniform(-REACH, REACH, size=(B, n_points, 3)), rng.uniform(0.0, 1.0, size=(B, n_points, 1))], axis=2)
    if n_pose:
        case["poses"] = transforms(rng, B * n_pose).reshape(B, n_pose, 12)
    if n_points > 1:
        case["points"][0, 1] = np.nan
        case["points"][-1, -1, 1] = np.inf
    if n_pose > 1:
        case["poses"][0, 0] = np.nan
    return case


def cases():
    out = [_case(name, B, n_points, n_pose, seed=100 + k) for k, (name, B, n_points, n_pose) in enumerate(SHAPES)]
    # a stream whose pose is NaN in a single element, between two valid streams
    c = _case("missing_between", 3, 5, 2, seed=200)
    c["T"][1, 6] = np.nan
    out.append(c)
    return out


def finite_cases():
    """The same shapes without the empty and infinite rows and without a missing pose: what the round-trip bound is stated for."""
    out = []
    for k, (name, B, n_points, n_pose) in enumerate(SHAPES):
        c = _case(name, B, n_points, n_pose, seed=300 + k)
        rng = np.random.default_rng(400 + k)
        if n_points > 1:
            c["points"][0, 1] = rng.uniform(-REACH, REACH, size=4)
            c["points"][-1, -1, 1] = 0.5
        if n_pose > 1:
            c["poses"][0, 0] = transforms(rng, 1)[0]
        out.append(c)
    return out
