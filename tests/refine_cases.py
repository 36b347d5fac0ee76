"""The fabricated cases of the pose refinement tests, as plain arrays: each holds the inputs of okp_refine_pose (tab, pose, assignment, n_obj,
model), the camera's focal lengths and the parameters.  The CPU tests (tests/test_refine_args.py) assert on the inputs, through the NumPy
specification (tests/refine_spec.py), that every case is away from every decision of the stage; the GPU tests (tests/test_gpu_refine.py)
compare the device with the specification on the same cases.

The tables of the "fitted" cases come from the pose stage's own scene helper (tests/object_pose_cases.py) and their start poses and
assignments from its specification (tests/object_pose_spec.py), as on the device.  The "crafted" case is built directly as tensors, one
object per status."""
import numpy as np

import object_pose_cases as pc
import object_pose_spec as pose_spec

FX = FY = 62.0            # a 64 x 64 map of a camera with a 55 degree field of view
DEFAULTS = dict(sigma_px=0.25, sigma_z=0.05, iters=6, damping=1e-9)
# a valve-like object - a stem of 12 cm over three handle points - with every key point a type of its own: one hypothesis, so the
# correspondence is not in question (resolving a symmetric model's assignment is not what the refinement does)
ONE_EACH = [1, 1, 1, 1]
VALVE_LIKE = pose_spec.model_of(np.array([[0.0, 0.0, 0.12], [0.09, 0.01, 0.0], [-0.05, 0.08, 0.01], [-0.03, -0.085, 0.02]]), ONE_EACH)


def perturbation(rng, angle, shift):
    """A rotation by `angle` radians about a random axis and a translation of length `shift`."""
    axis = rng.normal(size=3)
    axis /= np.linalg.norm(axis)
    Kx = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    d = rng.normal(size=3)
    return np.eye(3) + np.sin(angle) * Kx + (1 - np.cos(angle)) * Kx @ Kx, shift * d / np.linalg.norm(d)


def fitted(tab, n_obj, model, type_count):
    """The pose stage's outputs on a table, by its specification: (pose [B,max_obj,12], assignment [B,max_obj,S] int32)."""
    out = pose_spec.object_pose(tab, n_obj, model, type_count)
    return out["pose"], out["assignment"].astype(np.int32)


def depth_noise_scene(model, n, seed, depth_noise=0.03, pixel_noise=0.0, fx=FX, fy=FY):
    """n objects of `model` under random poses at 0.5 .. 1.5 m, every point seen along its exact bearing (plus pixel_noise map pixels) at
    a depth that is off by a factor 1 + N(0, depth_noise): what lifting through a noisy depth map gives.  -> tab [1,n,S,4], truth [(R, t)]."""
    rng = np.random.default_rng(seed)
    S = model.shape[0]
    tab = np.full((1, n, S, 4), np.nan)
    truth = []
    for o in range(n):
        R, t = pc.rotation(rng), np.array([rng.uniform(-0.3, 0.3), rng.uniform(-0.3, 0.3), rng.uniform(0.5, 1.5)])
        q = model @ R.T + t
        u = q[:, 0] / q[:, 2] + rng.normal(scale=1.0, size=S) * pixel_noise / fx
        v = q[:, 1] / q[:, 2] + rng.normal(scale=1.0, size=S) * pixel_noise / fy
        z = q[:, 2] * (1.0 + rng.normal(scale=depth_noise, size=S))
        tab[0, o] = np.stack([u * z, v * z, z, np.full(S, 0.9)], axis=1)
        truth.append((R, t))
    return tab, truth


def _case(name, tab, pose, assignment, n_obj, model, kind="fitted", **params):
    return dict(name=name, tab=tab, pose=pose, assignment=assignment, n_obj=np.asarray(n_obj, dtype=np.int32), model=model, fx=FX, fy=FY, kind=kind,
                params=dict(DEFAULTS, **params))


def _fitted_case(name, type_count, model, B, max_obj, n_obj, seed, miss=0.0, drawn=None, **params):
    """A scene of the pose stage with `drawn` objects per frame in the table (default n_obj) of which n_obj are live: rows past n_obj hold
    finite objects that must not influence any output (the kernel may load them; it never uses them)."""
    tab, _ = pc.scene(type_count, model, B, max_obj, n_obj if drawn is None else drawn, seed=seed, miss=miss)
    pose, assignment = fitted(tab, n_obj if drawn is None else drawn, model, type_count)
    return _case(name, tab, pose, assignment, n_obj, model, **params)


# rows 0 .. 2 lie on the x axis (the SINGULAR object uses only those), row 3 off it; refine takes the model as it is
CRAFTED_MODEL = np.array([[0.0, 0.0, 0.0], [0.125, 0.0, 0.0], [-0.125, 0.0, 0.0], [0.03, 0.09, 0.05]])
# the first seed of a search over far starts (`python tests/refine_cases.py --search`) whose single undamped step raises the cost in the
# specification: the start is a metre and a half too deep and 106 degrees off, J goes from 1.9e4 to 3.4e4 with every point in front
REJECTED_SEED = 1000


def far_start(seed, R):
    rng = np.random.default_rng(seed)
    dR, _ = perturbation(rng, rng.uniform(0.5, 3.1), 0.0)
    return dR @ R, np.array([rng.uniform(-0.6, 0.6), rng.uniform(-0.6, 0.6), rng.uniform(0.12, 3.0)])


def crafted():
    """One object per status, built directly: B = 1, max_obj = 8, S = 4.  Object 0 is a good one (status 0)."""
    rng = np.random.default_rng(40)
    model, S = CRAFTED_MODEL, 4
    tab = np.full((1, 8, S, 4), np.nan)
    pose = np.full((1, 8, 12), np.nan)
    assignment = np.full((1, 8, S), -1, dtype=np.int32)

    def place(o, R, t, start_R=None, start_t=None):
        tab[0, o] = np.concatenate([model @ R.T + t, np.full((S, 1), 0.8)], axis=1)
        assignment[0, o] = np.arange(S)
        dR, dt = perturbation(rng, 0.05, 0.03)
        pose[0, o] = np.concatenate([dR @ R if start_R is None else start_R, (t + dt if start_t is None else start_t)[:, None]], axis=1).reshape(12)

    R, t = pc.rotation(rng), np.array([0.1, -0.2, 1.0])
    place(0, R, t)                                                     # good: status 0
    place(1, R, t)
    pose[0, 1, 5] = np.nan                                             # a NaN in the pose: SKIPPED
    place(2, R, t)
    tab[0, 2, 2, :3] = [0.3, 0.1, 0.0]                                 # a pair with Z = 0: SKIPPED
    place(3, R, t)
    assignment[0, 3, [0, 2]] = -1                                      # two pairs: SKIPPED
    # three model points on the x axis under R = I: a rotation about the axis moves nothing and H[0][0] is exactly 0: SINGULAR
    place(4, np.eye(3), np.array([0.0, 0.0, 1.0]), start_R=np.eye(3), start_t=np.array([0.0, 0.0, 1.0]))
    assignment[0, 4, 3] = -1
    place(5, R, t, start_R=R, start_t=np.array([0.1, -0.2, 0.02]))     # the start puts model points behind the camera: BEHIND
    # a start far off, one undamped step: the cost goes up: REJECTED
    Rs, ts = far_start(REJECTED_SEED, R)
    place(6, R, t, start_R=Rs, start_t=ts)
    pose[0, 7] = np.arange(12.0)                                       # beyond n_obj: finite garbage that is not read
    tab[0, 7] = 1.0
    assignment[0, 7] = np.arange(S)
    return tab, pose, assignment


def cases():
    out = []
    cups, valve = pc.generic_model(pc.CUPS, 2), pc.generic_model(pc.VALVE, 1)
    out.append(_fitted_case("b1_obj1_S4", pc.CUPS, cups, 1, 1, [1], seed=50))
    # more than one workgroup of objects, a stream with none, live rows short of the table (finite objects past n_obj), empty slots
    out.append(_fitted_case("b3_obj64_n_0_5_64", pc.VALVE, valve, 3, 64, [0, 5, 64], seed=51, miss=0.25, drawn=[3, 9, 64]))
    wide = [1] * 15
    m16 = pc.generic_model(wide, 3, scale=0.2)
    out.append(_fitted_case("S16_full_iters16", wide, m16, 2, 3, [3, 2], seed=52, iters=16))
    out.append(_fitted_case("S16_iters1_mu0", wide, m16, 1, 5, [5], seed=53, miss=0.2, iters=1, damping=0.0))
    # exactly three pairs: the cups table with one slot emptied
    c = _fitted_case("three_pairs", pc.CUPS, cups, 2, 4, [4, 3], seed=54)
    for b in range(2):
        for o in range(4):
            c["tab"][b, o, (b + o) % 4] = np.nan
    c["pose"], c["assignment"] = fitted(c["tab"], [4, 3], cups, pc.CUPS)
    out.append(c)
    out.append(_fitted_case("no_depth_term", pc.VALVE, valve, 2, 6, [6, 4], seed=55, sigma_z=np.inf))
    out.append(_fitted_case("mu0_holes", pc.VALVE, valve, 2, 6, [5, 6], seed=56, miss=0.3, damping=0.0))
    tab, _ = depth_noise_scene(valve, 8, seed=57)
    pose, assignment = fitted(tab, [8], valve, pc.VALVE)
    out.append(_case("depth_noise", tab, pose, assignment, [8], valve))
    return out


def crafted_case():
    tab, pose, assignment = crafted()
    return dict(name="crafted_statuses", tab=tab, pose=pose, assignment=assignment, n_obj=np.array([7], dtype=np.int32), model=CRAFTED_MODEL, fx=FX, fy=FY,
                kind="crafted", params=dict(DEFAULTS, iters=1, damping=0.0), want=[0, 1, 1, 1, 2, 4, 8, 1])


if __name__ == "__main__":
    import sys

    import refine_spec as spec
    if "--search" in sys.argv:
        R, t = pc.rotation(np.random.default_rng(40)), np.array([0.1, -0.2, 1.0])
        tab_o = np.concatenate([CRAFTED_MODEL @ R.T + t, np.full((4, 1), 0.8)], axis=1)
        for seed in range(1000, 1020):
            Rs, ts = far_start(seed, R)
            d = {}
            status = spec.refine_object(tab_o, np.concatenate([Rs, ts[:, None]], axis=1).reshape(12), np.arange(4), CRAFTED_MODEL, FX, FY, 0.25, 0.05, 1, 0.0, diag=d)[3]
            print(seed, status, d["J_initial"], d["J_final"], d["min_qz"], d["pivot"])
