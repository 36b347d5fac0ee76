"""The inputs of test_gpu_triangulation_rigs.py, pinned on the CPU (triangulation_cases.py): what makes a comparison of the triangulation
kernels with the oracle mean something is the degree of the Hartley-Sturm polynomial, the size of f1 and the separation of the candidate
costs, and a later change of seed or rig must not be able to empty them unnoticed.  Every condition holds for EVERY pair of every batch:
no GPU test excludes a pair.

Measured on the family's batches (257 pairs each, 0.5 px noise):
  rig             degrees      waves of mixed degree   max |f1|   min cost gap   nearest epipole (px, left / right)
  zed             3            0                       5.5e-6     2.9e9          1.8e5 / 7.5e5
  verged12        4            0                       1.7e-4     3.0e4          6.0e3 / 6.4e3
  verged35        5            0                       5.0e-4     4.8e-3         2.0e3 / 1.7e3
  forward         5, 6         31                      0.52       1.1e-3         1.92 / 1.03
  vertical        4            0                       3.7e-4     5.6e-2         2.7e3 / 6.6e3
  rolled90        5            0                       4.5e-4     1.5e5          2.2e3 / 2.4e3
  small_forward   6            0                       0.89       2.3e-4         1.12 / 1.27
  small_verged20  5, 6         16                      4.0e-3     2.5e2          252 / 184
Teeth (pairs whose triangulated point moves by more than 1e-5 m when the sign of one term of g(t) is flipped, and the largest move):
  term        zed     forward           small_forward
  g6 r4*w2    0       0                 13   (1.5e-3 m)
  g5 r4*w1    0       0                 42   (2.7e-2 m)
  g4 r4*w0    0       1   (2.4e-5 m)    52   (5.9e-2 m)
  g3 r2*w1    0       5   (2.1e-4 m)    161  (1.8 m)
  g2 r2*w0    0       5   (2.9e-3 m)    171  (4.7 m)
"""
import numpy as np
import pytest

import triangulation_cases as tc
from oracle import geometry as og

DEGREES = {"zed": {3}, "verged12": {4}, "verged35": {5}, "forward": {5, 6}, "vertical": {4}, "rolled90": {5}, "small_forward": {6},
           "small_verged20": {5, 6}}
_CACHE = {}


def _profile(name):
    """(stereo, undistorted left, undistorted right, profile) of the rig's batch, computed once."""
    if name not in _CACHE:
        stereo = tc.oracle_rig(name)
        l, r = tc.undistorted(stereo, *tc.batch(name))
        _CACHE[name] = (stereo, l, r, tc.correction_profile(stereo.F, l, r))
    return _CACHE[name]


def test_small_cameras_undistort_over_the_whole_frame():
    """The 64 x 64 cameras' distortion is one the ten fixed-point steps of fisheye_undistort invert: projecting the undistorted ray gives
    the pixel back, over the whole frame and for both cameras."""
    ys, xs = np.meshgrid(np.arange(64.0), np.arange(64.0), indexing="ij")
    px = np.stack([xs.ravel(), ys.ravel()], axis=1)
    for K, D in ((tc.SMALL["K"], tc.SMALL["D"]), (tc.SMALL["Kp"], tc.SMALL["Dp"])):
        u = og.fisheye_undistort(px, K, D, P=K)
        rays = np.stack([(u[:, 0] - K[0, 2]) / K[0, 0], (u[:, 1] - K[1, 2]) / K[1, 1], np.ones(len(u))], axis=1)
        assert np.abs(og.fisheye_project(rays, K, D) - px).max() < 1e-9


@pytest.mark.parametrize("name", tc.FAMILY)
def test_profile_restates_the_oracle(name):
    """correction_profile writes g(t) out term by term (so that a term can be flipped); unflipped it is correct_matches."""
    stereo, l, r, prof = _profile(name)
    want_l, want_r = og.correct_matches(stereo.F, l, r)
    assert np.abs(prof["left"] - want_l).max() < 1e-9 and np.abs(prof["right"] - want_r).max() < 1e-9      # px; measured 2e-13


def test_the_committed_rig_only_ever_gives_a_cubic():
    assert set(_profile("zed")[3]["degree"].tolist()) == {3}
    assert np.abs(_profile("zed")[3]["f1"]).max() < 1e-5


@pytest.mark.parametrize("name", tc.FAMILY)
def test_degrees_of_every_rig(name):
    assert set(_profile(name)[3]["degree"].tolist()) == DEGREES[name]
    assert set().union(*DEGREES.values()) == {3, 4, 5, 6}


@pytest.mark.parametrize("name", ["forward", "small_verged20"])
def test_waves_of_mixed_degree(name):
    """Eight consecutive pairs are one wave of okp_triangulate_kernel: some waves hold octets of different degree, whose Durand-Kerner
    iterations end at different counts under one wave-wide vote.  The prefixes the GPU test runs (9, 256 pairs) hold such waves too."""
    deg = _profile(name)[3]["degree"]
    mixed = [len(set(deg[i:i + 8].tolist())) > 1 for i in range(0, len(deg), 8)]
    assert sum(mixed) >= 4 and sum(mixed[:32]) >= 4
    assert len(set(deg[:9].tolist())) > 1


def test_small_forward_has_large_f1():
    f1 = np.abs(_profile("small_forward")[3]["f1"])
    assert (f1 > 0.5).sum() >= 3 and (f1[:256] > 0.5).sum() >= 3                       # measured: 9 pairs, up to 0.89


@pytest.mark.parametrize("name", tc.FAMILY)
def test_conditions_on_every_pair(name):
    """Below a relative gap of ~1e-9 between the two lowest candidate costs the oracle's own choice of root is arbitrary; within a pixel
    of an epipole its normalisation divides by nearly nothing.  Neither happens in any batch, and t = infinity never wins."""
    stereo, l, r, prof = _profile(name)
    assert len(l) == tc.BATCH
    assert prof["gap"].min() >= 1e-6
    e_l, e_r = tc.epipoles(stereo.F)
    assert np.linalg.norm(l - e_l, axis=1).min() >= 1.0 and np.linalg.norm(r - e_r, axis=1).min() >= 1.0
    assert not prof["inf_wins"].any()
    h, w = stereo.left_camera.image_size
    pl, pr = tc.batch(name)
    inside = lambda p: ((p > -3) & (p < np.array([w, h]) + 3)).all()                    # (in frame before the noise: within 6 sigma after it)
    assert inside(pl) and inside(pr)


@pytest.mark.parametrize("flip", list(tc.FLIPS))
def test_a_wrong_sign_in_any_f1_term_moves_triangulated_points(flip):
    """Teeth: with the sign of one f1-dependent term of g(t) flipped, at least 3 pairs of some rig's batch triangulate (through the oracle's
    fp32 rounding and DLT) more than 1e-5 m away - ten times the bar of the GPU comparison - while the committed rig does not move at all
    for the terms of g[6], g[5] and g[4]: only the new rigs see them."""
    moved = {}
    for name in ("zed", "forward", "small_forward"):
        stereo, l, r, prof = _profile(name)
        mutated = tc.correction_profile(stereo.F, l, r, flip=flip)
        base = tc.triangulate_corrected(stereo, prof["left"], prof["right"])
        moved[name] = np.linalg.norm(tc.triangulate_corrected(stereo, mutated["left"], mutated["right"]) - base, axis=1)
    assert max(int((moved[name] > 1e-5).sum()) for name in ("forward", "small_forward")) >= 3
    assert int((moved["small_forward"][:256] > 1e-5).sum()) >= 3                        # (the wavefront kernel's 256 pairs see it too)
    if flip in ("g6", "g5", "g4"):
        assert moved["zed"].max() == 0.0


@pytest.mark.parametrize("name", ["small_forward", "small_verged20"])
@pytest.mark.parametrize("cap", [16, 64])
@pytest.mark.parametrize("gate", [1.5, 0.3])
def test_stereo_matching_cases(name, cap, gate):
    """The peak sets of the GPU stereo-matching test: no peak within 1 px of its epipole, no cost at the gate, some left peak without any
    admissible partner, and optima that are unique by more than 1e-6 (measured: at least 2.7e-6, so the device must reproduce the host's
    assignment index for index).  On small_forward both epipoles are inside the frame: all epipolar lines meet at a point in view."""
    stereo = tc.oracle_rig(name)
    e_l, e_r = tc.epipoles(stereo.F)
    if name == "small_forward":
        assert (e_l > 16).all() and (e_l < 48).all() and (e_r > 16).all() and (e_r < 48).all()
    unmatched_rows, unique, kept = 0, 0, 0
    for left, right in tc.match_cases(name, cap, gate):
        assert left.dtype == right.dtype == np.float32 and max(len(left), len(right)) <= cap
        for cam, e, pts in ((stereo.left_camera, e_l, left), (stereo.right_camera, e_r, right)):
            if len(pts):
                assert np.linalg.norm(og.fisheye_undistort(pts, cam.K, cam.D, P=cam.K) - e, axis=1).min() >= 1.0
                assert (pts >= 0).all() and (pts <= 63).all()
        if len(left) and len(right):
            cost = tc.epipolar_cost(stereo, left, right)
            assert not (np.abs(cost - gate) < 1e-9).any()
            unmatched_rows += int((cost > gate).all(axis=1).sum())
            rows, _, margin = tc.assignment_margin(cost, gate)
            unique += margin > 1e-6
            kept += len(rows)
    assert unmatched_rows > 0 and unique == 9 and kept > cap
