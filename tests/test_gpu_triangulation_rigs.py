"""Triangulation and stereo matching on converged, vertical, rolled and forward-displaced rigs (triangulation_cases.py): the Hartley-Sturm
correction at degrees 4, 5 and 6, waves of mixed degree, |f1| up to 0.9 and epipolar lines that meet inside the image - against the oracle
(cv2.correctMatches + cv2.triangulatePoints restated in fp64) and against the host assignment.  The committed calibration gives a cubic
for every pair, so a wrong f1^2 / f1^4 term of g(t) passes every test on it; test_triangulation_cases.py pins on the CPU that these
batches see each of those terms, and that no pair of them has to be excluded."""
import numpy as np
import pytest
import torch

import triangulation_cases as tc

pytestmark = pytest.mark.gpu

_WANT = {}


def _oracle(name):
    """(left, right, oracle points with the correction, without it) of the rig's 257-pair batch; per pair, so a slice serves a prefix."""
    if name not in _WANT:
        pl, pr = tc.batch(name)
        ostereo = tc.oracle_rig(name)
        _WANT[name] = (pl, pr, ostereo.triangulate(pl, pr), ostereo.triangulate(pl, pr, correct=False))
    return _WANT[name]


@pytest.mark.parametrize("m", [9, 256, 257])
@pytest.mark.parametrize("name", tc.FAMILY)
def test_triangulate_agrees_with_the_oracle_on_every_rig(name, m):
    """256 pairs: the last size of the wavefront kernel (an octet per pair); 257: the first of the thread kernel; 9: a last wave with
    seven idle octets.  One bound for every rig - the corrected pixels agree to 4e-12 px on the CPU, no conditioning here comes near it."""
    pl, pr, want, want_plain = _oracle(name)
    pl, pr, want, want_plain = pl[:m], pr[:m], want[:m], want_plain[:m]
    stereo = tc.device_rig(name)
    got = stereo.triangulate(pl, pr)
    got_plain = stereo.triangulate(pl, pr, correct_matches=False)
    print(f"{name} m={m}: corrected {np.abs(got - want).max():.3g} m, uncorrected {np.abs(got_plain - want_plain).max():.3g} m")
    assert got.shape == (m, 3) and np.isfinite(got).all() and np.isfinite(got_plain).all()
    # measured on an MI355X, the larger of the wavefront (256) and the thread (257) kernel, corrected / uncorrected, metres:
    #   zed 4.2e-14 / 4.8e-14    verged12 2.2e-14 / 3.8e-14    verged35 1.6e-14 / 2.6e-14    forward 7.3e-14 / 7.6e-14
    #   vertical 4.5e-14 / 4.0e-14    rolled90 6.0e-14 / 4.4e-14    small_forward 2.1e-12 / 4.0e-12    small_verged20 2.8e-14 / 3.9e-14
    # (small_forward: a 25 cm forward baseline seen through 42 px of focal length - the DLT itself is that much worse conditioned.)
    # With the sign of the g[6] term flipped in both kernels: 1.47e-3 m on small_forward at 256 and at 257 pairs (1.7e-6 m at 9), as the CPU
    # profile predicts (1.5e-3 m); every other rig of this file, and every test on the committed calibration, still passes.
    assert np.abs(got - want).max() < 1e-6
    assert np.abs(got_plain - want_plain).max() < 1e-6
    assert np.array_equal(stereo.triangulate(pl, pr), got)                     # run to run, bit for bit
    assert np.array_equal(stereo.triangulate(pl, pr, correct_matches=False), got_plain)


def test_wavefront_and_thread_kernels_agree_at_degree_six():
    """The octet kernel steps all six roots from the previous iterate (Jacobi order), the thread kernel uses each new root at once
    (Gauss-Seidel order): different iterates, the same roots.  The first 256 pairs of small_forward through the one, and as part of the
    257 through the other."""
    pl, pr, _, _ = _oracle("small_forward")
    stereo = tc.device_rig("small_forward")
    oct256, thread257 = stereo.triangulate(pl[:256], pr[:256]), stereo.triangulate(pl, pr)
    diff = np.abs(oct256 - thread257[:256]).max()
    print(f"octet against thread kernel at degree 6: {diff:.3g} m")
    assert diff < 1e-9                                                          # measured 5.9e-13 m


# ---- the stereo tick's triangulation (okp_stereo_triangulate / _rig) on a three-entry table --------------------------------------------
TABLE = ("zed64", "small_forward", "small_verged20")
K_TYPES, CAP = 3, 5                              # 15 slots per pair: two waves, the second with one live octet
COUNTS = [(0, 4), (5, 5), (3, 0), (1, 1), (4, 2), (2, 5), (5, 3), (3, 4), (4, 5)]      # (left, right) peaks per (pair, type): 0 and cap included


def _tick():
    """count [6, 3], xyc [6, 3, 5, 3], match [3, 3, 5] of a tick over the table's three pairs: per (pair, type) max(min(n, m) - 1, 1) views
    of common 3D points (0.4 px noise on the right one, none within 1 px of an epipole) at shuffled slots of both sides, matched to each
    other; the other peaks are clutter and stay unmatched (-1)."""
    rng = np.random.default_rng(17)
    P = len(TABLE)
    count = np.zeros((2 * P, K_TYPES), np.int32)
    xyc = np.zeros((2 * P, K_TYPES, CAP, 3), np.float32)
    match = np.full((P, K_TYPES, CAP), -1, np.int32)
    for c, (n, m) in enumerate(COUNTS):
        p, k = divmod(c, K_TYPES)
        ostereo = tc.oracle_rig(TABLE[p])
        t = max(min(n, m) - 1, 1) if n and m else 0
        _, pl, pr = tc.visible_points(ostereo, rng, t) if t else (None, np.zeros((0, 2)), np.zeros((0, 2)))
        pr = pr + rng.normal(0, 0.4, pr.shape)
        left = np.concatenate([pl, rng.uniform(5, 58, (n - t, 2))]).astype(np.float32)
        right = np.concatenate([pr, rng.uniform(5, 58, (m - t, 2))]).astype(np.float32)
        if t:
            ul, ur = tc.undistorted(ostereo, left[:t], right[:t])
            e_l, e_r = tc.epipoles(ostereo.F)
            assert np.linalg.norm(ul - e_l, axis=1).min() >= 1.0 and np.linalg.norm(ur - e_r, axis=1).min() >= 1.0
        at_l, at_r = rng.permutation(n), rng.permutation(m)                     # peak q of the lists above sits at slot at[q]
        count[2 * p, k], count[2 * p + 1, k] = n, m
        xyc[2 * p, k, at_l, :2], xyc[2 * p + 1, k, at_r, :2] = left, right
        xyc[2 * p, k, :n, 2], xyc[2 * p + 1, k, :m, 2] = rng.uniform(0.3, 1.0, n), rng.uniform(0.3, 1.0, m)
        match[p, k, at_l[:t]] = at_r[:t]
    return count, xyc, match


def _bits(x, y):
    assert x.shape == y.shape and torch.equal(x.isnan(), y.isnan()) and torch.equal(torch.nan_to_num(x, nan=0.0), torch.nan_to_num(y, nan=0.0))


@pytest.mark.parametrize("correct", [True, False])
def test_stereo_triangulate_on_a_table_of_different_rigs(correct):
    """okp_stereo_triangulate_rig on a tick whose three pairs are three different rigs (a cubic, sextics, mixed quintics and sextics), every
    (pair, type) with its own peak counts: the matched slots carry the bits of okp_triangulate_dlt on the same peaks - both kernels inline
    one per-pair function, compiled without contraction so that they round alike; before that they were 3e-15 m apart - and lie within
    1e-6 m of the oracle; the unmatched slots are NaN rows; the by-value entry point and a first_pair offset give the same bits."""
    from object_keypoints_amd import ops
    dev = torch.device("cuda", 0)
    count, xyc, match = _tick()
    rigs = [tc.device_rig(name) for name in TABLE]
    table = ops.stereo_rig(rigs).to(dev)
    count_d, xyc_d, match_d = torch.from_numpy(count).to(dev), torch.from_numpy(xyc).to(dev), torch.from_numpy(match).to(dev)
    pts_d = ops.stereo_triangulate_rig(table, count_d, xyc_d, match_d, correct_matches=correct)
    pts = pts_d.cpu().numpy()
    assert pts.shape == (3, K_TYPES, CAP, 4)
    assert np.array_equal(np.isnan(pts).any(axis=3), match < 0) and np.array_equal(np.isnan(pts).all(axis=3), match < 0)    # NaN rows exactly on the unmatched slots
    assert (match >= 0).sum() >= 12 and ((match >= 0).sum(axis=2) > 0).sum() == 7
    worst = 0.0
    for p, name in enumerate(TABLE):
        st = rigs[p]
        cl, cr = ops.make_camera(st.left_camera.K, st.left_camera.D), ops.make_camera(st.right_camera.K, st.right_camera.D)
        F = st.F if correct else None
        # the by-value entry point on this pair alone, and the rig form on the pairs from p on with first_pair = p: the same bits
        _bits(ops.stereo_triangulate(cl, cr, st.T_RL, count_d[2 * p:2 * p + 2], xyc_d[2 * p:2 * p + 2], match_d[p:p + 1], F=F), pts_d[p:p + 1])
        _bits(ops.stereo_triangulate_rig(table, count_d[2 * p:], xyc_d[2 * p:], match_d[p:], first_pair=p, correct_matches=correct), pts_d[p:])
        slots = [(k, i, int(match[p, k, i])) for k in range(K_TYPES) for i in range(CAP) if match[p, k, i] >= 0]
        li = np.stack([xyc[2 * p, k, i, :2] for k, i, _ in slots])
        ri = np.stack([xyc[2 * p + 1, k, j, :2] for k, _, j in slots])
        dlt = ops.triangulate_dlt(cl, cr, st.T_RL, torch.from_numpy(li).to(dev), torch.from_numpy(ri).to(dev), F=F).cpu().numpy()
        want = tc.oracle_rig(name).triangulate(li, ri, correct=correct)
        print(f"{name} correct={correct}: stereo_triangulate_rig - triangulate_dlt {np.abs(np.stack([pts[p, k, i, :3] for k, i, _ in slots]) - dlt).max():.3g} m")
        for (k, i, _), X, W in zip(slots, dlt, want):
            assert np.array_equal(pts[p, k, i, :3], X)                          # the per-pair code of okp_triangulate_dlt: the same bits
            assert pts[p, k, i, 3] == np.float64(xyc[2 * p, k, i, 2])
            worst = max(worst, float(np.abs(pts[p, k, i, :3] - W).max()))
    print(f"stereo_triangulate_rig against the oracle, correct={correct}: {worst:.3g} m")
    assert worst < 1e-6                                                         # measured 9.6e-15 m with the correction, 2.1e-14 m without


# ---- okp_stereo_match with the epipole in or next to the image ---------------------------------------------------------------------------
def _tick_tensors(cases, K, cap):
    P = (len(cases) + K - 1) // K
    count = np.zeros((2 * P, K), np.int32)
    xyc = np.zeros((2 * P, K, cap, 3), np.float32)
    rng = np.random.default_rng(5)
    for c, sides in enumerate(cases):
        p, k = divmod(c, K)
        for s, pts in enumerate(sides):
            count[2 * p + s, k] = len(pts)
            xyc[2 * p + s, k, :len(pts), :2] = pts
            xyc[2 * p + s, k, :len(pts), 2] = rng.uniform(0.3, 1.0, len(pts))
    return P, count, xyc


@pytest.mark.parametrize("cap", [16, 64])
@pytest.mark.parametrize("gate", [1.5, 0.3])
@pytest.mark.parametrize("name", ["small_forward", "small_verged20"])
def test_stereo_match_with_the_epipole_near_the_peaks(name, cap, gate):
    """small_forward: both epipoles inside the 64 x 64 frame, every epipolar line passes through a point in view and |l[0:2]| is small for
    the peaks next to it; small_verged20: strongly converging lines.  Against AssociationComponent (scipy's linear_sum_assignment on the
    gated fp64 cost): the optimum's size and summed cost always, the assignment itself where the CPU shows the optimum unique by more than
    1e-6 (every case: test_stereo_matching_cases)."""
    from object_keypoints_amd import ops
    from object_keypoints_amd.perception.pipeline import AssociationComponent
    stereo, ostereo = tc.device_rig(name), tc.oracle_rig(name)
    assoc = AssociationComponent(max_distance=gate)
    assoc.reset(stereo)
    cases = tc.match_cases(name, cap, gate)
    K = 3
    P, count, xyc = _tick_tensors(cases, K, cap)
    dev = torch.device("cuda", 0)
    match, overflow = ops.stereo_match(stereo.left_camera.okp(), stereo.right_camera.okp(), stereo.F, torch.from_numpy(count).to(dev),
                                       torch.from_numpy(xyc).to(dev), gate)
    match = match.cpu().numpy()
    assert int(overflow) == 0
    unmatched_rows = unique = 0
    for c, (left, right) in enumerate(cases):
        got = match[c // K, c % K]
        assert (got[len(left):] == -1).all()
        want = assoc(left.astype(np.float64), right.astype(np.float64))
        if not (len(left) and len(right)):
            assert (got == -1).all()
            continue
        cost = assoc.cost(left.astype(np.float64), right.astype(np.float64))
        assert not (np.abs(cost - gate) < 1e-9).any()                           # (no cost at the gate: the comparison is exact)
        unmatched_rows += int((cost > gate).all(axis=1).sum())
        got = got[:len(left)]
        sel = np.nonzero(got >= 0)[0]
        assert (got[sel] < len(right)).all() and len(set(got[sel].tolist())) == len(sel)       # one-to-one
        assert (cost[sel, got[sel]] <= gate).all()
        assert len(sel) == int((want >= 0).sum())
        assert abs(cost[sel, got[sel]].sum() - cost[want >= 0, want[want >= 0]].sum()) <= 1e-9 * max(len(sel), 1)
        if tc.assignment_margin(tc.epipolar_cost(ostereo, left, right), gate)[2] > 1e-6:
            unique += 1
            assert np.array_equal(got, want), (c, len(left), len(right))
    assert unmatched_rows > 0 and unique == 9
