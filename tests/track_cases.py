"""Fabricated tick sequences for okp_track_objects (tests/test_track_args.py asserts their conditions on the CPU, tests/test_gpu_track.py runs
them on the device).  Every case is at most 8 ticks; a tick is the pose stage's output (tab, pose, status, n_obj) built from a list of objects
per stream: (centre z, rotation R, kind) with kind "full" (status 0, pose [R | z - R m0]), "few" (status OKP_POSE_FEW, NaN pose, filled centre
slot z), "poor" (status OKP_POSE_POOR, finite pose, filled centre slot) or "none" (NaN pose, empty centre slot).

Conditions, by case["kind"]:
  "margin"  every gate decision, every order decision of step 3 between candidates that share a track or a measurement, and the s <= 1e-9
            branch have a relative margin of at least MARGIN = 1e-6 in the spec at every tick.
  "tie"     exact ties on purpose: every coordinate and the model's centre are multiples of 1/8 below 64, R = I, alpha = 1, beta = 0 (so v = 0
            and every c is again such a multiple): p, z - p and d2 are exact in fp64 on both sides, whatever the order of the operations.
"""
import numpy as np

MARGIN = 1e-6
FEW, POOR = 1, 4                                  # include/okp.h OKP_POSE_FEW / OKP_POSE_POOR
MODEL = np.array([[0.5, 0.25, 0.125], [0.6, 0.25, 0.125], [0.45, 0.35, 0.125], [0.45, 0.15, 0.125]])      # S = 4; row 0 = the centre m0
I3 = np.eye(3)


def rot(axis, angle):
    """Rodrigues' rotation about `axis` by `angle` radians."""
    u = np.asarray(axis, dtype=np.float64)
    u = u / np.linalg.norm(u)
    K = np.array([[0.0, -u[2], u[1]], [u[2], 0.0, -u[0]], [-u[1], u[0], 0.0]])
    return np.eye(3) + np.sin(angle) * K + (1.0 - np.cos(angle)) * (K @ K)


def cfg(gate=0.5, dt=0.125, alpha=1.0, beta=0.0, alpha_R=1.0, min_hits=2, max_misses=5):
    return dict(gate=gate, dt=dt, alpha=alpha, beta=beta, alpha_R=alpha_R, min_hits=min_hits, max_misses=max_misses)


def tick(streams, max_obj, model=MODEL, garbage=None):
    """streams: list over b of lists of (z, R, kind) -> dict(tab [B,max_obj,S,4], pose [B,max_obj,12], status [B,max_obj], n_obj [B]).
    garbage: a list of (z, R) written as finite full objects into the rows from n_obj[b] on (never measurements)."""
    B, S = len(streams), model.shape[0]
    tab = np.full((B, max_obj, S, 4), np.nan)
    pose = np.full((B, max_obj, 12), np.nan)
    status = np.zeros((B, max_obj), dtype=np.int32)
    n_obj = np.array([len(s) for s in streams], dtype=np.int32)

    def put(b, o, z, R, kind):
        z = np.asarray(z, dtype=np.float64)
        if kind in ("full", "poor"):
            pose[b, o] = np.concatenate([R, (z - R @ model[0])[:, None]], axis=1).reshape(12)
            status[b, o] = POOR if kind == "poor" else 0
        if kind == "few":
            status[b, o] = FEW
        if kind != "none":
            tab[b, o, 0] = (z[0], z[1], z[2], 1.0)

    for b, objs in enumerate(streams):
        assert len(objs) <= max_obj
        for o, (z, R, kind) in enumerate(objs):
            put(b, o, z, R, kind)
        for j, (z, R) in enumerate(garbage or []):
            if len(objs) + j < max_obj:
                put(b, len(objs) + j, z, R, "full")
    return dict(tab=tab, pose=pose, status=status, n_obj=n_obj)


def _case(name, kind, T, max_obj, config, ticks, **more):
    assert len(ticks) <= 8
    return dict(name=name, kind=kind, T=T, max_obj=max_obj, cfg=config, ticks=ticks, model=MODEL, **more)


def _full(z, R=I3):
    return (z, R, "full")


def lifecycle():
    """T = 1, max_obj = 1, max_misses = 2: birth, update, two coasting ticks, death on the third miss, rebirth with id 2 in slot 0."""
    R = rot([1, 2, 3], 0.4)
    seen = lambda x: [[_full((x, 0.2, 1.5), R)]]
    ticks = [tick(seen(0.0), 1), tick(seen(0.1), 1), tick([[]], 1), tick([[]], 1), tick([[]], 1), tick(seen(0.55), 1), tick(seen(0.6), 1)]
    return _case("lifecycle", "margin", 1, 1, cfg(alpha=0.6, beta=0.3, max_misses=2), ticks)


def tie_two_tracks():
    """Two tracks equidistant from one measurement (d2 = 1/4 both): the lower slot takes it, the other coasts."""
    ticks = [tick([[_full((0.0, 1.0, 2.0)), _full((1.0, 1.0, 2.0))]], 2), tick([[_full((0.5, 1.0, 2.0))]], 2)]
    return _case("tie_two_tracks", "tie", 2, 2, cfg(gate=1.0), ticks)


def tie_two_measurements():
    """One track equidistant from two measurements: the lower object index updates it, the other founds a track."""
    ticks = [tick([[_full((0.0, 1.0, 2.0))]], 2), tick([[_full((-0.5, 1.0, 2.0)), _full((0.5, 1.0, 2.0))]], 2)]
    return _case("tie_two_measurements", "tie", 3, 2, cfg(gate=1.0), ticks)


def crossing():
    """Tracks at x = 0 and x = 1, measurements at x = 0.7 and x = 1.6, gate 1: nearest-first gives (track 1, object 0) and leaves track 0
    without a candidate (object 1 is outside its gate) - per-track nearest in slot order would give (0, 0) and (1, 1)."""
    ticks = [tick([[_full((0.0, 0.0, 2.0)), _full((1.0, 0.0, 2.0))]], 2), tick([[_full((0.7, 0.0, 2.0)), _full((1.6, 0.0, 2.0))]], 2)]
    return _case("crossing", "margin", 4, 2, cfg(gate=1.0, alpha=0.5), ticks)


def _grid(n, shift=0.0, order=None):
    pts = [((i % 8) * 1.0 + shift, (i // 8) * 1.0 - shift, 3.0) for i in range(n)]
    return [pts[i] for i in (order if order is not None else range(n))]


def all_lanes():
    """T = 64 and max_obj = 64: 64 births, then all 64 matched from a permuted object order, with rotations blended."""
    order = np.random.default_rng(3).permutation(64)
    R0, R1 = rot([0, 0, 1], 0.2), rot([0, 1, 0], 0.3)
    ticks = [tick([[_full(z, R0) for z in _grid(64)]], 64), tick([[_full(z, R1) for z in _grid(64, 0.05, order)]], 64),
             tick([[_full(z, R1) for z in _grid(64, 0.11)]], 64)]
    return _case("all_lanes", "margin", 64, 64, cfg(gate=0.3, alpha=0.5, beta=0.25, alpha_R=0.5), ticks, order=order)


def full_house():
    """T = 64 full; then 63 objects match and one appears far from everything: no free slot - bit 8, track_of = -1, nothing else disturbed."""
    second = [_full(z) for z in _grid(64, 0.05)]
    second[17] = _full((20.0, 20.0, 3.0))
    ticks = [tick([[_full(z) for z in _grid(64)]], 64), tick([second], 64)]
    return _case("full_house", "margin", 64, 64, cfg(gate=0.3), ticks)


def death_and_births():
    """T = 3, max_misses = 0: slots 0 and 1 live; then slot 0 is not seen (it dies in this call) and two new objects arrive: slot 0 takes
    the first (id 3), slot 2 the second (id 4)."""
    ticks = [tick([[_full((0.0, 0.0, 2.0)), _full((2.0, 0.0, 2.0))]], 4),
             tick([[_full((5.0, 1.0, 2.0)), _full((2.1, 0.0, 2.0)), _full((7.0, 1.0, 2.0))]], 4)]
    return _case("death_and_births", "margin", 3, 4, cfg(max_misses=0), ticks)


def position_only():
    """A track founded by a full measurement, then updated by a OKP_POSE_FEW object with a filled centre slot (c moves, R keeps its bits),
    while an unmatched position-only object founds nothing; then a OKP_POSE_POOR object (finite pose, another rotation) is position-only too."""
    R = rot([3, 1, 2], 0.7)
    ticks = [tick([[_full((0.0, 0.0, 2.0), R)]], 3),
             tick([[((4.0, 0.0, 2.0), None, "few"), ((0.1, 0.05, 2.0), None, "few"), ((8.0, 0.0, 2.0), None, "none")]], 3),
             tick([[((0.2, 0.1, 2.0), rot([1, 0, 0], 1.0), "poor")]], 3)]
    return _case("position_only", "margin", 4, 3, cfg(alpha=0.5, beta=0.2, alpha_R=0.5), ticks)


def rotations(alpha_R):
    """R = I, then a quarter turn about z (an exact matrix of 0 and +-1), standing still: alpha_R = 1 copies the bits; alpha_R = 0.5 gives the
    eighth turn about the same axis."""
    z = (0.3, -0.2, 1.7)
    quarter = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    ticks = [tick([[_full(z, I3)]], 2), tick([[_full(z, quarter)]], 2)]
    return _case(f"rotation_alpha_R_{alpha_R:g}", "margin", 2, 2, cfg(alpha_R=alpha_R), ticks)


def same_rotation():
    """alpha_R = 0.5 and identical rotations: s = 0 exactly, the s <= 1e-9 branch copies R_meas."""
    R = rot([1, 1, 0], 0.9)
    ticks = [tick([[_full((0.3, -0.2, 1.7), R)]], 2), tick([[_full((0.31, -0.2, 1.7), R)]], 2)]
    return _case("same_rotation", "margin", 2, 2, cfg(alpha_R=0.5), ticks)


def garbage_rows():
    """Finite, plausible objects in the rows from n_obj on - one of them right on a track - are never measurements."""
    junk = [((0.0, 0.0, 2.0), I3), ((3.0, 3.0, 2.0), I3)]
    ticks = [tick([[_full((0.0, 0.0, 2.0))]], 4, garbage=junk), tick([[]], 4, garbage=junk), tick([[_full((0.05, 0.0, 2.0))]], 4, garbage=junk)]
    clean = [tick([[_full((0.0, 0.0, 2.0))]], 4), tick([[]], 4), tick([[_full((0.05, 0.0, 2.0))]], 4)]
    return _case("garbage_rows", "margin", 4, 4, cfg(), ticks, clean=clean)


def three_streams():
    """B = 3: streams with 2, 0..1 and 3 objects moving at their own constant velocities, one of them missed for a tick."""
    R = [rot([0, 0, 1], 0.1 * k) for k in range(8)]
    ticks = []
    for t in range(5):
        a = [_full((0.1 * t, 0.0, 2.0), R[t]), _full((3.0, 0.2 * t, 2.5), R[t + 1])]
        b = [] if t in (0, 3) else [_full((1.0 - 0.05 * t, 1.0, 1.5), R[2])]
        c = [_full((-2.0, 0.0, 2.0 + 0.1 * t), R[t]), _full((0.0, -2.0 + 0.15 * t, 2.0), R[3]), _full((2.0, 2.0, 2.0), R[t + 2])]
        if t == 2:
            c = c[::-1]
        ticks.append(tick([a, b, c], 4))
    return _case("three_streams", "margin", 4, 4, cfg(alpha=0.7, beta=0.4, alpha_R=0.5), ticks)


def constant_velocity():
    """One target at 0.4 m/s along x for 8 ticks with beta > 0 (the spec's property: predicted better at tick 8 than at tick 2)."""
    ticks = [tick([[_full((0.05 * t, 0.0, 2.0))]], 1) for t in range(8)]
    return _case("constant_velocity", "margin", 1, 1, cfg(alpha=0.5, beta=0.3), ticks, step=0.05)


def cases():
    return [lifecycle(), tie_two_tracks(), tie_two_measurements(), crossing(), all_lanes(), full_house(), death_and_births(), position_only(),
            rotations(1.0), rotations(0.5), same_rotation(), garbage_rows(), three_streams(), constant_velocity()]
