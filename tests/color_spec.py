"""NumPy restatement of the colour correction of okp_preprocess_raw8_color (include/okp.h), independent of the package: black level and
white balance on the mosaic, the demosaic of tests/bayer_spec.py on the balanced mosaic, a Q12 colour matrix and one tone curve of 256
bytes, all in integers.  The end of the file holds the simulation the issue's value statement rests on: a sensor model run backwards on
an sRGB image, which the correction then undoes - a simulation, not a camera."""
import math

import numpy as np

import bayer_spec

# the worked example of the header's specification: a sensor with a black pedestal, a green cast and primaries of its own
EXAMPLE_BLACK = 16
EXAMPLE_GAINS = (1.9, 1.0, 1.6)
EXAMPLE_MATRIX = ((1.6, -0.4, -0.2), (-0.3, 1.5, -0.2), (0.0, -0.6, 1.6))


def q12(x):
    """Numbers -> the integers the kernel takes: x * 4096 rounded."""
    return np.rint(np.asarray(x, np.float64) * 4096.0).astype(np.int64)


def srgb_oetf(x):
    return 12.92 * x if x <= 0.0031308 else 1.055 * math.pow(x, 1.0 / 2.4) - 0.055


def curve(gamma):
    """The tone curve as 256 bytes: floor(255 * f(v / 255) + 0.5); f is the identity (None), the sRGB transfer curve ("srgb") or
    x ** (1 / gamma)."""
    if gamma is None:
        return np.arange(256, dtype=np.uint8)
    f = srgb_oetf if gamma == "srgb" else (lambda x: math.pow(x, 1.0 / gamma))
    return np.array([math.floor(255.0 * f(v / 255.0) + 0.5) for v in range(256)], np.int64).astype(np.uint8)


def balance(samples, black, gain_q12):
    """Stage 1 on samples of one colour: min(255, (max(s - black, 0) * G + 2048) >> 12)."""
    s = np.maximum(np.asarray(samples).astype(np.int64) - int(black), 0)
    return np.minimum(255, (s * np.asarray(gain_q12, np.int64) + 2048) >> 12)


def balance_mosaic(M, pattern, black, gains_q12):
    """Stage 1 on a Bayer mosaic [..., H, W]: every site takes the gain of the colour it samples."""
    h, w = M.shape[-2:]
    g = np.asarray(gains_q12, np.int64)[bayer_spec.colour_index(pattern, h, w)]
    return balance(M, black, g).astype(np.uint8)


def apply_matrix(rgb, matrix_q12):
    """Stage 3 on RGB [..., 3]: clamp8((M_i0 R + M_i1 G + M_i2 B + 2048) >> 12); >> on a signed int64 is the arithmetic (floor) shift."""
    m = np.asarray(matrix_q12, np.int64).reshape(3, 3)
    assert np.abs(m).max() <= 65535
    acc = np.asarray(rgb).astype(np.int64) @ m.T
    return np.clip((acc + 2048) >> 12, 0, 255)


def correct_frames(frames, pattern, black, gains_q12, matrix_q12, curve256):
    """[N, H, W] uint8 frames (pattern: one of bayer_spec.PATTERNS, or "mono") -> the corrected RGB frames [N, H, W, 3] uint8."""
    frames = np.asarray(frames)
    assert frames.dtype == np.uint8 and 0 <= black <= 254 and len(curve256) == 256
    g = np.asarray(gains_q12, np.int64)
    assert g.shape == (3,) and g.min() >= 0 and g.max() <= 65535
    if pattern == "mono":
        rgb = balance(bayer_spec.mono_to_rgb(frames), black, g)          # replicated first: each channel takes its own gain
    else:
        rgb = bayer_spec.demosaic(balance_mosaic(frames, pattern, black, g), pattern)
    out = np.asarray(curve256, np.uint8)[apply_matrix(rgb, matrix_q12)]
    return np.ascontiguousarray(out)


def identity():
    """(black, gains_q12, matrix_q12, curve) of the correction that changes nothing."""
    return 0, q12((1.0, 1.0, 1.0)), q12(np.eye(3)).reshape(-1), curve(None)


def example(gamma="srgb"):
    """(black, gains_q12, matrix_q12, curve) of the worked example."""
    return EXAMPLE_BLACK, q12(EXAMPLE_GAINS), q12(EXAMPLE_MATRIX).reshape(-1), curve(gamma)


# ---- the simulation: an sRGB image seen by the example's sensor ---------------------------------------------------------------------------

def smooth_image(seed=3, size=64, grid=5, lo=30, hi=225):
    """A smooth sRGB image [size, size, 3] uint8: a grid x grid lattice of uniform values in [lo, hi], interpolated bilinearly."""
    knots = np.random.default_rng(seed).uniform(lo, hi, (grid, grid, 3))
    t = np.linspace(0.0, grid - 1.0, size)
    i0 = np.minimum(t.astype(np.int64), grid - 2)
    f = t - i0
    rows = knots[i0] * (1.0 - f)[:, None, None] + knots[i0 + 1] * f[:, None, None]
    img = rows[:, i0] * (1.0 - f)[None, :, None] + rows[:, i0 + 1] * f[None, :, None]
    return np.rint(img).astype(np.uint8)


def sensor_samples(srgb, black=EXAMPLE_BLACK, gains=EXAMPLE_GAINS, matrix=EXAMPLE_MATRIX):
    """What the modelled sensor records of an sRGB image [H, W, 3], per channel, before the colour filter picks one per site: the
    transfer curve undone (linear light), the colour matrix inverted (the sensor's own primaries), the gains divided out (its green
    cast), the black pedestal added, quantised to 8 bits."""
    x = srgb.astype(np.float64) / 255.0
    lin = np.where(x <= 0.04045, x / 12.92, ((x + 0.055) / 1.055) ** 2.4)
    cam = lin @ np.linalg.inv(np.asarray(matrix, np.float64)).T
    return np.clip(np.rint(cam * 255.0 / np.asarray(gains, np.float64) + black), 0, 255).astype(np.uint8)


def simulation(pattern):
    """(mean absolute error of the demosaic alone, of the corrected frames, the corrected frames' worst pixel) against the sRGB image, of 255."""
    img = smooth_image()
    M = bayer_spec.mosaic(sensor_samples(img), pattern)[None]
    plain = bayer_spec.demosaic(M, pattern)[0].astype(np.float64)
    fixed = correct_frames(M, pattern, *example())[0].astype(np.float64)
    return np.abs(plain - img).mean(), np.abs(fixed - img).mean(), np.abs(fixed - img).max()
