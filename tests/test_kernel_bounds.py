"""CPU: the per-element error bounds of tests/kernel_bounds.py are SOUND (a faithful emulation of every kernel family stays inside) and
SENSITIVE (seven planted defects, each far below the max-abs tolerances of tests/test_gpu_conv.py, land outside).

A faithful emulation is what docs/PRECISION.md claims the device does: torch CPU fp32 convolutions on the 16-bit-rounded operands,
rounded with .to(dtype) where the kernel stores.  tests/test_gpu_kernel_bounds.py holds the kernels themselves to the same bounds; this
file is what keeps those bounds from being inflated later - a bound that lets one of the defects through fails here, without a GPU."""
import pytest
import torch
import torch.nn.functional as F

import kernel_bounds as kb
import kernel_bounds_cases as kc

HALF = kc.HALF
NAME = {torch.bfloat16: "bf16", torch.float16: "fp16"}


def rnd(t, dtype):
    return t.to(dtype).float()


def check_inside(ref, emu, what, limit=1.0):
    r, worst, idx = ref.ratio(emu)
    print(f"{what}: max |emu - val| / err = {worst:.3g} at {idx}")
    assert worst <= limit, f"{what}: {int((r > 1).sum())} elements outside the bound, worst {worst:.3g} at {idx}"
    return worst


def count_outside(ref, emu):
    return int((ref.ratio(emu)[0] > 1.0).sum())


# ---- emulations ---------------------------------------------------------------------------------------------------------------------

def emu_conv(x, wt, b, k, stride, dtype, defect=None):
    """relu(conv + bias) rounded once; `defect` plants one of the wrong kernels of the sensitivity tests."""
    pad = (k - 1) // 2
    cin = x.shape[1]
    if defect == "halo":                # frame 1's top halo row holds frame 0's last row instead of zeros
        xp = F.pad(x, (pad, pad, pad, pad))
        xp[1, :, 0, pad:xp.shape[3] - pad] = x[0, :, -1, :]
        y = F.conv2d(xp, wt, None, stride=stride)
    elif defect == "partial16":         # partial sums kept in the 16-bit type across four K chunks
        y = None
        for ch in torch.tensor_split(torch.arange(cin), 4):
            part = F.conv2d(x[:, ch], wt[:, ch], None, stride=stride, padding=pad)
            y = rnd(part if y is None else y + part, dtype)
    else:
        y = F.conv2d(x, wt, None, stride=stride, padding=pad)
    if defect == "ktail":               # the last input channel missing from every tap, in the last output row only
        y[:, :, -1] = F.conv2d(x[:, :-1], wt[:, :-1], None, stride=stride, padding=pad)[:, :, -1]
    bb = b.clone()
    if defect == "bias125":             # the channel with the largest bias: a defect on a bias near zero is none
        bb[int(b.abs().argmax())] *= 1.25
    y = rnd(F.relu(y + bb.view(1, -1, 1, 1)), dtype)
    if defect == "swap":
        c = y.shape[1] // 2
        y = torch.cat([y[:, :c], y[:, c + 1:c + 2], y[:, c:c + 1], y[:, c + 2:]], 1)
    return y


def emu_conv_res(terms, b, res, dtype, relu=True):
    """The implicit-GEMM kernels with a residual: the sum is staged in the output type, then residual, ReLU and a second rounding."""
    y = rnd(sum(terms) + b.view(1, -1, 1, 1), dtype) + res
    return rnd(F.relu(y) if relu else y, dtype)


def emu_fire(x, m, dtype, dw_rounded, defect=None):
    half = m["wa"].shape[0]
    s = rnd(F.conv2d(x, m["w1"], m["b1"]), dtype)
    wd = rnd(m["wd"], dtype) if dw_rounded else m["wd"]
    ya = F.conv2d(s, m["wa"], m["ba"], stride=m["stride"])
    yd = F.conv2d(s, wd, m["bd"], stride=m["stride"], padding=1, groups=half)
    if defect == "dwtap":               # one depth-wise tap missing in one output column
        w0 = wd.clone()
        w0[:, :, 2, 1] = 0.0
        col = yd.shape[3] // 2
        yd[..., col] = F.conv2d(s, w0, m["bd"], stride=m["stride"], padding=1, groups=half)[..., col]
    y = torch.cat([ya, yd], 1)
    if m["skip"]:
        sk = x.clone()
        if defect == "skiprow":         # the skip of column 0 read one row up
            sk[:, :, 1:, 0] = x[:, :, :-1, 0]
        y = y + sk
    return rnd(F.relu(y), dtype)


def emu_heads(c, dtype):
    h1 = rnd(F.relu(F.conv2d(c.x, c.w1, c.b1)), dtype)
    h2 = rnd(F.relu(F.conv2d(h1, c.w2, c.b2)), dtype)
    K = c.K
    offs = [0] * K + [32] * K + [64] * (2 * K - 2)
    outs = [F.conv2d(h2[:, off:off + 32], c.w3[o].view(1, 32, 1, 1), c.b3[o:o + 1]) for o, off in enumerate(offs)]
    return {"heat": torch.sigmoid(torch.cat(outs[:K], 1)), "depth": torch.cat(outs[K:2 * K], 1), "centers": torch.cat(outs[2 * K:], 1)}


# ---- soundness: every family and dtype on its smallest case ----------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", HALF)
def test_emulated_convolutions_stay_inside_the_bound(dtype):
    worst = []
    for shape in kc.CONV_SHAPES:
        c = kc.conv(*shape, dtype)
        worst.append(check_inside(c.ref, emu_conv(c.x, c.wt, c.b, c.k, c.stride, dtype), f"conv {shape} {NAME[dtype]}"))
    c = kc.two_source(3, 32, 16, 2, 64, 2, 10, 12, dtype)
    emu = rnd(F.relu(F.conv2d(c.t, c.w0, c.b, padding=1) + F.conv2d(c.x, c.w1, stride=2)), dtype)
    worst.append(check_inside(c.ref, emu, f"two-source residual block {NAME[dtype]}"))
    c = kc.conv_res(1, 24, 16, 2, 6, 7, dtype, res_channels=32, res_c0=8)
    worst.append(check_inside(c.ref, emu_conv_res([F.conv2d(c.x, c.wt)], c.b, c.r[:, 8:24], dtype), f"1x1 + windowed residual {NAME[dtype]}"))
    c = kc.unpool(16, 2, 5, 7, dtype)
    emu = emu_conv_res([F.conv_transpose2d(c.low, c.wt, None, stride=2, padding=1)], c.b, c.up1, dtype, relu=False)
    worst.append(check_inside(c.ref, emu, f"transposed convolution + merge {NAME[dtype]}"))
    c = kc.conv(3, 1, 256, 256, 1, 16, 16, dtype, seed=21)
    worst.append(check_inside(c.ref, emu_conv(c.x, c.wt, c.b, 3, 1, dtype), f"patch-resident 3x3, 256 channels {NAME[dtype]}"))
    c = kc.stem(1, 37, 45, dtype)
    worst.append(check_inside(c.ref, rnd(F.relu(F.conv2d(c.x, c.wt, c.b, stride=2, padding=3)), dtype), f"stem {NAME[dtype]}"))
    c = kc.depthwise(192, 9, 7, 1, 1, dtype)
    emu = rnd(F.relu(F.conv2d(c.x, c.wt, c.b, padding=1, groups=192) + c.r), dtype)
    worst.append(check_inside(c.ref, emu, f"stand-alone depth-wise {NAME[dtype]}"))
    assert max(worst) > 0.5             # the bound is not slack by construction: a single rounded convolution comes close to it


@pytest.mark.parametrize("dtype", HALF)
@pytest.mark.parametrize("stride,h,w,dw_rounded", [(1, 16, 16, True), (2, 16, 16, True), (1, 7, 5, False)])
def test_emulated_fire_module_stays_inside_the_bound(stride, h, w, dw_rounded, dtype):
    """Matrix-pipe geometries with the depth-wise taps rounded to the activation type, and a vector-ALU geometry with fp32 taps: the bound
    carries the weight-rounding term in both."""
    c = kc.fire2(256, 128, stride, 2, h, w, dtype)
    check_inside(c.ref, emu_fire(c.x, c.mods[0], dtype, dw_rounded), f"fire 256 -> 128 -> 256 stride {stride} {h}x{w} {NAME[dtype]}")


@pytest.mark.parametrize("dtype", HALF)
def test_emulated_resident_chains_stay_inside_the_bound(dtype):
    for what, c in (("512-wide chain 1x1x3 count 3", kc.chain(512, 1, 1, 3, 3, dtype)), ("384-wide chain 3x8x8 count 1", kc.chain(384, 3, 8, 8, 1, dtype)),
                    ("framed chain 2x1x1 count 1", kc.framed_chain(2, 1, 1, 1, dtype))):
        y = c.x
        for m in c.mods:
            y = emu_fire(y, m, dtype, False)
        check_inside(c.ref, y, f"{what} {NAME[dtype]}")


@pytest.mark.parametrize("dtype", HALF)
def test_emulated_heads_stay_inside_the_bound(dtype):
    c = kc.heads(3, 2, 9, 7, dtype)
    emu = emu_heads(c, dtype)
    for name in ("heat", "depth", "centers"):
        check_inside(c.ref[name], emu[name], f"heads {name} {NAME[dtype]}")


# ---- sensitivity: planted defects land outside -----------------------------------------------------------------------------------------

def gpu_conv_tol(dtype, ref):
    """tests/test_gpu_conv.py::_tol restated: the max-abs tolerance the convolution tests use, scaled by the tensor's largest value."""
    return (0.02 if dtype == torch.bfloat16 else 0.003) * (float(ref.abs().max()) + 1.0)


DEFECT_SHAPES = kc.CONV_SHAPES[:3]      # the three shapes with a K worth quartering and more than one frame
DEFECTS = [(d, s) for d in ("partial16", "ktail", "bias125", "swap", "halo") for s in DEFECT_SHAPES if d != "halo" or s[0] == 3]     # (a 1x1 has no halo)


@pytest.mark.parametrize("dtype", HALF)
@pytest.mark.parametrize("defect,shape", DEFECTS)
def test_planted_convolution_defect_lands_outside_the_bound(defect, shape, dtype):
    k, stride, cin, cout, n, h, w = shape
    c = kc.conv(*shape, dtype)
    assert count_outside(c.ref, emu_conv(c.x, c.wt, c.b, k, stride, dtype)) == 0
    bad = emu_conv(c.x, c.wt, c.b, k, stride, dtype, defect)
    outside = count_outside(c.ref, bad)
    print(f"{defect} {shape} {NAME[dtype]}: {outside} elements outside the bound")
    assert outside >= 1
    if defect in ("partial16", "bias125") and dtype == torch.bfloat16:
        # why this file exists: the tolerance of test_conv_matches_torch accepts the same wrong result
        ref32 = F.relu(F.conv2d(c.x, c.wt, c.b, stride=stride, padding=(k - 1) // 2))
        err = float((bad - ref32).abs().max())
        print(f"    max-abs error {err:.4f}, tolerance of test_gpu_conv.py {gpu_conv_tol(dtype, ref32):.4f}")
        assert err <= gpu_conv_tol(dtype, ref32)


@pytest.mark.parametrize("dtype", HALF)
@pytest.mark.parametrize("defect", ["dwtap", "skiprow"])
def test_planted_fire_module_defect_lands_outside_the_bound(defect, dtype):
    c = kc.fire2(256, 128, 1, 2, 16, 16, dtype)
    assert count_outside(c.ref, emu_fire(c.x, c.mods[0], dtype, True)) == 0
    outside = count_outside(c.ref, emu_fire(c.x, c.mods[0], dtype, True, defect))
    print(f"{defect} {NAME[dtype]}: {outside} elements outside the bound")
    assert outside >= 1
