"""The split-product kernels (ops.F32X3: fp32 tensors, every product as x_hi w_hi + x_lo w_hi + x_hi w_lo on the fp16 matrix pipe) and the
exact-fp32 plans, bit for bit, on exactly summable operands (tests/exact_operands.py, docs/PRECISION.md "Exact operands").

The kernels round nowhere but in their fp32 accumulator; on the lattice of tests/exact_operands_cases.py every term and every partial sum is an
fp32 number, so no summation order, MFMA shape or tile may change a bit of the result: torch.equal against the three-term sum computed in
fp64, through the public entry points, outputs pre-filled with NaN.  A failure names the first differing (n, c, y, x) with both values in hex."""
import pytest
import torch

import exact_operands as eo
import exact_operands_cases as ec

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _stop_at_a_device_fault():
    """A launch that faulted leaves the device unusable for this process: end the session there instead of reporting every later test."""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"device fault: {e}", returncode=3)


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def nan_act(n, h, w, c, dtype=torch.float32):
    """An output the kernel has to write completely: what it leaves out stays NaN."""
    from object_keypoints_amd import ops
    return ops.Act(torch.full((n, h, w, c), float("nan"), dtype=dtype, device=_dev()))


def act(x, window=False, dtype=torch.float32):
    """fp64 NCHW on the CPU -> NHWC activation on the device (exact on the lattice).  window: as channels [8, 8 + C) of a tensor of C + 16
    channels whose other channels hold finite junk (pix_stride > cin)."""
    from object_keypoints_amd import ops
    assert torch.equal(x.to(dtype).double(), x)
    t = x.permute(0, 2, 3, 1).contiguous().to(dtype)
    if not window:
        return ops.Act(t.to(_dev()))
    big = torch.full(tuple(t.shape[:3]) + (t.shape[3] + 16,), 1.5, dtype=dtype)
    big[..., 8:8 + t.shape[3]] = t
    return ops.Act(big.to(_dev())).slice(8, t.shape[3])


def assert_bits(got, want, what):
    diff = eo.first_difference(got.detach().cpu(), want)
    assert diff is None, f"{what}: {diff} [(n, c, y, x)]"


class flagged:
    """Plans built inside are split-product plans; with a range flag attached if asked (okp_conv_set_range_flag), which must stay 0."""

    def __init__(self, flag, split=True):
        self.flag = torch.zeros(1, dtype=torch.int32, device=_dev()) if flag else None
        self.split = split

    def __enter__(self):
        from object_keypoints_amd import ops
        self.ctx = ops.f32_split(self.split, False, self.flag)
        self.ctx.__enter__()
        return self

    def __exit__(self, *exc):
        self.ctx.__exit__(*exc)

    def clear(self, what):
        if self.flag is not None:
            torch.cuda.synchronize()
            assert int(self.flag) == 0, f"{what}: the fp16 range flag was raised on operands far inside the range"


def build_plan(c, flag=False, split=True):
    from object_keypoints_amd import ops
    from object_keypoints_amd.perception.backbone import conv_taps
    taps, terms = [], []
    for i, (d, w) in enumerate(zip(c.srcs, c.ws)):
        assert torch.equal(w.float().double(), w)
        t = conv_taps(w.float().numpy(), src=i)
        taps += t
        terms += [d["terms"]] * len(t)
    with flagged(flag, split) as g:
        plan = ops.ConvPlan(torch.float32, [d["cin"] for d in c.srcs], [d["stride"] for d in c.srcs], c.cout, taps,
                            c.bias.float().numpy() if c.bias is not None else None, relu=c.relu, tap_terms=terms if any(t != 3 for t in terms) else None)
    assert plan.split == split
    return plan, g


def run_plan(c, plan, tile, window=False, **kw):
    """One launch of the case's plan -> (NCHW result on the CPU, the output activation)."""
    srcs = [act(x, window) for x in c.xs]
    res = None
    if c.res is not None:
        res = act(c.res, window, torch.float16 if c.res16 else torch.float32)
    out = kw.pop("out", None) or nan_act(c.n, c.ho, c.wo, c.cout)
    plan(srcs, out, c.ho, c.wo, res=res, tile=tile, **kw)
    torch.cuda.synchronize()
    return out


# ---- gather tiles of okp_igemm_kernel<F32S> --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("flag", [False, True], ids=["", "range_flag"])
@pytest.mark.parametrize("tile", [1, 2, 3, 4])
@pytest.mark.parametrize("name", [k for k in ec.GATHER if k != "out16_sub2"])
def test_gather_tile_gives_the_three_term_sum_bit_for_bit(name, tile, flag):
    """Single- and two-source plans, stride 1 / 2, 1x1 with a ragged K-slice, single-term taps in front of three-term ones, residual + ReLU,
    subnormal low halves; the two-source case reads its sources and residual through channel windows.  The range flag changes no bit."""
    c = ec.get(name)
    plan, g = build_plan(c, flag)
    out = run_plan(c, plan, tile, window=(name == "two_source"))
    assert_bits(out.to_nchw(), c.expected, f"{name} tile {tile} (certificate 2^{c.cert:.2f})")
    g.clear(name)


@pytest.mark.parametrize("flag", [False, True], ids=["", "range_flag"])
@pytest.mark.parametrize("tile", [1, 2, 3, 4])
def test_gather_fp16_shadow_and_even_grid_output(tile, flag):
    """okp_conv_args.out16 + res_is_f16 + out_subsample = 2 at an odd 13 x 9: the fp32 result on the full grid, the fp16 copy = fp16(expected),
    the even-grid fp32 tensor = exactly the even pixels."""
    c = ec.get("out16_sub2")
    plan, g = build_plan(c, flag)
    o16 = nan_act(c.n, c.ho, c.wo, c.cout, torch.float16)
    out = run_plan(c, plan, tile, out16=o16)
    assert_bits(out.to_nchw(), c.expected, f"out16 tile {tile}: fp32 result")
    want16 = eo.round_fp16(c.expected)
    assert_bits(o16.t.permute(0, 3, 1, 2).float(), want16.float(), f"out16 tile {tile}: fp16 copy")
    assert bool((want16.float() != c.expected).any())                           # (the copy does round here)
    s16 = nan_act(c.n, c.ho, c.wo, c.cout, torch.float16)
    sub = run_plan(c, plan, tile, out16=s16, out_subsample=2, out=nan_act(c.n, (c.ho + 1) // 2, (c.wo + 1) // 2, c.cout))
    assert_bits(sub.to_nchw(), c.expected[:, :, ::2, ::2].contiguous(), f"out_subsample tile {tile}: even grid")
    assert_bits(s16.t.permute(0, 3, 1, 2).float(), want16.float(), f"out_subsample tile {tile}: fp16 copy")
    g.clear("out16_sub2")


class _LaunchSpy:
    """ops.LAUNCH_HOOK: (plan, tile) of every convolution launch."""

    def __init__(self):
        self.launches = []

    def before(self, plan, tile, macs):
        self.launches.append((plan, tile))

    def after(self, token):
        pass


def run_unpool(c, tile, flag=False):
    from object_keypoints_amd.perception import backbone as bb
    m = bb.unpool_merge(c.dim).eval()
    with torch.no_grad():
        m.weight.copy_(c.wt.float())
        m.bias.copy_(c.bias.float())
    from object_keypoints_amd import ops
    keep = bb.UNPOOL_TILE
    ops.LAUNCH_HOOK = spy = _LaunchSpy()
    try:
        bb.UNPOOL_TILE = tile
        with flagged(flag) as g:
            got = m(act(c.low), act(c.up1))
    finally:
        bb.UNPOOL_TILE = keep
        ops.LAUNCH_HOOK = None
    torch.cuda.synchronize()
    g.clear(c.name)
    (plan, launched), = spy.launches                       # one launch, of a split-product plan, on the tile asked for
    assert plan.split and launched == tile
    if tile == 13:
        assert plan.picks_patch(c.n, c.h, c.w, [c.dim], out_step=2, n_classes=4, tile=13), f"{c.name}: okp_conv_patch_applies refuses the plan"
    return got


@pytest.mark.parametrize("flag", [False, True], ids=["", "range_flag"])
@pytest.mark.parametrize("tile", [1, 2, 3, 4])
def test_gather_transposed_convolution_classes(tile, flag):
    """4x4 / stride-2 transposed convolution + merge add as four sub-pixel classes of one launch, 4 x 5 -> 8 x 10."""
    c = ec.get("unpool_c32")
    assert_bits(run_unpool(c, tile, flag).to_nchw(), c.expected, f"unpool_c32 tile {tile} (certificate 2^{c.cert:.2f})")


# ---- exact-fp32 plans (OKP_F32) -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("tile", [1, 2, 3, 4, 6, 8])
@pytest.mark.parametrize("name", list(ec.F32))
def test_exact_fp32_plan_gives_the_plain_sum_bit_for_bit(name, tile):
    """Integer-valued operands (products of up to 17 bits): the expectation is the plain fp64 sum, no split."""
    c = ec.get(name)
    plan, _ = build_plan(c, split=False)
    assert_bits(run_plan(c, plan, tile).to_nchw(), c.expected, f"{name} tile {tile}")


# ---- patch-resident kernel (okp_igemm_patch_x3.hip: tile 13) --------------------------------------------------------------------------------------

def picks_patch(c, plan, window=False):
    return plan.picks_patch(c.n, c.ho, c.wo, [d["cin"] + (16 if window else 0) for d in c.srcs], tile=13)


@pytest.mark.parametrize("flag", [False, True], ids=["", "range_flag"])
@pytest.mark.parametrize("name", list(ec.PATCH))
def test_patch_kernel_gives_the_three_term_sum_bit_for_bit(name, flag):
    """One and two channel chunks, one tile and several, windows, stride 2 from an even and an odd map (four lattice geometries, the one-step
    group included), a one-step skip group behind a nine-step group, subnormal low halves - and the gather tile's bits on the same plan."""
    c = ec.get(name)
    window = name.endswith("windows")
    plan, g = build_plan(c, flag)
    assert picks_patch(c, plan, window), f"{name}: okp_conv_patch_applies refuses the plan - the case does not reach the kernel"
    out = run_plan(c, plan, 13, window=window)
    assert_bits(out.to_nchw(), c.expected, f"{name} tile 13 (certificate 2^{c.cert:.2f})")
    out3 = run_plan(c, plan, 3, window=window)
    assert_bits(out3.to_nchw(), c.expected, f"{name} tile 3")
    g.clear(name)


@pytest.mark.parametrize("flag", [False, True], ids=["", "range_flag"])
def test_patch_kernel_transposed_classes(flag):
    c = ec.get("p_unpool_c256")
    assert_bits(run_unpool(c, 13, flag).to_nchw(), c.expected, f"p_unpool_c256 tile 13 (certificate 2^{c.cert:.2f})")
    assert_bits(run_unpool(c, 3, flag).to_nchw(), c.expected, "p_unpool_c256 tile 3")


def pairs_act(x):
    """fp64 NCHW on the CPU -> pair-format activation on the device: per 8 channels [8 x fp16 hi | 8 x fp16 lo] in the storage of 8 floats
    (include/okp.h, okp_conv_args.out_pairs), halves by exact_operands.round_pairs."""
    from object_keypoints_amd import ops
    hi, lo = eo.round_pairs(x.permute(0, 2, 3, 1).contiguous())
    assert torch.equal(hi.double() + lo.double(), x.permute(0, 2, 3, 1))
    n, h, w, ch = hi.shape
    t = torch.stack((hi.reshape(n, h, w, ch // 8, 8), lo.reshape(n, h, w, ch // 8, 8)), dim=4).reshape(n, h, w, 2 * ch).contiguous()
    a = ops.Act(t.view(torch.float32).to(_dev()))
    a.pairs = True
    return a


def decode_pairs(a):
    """A pair-format activation [N,H,W,C] -> (hi, lo) fp16 NCHW on the CPU."""
    n, h, w, ct = a.t.shape
    hl = a.t.view(torch.float16).view(n, h, w, ct // 8, 2, 8).cpu()
    return tuple(hl[..., i, :].reshape(n, h, w, ct).permute(0, 3, 1, 2).contiguous() for i in (0, 1))


@pytest.mark.parametrize("name", ["p_c32_16x16", "p_s2_c64_from_31", "p_pair_a"])
def test_patch_kernel_pair_output_is_hi_lo_of_the_expected_tensor(name):
    """okp_conv_args.out_pairs: hi = fp16(y), lo = fp16(y - hi) of the exact result, decoded on the host."""
    c = ec.get(name)
    plan, _ = build_plan(c)
    assert picks_patch(c, plan)
    out = run_plan(c, plan, 13, out_pairs=True)
    assert out.pairs
    hi, lo = decode_pairs(out)
    want_hi, want_lo = eo.round_pairs(c.expected)
    assert_bits(hi.float(), want_hi.float(), f"{name}: high halves")
    assert_bits(lo.float(), want_lo.float(), f"{name}: low halves")
    assert bool((want_lo != 0).any())


def test_patch_kernel_reads_pairs_as_it_reads_fp32():
    """Conv B on conv A's pair-format output (okp_conv_args.src_pairs) = conv B on A's fp32 output = the reference.  A's exact result has
    integer high halves by construction (exact_operands_cases._pair_a), so B's re-split of it is lossless and B is certified on it."""
    a, b = ec.get("p_pair_a"), ec.get("p_pair_b")
    eo.resplit(a.exact, "conv A's result")
    plan_a, _ = build_plan(a)
    plan_b, _ = build_plan(b)
    assert picks_patch(a, plan_a) and picks_patch(b, plan_b)
    a32 = run_plan(a, plan_a, 13)
    assert_bits(a32.to_nchw(), a.expected, "conv A, fp32 output")
    assert_bits(run_plan(a, plan_a, 3).to_nchw(), a.expected, "conv A, gather tile 3")
    out3 = nan_act(b.n, b.ho, b.wo, b.cout)
    plan_b([a32], out3, b.ho, b.wo, tile=3)
    torch.cuda.synchronize()
    assert_bits(out3.to_nchw(), b.expected, "conv B on A's fp32 source, gather tile 3")
    a_pairs = run_plan(a, plan_a, 13, out_pairs=True)
    for src, what in ((a32, "fp32 source"), (a_pairs, "pair-format source")):
        out = nan_act(b.n, b.ho, b.wo, b.cout)
        plan_b([src], out, b.ho, b.wo, tile=13)
        torch.cuda.synchronize()
        assert_bits(out.to_nchw(), b.expected, f"conv B on A's {what} (certificate 2^{b.cert:.2f})")


# ---- okp_fire_x3 (one-launch fire module 256 -> 128 -> 256) -----------------------------------------------------------------------------------------

def fire_plans(c, flag):
    from object_keypoints_amd import ops
    f32 = lambda t: t.float().numpy()
    with flagged(flag) as g:
        squeeze = ops.ConvPlan(torch.float32, [256], [1], 128, [(0, 0, 0, f32(c.w1))], f32(c.b1), relu=False)
        expand = ops.ConvPlan(torch.float32, [128], [c.stride], 128, [(0, 0, 0, f32(c.wa))], f32(c.ba), relu=True)
    wd = c.wd.permute(1, 2, 0).reshape(9, 128).contiguous().float().to(_dev())        # tap-major [9][C]
    return squeeze, expand, wd, c.bd.float().to(_dev()), g


@pytest.mark.parametrize("flag", [False, True], ids=["", "range_flag"])
@pytest.mark.parametrize("name", list(ec.FIRE))
def test_fire_module_in_one_launch_and_in_two(name, flag):
    """Stride 1 with skip, stride 2 without; a full and a partial tile in each axis.  The squeeze tile is re-split in the kernel - losslessly
    on these operands (exact_operands_cases.fire_case) - so the expand stage's three-term sum is taken on the exact tile; the depth-wise branch
    is plain fp32 arithmetic.  Both plans carry a 2^-20 row (the squeeze plan's is seen through the depth-wise branch): the pre-scale of the
    fragment-order weight copies the one-launch kernel reads is needed.  One launch = the reference = the squeeze + fused-tail launches."""
    from object_keypoints_amd import ops
    c = ec.get(name)
    squeeze, expand, wd, bd, g = fire_plans(c, flag)
    x = act(c.x)
    ho, wo = (c.h - 1) // c.stride + 1, (c.w - 1) // c.stride + 1
    out = nan_act(c.n, ho, wo, 256)
    ops.fire_fused(squeeze, expand, wd, bd, x, out, c.stride, c.skip)
    torch.cuda.synchronize()
    assert_bits(out.to_nchw(), c.expected, f"{name}: one launch (certificates 2^{c.certs[0]:.2f} squeeze, 2^{c.certs[1]:.2f} expand, 2^{c.certs[2]:.2f} depth-wise)")
    s = nan_act(c.n, c.h, c.w, 128)
    squeeze([x], s, c.h, c.w)
    assert_bits(s.to_nchw(), c.squeeze.float(), f"{name}: squeeze launch")
    two = nan_act(c.n, ho, wo, 256)
    expand([s], two.slice(0, 128), ho, wo, res=x.slice(0, 128) if c.skip else None,
           dw=(wd, bd, two.slice(128, 128), x.slice(128, 128) if c.skip else None))
    torch.cuda.synchronize()
    assert_bits(two.to_nchw(), c.expected, f"{name}: two launches")
    g.clear(name)


# ---- split stem (okp_stem_x3_kernel) ------------------------------------------------------------------------------------------------------------------

def stem_plan(c, flag=False):
    from object_keypoints_amd import ops
    with flagged(flag) as g:
        plan = ops.StemPlan(c.wt.float().numpy(), c.bias.float().numpy(), torch.float32)
    assert plan.split
    return plan, g


@pytest.mark.parametrize("flag", [False, True], ids=["", "range_flag"])
@pytest.mark.parametrize("name", list(ec.STEM))
def test_split_stem_fp32_and_pair_output(name, flag):
    """stem_forward_nchw and stem_forward_nchw_pairs on lattice frames (normal and subnormal low halves) and on frames holding whole numbers
    0 .. 255; maps with partial tiles."""
    c = ec.get(name)
    plan, g = stem_plan(c, flag)
    frames = c.x.float().to(_dev())
    ho, wo = c.expected.shape[2:]
    out = nan_act(c.n, ho, wo, 128)
    plan.from_nchw(frames, out)
    torch.cuda.synchronize()
    assert_bits(out.to_nchw(), c.expected, f"{name} (certificate 2^{c.cert:.2f})")
    pairs = nan_act(c.n, ho, wo, 128)
    plan.from_nchw(frames, pairs, out_pairs=True)
    torch.cuda.synchronize()
    hi, lo = decode_pairs(pairs)
    want_hi, want_lo = eo.round_pairs(c.expected)
    assert_bits(hi.float(), want_hi.float(), f"{name}: high halves")
    assert_bits(lo.float(), want_lo.float(), f"{name}: low halves")
    g.clear(name)


@pytest.mark.parametrize("name", ["stem_33x33", "stem_2x15x130"])
def test_stride4_stem_launch_of_the_mixed_configuration(name):
    """ops.MIX_STEM_FP16: the fp32 stream of the mixed configuration's stem is a stride-4 three-term launch of the gather kernel on the
    packed frames - the even pixels of the stem's map, bit for bit."""
    from object_keypoints_amd import ops
    from object_keypoints_amd.perception import backbone as bb
    c = ec.get(name)
    m = bb.convolution(7, 3, 128, stride=2, with_bn=False).eval()
    with torch.no_grad():
        m.conv.weight.copy_(c.wt.float())
        m.conv.bias.copy_(c.bias.float())
    with ops.f32_split(True, True):
        assert ops.F32_MIX and ops.MIX_STEM_FP16
        out = m.forward_frames(c.x.float().to(_dev()), torch.float32, shadow=True, compact=True)
    torch.cuda.synchronize()
    assert out.compact and out.shadow is not None
    assert_bits(out.to_nchw(), c.expected[:, :, ::2, ::2].contiguous(), f"{name}: even pixels")


# ---- one-launch heads of the split configurations (okp_heads_x3_kernel) ----------------------------------------------------------------------------------

def run_heads(c, fused, sigmoid, flag=False):
    from object_keypoints_amd import ops
    f32 = lambda t: t.float().numpy()
    with flagged(flag) as g:
        l1 = ops.ConvPlan(torch.float32, [256], [1], 384, [(0, 0, 0, f32(c.w1))], f32(c.b1), relu=True)
        l2 = ops.ConvPlan(torch.float32, [384], [1], 96, [(0, 0, 0, f32(c.w2))], f32(c.b2), relu=True, alg_k=128)
    w3, b3 = c.w3.float().contiguous().to(_dev()), c.b3.float().to(_dev())
    K, n, h, w = c.K, c.n, c.h, c.w
    full = lambda ch: torch.full((n, ch, h, w), float("nan"), dtype=torch.float32, device=_dev())
    heat, depth, centers = full(K), full(K), full(2 * (K - 1))
    outs = [(0, ops.ACT_SIGMOID if sigmoid else ops.ACT_NONE, heat, k) for k in range(K)]
    outs += [(32, ops.ACT_NONE, depth, k) for k in range(K)]
    outs += [(64, ops.ACT_NONE, centers, k) for k in range(2 * (K - 1))]
    if fused:
        ops.heads_fused(l1, l2, pairs_act(c.x), outs, w3, b3)
    else:
        x = act(c.x)
        a1 = nan_act(n, h, w, 384)
        l1([x], a1, h, w)
        assert_bits(a1.to_nchw(), c.h1.float(), f"{c.name}: hidden layer 1")
        a2 = nan_act(n, h, w, 96)
        l2([a1], a2, h, w)
        assert_bits(a2.to_nchw(), c.h2.float(), f"{c.name}: hidden layer 2")
        ops.head_out(a2, outs, w3, b3)
    torch.cuda.synchronize()
    g.clear(c.name)
    return heat.cpu(), depth.cpu(), centers.cpu()


@pytest.mark.parametrize("flag", [False, True], ids=["", "range_flag"])
@pytest.mark.parametrize("fused", [True, False], ids=["one_launch", "three_launches"])
@pytest.mark.parametrize("name", list(ec.HEADS))
def test_heads_linear_outputs_bit_for_bit_and_sigmoid_within_its_allowance(name, fused, flag):
    """K = 3 and 4.  The hidden layers are re-split as the kernel does (okp_heads.hip: okp_split4 of relu(fma(acc, scale, bias)) for layer 1;
    layer 2 stays fp32 and feeds a 32-term fp32 dot product) - losslessly on these operands.  Linear outputs: bits; the sigmoid of the heat
    head: within 4 x 2^-24 of the fp64 sigmoid of the exact logit (tests/kernel_bounds.py::sigmoid)."""
    c = ec.get(name)
    heat, depth, centers = run_heads(c, fused, sigmoid=False, flag=flag)
    what = f"{name} {'one launch' if fused else 'three launches'} (certificates 2^{c.certs[0]:.2f}, 2^{c.certs[1]:.2f}, 2^{c.certs[2]:.2f})"
    assert_bits(heat, c.heat.float(), what + ": heat logits")
    assert_bits(depth, c.depth.float(), what + ": depth")
    assert_bits(centers, c.centers.float(), what + ": centers")
    prob, depth2, _ = run_heads(c, fused, sigmoid=True, flag=flag)
    err = (prob.double() - torch.sigmoid(c.heat)).abs().max()
    print(f"{what}: sigmoid max |err| {float(err):.3g} (allowance {4 * 2.0 ** -24:.3g})")
    assert bool(torch.isfinite(prob).all()) and float(err) <= 4.0 * 2.0 ** -24
    assert_bits(depth2, c.depth.float(), what + ": depth beside the sigmoid")
