"""Every 16-bit kernel against its fp64 reference, element by element: |device - exact| <= the propagated bound of tests/kernel_bounds.py.

The bound knows only where a kernel rounds (docs/PRECISION.md, "Kernel-level bounds"); tests/test_kernel_bounds.py shows on the CPU that
seven kinds of wrong kernel, all invisible to the max-abs tolerances of test_gpu_conv.py, land outside it.  Every case builds its plans from
weights the test has already rounded, runs through the public entry points and prints the worst ratio with its index (pytest -s):
the index names the frame, channel and pixel - hence the tile, edge and channel group - to look at when a kernel rewrite fails here."""
import numpy as np
import pytest
import torch

import kernel_bounds_cases as kc

pytestmark = pytest.mark.gpu
HALF = kc.HALF
NAME = {torch.bfloat16: "bf16", torch.float16: "fp16"}


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def act(x, dtype):
    from object_keypoints_amd import ops
    return ops.Act.from_nchw(x.to(_dev()), dtype)


def empty(n, h, w, c, dtype, fill=float("nan")):
    """An output the kernel has to write completely: what it leaves out stays NaN and fails the bound."""
    from object_keypoints_amd import ops
    return ops.Act(torch.full((n, h, w, c), fill, dtype=dtype, device=_dev()))


def check(ref, got, what):
    got = got.detach().cpu()
    assert tuple(got.shape) == tuple(ref.val.shape), (what, got.shape, ref.val.shape)
    r, worst, idx = ref.ratio(got)
    print(f"KBOUND {what}: max |got - val| / err = {worst:.3g} at (n, c, y, x) = {idx}")
    assert bool((r <= 1.0).all()), f"{what}: {int((~(r <= 1.0)).sum())} elements outside the bound, worst {worst:.3g} at {idx}"
    return worst


def conv_plan(dtype, cins, strides, cout, taps, b, relu=True):
    from object_keypoints_amd import ops
    return ops.ConvPlan(dtype, cins, strides, cout, taps, b.numpy(), relu=relu)


def taps_of(w, src=0):
    from object_keypoints_amd.perception.backbone import conv_taps
    return conv_taps(w.numpy(), src=src)


class guarded:
    """Plans built inside are range-guarded fp16 plans (separate template instances of every kernel); the flag must stay clear."""

    def __init__(self, on):
        self.flag = torch.zeros(1, dtype=torch.int32, device=_dev()) if on else None

    def __enter__(self):
        from object_keypoints_amd import ops
        self.ctx = ops.f32_split(False, False, self.flag, guard16=True) if self.flag is not None else None
        if self.ctx is not None:
            self.ctx.__enter__()
        return self

    def __exit__(self, *exc):
        if self.ctx is not None:
            self.ctx.__exit__(*exc)

    def clear(self, what):
        if self.flag is not None:
            torch.cuda.synchronize()
            assert int(self.flag) == 0, f"{what}: the fp16 range flag was raised on healthy operands"


# ---- gather implicit GEMM (okp_igemm_kernel.h) ------------------------------------------------------------------------------------------

def run_conv(c, shape, tile, dtype, guard=False):
    k, stride, cin, cout, n, h, w = shape
    ho, wo = kc.out_size(h, k, stride, (k - 1) // 2), kc.out_size(w, k, stride, (k - 1) // 2)
    with guarded(guard) as g:
        plan = conv_plan(dtype, [cin], [stride], cout, taps_of(c.wt), c.b)
    out = empty(n, ho, wo, cout, dtype)
    plan([act(c.x, dtype)], out, ho, wo, tile=tile)
    check(c.ref, out.to_nchw(), f"gather conv {shape} tile {tile} {NAME[dtype]}{' guarded' if guard else ''}")
    g.clear("gather conv")


@pytest.mark.parametrize("dtype", HALF)
@pytest.mark.parametrize("tile", [1, 2, 3, 4, 6, 8])
@pytest.mark.parametrize("shape", kc.CONV_SHAPES)
def test_gather_convolution(shape, tile, dtype):
    run_conv(kc.conv(*shape, dtype), shape, tile, dtype)


@pytest.mark.parametrize("dtype", HALF)
def test_gather_two_source_residual_block(dtype):
    n, c0, c1, cout, h, w = 2, 32, 16, 64, 10, 12
    c = kc.two_source(3, c0, c1, 2, cout, n, h, w, dtype)
    plan = conv_plan(dtype, [c0, c1], [1, 2], cout, taps_of(c.w0) + [(1, 0, 0, np.ascontiguousarray(c.w1.numpy()[:, :, 0, 0]))], c.b)
    out = empty(n, h, w, cout, dtype)
    plan([act(c.t, dtype), act(c.x, dtype)], out, h, w)
    check(c.ref, out.to_nchw(), f"gather two-source block {NAME[dtype]}")


@pytest.mark.parametrize("dtype", HALF)
def test_gather_1x1_through_channel_windows(dtype):
    """1x1 convolution writing channels [8, 24) of a 32-channel tensor, residual read from the same window of another."""
    n, cin, cout, h, w = 2, 24, 16, 6, 7
    c = kc.conv_res(1, cin, cout, n, h, w, dtype, res_channels=32, res_c0=8)
    plan = conv_plan(dtype, [cin], [1], cout, taps_of(c.wt), c.b)
    big = empty(n, h, w, 32, dtype, fill=-7.0)
    plan([act(c.x, dtype)], big.slice(8, 16), h, w, res=act(c.r, dtype).slice(8, 16))
    full = big.t.float().cpu()
    check(c.ref, full[..., 8:24].permute(0, 3, 1, 2), f"gather 1x1 + windowed residual {NAME[dtype]}")
    assert bool((full[..., :8] == -7.0).all()) and bool((full[..., 24:] == -7.0).all())         # neighbour channels untouched


def run_unpool(c, dim, dtype, tile, what):
    from object_keypoints_amd.perception import backbone as bb
    m = bb.unpool_merge(dim).eval()
    with torch.no_grad():
        m.weight.copy_(c.wt)
        m.bias.copy_(c.b)
    keep = bb.UNPOOL_TILE
    try:
        bb.UNPOOL_TILE = tile
        got = m(act(c.low, dtype), act(c.up1, dtype)).to_nchw()
    finally:
        bb.UNPOOL_TILE = keep
    check(c.ref, got, what)


@pytest.mark.parametrize("dtype", HALF)
def test_gather_transposed_convolution_and_merge(dtype):
    run_unpool(kc.unpool(16, 2, 5, 7, dtype), 16, dtype, 0, f"gather transposed conv + merge {NAME[dtype]}")


# ---- patch-resident kernel (okp_igemm_patch.hip), tiles 13 and 14 -------------------------------------------------------------------------

def run_patch(plan, srcs, n, h, w, tile, dtype, ref, what, res=None):
    """Into channels [16, 272) of a 288-channel tensor: the neighbours must keep their -7."""
    big = empty(n, h, w, 288, dtype, fill=-7.0)
    big.t[..., 16:272] = float("nan")
    plan(srcs, big.slice(16, 256), h, w, res=res, tile=tile)
    full = big.t.float().cpu()
    check(ref, full[..., 16:272].permute(0, 3, 1, 2), f"patch {what} {n}x{h}x{w} tile {tile} {NAME[dtype]}")
    assert bool((full[..., :16] == -7.0).all()) and bool((full[..., 272:] == -7.0).all())


@pytest.mark.parametrize("dtype", HALF)
@pytest.mark.parametrize("tile", [13, 14])
@pytest.mark.parametrize("n,h,w", [(1, 16, 16), (2, 16, 32)])
@pytest.mark.parametrize("case", ["conv3x3", "res_window", "src_window", "two_chunks"])
def test_patch_resident_3x3(case, n, h, w, tile, dtype):
    if case == "res_window":
        c = kc.conv_res(3, 256, 256, n, h, w, dtype, res_channels=320, res_c0=32, seed=24)
    else:
        c = kc.conv(3, 1, 128 if case == "two_chunks" else 256, 256, n, h, w, dtype, seed=21)
    cin = c.x.shape[1]
    plan = conv_plan(dtype, [cin], [1], 256, taps_of(c.wt), c.b)
    srcs, res = [act(c.x, dtype)], None
    if case == "src_window":            # the source is a 256-channel window of a 320-channel tensor
        wide = torch.cat([kc.q(kc.rand((n, 32, h, w), 44), dtype), c.x, kc.q(kc.rand((n, 32, h, w), 45), dtype)], dim=1)
        srcs = [act(wide, dtype).slice(32, 256)]
    if case == "res_window":
        res = act(c.r, dtype).slice(32, 256)
    run_patch(plan, srcs, n, h, w, tile, dtype, c.ref, case, res=res)


@pytest.mark.parametrize("dtype", HALF)
@pytest.mark.parametrize("tile", [13, 14])
@pytest.mark.parametrize("hi,wi", [(32, 64), (31, 63)])
def test_patch_resident_3x3_stride_2(hi, wi, tile, dtype):
    n = 2
    c = kc.conv(3, 2, 256, 256, n, hi, wi, dtype, seed=36)
    plan = conv_plan(dtype, [256], [2], 256, taps_of(c.wt), c.b)
    run_patch(plan, [act(c.x, dtype)], n, 16, 32, tile, dtype, c.ref, f"3x3 stride 2 from {hi}x{wi}")


@pytest.mark.parametrize("dtype", HALF)
@pytest.mark.parametrize("tile", [13, 14])
@pytest.mark.parametrize("case", ["3x3_plus_s2_1x1", "merge_1x1"])
def test_patch_resident_two_sources(case, tile, dtype):
    n, h, w = 2, 16, 32
    if case == "3x3_plus_s2_1x1":
        c = kc.two_source(3, 256, 128, 2, 256, n, h, w, dtype, seed=25)
        plan = conv_plan(dtype, [256, 128], [1, 2], 256, taps_of(c.w0) + [(1, 0, 0, np.ascontiguousarray(c.w1.numpy()[:, :, 0, 0]))], c.b)
    else:
        c = kc.two_source(1, 256, 256, 1, 256, n, h, w, dtype, seed=30)
        plan = conv_plan(dtype, [256, 256], [1, 1], 256, [(0, 0, 0, np.ascontiguousarray(c.w0.numpy()[:, :, 0, 0])),
                                                             (1, 0, 0, np.ascontiguousarray(c.w1.numpy()[:, :, 0, 0]))], c.b)
    run_patch(plan, [act(c.t, dtype), act(c.x, dtype)], n, h, w, tile, dtype, c.ref, case)


@pytest.mark.parametrize("dtype", HALF)
@pytest.mark.parametrize("tile", [13, 14])
def test_patch_resident_transposed_classes(tile, dtype):
    run_unpool(kc.unpool(256, 2, 16, 16, dtype, seed=40), 256, dtype, tile, f"patch transposed classes 2x16x16 tile {tile} {NAME[dtype]}")


# ---- stem (okp_stem.hip) --------------------------------------------------------------------------------------------------------------------

def run_stem(c, n, h, w, dtype, guard=False):
    from object_keypoints_amd import ops
    with guarded(guard) as g:
        plan = ops.StemPlan(c.wt.numpy(), c.b.numpy(), dtype)
    ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    x = c.x.to(_dev())
    tag = f"{n}x{h}x{w} {NAME[dtype]}{' guarded' if guard else ''}"
    out = empty(n, ho, wo, 128, dtype)
    plan(ops.pack_frames(x, dtype), out)
    check(c.ref, out.to_nchw(), f"stem, packed frames {tag}")
    out2 = empty(n, ho, wo, 128, dtype)
    plan.from_nchw(x, out2)
    check(c.ref, out2.to_nchw(), f"stem, from_nchw {tag}")
    g.clear("stem")


@pytest.mark.parametrize("dtype", HALF)
@pytest.mark.parametrize("n,h,w", [(1, 37, 45), (2, 15, 130)])
def test_stem(n, h, w, dtype):
    run_stem(kc.stem(n, h, w, dtype), n, h, w, dtype)


# ---- stand-alone depth-wise kernel (okp_pointwise.hip) ---------------------------------------------------------------------------------------

def dw_taps(wd):
    """[C, 1, 3, 3] -> tap-major [9, C] fp32 on the device."""
    return torch.from_numpy(np.ascontiguousarray(np.transpose(wd.numpy()[:, 0], (1, 2, 0)).reshape(9, wd.shape[0]))).to(_dev())


@pytest.mark.parametrize("dtype", HALF)
@pytest.mark.parametrize("c_,h,w,stride,n", kc.DW_SHAPES)
def test_standalone_depthwise(c_, h, w, stride, n, dtype):
    from object_keypoints_amd import ops
    c = kc.depthwise(c_, h, w, stride, n, dtype)
    ho, wo = kc.out_size(h, 3, stride, 1), kc.out_size(w, 3, stride, 1)
    out = empty(n, ho, wo, c_, dtype)
    ops.dwconv3x3(act(c.x, dtype), dw_taps(c.wt), c.b.to(_dev()), out, stride, res=act(c.r, dtype), relu=True)
    check(c.ref, out.to_nchw(), f"depth-wise {(c_, h, w, stride, n)} {NAME[dtype]}")


# ---- one-launch fire module (okp_fire2.hip) and the resident chains (okp_fire_chain.hip) -------------------------------------------------------

def fire_plans(m, dtype):
    from object_keypoints_amd import ops
    mid, cin = m["w1"].shape[:2]
    half = m["wa"].shape[0]
    squeeze = ops.ConvPlan(dtype, [cin], [1], mid, taps_of(m["w1"]), m["b1"].numpy(), relu=False)
    expand = ops.ConvPlan(dtype, [mid], [m["stride"]], half, taps_of(m["wa"]), m["ba"].numpy(), relu=True)
    return squeeze, expand, dw_taps(m["wd"]), m["bd"].to(_dev())


def run_fire2(cin, mid, stride, n, h, w, dtype, skip=None, guard=False):
    from object_keypoints_amd import ops
    c = kc.fire2(cin, mid, stride, n, h, w, dtype, skip=skip)
    m = c.mods[0]
    keep, ops.FUSE_FIRE_MIN_HW = ops.FUSE_FIRE_MIN_HW, 0
    try:
        assert ops.fire_fusable(cin, mid, stride, h, w, guarded=guard)
        with guarded(guard) as g:
            sq, ex, wd, bd = fire_plans(m, dtype)
        ho, wo = kc.out_size(h, 3, stride, 1), kc.out_size(w, 3, stride, 1)
        out = empty(n, ho, wo, 2 * mid, dtype)
        l0 = ops.COUNTERS["launches"]
        ops.fire_fused(sq, ex, wd, bd, act(c.x, dtype), out, stride, m["skip"])
        assert ops.COUNTERS["launches"] - l0 == 1
    finally:
        ops.FUSE_FIRE_MIN_HW = keep
    check(c.ref, out.to_nchw(), f"fire2 {cin} -> {mid} stride {stride} skip {int(m['skip'])} {n}x{h}x{w} {NAME[dtype]}{' guarded' if guard else ''}")
    g.clear("fire2")


FIRE2_INSTANCES = {1: [(256, 128), (384, 128), (384, 192), (512, 192), (512, 256)], 2: [(256, 128), (256, 192), (384, 192), (384, 256)]}     # ops._FIRE2_CONFIGS
FIRE2_GEOMETRIES = {1: [(16, 16), (33, 21)], 2: [(16, 16), (21, 35)]}     # a matrix-pipe geometry; a vector-ALU one with partial tiles on both axes
FIRE2_CASES = [(cin, mid, stride, h, w) for stride in (1, 2) for cin, mid in FIRE2_INSTANCES[stride] for h, w in FIRE2_GEOMETRIES[stride]]


def test_every_fire2_instance_has_its_cases():
    from object_keypoints_amd import ops
    assert {s: sorted(v) for s, v in ops._FIRE2_CONFIGS.items()} == FIRE2_INSTANCES


@pytest.mark.parametrize("dtype", HALF)
@pytest.mark.parametrize("cin,mid,stride,h,w", FIRE2_CASES)
def test_one_launch_fire_module(cin, mid, stride, h, w, dtype):
    run_fire2(cin, mid, stride, 2, h, w, dtype)


@pytest.mark.parametrize("dtype", HALF)
def test_one_launch_fire_module_without_skip(dtype):
    run_fire2(256, 128, 1, 2, 19, 23, dtype, skip=False)


def run_chain(c, n, ho, wo, cout, dtype, what, guard=False):
    from object_keypoints_amd import ops
    with guarded(guard) as g:
        plans = [fire_plans(m, dtype) for m in c.mods]
    out = empty(n, ho, wo, cout, dtype)
    l0 = ops.COUNTERS["launches"]
    ops.fire_chain(plans, act(c.x, dtype), out)
    assert ops.COUNTERS["launches"] - l0 == 1
    check(c.ref, out.to_nchw(), f"{what} {NAME[dtype]}{' guarded' if guard else ''}")
    g.clear(what)


@pytest.mark.parametrize("dtype", HALF)
@pytest.mark.parametrize("c_,n,h,w,count", [(512, 2, 4, 4, 2), (512, 2, 3, 4, 2), (512, 1, 1, 3, 3), (512, 2, 4, 4, 1), (384, 3, 8, 8, 1), (384, 2, 7, 5, 2)])
def test_resident_chain(c_, n, h, w, count, dtype):
    run_chain(kc.chain(c_, n, h, w, count, dtype), n, h, w, c_, dtype, f"chain {c_}-wide {n}x{h}x{w} count {count}")


@pytest.mark.parametrize("dtype", HALF)
@pytest.mark.parametrize("c_,n,h,w,count", [(512, 2, 4, 4, 2), (512, 2, 3, 4, 2), (512, 1, 1, 3, 3), (384, 2, 7, 5, 2)])
def test_resident_chain_last_module_from_the_device_input(c_, n, h, w, count, dtype):
    """A worst-case bound carried through several modules grows far beyond the true error (docs/PRECISION.md).  Every module boundary of
    the chain is a store in the activation type, so the chain of the first count - 1 modules hands out exactly what the full chain's last
    module reads: bounded from THAT input (err = 0) the last module of a long chain is held as tightly as a chain of one."""
    import kernel_bounds as kb
    from object_keypoints_amd import ops
    c = kc.chain(c_, n, h, w, count, dtype)
    plans = [fire_plans(m, dtype) for m in c.mods]
    x = act(c.x, dtype)
    mid, out = empty(n, h, w, c_, dtype), empty(n, h, w, c_, dtype)
    ops.fire_chain(plans[:-1], x, mid)
    ops.fire_chain(plans, x, out)
    ref = kb.fire_chain_module(kb.exact(mid.to_nchw().cpu()), c.mods[-1], dtype, False)
    check(ref, out.to_nchw(), f"chain {c_}-wide {n}x{h}x{w} module {count} of {count} from the device's input {NAME[dtype]}")


@pytest.mark.parametrize("dtype", HALF)
@pytest.mark.parametrize("n,h,w,count", [(2, 8, 8, 1), (3, 7, 5, 2), (2, 1, 1, 1)])
def test_framed_resident_chain(n, h, w, count, dtype):
    """Entry (stride 2), chain and exit modules in one launch.  Carried through three or four modules without a stored tensor in between, the
    worst-case bound exceeds the activations themselves (measured ratios 1e-4 and below, docs/PRECISION.md): this holds the form to finite
    values in every element of the right shape; its arithmetic stays pinned by test_gpu_conv.py at that file's tolerance."""
    run_chain(kc.framed_chain(n, h, w, count, dtype), n, (h - 1) // 2 + 1, (w - 1) // 2 + 1, 384, dtype, f"framed chain {n}x{h}x{w} count {count}")


# ---- heads (okp_heads.hip; ConvPlan x 2 + okp_head_out) ---------------------------------------------------------------------------------------

def run_heads(K, n, h, w, dtype, fused, guard=False):
    from object_keypoints_amd import ops
    c = kc.heads(K, n, h, w, dtype)
    dev = _dev()
    with guarded(guard) as g:
        l1 = ops.ConvPlan(dtype, [256], [1], 384, [(0, 0, 0, np.ascontiguousarray(c.w1.numpy()[:, :, 0, 0]))], c.b1.numpy(), relu=True)
        l2 = ops.ConvPlan(dtype, [384], [1], 96, [(0, 0, 0, np.ascontiguousarray(c.w2.numpy()[:, :, 0, 0]))], c.b2.numpy(), relu=True, alg_k=128)
    w3, b3 = c.w3.to(dev), c.b3.to(dev)
    nan = lambda ch: torch.full((n, ch, h, w), float("nan"), dtype=torch.float32, device=dev)
    x = act(c.x, dtype)

    hidden = []                         # three launches: the hidden tensors the device stored

    def launch(heat_act):
        heat, depth, centers = nan(K), nan(K), nan(2 * (K - 1))
        outs = [(0, heat_act, heat, k) for k in range(K)] + [(32, ops.ACT_NONE, depth, k) for k in range(K)]
        outs += [(64, ops.ACT_NONE, centers, k) for k in range(2 * (K - 1))]
        if fused:
            ops.heads_fused(l1, l2, x, outs, w3, b3)
        else:
            a1 = empty(n, h, w, 384, dtype)
            l1([x], a1, h, w)
            a2 = empty(n, h, w, 96, dtype)
            l2([a1], a2, h, w)
            ops.head_out(a2, outs, w3, b3)
            hidden.append((a1.to_nchw().cpu(), a2.to_nchw().cpu()))
        return heat, depth, centers

    tag = f"heads {'one launch' if fused else 'three launches'} K={K} {n}x{h}x{w} {NAME[dtype]}{' guarded' if guard else ''}"
    heat, depth, centers = launch(ops.ACT_SIGMOID)
    logits = launch(ops.ACT_NONE)[0]
    check(c.ref["heat"], heat, f"{tag} heat")
    check(c.ref["depth"], depth, f"{tag} depth")
    check(c.ref["centers"], centers, f"{tag} centers")
    check(c.ref["logits"], logits, f"{tag} heat logits")
    # what the device's exp and reciprocal use of the sigmoid stage's 4 a: its output against the fp64 sigmoid of its own logits
    share = float((heat.double() - torch.sigmoid(logits.double())).abs().max()) / (4.0 * 2.0 ** -24)
    print(f"KBOUND {tag}: sigmoid allowance used {share:.3f}")
    g.clear(tag)
    if not fused:
        # the bound carried through three stages is far above the true error (docs/PRECISION.md): as three launches every stage can be
        # bounded from the device's own stored input (err = 0), which holds each as tightly as a single convolution
        import kernel_bounds as kb
        a1, a2 = hidden[0]
        check(kb.conv_chain([kb.Term(kb.exact(c.x), c.w1)], c.b1, dtype), a1, f"{tag} h1")
        check(kb.conv_chain([kb.Term(kb.exact(a1), c.w2)], c.b2, dtype), a2, f"{tag} h2 from the device's h1")
        last = kb.heads_out(kb.exact(a2), c.rows)
        got = torch.cat([heat, depth, centers], 1)
        check(kb.Bounded(torch.cat([v.val for v in last], 1), torch.cat([v.err for v in last], 1)), got, f"{tag} last layer from the device's h2")


@pytest.mark.parametrize("dtype", HALF)
@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("n,h,w", [(2, 9, 7), (1, 8, 24)])
@pytest.mark.parametrize("K", [3, 4])
def test_heads(K, n, h, w, fused, dtype):
    run_heads(K, n, h, w, dtype, fused)


# ---- the range-guarded fp16 instantiations: the same bounds, the flag clear ---------------------------------------------------------------------

def test_guarded_gather_convolution():
    shape = kc.CONV_SHAPES[0]
    run_conv(kc.conv(*shape, torch.float16), shape, 1, torch.float16, guard=True)


def test_guarded_stem():
    run_stem(kc.stem(1, 37, 45, torch.float16), 1, 37, 45, torch.float16, guard=True)


def test_guarded_fire_module_on_the_matrix_pipe():
    run_fire2(256, 128, 1, 2, 16, 16, torch.float16, guard=True)


def test_guarded_resident_chain():
    run_chain(kc.chain(512, 2, 4, 4, 2, torch.float16), 2, 4, 4, 512, torch.float16, "chain 512-wide 2x4x4 count 2", guard=True)


def test_guarded_heads():
    run_heads(3, 2, 9, 7, torch.float16, True, guard=True)
