"""The cases of tests/test_gpu_split_exact.py, built on the CPU (no product import): operands on the lattice of tests/exact_operands.py, the
expected bits, and the certificate that makes them the only admissible answer.  Every builder asserts its certificate and the lossless
split before it hands a case out; tests/test_exact_operands.py runs all of them on a machine without a GPU."""
import functools
from types import SimpleNamespace

import torch
import torch.nn.functional as F

import exact_operands as eo

TINY = 2.0 ** -20          # the output channel every plan carries whose weights are the lattice times 2^-20: without the per-channel pre-scale of
TINY_ROW = 5               # okp_conv_create its low halves fall below fp16's range (hi + lo != w for that row when unscaled)


def chan_scale(cout, tiny_row=TINY_ROW):
    cs = torch.ones(cout, dtype=torch.float64)
    if tiny_row is not None:
        cs[tiny_row] = TINY
    return cs


def out_size(n, k, stride):
    return (n + 2 * ((k - 1) // 2) - k) // stride + 1


def _src(cin, k, stride, h, w, terms=3, Ax=1, Aw=1, zx=0.0, zw=0.0, x=None, wt=None):
    """One source of a plan.  x: a given activation tensor (an earlier case's exact output) instead of a generated one; wt: given weights
    (before the channel scale)."""
    return dict(cin=cin, k=k, stride=stride, h=h, w=w, terms=terms, Ax=Ax, Aw=Aw, zx=zx, zw=zw, x=x, wt=wt)


def conv_case(name, seed, s, n, cout, srcs, B=3, bias=True, res=None, relu=True, integer=False, tiny_row=TINY_ROW):
    """A one- or two-source convolution plan.  srcs: _src(...) dicts; res: None, "f32" or "f16" (an fp16 residual: integer-valued);
    integer: operands for the exact-fp32 plans (integer-valued, no split; the expectation is the plain fp64 sum)."""
    cs = chan_scale(cout, tiny_row)
    step = 2.0 ** -s * cs if not integer else cs.clone()
    ho, wo = out_size(srcs[0]["h"], srcs[0]["k"], srcs[0]["stride"]), out_size(srcs[0]["w"], srcs[0]["k"], srcs[0]["stride"])
    xs, ws = [], []
    for i, d in enumerate(srcs):
        assert (out_size(d["h"], d["k"], d["stride"]), out_size(d["w"], d["k"], d["stride"])) == (ho, wo), name
        if integer:
            x = eo.integers((n, d["cin"], d["h"], d["w"]), seed + 10 * i, d["Ax"], d["zx"])
            w = eo.integers((cout, d["cin"], d["k"], d["k"]), seed + 10 * i + 1, d["Aw"], d["zw"])
        else:
            x = eo.lattice((n, d["cin"], d["h"], d["w"]), seed + 10 * i, d["Ax"], B, s, d["zx"])
            w = eo.lattice((cout, d["cin"], d["k"], d["k"]), seed + 10 * i + 1, d["Aw"], B, s, d["zw"])
        if d["x"] is not None:
            x = d["x"]
        if d["wt"] is not None:
            w = d["wt"]
        xs.append(x)
        ws.append(w * cs.view(-1, 1, 1, 1))
    b = (eo.integers((cout,), seed + 100, 3) if integer else eo.lattice((cout,), seed + 100, 3, B, s)) * cs if bias else None
    if res == "f16" or (res and integer):
        r = eo.integers((n, cout, ho, wo), seed + 101, 4) * cs.view(1, -1, 1, 1)
        assert torch.equal(r.half().double(), r)
    elif res:
        r = eo.lattice((n, cout, ho, wo), seed + 101, 4, B, s) * cs.view(1, -1, 1, 1)
    else:
        r = None
    scale = eo.row_scale(ws)
    y = torch.zeros((n, cout, ho, wo), dtype=torch.float64)
    a = torch.zeros_like(y)
    for d, x, w in zip(srcs, xs, ws):
        pad = (d["k"] - 1) // 2
        if integer:
            op = eo.conv2d_op(d["stride"], pad)
            y, a = y + op(x, w), a + op(x.abs(), w.abs())
        else:
            eo.assert_lossless(x, f"{name}: activations")
            eo.assert_split_on_lattice(x, s, f"{name}: activations")
            eo.assert_lossless(w, f"{name}: weights", scale=scale)
            v, av = eo.conv2d_three_term(x, w, d["stride"], pad, scale=scale, terms=d["terms"])
            y, a = y + v, a + av
    if b is not None:
        y, a = y + b.view(1, -1, 1, 1), a + b.abs().view(1, -1, 1, 1)
    if r is not None:
        y, a = y + r, a + r.abs()
    cert = eo.assert_certificate(a, step, name)
    eo.assert_on_lattice(y, step, name)
    if relu:
        y = F.relu(y)
    return SimpleNamespace(name=name, s=s, n=n, cout=cout, ho=ho, wo=wo, srcs=srcs, xs=xs, ws=ws, bias=b, res=r, res16=res == "f16", relu=relu,
                           expected=y.float(), exact=y, cert=cert, step=step, cs=cs, scale=scale, integer=integer, abs_sum=a)


def unpool_case(name, seed, s, dim, n, h, w, zw=0.0, Ax=1, B=3):
    """ConvTranspose2d(dim, dim, 4, 2, 1) with bias plus the merge add of the hourglass (no ReLU): four sub-pixel classes of one launch."""
    cs = chan_scale(dim)
    step = 2.0 ** -s * cs
    low = eo.lattice((n, dim, h, w), seed, Ax, B, s)
    wt = eo.lattice((dim, dim, 4, 4), seed + 1, 1, B, s, zw) * cs.view(1, -1, 1, 1)        # [cin, cout, ky, kx]
    b = eo.lattice((dim,), seed + 2, 3, B, s) * cs
    up1 = eo.lattice((n, dim, 2 * h, 2 * w), seed + 3, 4, B, s) * cs.view(1, -1, 1, 1)
    scale = eo.row_scale([wt], cout_dim=1)
    eo.assert_lossless(low, f"{name}: activations")
    eo.assert_lossless(wt, f"{name}: weights", scale=scale, cout_dim=1)
    v, av = eo.conv_transpose2d_three_term(low, wt, scale=scale)
    y = v + b.view(1, -1, 1, 1) + up1
    a = av + b.abs().view(1, -1, 1, 1) + up1.abs()
    cert = eo.assert_certificate(a, step, name)
    eo.assert_on_lattice(y, step, name)
    return SimpleNamespace(name=name, s=s, dim=dim, n=n, h=h, w=w, low=low, wt=wt, bias=b, up1=up1, expected=y.float(), exact=y, cert=cert, step=step)


# ---- gather tiles of okp_igemm_kernel<F32S> --------------------------------------------------------------------------------------------------

GATHER = {
    # 3x3 stride 1, ragged pixel tiles, cout below every tile
    "3x3_c32": lambda: conv_case("3x3_c32", 100, 14, 2, 64, [_src(32, 3, 1, 9, 7, Ax=2)]),
    # ... with low halves in the fp16 subnormal range (activations: the weights are scaled per row)
    "3x3_c32_subnormal": lambda: conv_case("3x3_c32_subnormal", 110, 16, 2, 64, [_src(32, 3, 1, 9, 7, zx=0.3, zw=0.3)]),
    # 1x1, a K-slice with nvalid < 8, cout_pad 128
    "1x1_c36": lambda: conv_case("1x1_c36", 120, 14, 2, 72, [_src(36, 1, 1, 9, 7, Ax=2, Aw=2)]),
    # 3x3 stride 2 on an odd input
    "3x3_s2_c64": lambda: conv_case("3x3_s2_c64", 130, 14, 2, 64, [_src(64, 3, 2, 11, 13, zw=0.25)]),
    # two sources: 3x3 + stride-2 1x1 skip (odd input), residual and ReLU
    "two_source": lambda: conv_case("two_source", 140, 14, 2, 64, [_src(32, 3, 1, 9, 7), _src(64, 1, 2, 17, 13)], res="f32"),
    # single-term 3x3 taps plus a three-term skip: n_single_slices partitions K
    "mixed_terms": lambda: conv_case("mixed_terms", 150, 14, 2, 64, [_src(32, 3, 1, 9, 7, terms=1, Ax=2), _src(32, 1, 2, 18, 14, Ax=2)]),
    # fp16 residual, fp16 side output, even-grid fp32 output at an odd size
    "out16_sub2": lambda: conv_case("out16_sub2", 160, 14, 2, 64, [_src(32, 3, 1, 13, 9, Ax=2)], res="f16"),
}
GATHER_UNPOOL = {"unpool_c32": lambda: unpool_case("unpool_c32", 170, 14, 32, 2, 4, 5)}

# ---- exact-fp32 plans (OKP_F32): integer-valued operands, the plain fp64 sum ----------------------------------------------------------------------

F32 = {
    "f32_3x3_c32": lambda: conv_case("f32_3x3_c32", 200, 0, 2, 64, [_src(32, 3, 1, 9, 7, Ax=100, Aw=100)], integer=True),
    "f32_1x1_c36": lambda: conv_case("f32_1x1_c36", 210, 0, 2, 72, [_src(36, 1, 1, 9, 7, Ax=300, Aw=300)], integer=True),
    "f32_3x3_s2_c64": lambda: conv_case("f32_3x3_s2_c64", 220, 0, 2, 64, [_src(64, 3, 2, 11, 13, Ax=60, Aw=60)], integer=True),
}

# ---- patch-resident kernel (tile 13): cout 256, whole 16 x 16 blocks -----------------------------------------------------------------------------

PATCH = {
    "p_c32_16x16": lambda: conv_case("p_c32_16x16", 300, 14, 1, 256, [_src(32, 3, 1, 16, 16, Ax=2)]),
    "p_c32_subnormal": lambda: conv_case("p_c32_subnormal", 305, 16, 1, 256, [_src(32, 3, 1, 16, 16, zx=0.3, zw=0.3)]),
    "p_c64_2x16x32_windows": lambda: conv_case("p_c64_2x16x32_windows", 310, 14, 2, 256, [_src(64, 3, 1, 16, 32, zw=0.25)], res="f32"),
    "p_s2_c32_from_32": lambda: conv_case("p_s2_c32_from_32", 320, 14, 1, 256, [_src(32, 3, 2, 32, 32, Ax=2)]),
    "p_s2_c64_from_31": lambda: conv_case("p_s2_c64_from_31", 330, 14, 1, 256, [_src(64, 3, 2, 31, 31, zw=0.25)]),
    "p_3x3_plus_s2_skip": lambda: conv_case("p_3x3_plus_s2_skip", 340, 14, 1, 256, [_src(32, 3, 1, 16, 16), _src(32, 1, 2, 32, 32)]),
    "p_merge_1x1": lambda: conv_case("p_merge_1x1", 350, 14, 1, 256, [_src(64, 1, 1, 16, 16, Ax=2), _src(32, 1, 1, 16, 16, Ax=2)]),
}
PATCH_UNPOOL = {"p_unpool_c256": lambda: unpool_case("p_unpool_c256", 360, 14, 256, 2, 16, 16, zw=0.5)}


def sparse_rows(cout, cin, seed, nnz=3, a=4.0, s=14, exclude=()):
    """[cout, cin] weights with exactly `nnz` (odd) non-zero entries per row, each +-a + b 2^-s with |b| <= 1.  On activations +-1 + b 2^-s
    (|b| <= 1, none zero) and with a bias that is a multiple of 2a, the row's sum is an odd multiple of a plus a fraction of at most
    nnz (a + 1) 2^-s - never near zero.  With a = 4, nnz = 3 (fraction <= 15 x 2^-14; half an fp16 step just below 4 is 16 x 2^-14) fp16 of the
    sum is the integer: the next stage's split of this tensor is lossless with INTEGER high halves, so its products stay on the 2^-s
    lattice and it can be certified.  This is how sparse the producer of a re-split tensor has to be here.  exclude: input channels that
    hold zeros (no row may count on them for its parity)."""
    g = torch.Generator().manual_seed(seed)
    w = torch.zeros((cout, cin), dtype=torch.float64)
    allowed = torch.tensor([c for c in range(cin) if c not in exclude])
    for co in range(cout):
        ci = allowed[torch.randperm(len(allowed), generator=g)[:nnz]]
        w[co, ci] = a * (torch.randint(0, 2, (nnz,), generator=g).double() * 2 - 1) + torch.randint(-1, 2, (nnz,), generator=g).double() * 2.0 ** -s
    return w


def even_bias(cout, seed, a=4.0):
    g = torch.Generator().manual_seed(seed)
    return 2.0 * a * torch.randint(-1, 2, (cout,), generator=g).double()


def _pair_a():
    """Conv A of the pair-format chain: a 3x3 plan whose only non-zero weights are three channels of the centre tap per output channel
    (sparse_rows), no bias: +-4 or +-12 plus a small fraction at EVERY pixel (borders included), or 0 behind the ReLU.  Conv B's split of it
    is lossless with integer high halves, and B is certified on it.  No 2^-20 row: B re-splits this tensor, and a channel at 2^-20 would
    reach B with a high half that is no integer and a low half below fp16's range (the other patch cases carry the row on this kernel)."""
    w = torch.zeros((256, 32, 3, 3), dtype=torch.float64)
    w[:, :, 1, 1] = sparse_rows(256, 32, 377)
    return conv_case("p_pair_a", 370, 14, 1, 256, [_src(32, 3, 1, 16, 16, wt=w)], B=1, bias=False, tiny_row=None)


PAIR = {
    "p_pair_a": _pair_a,
    "p_pair_b": lambda: conv_case("p_pair_b", 380, 14, 1, 256, [_src(256, 3, 1, 16, 16, zw=0.94, x=get("p_pair_a").exact)], B=1),
}


# ---- okp_fire_x3: squeeze 1x1 -> [expand 1x1 | depth-wise 3x3] (+ skip) -> ReLU ---------------------------------------------------------------------

def one_by_one(x, w, b, s, what, step=None, res=None):
    """relu-less three-term 1x1 layer on the lattice: -> (exact value fp64, certificate); asserts lossless splits, the certificate and the
    lattice.  x [n, cin, h, w], w [cout, cin], b [cout]; step: per-channel lattice step (default 2^-s)."""
    scale = eo.row_scale([w])
    eo.assert_lossless(x, f"{what}: activations")
    eo.assert_split_on_lattice(x, s, f"{what}: activations")
    eo.assert_lossless(w, f"{what}: weights", scale=scale)
    v, a = eo.conv2d_three_term(x, w[:, :, None, None], scale=scale)
    y, a = v + b.view(1, -1, 1, 1), a + b.abs().view(1, -1, 1, 1)
    if res is not None:
        y, a = y + res, a + res.abs()
    step = 2.0 ** -s if step is None else step
    cert = eo.assert_certificate(a, step, what)
    eo.assert_on_lattice(y, step, what)
    return y, cert


SQ_TINY = 9                # the squeeze channel at 2^-20


def fire_case(name, seed, n, h, w, stride, s=14):
    """fire_module(256, 256) as okp_fire_x3 computes it.  The squeeze rows are sparse (sparse_rows) so that the squeeze tile keeps to 22
    significant bits with integer high halves: its in-kernel re-split is lossless, and the expand stage is certified ON THAT TILE.  The
    depth-wise branch is plain fp32 arithmetic on the fp32 squeeze tile (integer-valued weights: exact).  Stride 1: with skip; stride 2: without.

    Both plans carry a 2^-20 row.  Squeeze channel SQ_TINY: its re-split loses the low half (below fp16's range whatever the pre-scale), so
    the expand weights of that input channel are zero and the channel is seen by the depth-wise branch alone, which reads the fp32 tile -
    depth-wise bias of that channel at 2^-20 as well.  Expand row TINY_ROW as everywhere.  With the skip the residuals of those two output
    channels are x itself, 2^20 lattice steps above the sums: input channels TINY_ROW and 128 + SQ_TINY hold zeros in the stride-1 cases."""
    skip = stride == 1
    x = eo.lattice((n, 256, h, w), seed, 1, 1, s)
    dead = (TINY_ROW, 128 + SQ_TINY) if skip else ()
    for c in dead:
        x[:, c] = 0.0
    cs1 = chan_scale(128, SQ_TINY)
    w1, b1 = sparse_rows(128, 256, seed + 1, s=s, exclude=dead) * cs1.view(-1, 1), even_bias(128, seed + 2) * cs1
    sq, cert1 = one_by_one(x, w1, b1, s, f"{name}: squeeze", step=2.0 ** -s * cs1)       # the fp32 tile: what the depth-wise branch reads
    sq_e = sq.clone()
    sq_e[:, SQ_TINY] = 0.0                                             # what the expand GEMM sees of it: that channel meets zero weights
    assert eo.significant_bits(sq_e) <= 22
    sq_e = eo.resplit(sq_e, f"{name}: squeeze tile")
    assert not torch.equal(eo.resplit(sq[:, SQ_TINY]), sq[:, SQ_TINY])  # (the 2^-20 channel's own re-split does round)
    cs = chan_scale(128)
    wa = eo.lattice((128, 128), seed + 3, 1, 1, s, zero=0.5) * cs.view(-1, 1)
    wa[:, SQ_TINY] = 0.0
    ba = eo.lattice((128,), seed + 4, 3, 1, s) * cs
    sq_a = sq_e[:, :, ::stride, ::stride]                              # the pixels the strided 1x1 samples
    ya, cert2 = one_by_one(sq_a, wa, ba, s, f"{name}: expand", step=2.0 ** -s * cs, res=x[:, :128] if skip else None)
    wd = eo.integers((128, 3, 3), seed + 5, 2)
    assert bool((wd[SQ_TINY] != 0).any())
    bd = eo.lattice((128,), seed + 6, 3, 1, s) * cs1
    op = eo.conv2d_op(stride, 1, groups=128)
    yb = op(sq, wd[:, None]) + bd.view(1, -1, 1, 1)
    ab = op(sq.abs(), wd.abs()[:, None]) + bd.abs().view(1, -1, 1, 1)
    if skip:
        yb, ab = yb + x[:, 128:], ab + x[:, 128:].abs()
    cert3 = eo.assert_certificate(ab, 2.0 ** -s * cs1, f"{name}: depth-wise branch")
    eo.assert_on_lattice(yb, 2.0 ** -s * cs1, f"{name}: depth-wise branch")
    y = F.relu(torch.cat([ya, yb], dim=1))
    assert bool((y[:, TINY_ROW] > 0).any()) and bool((y[:, 128 + SQ_TINY] > 0).any())
    return SimpleNamespace(name=name, s=s, n=n, h=h, w=w, stride=stride, skip=skip, x=x, w1=w1, b1=b1, wa=wa, ba=ba, wd=wd, bd=bd, squeeze=sq,
                           expected=y.float(), exact=y, cert=max(cert1, cert2, cert3), certs=(cert1, cert2, cert3))


FIRE = {
    "fire_s1_16x16": lambda: fire_case("fire_s1_16x16", 400, 1, 16, 16, 1),
    "fire_s1_2x20x37": lambda: fire_case("fire_s1_2x20x37", 410, 2, 20, 37, 1),
    "fire_s2_from_32x32": lambda: fire_case("fire_s2_from_32x32", 420, 1, 32, 32, 2),
    "fire_s2_from_2x38x50": lambda: fire_case("fire_s2_from_2x38x50", 430, 2, 38, 50, 2),
}


# ---- split stem (okp_stem_x3_kernel): 7x7 / stride 2, 3 -> 128, ReLU -----------------------------------------------------------------------------------

def stem_case(name, seed, s, n, h, w, Ax=2, Aw=2, zw=0.0, u8=False):
    """u8: frames holding whole numbers 0 .. 255 (no low halves), on weights with three non-zero entries per output channel - 3 x 255 of the
    2^10 integer steps a 2^-14 lattice leaves under 2^24."""
    cs = chan_scale(128)
    if u8:
        g = torch.Generator().manual_seed(seed)
        x = torch.randint(0, 256, (n, 3, h, w), generator=g).double()
        wt = (sparse_rows(128, 147, seed + 1, a=1.0, s=s) + 0.0).reshape(128, 3, 7, 7)
    else:
        x = eo.lattice((n, 3, h, w), seed, Ax, 3, s)
        wt = eo.lattice((128, 3, 7, 7), seed + 1, Aw, 3, s, zw)
    wt = wt * cs.view(-1, 1, 1, 1)
    b = eo.lattice((128,), seed + 2, 3, 3, s) * cs
    scale = eo.row_scale([wt])
    eo.assert_lossless(x, f"{name}: frames", nontrivial=not u8)
    eo.assert_split_on_lattice(x, s, f"{name}: frames")
    eo.assert_lossless(wt, f"{name}: weights", scale=scale)
    v, a = eo.conv2d_three_term(x, wt, 2, 3, scale=scale)
    y, a = v + b.view(1, -1, 1, 1), a + b.abs().view(1, -1, 1, 1)
    step = 2.0 ** -s * cs
    cert = eo.assert_certificate(a, step, name)
    eo.assert_on_lattice(y, step, name)
    y = F.relu(y)
    return SimpleNamespace(name=name, s=s, n=n, h=h, w=w, x=x, wt=wt, bias=b, expected=y.float(), exact=y, cert=cert)


STEM = {
    "stem_33x33": lambda: stem_case("stem_33x33", 500, 14, 1, 33, 33),
    "stem_2x15x130": lambda: stem_case("stem_2x15x130", 510, 14, 2, 15, 130),
    "stem_33x33_subnormal": lambda: stem_case("stem_33x33_subnormal", 520, 16, 1, 33, 33, Ax=1, Aw=1),
    "stem_33x33_u8": lambda: stem_case("stem_33x33_u8", 530, 14, 1, 33, 33, u8=True),
}


# ---- one-launch heads (okp_heads_x3_kernel): 256 -> 3 x 128 -> 3 x 32 -> outputs ------------------------------------------------------------------------

def heads_case(name, seed, K, n, h, w, s=14):
    """Layer 1 rows are sparse (sparse_rows) so that the hidden tensor h1 is re-split without loss, with integer high halves; layer 2 (block
    diagonal: the heads do not mix) is certified on it; the last layer is a 32-term fp32 dot product with integer-valued weights - exact
    under its own certificate.  -> logits [n_out] per pixel in the order heat (K), depth (K), centers (2 (K - 1)).

    Layer 2 carries the 2^-20 row: channel TINY_ROW of the third head.  The last layer adds fp32 products, so that channel is read by ONE
    output alone - the last centre map, whose other weights are zero and whose bias is at 2^-20 too - and by no other.  Layer 1 carries none:
    h1 has no fp32 reader in the one-launch kernel, and the fraction of a 2^-20 channel of h1 has the unit of that row's weight low halves -
    if those are below fp16's range without the pre-scale, so is the low half of the re-split, and nothing downstream could tell."""
    x = eo.lattice((n, 256, h, w), seed, 1, 1, s)
    w1, b1 = sparse_rows(384, 256, seed + 1, s=s), even_bias(384, seed + 2)
    h1, cert1 = one_by_one(x, w1, b1, s, f"{name}: layer 1")
    h1 = eo.resplit(F.relu(h1), f"{name}: hidden layer 1")
    w2 = torch.zeros((96, 384), dtype=torch.float64)
    for i in range(3):
        w2[32 * i:32 * i + 32, 128 * i:128 * i + 128] = eo.lattice((32, 128), seed + 3 + i, 1, 1, s, zero=0.8)
    cs2 = torch.ones(96, dtype=torch.float64)
    cs2[64 + TINY_ROW] = TINY
    w2 = w2 * cs2.view(-1, 1)
    b2 = eo.lattice((96,), seed + 6, 3, 1, s) * cs2
    h2, cert2 = one_by_one(h1, w2, b2, s, f"{name}: layer 2", step=2.0 ** -s * cs2)
    h2 = F.relu(h2)
    assert bool((h2[:, 64 + TINY_ROW] > 0).any())
    n_out = [K, K, 2 * (K - 1)]
    w3 = eo.integers((sum(n_out), 32), seed + 7, 1, zero=0.3)
    b3 = eo.lattice((sum(n_out),), seed + 8, 3, 1, s)
    w3[2 * K:, TINY_ROW] = 0.0
    w3[-1] = 0.0
    w3[-1, TINY_ROW] = 2.0
    b3[-1] = b3[-1] * TINY
    step3 = torch.full((sum(n_out),), 2.0 ** -s, dtype=torch.float64)
    step3[-1] = 2.0 ** -s * TINY
    head_of = [i for i, c in enumerate(n_out) for _ in range(c)]
    logits = torch.stack([(h2[:, 32 * hd:32 * hd + 32] * w3[o].view(1, 32, 1, 1)).sum(1) + b3[o] for o, hd in enumerate(head_of)], dim=1)
    a3 = torch.stack([(h2[:, 32 * hd:32 * hd + 32] * w3[o].abs().view(1, 32, 1, 1)).sum(1) + b3[o].abs() for o, hd in enumerate(head_of)], dim=1)
    cert3 = eo.assert_certificate(a3, step3, f"{name}: last layer")
    eo.assert_on_lattice(logits, step3, f"{name}: last layer")
    return SimpleNamespace(name=name, s=s, K=K, n=n, h=h, w=w, x=x, w1=w1, b1=b1, w2=w2, b2=b2, w3=w3, b3=b3, head_of=head_of, h1=h1, h2=h2,
                           heat=logits[:, :K], depth=logits[:, K:2 * K], centers=logits[:, 2 * K:], cert=max(cert1, cert2, cert3),
                           certs=(cert1, cert2, cert3))


HEADS = {
    "heads_k3_2x9x7": lambda: heads_case("heads_k3_2x9x7", 600, 3, 2, 9, 7),
    "heads_k4_1x8x24": lambda: heads_case("heads_k4_1x8x24", 610, 4, 1, 8, 24),
}

TABLES = (GATHER, GATHER_UNPOOL, F32, PATCH, PATCH_UNPOOL, PAIR, FIRE, STEM, HEADS)


@functools.lru_cache(maxsize=None)
def get(name):
    for table in TABLES:
        if name in table:
            return table[name]()
    raise KeyError(name)


def all_names():
    return [k for table in TABLES for k in table]
