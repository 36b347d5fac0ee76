"""Exactly summable operands for the split-product kernels (docs/PRECISION.md, "Exact operands").  CPU only, does not import the product.

The split-product kernels round nowhere but in their fp32 accumulator.  On operands chosen so that every term and every partial sum of an
output element is an fp32 number, the result does not depend on the order of the sum - MFMA shape, tile, K order - and has to equal the
three-term sum  sum(x_hi w_hi + x_lo w_hi + x_hi w_lo)  bit for bit.

  lattice      an operand is 0 or a + b 2^-s with integers 1 <= |a| <= A, |b| <= B, B 2^-s < 2^-11: fp16(x) = a and fp16(x - a) = b 2^-s, both
               exactly - the split is lossless and the low half is not trivial.  s = 14: normal fp16 low halves; s = 16: subnormal ones.
  certificate  (sum of |term| over everything an output element accumulates, |bias| and |residual| included) / step < 2^24, step = 2^-s times
               the power of two of the output channel's weight row: every partial sum in any order is then a multiple of `step` below
               2^24 steps, i.e. an fp32 number.
  reference    the three-term sum in fp64 (exact under the certificate), NOT sum(x w): the lo * lo products are dropped.

Everything here is float64 on the CPU unless it says otherwise; a tensor is handed to the device as `.float()`, which is exact on the lattice."""
import math

import torch
import torch.nn.functional as F

LIMIT = 2.0 ** 24          # steps an IEEE fp32 accumulator holds exactly


# ---- lattice ----------------------------------------------------------------------------------------------------------------------------

def lattice(shape, seed, A, B, s, zero=0.0, scale=1.0):
    """Seeded lattice tensor: a + b 2^-s with a uniform in +-[1, A] and b uniform in [-B, B]; a fraction `zero` of the elements is 0.
    (a = 0 with b != 0 is not generated: it would make the high half tiny and the lattice step 2^-2s.)  `scale`: a power of two."""
    assert B * 2.0 ** -s < 2.0 ** -11 and A >= 1 and math.log2(scale) == int(math.log2(scale))
    g = torch.Generator().manual_seed(seed)
    a = torch.randint(1, A + 1, shape, generator=g).double() * (torch.randint(0, 2, shape, generator=g).double() * 2 - 1)
    b = torch.randint(-B, B + 1, shape, generator=g).double()
    x = a + b * 2.0 ** -s
    if zero > 0.0:
        x = x * (torch.rand(shape, generator=g) >= zero).double()
    return x * scale


def integers(shape, seed, A, zero=0.0):
    """Integer-valued operands in [-A, A] for the exact-fp32 plans: the certificate holds without a split."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(-A, A + 1, shape, generator=g).double()
    if zero > 0.0:
        x = x * (torch.rand(shape, generator=g) >= zero).double()
    return x


def split(x):
    """hi = fp16(x), lo = fp16(x - hi) of the fp32 value of x, as the kernels split an activation; both returned in fp64."""
    x32 = x.float()
    hi = x32.half()
    lo = (x32 - hi.float()).half()
    return hi.double(), lo.double()


def row_scale(ws, cout_dim=0):
    """The power of two a split-product plan multiplies an output channel's weights by before it splits them: the largest |w| of the row
    (over all taps and sources: `ws` is a list of weight tensors sharing the output-channel dimension) lands in [256, 512).  1 for a row of
    zeros.  -> [cout] fp64."""
    mx = torch.stack([w.abs().transpose(0, cout_dim).flatten(1).amax(dim=1) for w in ws]).amax(dim=0).double()
    _, e = torch.frexp(torch.where(mx > 0, mx, torch.ones_like(mx)))            # mx = f 2^e, f in [0.5, 1)
    return torch.where(mx > 0, torch.ldexp(torch.ones_like(mx), 9 - e), torch.ones_like(mx))


def split_weights(w, scale=None, cout_dim=0):
    """hi | lo of a weight tensor as a split-product plan stores them: scaled per output channel (`scale` = row_scale of the whole plan;
    None: of this tensor alone; False: not scaled - the defect), split in fp16, and scaled back (exact) so that the halves multiply unscaled
    activations.  -> (hi, lo) fp64."""
    if scale is False:
        return split(w)
    sc = row_scale([w], cout_dim) if scale is None else scale
    shape = [1] * w.dim()
    shape[cout_dim] = -1
    sc = sc.reshape(shape)
    hi, lo = split(w.double() * sc)
    return hi / sc, lo / sc


def assert_lossless(x, what, scale=None, cout_dim=0, nontrivial=True):
    """hi + lo == x exactly, and (nontrivial) the low halves are in use: non-zero in most non-zero elements."""
    hi, lo = split(x) if scale is None else split_weights(x, scale, cout_dim)
    assert torch.equal(hi + lo, x.double()), f"{what}: the fp16 split loses bits"
    if nontrivial:
        nz = x != 0
        assert int(nz.sum()) > 0 and float((lo[nz] != 0).double().mean()) > 0.5, f"{what}: trivial low halves"
    return hi, lo


def assert_split_on_lattice(x, s, what):
    """The halves of an activation lie where the certificate assumes them: hi integer-valued, lo a whole number of 2^-s (a GIVEN tensor - an
    earlier stage's output - has to show this; a generated one does by construction).  All products are then multiples of 2^-s."""
    hi, lo = split(x)
    assert torch.equal(hi, hi.round()) and torch.equal(lo * 2.0 ** s, (lo * 2.0 ** s).round()), f"{what}: halves off the lattice"


def significant_bits(x):
    """Largest number of significant bits of any element (0 for zeros): position of the leading one minus that of the trailing one, plus 1."""
    x = x.double().abs().flatten()
    x = x[x != 0]
    if x.numel() == 0:
        return 0
    m, _ = torch.frexp(x)                       # m in [0.5, 1): 53-bit integers after scaling
    k = (m * 2.0 ** 53).to(torch.int64)
    low = (k & -k).double().log2()              # trailing zeros
    return int((53 - low).max())


# ---- the three-term product of a linear operation -----------------------------------------------------------------------------------------

def split_product(op, x, w_hi, w_lo, terms=3, lo_lo=False):
    """op(x_hi, w_hi) + op(x_lo, w_hi) + op(x_hi, w_lo) in fp64 for a bilinear `op(x, w)` (terms = 1: the first product only, a single-term
    tap).  lo_lo adds op(x_lo, w_lo) - what the kernels must NOT compute."""
    x_hi, x_lo = split(x)
    y = op(x_hi, w_hi)
    if terms == 3:
        y = y + op(x_lo, w_hi) + op(x_hi, w_lo)
        if lo_lo:
            y = y + op(x_lo, w_lo)
    return y


def split_product_abs(op, x, w_hi, w_lo, terms=3):
    """Sum of the absolute values of the terms split_product adds up, per output element."""
    x_hi, x_lo = split(x)
    y = op(x_hi.abs(), w_hi.abs())
    if terms == 3:
        y = y + op(x_lo.abs(), w_hi.abs()) + op(x_hi.abs(), w_lo.abs())
    return y


def conv2d_op(stride=1, padding=0, groups=1):
    return lambda x, w: F.conv2d(x, w, stride=stride, padding=padding, groups=groups)


def conv_transpose2d_op(stride=2, padding=1):
    return lambda x, w: F.conv_transpose2d(x, w, stride=stride, padding=padding)


def conv2d_three_term(x, w, stride=1, padding=0, groups=1, scale=None, terms=3):
    """-> (value, sum of |terms|) of a (grouped) convolution as a split-product plan computes it, fp64."""
    w_hi, w_lo = split_weights(w, scale)
    op = conv2d_op(stride, padding, groups)
    return split_product(op, x, w_hi, w_lo, terms), split_product_abs(op, x, w_hi, w_lo, terms)


def conv_transpose2d_three_term(x, w, stride=2, padding=1, scale=None):
    """The same for a transposed convolution (weight [cin, cout, kh, kw]: the row scale runs over dimension 1)."""
    w_hi, w_lo = split_weights(w, scale, cout_dim=1)
    op = conv_transpose2d_op(stride, padding)
    return split_product(op, x, w_hi, w_lo), split_product_abs(op, x, w_hi, w_lo)


def conv2d_single_term(x, w, stride=1, padding=0, scale=None):
    """x_hi w_hi only: a tap with tap_terms = 1."""
    return conv2d_three_term(x, w, stride, padding, scale=scale, terms=1)


# ---- certificate ------------------------------------------------------------------------------------------------------------------------

def certificate(abs_sum, step):
    """log2 of the largest (sum of |terms|) / step over the tensor; `step`: the lattice step, a number or one per channel (dimension 1)."""
    if isinstance(step, torch.Tensor):
        step = step.reshape(1, -1, *([1] * (abs_sum.dim() - 2)))
    return float((abs_sum / step).max().log2())


def assert_certificate(abs_sum, step, what, limit=LIMIT):
    c = certificate(abs_sum, step)
    assert c < math.log2(limit), f"{what}: certificate 2^{c:.2f} is not below 2^{math.log2(limit):.0f} - partial sums may round"
    return c


def assert_on_lattice(y, step, what):
    """Every element of y is a whole number of steps below 2^24 of them: an fp32 number that any summation order reaches exactly."""
    if isinstance(step, torch.Tensor):
        step = step.reshape(1, -1, *([1] * (y.dim() - 2)))
    q = y.double() / step
    assert torch.equal(q, q.round()) and float(q.abs().max()) < LIMIT, f"{what}: not on the lattice"
    assert torch.equal(y.float().double(), y.double()), f"{what}: not an fp32 number"


# ---- deterministic roundings some outputs apply to the exact value ------------------------------------------------------------------------

def round_fp16(y):
    """The fp16 side output (okp_conv_args.out16): fp16 of the fp32 result, round to nearest even."""
    return y.float().half()


def round_pairs(y):
    """Pair format (okp_conv_args.out_pairs): hi = fp16(y), lo = fp16(y - hi) -> (hi, lo) as fp16 tensors."""
    y32 = y.float()
    hi = y32.half()
    return hi, (y32 - hi.float()).half()


def resplit(t, what=None, bits=22):
    """An intermediate tensor re-split by the next product stage (the fire module's squeeze tile, the heads' hidden layers): the value that
    stage multiplies is hi + lo.  Exact - returned unchanged - when the tensor keeps to `bits` significant bits (what = a name: asserted);
    explicitly rounded otherwise (what = None)."""
    hi, lo = split(t)
    if what is not None:
        assert significant_bits(t) <= bits, f"{what}: {significant_bits(t)} significant bits, the re-split would round"
        assert torch.equal(hi + lo, t.double()), f"{what}: the re-split loses bits"
    return hi + lo


# ---- fp32 accumulation of explicit term lists, in a given order (tests/test_exact_operands.py) -----------------------------------------------

def conv_terms(x, w_hi, w_lo, padding):
    """The terms of a stride-1 k x k convolution, one list per output element: -> fp32 [3, K, cout, n * L] with K = k k cin in (tap, channel)
    order, term kinds (x_hi w_hi, x_lo w_hi, x_hi w_lo)."""
    k = w_hi.shape[2]
    x_hi, x_lo = split(x)
    cin = x.shape[1]

    def unfold(t):                                  # [n, cin k k, L] with rows (channel, tap) -> [K = (tap, channel), n L]
        u = F.unfold(t, k, padding=padding)
        n, _, L = u.shape
        return u.reshape(n, cin, k * k, L).permute(2, 1, 0, 3).reshape(k * k * cin, n * L)

    def rows(t):                                    # [cout, cin, k, k] -> [K, cout]
        return t.permute(2, 3, 1, 0).reshape(k * k * cin, -1)

    xh, xl, wh, wl = unfold(x_hi), unfold(x_lo), rows(w_hi), rows(w_lo)
    t = torch.stack([xh[:, None, :] * wh[:, :, None], xl[:, None, :] * wh[:, :, None], xh[:, None, :] * wl[:, :, None]])
    assert torch.equal(t.float().double(), t)       # every term is an fp32 number
    return t.float()


def accumulate_fp32(terms, order):
    """Sequential fp32 sum of terms[kind, k] over the (kind, k) pairs of `order`."""
    acc = torch.zeros(terms.shape[2:], dtype=torch.float32)
    for kind, k in order:
        acc = acc + terms[kind, k]
    return acc


def order_k_steps(K, step):
    """Terms interleaved per K-step: the `step` x_hi w_hi products of a step, then its x_lo w_hi, then its x_hi w_lo."""
    return [(kind, k) for k0 in range(0, K, step) for kind in range(3) for k in range(k0, min(K, k0 + step))]


def order_chunks_outermost(n_taps, cin, chunk=32):
    """Channel chunk outermost, taps inside (the patch-resident kernel); order_k_steps is taps outermost (the gather tiles)."""
    return [(kind, t * cin + c) for c0 in range(0, cin, chunk) for t in range(n_taps) for kind in range(3) for c in range(c0, min(cin, c0 + chunk))]


def order_random(K, seed):
    g = torch.Generator().manual_seed(seed)
    return [(int(i) // K, int(i) % K) for i in torch.randperm(3 * K, generator=g)]


# ---- reporting --------------------------------------------------------------------------------------------------------------------------

def first_difference(got, want):
    """None if the tensors are bit-identical, else a line naming the first differing index with both values in hex."""
    assert tuple(got.shape) == tuple(want.shape), (tuple(got.shape), tuple(want.shape))
    if torch.equal(got, want):
        return None
    bad = (got != want) | (torch.isnan(got) != torch.isnan(want))
    idx = tuple(int(v) for v in bad.nonzero()[0])
    g, w = float(got[idx]), float(want[idx])
    hx = lambda v: v.hex() if math.isfinite(v) else repr(v)
    return f"{int(bad.sum())} of {bad.numel()} elements differ; first at {idx}: got {hx(g)} ({g!r}), expected {hx(w)} ({w!r})"
