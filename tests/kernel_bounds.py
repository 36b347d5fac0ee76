"""TEST INFRASTRUCTURE (CPU, fp64): the exact value of what a 16-bit kernel computes, and a rigorous per-element bound on how far the
device may be from it.

docs/PRECISION.md ("Kernel-level bounds") states the claim the bound rests on: the device arithmetic is an fp32-accumulated sum of exact
products of 16-bit operands, rounded once wherever a kernel stores.  A pair (val, err) of fp64 NCHW tensors is carried through the
stages a kernel performs:

    val   the exact value on the given operands - no intermediate rounding anywhere
    err   a bound on |device value - val|, element by element

The stages and their formulas are the whole model; there is no per-kernel multiplier.  Which stages a kernel performs, and where it
stores, is read from the kernel and written down where the chains are composed (the `*_chain` functions below cite file:line).

This module does not import the product.
"""
import torch
import torch.nn.functional as F

U = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11, torch.float32: 2.0 ** -24}      # half an ulp, relative
A = 2.0 ** -24                                                                             # unit roundoff of the fp32 accumulation
F16_TINY = 2.0 ** -14           # absolute term of a store to fp16: covers subnormal results however the hardware treats them

F64 = torch.float64


class Bounded:
    __slots__ = ("val", "err")

    def __init__(self, val, err=None):
        self.val = val.to(F64)
        self.err = torch.zeros_like(self.val) if err is None else err.to(F64)

    def ch(self, c0, c):
        return Bounded(self.val[:, c0:c0 + c], self.err[:, c0:c0 + c])

    @staticmethod
    def cat(parts):
        return Bounded(torch.cat([p.val for p in parts], 1), torch.cat([p.err for p in parts], 1))

    def ratio(self, got):
        """|got - val| / err per element (0 / 0 = 0: an element both sides know exactly; NaN counts as infinitely far), and the worst
        one with its index."""
        d = (got.to(F64) - self.val).abs()
        r = torch.where(d == 0, torch.zeros_like(d), d / self.err)
        r = torch.where(torch.isnan(r), torch.full_like(r, float("inf")), r)
        i = int(torch.argmax(r))
        return r, float(r.reshape(-1)[i]), tuple(int(v) for v in torch.unravel_index(torch.tensor(i), r.shape))


def exact(x):
    """An operand the test has rounded to the 16-bit type itself: err = 0."""
    return Bounded(x)


class Term:
    """One source of a linear stage: W applied to x as conv2d (dense or grouped) or conv_transpose2d."""

    def __init__(self, x, w, stride=1, padding=0, groups=1, transposed=False):
        self.x, self.w = x, w.to(F64)
        self.stride, self.padding, self.groups, self.transposed = stride, padding, groups, transposed

    def apply(self, t, w):
        if self.transposed:
            return F.conv_transpose2d(t, w, stride=self.stride, padding=self.padding)
        return F.conv2d(t, w, stride=self.stride, padding=self.padding, groups=self.groups)

    def n_terms(self):
        """Products accumulated per output element: cin of every tap that reaches it."""
        if self.transposed:         # [cin, cout, k, k]: an output element of sub-pixel class (a, b) sees (k / stride)^2 taps
            return self.w.shape[0] * (self.w.shape[2] // self.stride) * (self.w.shape[3] // self.stride)
        return self.w.shape[1] * self.w.shape[2] * self.w.shape[3]


def linear(terms, bias=None, res=None, w_round=None):
    """y = sum_terms W x + b (+ res), accumulated in fp32:
        err_y = L(|W|, err_x) + err_res + 2 (n + 2) a (L(|W|, |x|) + |b| + |res|)  [+ u L(|W|, |x|) where the kernel rounds W to w_round]
    The factor 2 over the classical any-order summation bound allows for the matrix instructions' internal accumulation order."""
    val = sum(t.apply(t.x.val, t.w) for t in terms)
    mag = sum(t.apply(t.x.val.abs(), t.w.abs()) for t in terms)
    err = sum(t.apply(t.x.err, t.w.abs()) for t in terms)
    n = sum(t.n_terms() for t in terms)
    if w_round is not None:
        err = err + U[w_round] * mag
    if bias is not None:
        b = bias.to(F64).view(1, -1, 1, 1)
        val, mag, n = val + b, mag + b.abs(), n + 1
    if res is not None:
        val, mag, err, n = val + res.val, mag + res.val.abs(), err + res.err, n + 1
    return Bounded(val, err + 2.0 * (n + 2) * A * mag)


def add(y, res):
    """y + res in fp32: the linear stage of one unit tap and a residual."""
    return linear([Term(y, torch.ones((y.val.shape[1], 1, 1, 1), dtype=F64), groups=y.val.shape[1])], res=res)


def relu(y):
    return Bounded(F.relu(y.val), y.err)


def store(y, dtype):
    """Round to nearest in `dtype`: err += u (|val| + err)."""
    err = y.err + U[dtype] * (y.val.abs() + y.err)
    if dtype == torch.float16:
        err = err + F16_TINY
    return Bounded(y.val, err)


def sigmoid(y):
    """fp32 sigmoid of the heat head: slope at most 1/4; 4 a allows for the device's exp and reciprocal."""
    return Bounded(torch.sigmoid(y.val), 0.25 * y.err + 4.0 * A)


# ------------------------------------------------------------------------------------------------------------------------------------
# Chains: the stages of each kernel, in the order its code performs them
# ------------------------------------------------------------------------------------------------------------------------------------

def conv_chain(terms, bias, dtype, relu_=True, res=None):
    """The implicit-GEMM convolutions: the gather kernel and the patch-resident kernel.
    Without a residual: acc + bias is rounded once into the LDS staging image (csrc/okp_igemm_kernel.h:603, csrc/okp_igemm_patch.hip:363)
    and the ReLU acts on the packed words (okp_igemm_kernel.h:697-707, okp_igemm_patch.hip:401-408): relu(round(x)) = round(relu(x)).
    With a residual the staged value is ALREADY rounded to the output type; the residual is added to it in fp32 and the sum is rounded a
    second time (okp_igemm_kernel.h:711-742, okp_igemm_patch.hip:410-419): two store points."""
    y = linear(terms, bias)
    if res is None:
        return store(relu(y) if relu_ else y, dtype)
    y = add(store(y, dtype), res)
    return store(relu(y) if relu_ else y, dtype)


def stem_chain(x, w, bias, dtype):
    """7x7 / stride 2 stem: bias in the accumulator, ReLU, one rounding where the pair is packed (csrc/okp_stem.hip:216)."""
    return store(relu(linear([Term(x, w, stride=2, padding=3)], bias)), dtype)


def dw_chain(x, w, bias, dtype, stride, res=None, relu_=True):
    """Stand-alone depth-wise 3x3: fp32 weights, fma chain from the bias, residual, ReLU, one rounding (csrc/okp_pointwise.hip:93-105)."""
    y = linear([Term(x, w, stride=stride, padding=1, groups=x.val.shape[1])], bias, res)
    return store(relu(y) if relu_ else y, dtype)


def fire_chain_module(x, m, dtype, dw_weights_rounded):
    """One fire module.  m: dict w1 [mid, cin, 1, 1], b1, wa [half, mid, 1, 1], ba, wd [half, 1, 3, 3] (fp32), bd, stride, skip.
    The squeeze tensor is rounded where it is written to LDS (okp_fire2.hip:563; okp_fire_chain.hip:218 entry, :341 chain, :490 exit) and is
    zero outside the frame; both branches add bias and skip in fp32 and round once (okp_fire2.hip:98 through relu_add_pack8, :954 on the
    vector ALUs; okp_fire_chain.hip:250 / :276 entry, :387-388 / :438 chain, :511 / :536 exit).
    dw_weights_rounded: the depth-wise taps are rounded to the activation type by the kernel (okp_fire2.hip:383, its matrix-pipe forms)."""
    half = m["wa"].shape[0]
    s = store(linear([Term(x, m["w1"])], m["b1"]), dtype)
    ra = x.ch(0, half) if m["skip"] else None
    rd = x.ch(half, half) if m["skip"] else None
    ya = linear([Term(s, m["wa"], stride=m["stride"])], m["ba"], ra)
    yd = linear([Term(s, m["wd"], stride=m["stride"], padding=1, groups=half)], m["bd"], rd, w_round=dtype if dw_weights_rounded else None)
    return store(relu(Bounded.cat([ya, yd])), dtype)


def fire2_chain(x, m, dtype):
    """okp_fire2: the launcher picks the matrix-pipe or the vector-ALU form by geometry; the weight-rounding term is added in every
    geometry, so the bound holds for either."""
    return fire_chain_module(x, m, dtype, True)


def resident_chain(x, mods, dtype):
    """okp_fire_chain: every module boundary is a store to LDS in the activation type; its depth-wise taps are fp32 in every phase
    (okp_fire_chain.hip:270-272, :422-429, :530-532 multiply by the fp32 table fetched by fetch_consts, :134-151)."""
    for m in mods:
        x = fire_chain_module(x, m, dtype, False)
    return x


def heads_chain(x, w1, b1, w2, b2, rows, dtype):
    """The three heads as the kernels lay them out: w1 [384, 256], w2 [96, 384] block diagonal, w3 [n_out, 32] with `src_off` per row.
    h1 is rounded where it is written to LDS (csrc/okp_heads.hip:140) and h2 is rounded to the activation type as well - kept as fp32
    bits, but of the rounded value (okp_heads.hip:162-163, in every instantiation); the three-launch path stores both as tensors
    (okp_igemm_kernel.h:603).  The last layer is an fp32 fma chain on fp32 weights (okp_heads.hip:176-178, okp_pointwise.hip:400-402).
    rows: (offset of the 32 input channels, weight row [32], bias, sigmoid?) per output map."""
    h1 = store(relu(linear([Term(x, w1)], b1)), dtype)
    h2 = store(relu(linear([Term(h1, w2)], b2)), dtype)
    return heads_out(h2, rows)


def heads_out(h2, rows):
    """The last layer of the heads on the 96 hidden channels h2: one map per row."""
    outs = []
    for off, w, b, sig in rows:
        y = linear([Term(h2.ch(off, 32), w.reshape(1, 32, 1, 1))], b.reshape(1))
        outs.append(sigmoid(y) if sig else y)
    return outs
