"""Operands and fp64 references (tests/kernel_bounds.py) of the kernel-level bound tests, shared by the CPU emulations
(tests/test_kernel_bounds.py) and the device runs (tests/test_gpu_kernel_bounds.py).

Operands are synth.normal_like as in tests/test_gpu_conv.py: weights scaled by 1 / sqrt(fan-in), bias 0.1 * normal.  Activations and
the weights of the matrix-pipe convolutions are rounded to the 16-bit type HERE, so that plan creation rounds nothing further; biases
and depth-wise taps stay fp32.  Every builder is cached: a reference is computed once and shared (callers do not modify it).
"""
import functools

import numpy as np
import torch

import kernel_bounds as kb

HALF = [torch.bfloat16, torch.float16]

CONV_SHAPES = [                         # (k, stride, cin, cout, n, h, w): the five shapes of test_gpu_conv.py::test_conv_matches_torch
    (3, 1, 64, 256, 2, 20, 24),
    (3, 2, 32, 64, 3, 17, 15),
    (1, 1, 192, 96, 2, 9, 7),
    (1, 2, 16, 8, 1, 8, 8),
    (3, 1, 8, 16, 1, 5, 5),
]
DW_SHAPES = [(128, 16, 16, 1, 2), (192, 9, 7, 1, 1), (64, 12, 12, 2, 2), (256, 8, 20, 1, 1)]      # (c, h, w, stride, n): test_standalone_depthwise_kernel


def rand(shape, seed):
    from object_keypoints_amd import synth
    return torch.from_numpy(synth.normal_like(f"kbound{seed}", tuple(shape), seed))


def q(v, dtype):
    return v.to(dtype).float()


def out_size(n, k, stride, pad):
    return (n + 2 * pad - k) // stride + 1


class Case:
    """Operands (fp32 tensors holding 16-bit values where the kernel takes 16-bit operands) + the fp64 reference with its bound."""

    def __init__(self, ref, **ops):
        self.ref = ref
        self.__dict__.update(ops)


@functools.lru_cache(maxsize=None)
def conv(k, stride, cin, cout, n, h, w, dtype, seed=1):
    x = q(rand((n, cin, h, w), seed), dtype)
    wt = q(rand((cout, cin, k, k), seed + 1) / np.sqrt(cin * k * k), dtype)
    b = rand((cout,), seed + 2) * 0.1
    ref = kb.conv_chain([kb.Term(kb.exact(x), wt, stride=stride, padding=(k - 1) // 2)], b, dtype)
    return Case(ref, x=x, wt=wt, b=b, k=k, stride=stride)


@functools.lru_cache(maxsize=None)
def conv_res(k, cin, cout, n, h, w, dtype, res_channels=None, res_c0=0, seed=9):
    """Stride-1 convolution + residual (read through a channel window of a `res_channels`-wide tensor) + ReLU."""
    x = q(rand((n, cin, h, w), seed), dtype)
    r = q(rand((n, res_channels or cout, h, w), seed + 1), dtype)
    wt = q(rand((cout, cin, k, k), seed + 2) / np.sqrt(cin * k * k), dtype)
    b = rand((cout,), seed + 3) * 0.1
    ref = kb.conv_chain([kb.Term(kb.exact(x), wt, padding=(k - 1) // 2)], b, dtype, res=kb.exact(r[:, res_c0:res_c0 + cout]))
    return Case(ref, x=x, r=r, wt=wt, b=b, res_c0=res_c0)


@functools.lru_cache(maxsize=None)
def two_source(k0, c0, c1, s1, cout, n, h, w, dtype, seed=4):
    """relu(conv k0 x k0 (t) + conv1x1 stride s1 (x) + bias): t at h x w, x at s1 h x s1 w."""
    t = q(rand((n, c0, h, w), seed), dtype)
    x = q(rand((n, c1, s1 * h, s1 * w), seed + 1), dtype)
    w0 = q(rand((cout, c0, k0, k0), seed + 2) / np.sqrt(c0 * k0 * k0), dtype)
    w1 = q(rand((cout, c1, 1, 1), seed + 3) / np.sqrt(c1), dtype)
    b = rand((cout,), seed + 4) * 0.1
    ref = kb.conv_chain([kb.Term(kb.exact(t), w0, padding=(k0 - 1) // 2), kb.Term(kb.exact(x), w1, stride=s1)], b, dtype)
    return Case(ref, t=t, x=x, w0=w0, w1=w1, b=b)


@functools.lru_cache(maxsize=None)
def unpool(c, n, h, w, dtype, seed=12):
    """up1 + conv_transpose2d(low, 4 x 4, stride 2, padding 1) + bias: no ReLU, the merge add is the residual of the four classes."""
    wt = q(rand((c, c, 4, 4), seed) / np.sqrt(4 * c), dtype)
    b = rand((c,), seed + 1) * 0.1
    low = q(rand((n, c, h, w), seed + 2), dtype)
    up1 = q(rand((n, c, 2 * h, 2 * w), seed + 3), dtype)
    ref = kb.conv_chain([kb.Term(kb.exact(low), wt, stride=2, padding=1, transposed=True)], b, dtype, relu_=False, res=kb.exact(up1))
    return Case(ref, wt=wt, b=b, low=low, up1=up1)


@functools.lru_cache(maxsize=None)
def stem(n, h, w, dtype, seed=11):
    x = q(rand((n, 3, h, w), seed), dtype)
    wt = q(rand((128, 3, 7, 7), seed + 1) / np.sqrt(147.0), dtype)
    b = rand((128,), seed + 2) * 0.1
    return Case(kb.stem_chain(kb.exact(x), wt, b, dtype), x=x, wt=wt, b=b)


@functools.lru_cache(maxsize=None)
def depthwise(c, h, w, stride, n, dtype, seed=41):
    x = q(rand((n, c, h, w), seed), dtype)
    wt = rand((c, 1, 3, 3), seed + 1) / 3.0                     # fp32 taps: the kernel multiplies by them as they are
    b = rand((c,), seed + 2) * 0.1
    r = q(rand((n, c, out_size(h, 3, stride, 1), out_size(w, 3, stride, 1)), seed + 3), dtype)
    return Case(kb.dw_chain(kb.exact(x), wt, b, dtype, stride, res=kb.exact(r)), x=x, wt=wt, b=b, r=r, stride=stride)


def fire_weights(cin, mid, stride, skip, dtype, seed):
    half = mid
    return {"w1": q(rand((mid, cin, 1, 1), seed) / np.sqrt(cin), dtype), "b1": rand((mid,), seed + 1) * 0.1,
            "wa": q(rand((half, mid, 1, 1), seed + 2) / np.sqrt(mid), dtype), "ba": rand((half,), seed + 3) * 0.1,
            "wd": rand((half, 1, 3, 3), seed + 4) / 3.0, "bd": rand((half,), seed + 5) * 0.1, "stride": stride, "skip": skip}


@functools.lru_cache(maxsize=None)
def fire2(cin, mid, stride, n, h, w, dtype, skip=None, seed=21):
    skip = (stride == 1 and cin == 2 * mid) if skip is None else skip
    m = fire_weights(cin, mid, stride, skip, dtype, seed)
    x = q(rand((n, cin, h, w), seed + 10), dtype)
    return Case(kb.fire2_chain(kb.exact(x), m, dtype), x=x, mods=[m])


@functools.lru_cache(maxsize=None)
def chain(c, n, h, w, count, dtype, seed=30):
    mods = [fire_weights(c, c // 2, 1, True, dtype, seed + 7 * i) for i in range(count)]
    x = q(rand((n, c, h, w), seed + 100), dtype)
    return Case(kb.resident_chain(kb.exact(x), mods, dtype), x=x, mods=mods)


@functools.lru_cache(maxsize=None)
def framed_chain(n, h, w, count, dtype, seed=60):
    """Stride-2 fire(384, 512) on an h x w map, `count` fire(512, 512), fire(512, 384)."""
    dims = [(384, 256, 2, False)] + [(512, 256, 1, True)] * count + [(512, 192, 1, False)]
    mods = [fire_weights(a, mid, st, sk, dtype, seed + 7 * i) for i, (a, mid, st, sk) in enumerate(dims)]
    x = q(rand((n, 384, h, w), seed + 100), dtype)
    return Case(kb.resident_chain(kb.exact(x), mods, dtype), x=x, mods=mods)


@functools.lru_cache(maxsize=None)
def heads(K, n, h, w, dtype, seed=80):
    """The three heads of a stack as KeypointNet._build_heads lays them out: 256 -> 3 x 128 -> 3 x 32 (block diagonal) -> K heat (sigmoid),
    K depth, 2 (K - 1) centre maps."""
    Fh = 128
    x = q(rand((n, 256, h, w), seed), dtype)
    w1 = q(rand((3 * Fh, 256, 1, 1), seed + 1) / 16.0, dtype)
    b1 = rand((3 * Fh,), seed + 2) * 0.1
    w2 = torch.zeros((96, 3 * Fh, 1, 1))
    for i in range(3):
        w2[32 * i:32 * i + 32, Fh * i:Fh * i + Fh] = q(rand((32, Fh, 1, 1), seed + 3 + i) / np.sqrt(Fh), dtype)
    b2 = rand((96,), seed + 6) * 0.1
    n_out = [K, K, 2 * (K - 1)]
    w3 = rand((sum(n_out), 32), seed + 7) / np.sqrt(32.0)       # fp32 weights of the last layer
    b3 = rand((sum(n_out),), seed + 8) * 0.1
    rows, o = [], 0
    for i, cnt in enumerate(n_out):
        for _ in range(cnt):
            rows.append((32 * i, w3[o], b3[o], i == 0))
            o += 1
    outs = kb.heads_chain(kb.exact(x), w1, b1, w2, b2, rows, dtype)
    cat = lambda lo, hi: kb.Bounded(torch.cat([v.val for v in outs[lo:hi]], 1), torch.cat([v.err for v in outs[lo:hi]], 1))
    ref = {"heat": cat(0, K), "depth": cat(K, 2 * K), "centers": cat(2 * K, 4 * K - 2)}
    # the heat logits (no sigmoid): what the measured share of the sigmoid allowance is taken against
    rows_l = [(off, wr, br, False) for off, wr, br, _ in rows[:K]]
    logits = kb.heads_chain(kb.exact(x), w1, b1, w2, b2, rows_l, dtype)
    ref["logits"] = kb.Bounded(torch.cat([v.val for v in logits], 1), torch.cat([v.err for v in logits], 1))
    return Case(ref, x=x, w1=w1, b1=b1, w2=w2, b2=b2, w3=w3, b3=b3, K=K, rows=rows)
