"""The exact-operand instrument itself, on the CPU (docs/PRECISION.md, "Exact operands"):

 1. every case tests/test_gpu_split_exact.py runs passes its certificate and the lossless-split check;
 2. an fp32 emulation of the accumulation gives the reference's bits in every order tried - the certificate does what it claims;
 3. each of seven planted kernel defects changes at least one bit of the result on the lattice, and the table printed here (pytest -s) says
    how far the same defect moves a GENERIC random-operand result relative to the tolerance the other split-product tests allow,
    1e-5 (1 + max|ref|): two of the seven stay inside it, three more pass it by less than a factor of ten."""
import pytest
import torch
import torch.nn.functional as F

import exact_operands as eo
import exact_operands_cases as ec


# ---- 1. the cases of the GPU file -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ec.all_names())
def test_case_passes_its_certificate_and_splits_without_loss(name):
    c = ec.get(name)                                            # (the builder asserts both; a case that cannot be certified does not exist)
    print(f"CERT {name}: 2^{c.cert:.2f}")
    assert c.cert < 24.0


def test_lattice_halves_and_the_row_that_needs_the_pre_scale():
    for s in (14, 16):
        x = eo.lattice((4, 32, 9, 7), 1, 2 if s == 14 else 1, 3, s)
        hi, lo = eo.assert_lossless(x, f"s = {s}")
        assert torch.equal(hi, hi.round()) and float(hi.abs().min()) >= 1.0
        tiny = lo[lo != 0].abs()
        assert bool((tiny < 2.0 ** -14).all()) == (s == 16)     # s = 16: every low half is an fp16 subnormal; s = 14: none is
    c = ec.get("3x3_c32")
    w = c.ws[0]
    hi, lo = eo.split_weights(w, False)                          # not scaled: the 2^-20 row loses its low halves ...
    assert not torch.equal((hi + lo)[ec.TINY_ROW], w[ec.TINY_ROW]) and bool((lo[ec.TINY_ROW] == 0).all())
    hi, lo = eo.split_weights(w, c.scale)                        # ... and keeps them with the plan's per-channel power of two
    assert torch.equal(hi + lo, w) and bool((lo[ec.TINY_ROW] != 0).any())
    assert bool((torch.log2(c.scale) == torch.log2(c.scale).round()).all())


def test_the_reference_is_the_three_term_sum_not_the_full_product():
    """The dropped lo * lo products are non-zero in almost every element: `lo * lo is dropped` is pinned too."""
    c = ec.get("3x3_c32")
    full = F.relu(F.conv2d(c.xs[0], c.ws[0], c.bias, padding=1))
    live = c.exact > 0
    assert float((full[live] != c.exact[live]).double().mean()) > 0.95


def test_resplit_and_output_roundings():
    t = torch.tensor([37.0 + 5 * 2.0 ** -14, -4.0 + 15 * 2.0 ** -14, 0.0, 12.0 - 2.0 ** -14], dtype=torch.float64)
    assert torch.equal(eo.resplit(t, "exact tensor"), t)
    wide = torch.tensor([1.0 + 2.0 ** -11 + 2.0 ** -23], dtype=torch.float64)              # 24 significant bits: the re-split rounds
    assert eo.significant_bits(wide) == 24 and not torch.equal(eo.resplit(wide), wide)
    with pytest.raises(AssertionError):
        eo.resplit(wide, "wide tensor")
    hi, lo = eo.round_pairs(t)
    assert torch.equal(hi.double() + lo.double(), t) and torch.equal(eo.round_fp16(t), hi)


# ---- 2. fp32 accumulation in several orders ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["3x3_c32", "3x3_c32_subnormal", "1x1_c36", "defect_s14"])
def test_fp32_accumulation_in_any_order_gives_the_reference_bits(name):
    c = defect_case(14) if name == "defect_s14" else ec.get(name)
    d, x, w = c.srcs[0], c.xs[0], c.ws[0]
    w_hi, w_lo = eo.split_weights(w, c.scale)
    terms = eo.conv_terms(x, w_hi, w_lo, (d["k"] - 1) // 2)
    K, n_taps, cin = terms.shape[1], d["k"] ** 2, d["cin"]
    orders = {
        "K-steps of 16, taps outermost": eo.order_k_steps(K, 16),
        "K-steps of 32, taps outermost": eo.order_k_steps(K, 32),
        "channel chunks of 16 outermost": eo.order_chunks_outermost(n_taps, cin, 16),
        "reversed": eo.order_k_steps(K, 32)[::-1],
        "random permutation": eo.order_random(K, 5),
    }
    want = c.expected.permute(1, 0, 2, 3).reshape(c.cout, -1)
    for what, order in orders.items():
        assert sorted(order) == sorted(eo.order_k_steps(K, 16)), what          # every term once
        acc = eo.accumulate_fp32(terms, order)
        got = F.relu(acc + c.bias.float().view(-1, 1))                          # (fp32: one more exact addition)
        diff = eo.first_difference(got, want)
        assert diff is None, f"{name}, {what}: {diff}"


# ---- 3. planted defects ---------------------------------------------------------------------------------------------------------------------------

DEFECTS = ["kstep", "halo", "flush", "lolo", "prescale", "bias_order", "khalves"]
DEFECT_TEXT = {
    "kstep": "x_lo w_hi missing in one 32-channel K-step of one tap",
    "halo": "low halves missing on the halo ring of one 16x16 block",
    "flush": "subnormal low halves flushed to zero (s = 16)",
    "lolo": "lo * lo added",
    "prescale": "weight pre-scale skipped for the 2^-20 row",
    "bias_order": "bias added before the output scale",
    "khalves": "K halves of one 128-byte weight row exchanged",
}


def defect_case(s):
    """3x3, 64 -> 64 channels on one 18 x 18 map: a whole 16 x 16 block with a halo ring inside the map, two 32-channel K-steps per tap."""
    return ec.conv_case(f"defect_s{s}", 700 + s, s, 1, 64, [ec._src(64, 3, 1, 18, 18, zx=0.5 if s == 16 else 0.0, zw=0.5 if s == 16 else 0.25)])


def split_conv_model(x, w, b, defect=None):
    """relu(3x3 split-product convolution + bias) in fp64 with one defect planted (None: the specification)."""
    scale = eo.row_scale([w])
    w_hi, w_lo = eo.split_weights(w, scale)
    x_hi, x_lo = eo.split(x)
    op = eo.conv2d_op(1, 1)
    if defect == "prescale":
        u_hi, u_lo = eo.split_weights(w, False)
        w_hi, w_lo = w_hi.clone(), w_lo.clone()
        w_hi[ec.TINY_ROW], w_lo[ec.TINY_ROW] = u_hi[ec.TINY_ROW], u_lo[ec.TINY_ROW]
    if defect == "khalves":                                       # row 9, tap (2, 0), channels 32 .. 63: [k0-15] <-> [k16-31]
        w_hi, w_lo = w_hi.clone(), w_lo.clone()
        for t in (w_hi, w_lo):
            t[9, 32:64, 2, 0] = torch.cat([t[9, 48:64, 2, 0], t[9, 32:48, 2, 0]])
    if defect == "flush":
        x_lo = torch.where(x_lo.abs() < 2.0 ** -14, torch.zeros_like(x_lo), x_lo)
    lh = op(x_lo, w_hi)
    if defect == "kstep":                                         # tap (0, 2), channels 32 .. 63
        wk, xk = torch.zeros_like(w_hi), torch.zeros_like(x_lo)
        wk[:, 32:, 0, 2], xk[:, 32:] = w_hi[:, 32:, 0, 2], x_lo[:, 32:]
        lh = lh - op(xk, wk)
    if defect == "halo":                                          # block rows / columns 0 .. 15: its patch's ring is row 16 and column 16
        ring = x_lo.clone()
        ring[:, :, 16, :17] = 0.0
        ring[:, :, :17, 16] = 0.0
        lh[:, :, :16, :16] = op(ring, w_hi)[:, :, :16, :16]
    acc = op(x_hi, w_hi) + lh + op(x_hi, w_lo)
    if defect == "lolo":
        acc = acc + op(x_lo, w_lo)
    bias = b / scale if defect == "bias_order" else b             # (acc scale + bias) / scale instead of fma(acc, 1 / scale, bias)
    return F.relu(acc + bias.view(1, -1, 1, 1))


def generic_operands(seed=11):
    """What the other split-product tests feed: normal activations, weights of unit output variance (one row at 2^-20 of that), small bias."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((1, 64, 18, 18), generator=g, dtype=torch.float64).float().double()
    w = (torch.randn((64, 64, 3, 3), generator=g, dtype=torch.float64) / 24.0 * ec.chan_scale(64).view(-1, 1, 1, 1)).float().double()
    b = (0.1 * torch.randn((64,), generator=g, dtype=torch.float64) * ec.chan_scale(64)).float().double()
    return x, w, b


def test_every_planted_defect_changes_a_bit_and_some_pass_the_max_abs_tolerance():
    gx, gw, gb = generic_operands()
    g_ref = split_conv_model(gx, gw, gb)
    tol = 1e-5 * (1.0 + float(g_ref.abs().max()))
    rows, inside = [], []
    for d in DEFECTS:
        c = defect_case(16 if d == "flush" else 14)
        x, w, b = c.xs[0], c.ws[0], c.bias
        assert torch.equal(split_conv_model(x, w, b).float(), c.expected)                      # the model IS the reference
        bad = split_conv_model(x, w, b, d).float()
        changed = int((bad != c.expected).sum())
        assert changed >= 1, f"{DEFECT_TEXT[d]}: no bit of the exact-operand result changes"
        move = float((split_conv_model(gx, gw, gb, d) - g_ref).abs().max())
        rows.append((DEFECT_TEXT[d], changed, c.expected.numel(), move / tol))
        if move <= tol:
            inside.append(d)
    print("\nDEFECT TABLE: elements changed on exact operands | largest move of a generic result / (1e-5 (1 + max|ref|))")
    for text, changed, total, ratio in rows:
        print(f"DEFECT | {text:<62} | {changed:>5} of {total} | {ratio:9.3g} | {'passes the tolerance' if ratio <= 1.0 else 'caught by the tolerance'}")
    # the gap this file closes: defects the max-abs tolerance passes (docs/PRECISION.md lists them; if this list changes, so must the text)
    assert inside == ["lolo", "prescale"], inside
