"""oracle/tower_fp64.py (the fp64 restatement the bf16 tower kernels are held to) checked without a GPU:
(a) against torch's float64 convolution / linear ops on random data, and (b) that the 11x11 exact-regime cases of
tests/tower_cases.py meet the conditions, stated there, under which a bf16 MFMA kernel must reproduce fp64 bit for bit."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import tower_cases as gen
from oracle import tower_fp64 as ref64

S, W = 11, gen.W
NPIX = gen.SIZES[S].NPIX



def _close(a, b):
    """1e-12 relative to the largest reference value (plain fp64 sums of a few thousand terms in another order)."""
    b = b.numpy() if isinstance(b, torch.Tensor) else b
    assert a.shape == b.shape
    assert np.abs(a - b).max() <= 1e-12 * max(1.0, np.abs(b).max())


def test_bf16_round_is_round_to_nearest_even():
    rng = np.random.default_rng(0)
    x = np.concatenate([rng.standard_normal(20000) * 10.0 ** rng.integers(-6, 6, 20000),
                        [0.0, 1.0, -1.0, 256.0, 257.0, 258.0, 259.0, 1.00390625, 1.01171875, -1.00390625]]).astype(np.float32)
    want = torch.from_numpy(x).bfloat16().double().numpy()           # fp32 -> bf16 on the CPU is round-to-nearest-even
    assert np.array_equal(ref64.bf16_round(x.astype(np.float64)), want)
    # ties: 257 lies between 256 and 258 -> even mantissa 256; 259 between 258 and 260 -> 260
    assert ref64.bf16_round(257.0) == 256.0 and ref64.bf16_round(259.0) == 260.0
    # straight from fp64: just above a tie rounds up, although a detour through fp32 would land on the tie and round to even
    assert ref64.bf16_round(1.00390625 + 2.0 ** -40) == 1.0078125


def test_reference_layers_match_torch_float64():
    rng = np.random.default_rng(1)
    r = lambda *s: rng.standard_normal(s)  # noqa: E731
    t = torch.from_numpy
    B = 5
    planes, sw, sb = r(B, 3, S, S), r(W, 3, 5, 5) * 0.2, r(W)
    y, A = ref64.stem(planes, sw, sb)
    _close(y, F.elu(F.conv2d(t(planes), t(sw), t(sb), padding=2)))
    _close(A, F.conv2d(t(planes).abs(), t(sw).abs(), t(sb).abs(), padding=2))
    h = r(B, W, S, S)
    c1, c2, res = (r(W, W, 3, 3) * 0.05, r(W)), (r(W, W, 3, 3) * 0.05, r(W)), (r(W, W, 1, 1) * 0.1, r(W))
    g, A1, out, A2 = ref64.block(h, c1, c2, res)
    tg = F.elu(F.conv2d(t(h), t(c1[0]), t(c1[1]), padding=1))
    _close(g, tg)
    _close(A1, F.conv2d(t(h).abs(), t(c1[0]).abs(), t(c1[1]).abs(), padding=1))
    mid = t(ref64.bf16_round(g))                                     # the mid activation is rounded to bf16 where the kernel stores it
    assert torch.equal(mid.bfloat16().double(), mid) and bool(((mid - tg).abs() <= 2.0 ** -8 * tg.abs()).all())
    _close(out, F.elu(F.conv2d(t(h), t(res[0]), t(res[1])) + F.conv2d(mid, t(c2[0]), t(c2[1]), padding=1)))
    _close(A2, F.conv2d(t(h).abs(), t(res[0]).abs(), t(res[1]).abs()) + F.conv2d(mid.abs(), t(c2[0]).abs(), t(c2[1]).abs(), padding=1))
    other = r(B, W, S, S)                                            # ... or is the one the caller read back
    _, _, out_m, _ = ref64.block(h, c1, c2, res, mid=other)
    _close(out_m, F.elu(F.conv2d(t(h), t(res[0]), t(res[1])) + F.conv2d(t(other), t(c2[0]), t(c2[1]), padding=1)))
    vconv, pconv = (r(4, W, 1, 1) * 0.1, r(4)), (r(16, W, 1, 1) * 0.1, r(16))
    vin, Av, pin, Ap = ref64.heads(h, vconv, pconv)
    _close(vin, F.elu(F.conv2d(t(h), t(vconv[0]), t(vconv[1]))).reshape(B, -1))          # flattened in NCHW order
    _close(pin, F.elu(F.conv2d(t(h), t(pconv[0]), t(pconv[1]))).reshape(B, -1))
    _close(Av, F.conv2d(t(h).abs(), t(vconv[0]).abs(), t(vconv[1]).abs()).reshape(B, -1))
    _close(Ap, F.conv2d(t(h).abs(), t(pconv[0]).abs(), t(pconv[1]).abs()).reshape(B, -1))
    vfc1, vfc2, pfc = (r(4 * NPIX, 64) * 0.05, r(64)), (r(64, 1) * 0.1, r(1)), (r(16 * NPIX, NPIX) * 0.02, r(NPIX))
    policy, value, logits, z = ref64.dense(vin, pin, vfc1, vfc2, pfc)
    tz = F.linear(F.elu(F.linear(t(vin), t(vfc1[0]).T, t(vfc1[1]))), t(vfc2[0]).T, t(vfc2[1]))[:, 0]
    tl = F.linear(t(pin), t(pfc[0]).T, t(pfc[1]))
    _close(z, tz)
    _close(value, torch.tanh(tz / 2))
    _close(logits, tl)
    _close(policy, torch.softmax(tl, dim=1))


@pytest.mark.parametrize("iso", gen.ISOLATIONS)
def test_exact_block_generators_meet_the_exactness_conditions(iso):
    gen.check_exact_block_generator(S, iso)


def test_exact_stem_generator_meets_the_exactness_conditions():
    gen.check_exact_stem_generator(S)


def test_exact_heads_generator_meets_the_exactness_conditions():
    gen.check_exact_heads_generator(S)


def test_exact_dense_generator_meets_the_exactness_conditions():
    gen.check_exact_dense_generator(S)
