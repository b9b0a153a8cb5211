"""oracle/tower_fp64.py (the fp64 restatement the bf16 tower kernels are held to) checked without a GPU:
(a) against torch's float64 convolution / linear ops on random data, and (b) that the exact-regime generators of
tests/test_gpu_tower_exact.py meet the conditions under which a bf16 MFMA kernel must reproduce fp64 bit for bit."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import test_gpu_tower_exact as gen
from oracle import tower_fp64 as ref64

S, W, NPIX = gen.S, gen.W, gen.NPIX


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


def _integers_in(a, lo, hi):
    return bool((a == np.rint(a)).all() and a.min() >= lo and a.max() <= hi)


@pytest.mark.parametrize("iso", gen.ISOLATIONS)
def test_exact_block_generators_meet_the_exactness_conditions(iso):
    case = gen.exact_block_case(iso)
    h = case["h"]
    g, A1, out, A2 = gen.exact_block_reference(iso)
    assert A1.max() <= 256 and A2.max() <= 256
    assert _integers_in(g, 0, 256) and _integers_in(out, 0, 256) and _integers_in(h, 0, 256)
    assert (h[:NPIX] != 0).any(axis=0).all()                         # every (cin, pixel) site is non-zero in some position
    for c in range(W):                                               # no two positions share an input plane
        assert len(np.unique(h[:, c].reshape(gen.NPOS, NPIX), axis=0)) == gen.NPOS
    for k in ("c1", "c2", "res"):
        assert set(np.unique(case[k][0])) <= {-1.0, 0.0, 1.0} and _integers_in(case[k][1], -256, 256)
    # what the isolation is for: distinct biases per cout on the convolution under test, and an output that depends on it
    total = case["c2"][1] + case["res"][1]
    if iso == "conv1":
        assert len(set(case["c1"][1])) == W and not total.any() and case["res"][1].all() and np.array_equal(out, g)
    else:
        assert len(set(total)) == W and case["res"][1].all() and case["c2"][1].all()
        assert np.array_equal(g, h) if iso == "conv2" else not case["c2"][0].any()
    assert len(np.unique(out.reshape(gen.NPOS, -1), axis=0)) == gen.NPOS    # a stale buffer (another position's result) shows
    assert out.std() > 5                                             # ... and the outputs are not just the biases


def test_exact_stem_generator_meets_the_exactness_conditions():
    c = gen.exact_stem_case()
    y, A = ref64.stem(c["planes"], c["w"], c["b"])
    assert A.max() <= 256 and _integers_in(y, 0, 256)
    assert set(np.unique(c["planes"])) == {0.0, 1.0} and set(np.unique(c["w"])) == {-1.0, 0.0, 1.0} and len(set(c["b"])) == W
    p = c["planes"]
    assert p[0].all() and not p[1].any() and len(np.unique(p.reshape(gen.NDIST, -1), axis=0)) == gen.NDIST
    single = p[p.reshape(gen.NDIST, -1).sum(1) == 1]
    for cin in range(3):                                             # a single stone at every corner and edge of every plane
        for (yy, xx) in ((0, 0), (0, S - 1), (S - 1, 0), (S - 1, S - 1), (0, 5), (5, 0), (S - 1, 5), (5, S - 1)):
            assert single[:, cin, yy, xx].any()
    assert (np.abs(c["w"]).sum(axis=0) > 0).all()                    # every one of the 75 taps carries weight for some cout


def test_exact_heads_generator_meets_the_exactness_conditions():
    c = gen.exact_heads_case()
    vin, Av, pin, Ap = ref64.heads(c["h"], c["vconv"], c["pconv"])
    assert Av.max() <= 256 and Ap.max() <= 256 and _integers_in(vin, 0, 256) and _integers_in(pin, 0, 256)
    assert _integers_in(c["h"], 0, 256) and (c["h"] != 0).any(axis=0).all()
    assert len(np.unique(c["h"].reshape(gen.NDIST, -1), axis=0)) == gen.NDIST
    assert len(set(c["vconv"][1]) | set(c["pconv"][1])) == 20         # 20 distinct biases over the two heads


def test_exact_dense_generator_meets_the_exactness_conditions():
    c = gen.exact_dense_case()
    policy, value, logits, z = ref64.dense(c["vin"], c["pin"], c["vfc1"], c["vfc2"], c["pfc"])
    assert _integers_in(c["vin"], 0, 256) and _integers_in(c["pin"], 0, 256)
    assert _integers_in(logits * 4, -64, 64)                         # multiples of 2^-2, |logit| <= 16
    assert (np.abs(z) < 3).mean() >= 0.9                             # tanh is not saturated
    v1 = c["vin"] @ c["vfc1"][0] + c["vfc1"][1]
    av1 = np.abs(c["vin"]) @ np.abs(c["vfc1"][0]) + np.abs(c["vfc1"][1])
    assert _integers_in(v1, 0, 2 ** 24) and av1.max() < 2 ** 24      # fc1 stays on the ELU's x >= 0 side and is exact in fp32
    az = av1 @ np.abs(c["vfc2"][0])[:, 0] + abs(c["vfc2"][1][0])
    assert _integers_in(z * 2 ** 12, -2 ** 24, 2 ** 24) and az.max() * 2 ** 12 < 2 ** 24     # z: multiples of 2^-12 below 2^12
    al = np.abs(c["pin"]) @ np.abs(c["pfc"][0]) + np.abs(c["pfc"][1])
    assert al.max() * 4 < 2 ** 24
    assert set(np.unique(c["vfc2"][0] * 2 ** 12)) == {-1.0, 0.0, 1.0} and c["vfc2"][1][0] != 0
    assert set(np.unique(c["pfc"][0] * 4)) == {-1.0, 0.0, 1.0} and _integers_in(c["pfc"][1] * 4, -64, 64) and c["pfc"][1].any()
    for name in ("vin", "pin"):
        assert len(np.unique(c[name], axis=0)) == gen.NDIST
    for w in (c["vfc1"], c["vfc2"], c["pfc"]):                       # the packers round to bf16: nothing may change
        assert np.array_equal(ref64.bf16_round(w[0]), w[0]) and np.array_equal(ref64.bf16_round(w[1]), w[1])
    assert len(np.unique(np.round(value, 6))) > gen.NDIST // 2 and value.std() > 1e-3       # the positions do differ in value
    assert (policy.max(axis=1) > 0.05).all()                         # peaked enough that seven stray exp(0 - max) terms would show
