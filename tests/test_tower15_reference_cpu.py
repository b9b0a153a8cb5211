"""The 15x15 cases of the bf16 tower kernels (csrc/af_tower_bf16.hip, Geo<15>): their generators, and — without a GPU, from
oracle/tower_fp64.py alone — the conditions under which a bf16 MFMA kernel must reproduce fp64 bit for bit on them: every stored
activation is an integer in [0, 256], every partial sum is exact in fp32 in any order, every pre-activation of the exact regime is
>= 0 (the kernels' ELU returns x itself there).  tests/test_gpu_tower15_exact.py runs the kernels on these cases; the regimes and
the three isolations of a residual block are those of tests/test_gpu_tower_exact.py:
    "conv1": c2 = centre-tap identity, projection 0, b2 + b_res = 0   ->  h' = ELU(g),  g = ELU(conv1(h) + b1)
    "conv2": c1 = centre-tap identity, b1 = 0 (g = ELU(h))            ->  h' = ELU(conv2(g) + b2 + b_res)
    "proj" : c2 = 0                                                   ->  h' = ELU(proj(h) + b_res + b2)

What the larger board changes in the generators: 225 pixels (a stone stride of 37 is coprime to 225 as it is to 121), stones on both
sides of the row-7 / row-8 seam at which the convolution splits a board into halves, and the dense layers' fan-in: value fc1 sums
900 terms instead of 484 and the policy 3600 instead of 1936, so fc1's biases start at 192 (even above 256: bf16 values) instead of
128, and the policy weights are thinned to keep |logit| <= 16."""
import functools

import numpy as np
import pytest

from oracle import tower_fp64 as ref64

S, W, NPIX = 15, 128, 225
STRIDE = 37                      # coprime to 225: (37 c + b) mod 225 walks every pixel as b does
NPOS = 232                       # positions of the block generators: 225 cover every (cin, pixel) site once, 7 more carry a second stone
NDIST = 64                       # distinct positions of the stem / heads / dense generators (larger batches tile them)
NROUND = 140                     # rounded regime: 280 half boards, more than one pass of 256 workgroups; its first 33 are the other batch
ISOLATIONS = ("conv1", "conv2", "proj")
# single stones of the stem planes: corners, edge midpoints, centre, and both sides of the seam between board rows 7 and 8
STEM_STONES = ((0, 0), (0, S - 1), (S - 1, 0), (S - 1, S - 1), (0, 7), (7, 0), (S - 1, 7), (7, S - 1), (7, 7),
               (8, 7), (8, 0), (8, S - 1), (7, 3), (8, 3))


def _identity3():
    w = np.zeros((W, W, 3, 3))
    w[np.arange(W), np.arange(W), 1, 1] = 1.0
    return w


def _distinct_bias(rng, lo):
    """128 distinct integers lo .. lo + 127, shuffled: a bias delivered to the wrong cout is a wrong integer."""
    return (lo + rng.permutation(W)).astype(np.float64)


def exact_block_input():
    """[NPOS, 128, 15, 15]: position b holds one stone of value 1..3 per channel c, at pixel (37 c + b) mod 225 — over the first
    225 positions every (cin, pixel) site is non-zero exactly once; positions 225..231 hold a second stone 112 pixels on."""
    h = np.zeros((NPOS, W, NPIX))
    c = np.arange(W)
    for b in range(NPOS):
        h[b, c, (STRIDE * c + b) % NPIX] = 1 + (c + b) % 3
        if b >= NPIX:
            h[b, c, (STRIDE * c + b + 112) % NPIX] = 1 + (2 * c + b) % 3
    return h.reshape(NPOS, W, S, S)


def _split(total, rng):
    """total = b2 + b_res with both parts positive integers (the kernels see only their sum)."""
    b_res = 1.0 + rng.permutation(W) % 32
    return total - b_res, b_res


@functools.lru_cache(maxsize=None)
def exact_block_case(iso):
    """-> dict(h, c1, c2, res): weights in {-1, 0, 1}, integer biases distinct per cout."""
    rng = np.random.default_rng({"conv1": 51, "conv2": 52, "proj": 53}[iso])
    w3 = lambda: rng.integers(-1, 2, size=(W, W, 3, 3)).astype(np.float64)  # noqa: E731
    zero3, zero1, zb = np.zeros((W, W, 3, 3)), np.zeros((W, W, 1, 1)), np.zeros(W)
    if iso == "conv1":
        b2 = 1.0 + rng.permutation(W) % 8
        case = dict(c1=(w3(), _distinct_bias(rng, 48)), c2=(_identity3(), b2), res=(zero1, -b2))
    elif iso == "conv2":
        b2, b_res = _split(_distinct_bias(rng, 48), rng)
        case = dict(c1=(_identity3(), zb), c2=(w3(), b2), res=(zero1, b_res))
    else:
        b2, b_res = _split(_distinct_bias(rng, 48), rng)
        case = dict(c1=(w3(), _distinct_bias(rng, 48)), c2=(zero3, b2),
                    res=(rng.integers(-1, 2, size=(W, W, 1, 1)).astype(np.float64), b_res))
    case["h"] = exact_block_input()
    return case


@functools.lru_cache(maxsize=None)
def exact_block_reference(iso):
    """-> (g, A1, h', A2) of oracle.tower_fp64.block on the NPOS positions of the case."""
    c = exact_block_case(iso)
    return ref64.block(c["h"], c["c1"], c["c2"], c["res"])


def _stone_planes(rng, n):
    """[n, 3, 15, 15] of 0 / 1: a full board, an empty one, a single stone in every plane at each of STEM_STONES, random fill."""
    x = np.zeros((n, 3, S, S))
    x[0] = 1.0
    k = 2
    for (yy, xx) in STEM_STONES:
        for c in range(3):
            x[k, c, yy, xx] = 1.0
            k += 1
    for b in range(k, n):
        x[b] = rng.random((3, S, S)) < (0.1 + 0.8 * (b - k) / (n - k))
    return x


@functools.lru_cache(maxsize=None)
def exact_stem_case():
    rng = np.random.default_rng(61)
    w = rng.integers(-1, 2, size=(W, 3, 5, 5)) * (rng.random((W, 3, 5, 5)) < 0.75)
    return dict(planes=_stone_planes(rng, NDIST), w=w.astype(np.float64), b=_distinct_bias(rng, 60))


@functools.lru_cache(maxsize=None)
def exact_heads_case():
    rng = np.random.default_rng(62)
    h = rng.integers(1, 3, size=(NDIST, W, S, S)) * (rng.random((NDIST, W, S, S)) < 0.5)
    wgt = lambda n: (rng.integers(-1, 2, size=(n, W, 1, 1)) * (rng.random((n, W, 1, 1)) < 0.75)).astype(np.float64)  # noqa: E731
    return dict(h=h.astype(np.float64), vconv=(wgt(4), 100.0 + rng.permutation(4)), pconv=(wgt(16), 104.0 + rng.permutation(16)))


@functools.lru_cache(maxsize=None)
def exact_dense_case():
    """vin / pin integers, vfc1 in {-1, 0, 1} under biases that keep its ELU on x >= 0, vfc2 in {0, +-2^-12} with bias 0.25,
    pfc in {0, +-2^-2} with biases that are multiples of 2^-2: logits and z are exact in fp32 in any summation order.
    fc1 sums 900 terms of standard deviation 0.91 (x in {0, 1, 2} with P(0) = 1/2, w in {-1, 0, 1}): sigma = 27.4, so the biases
    192, 194 .. 318 (even: bf16 values above 256) start at 7 sigma.  The policy sums 3600 terms; its weights are non-zero with
    probability 0.2 * 2/3, which gives the logits the standard deviation (2.7) they have on the 11x11 board."""
    rng = np.random.default_rng(63)
    vin = rng.integers(1, 3, size=(NDIST, 4 * NPIX)) * (rng.random((NDIST, 4 * NPIX)) < 0.5)
    pin = rng.integers(1, 3, size=(NDIST, 16 * NPIX)) * (rng.random((NDIST, 16 * NPIX)) < 0.1)
    vfc1 = (rng.integers(-1, 2, size=(4 * NPIX, 64)).astype(np.float64), 192.0 + 2.0 * rng.permutation(64))
    vfc2 = (rng.choice([1.0, 1.0, -1.0, 0.0], size=(64, 1)) * 2.0 ** -12, np.array([0.25]))
    pfc = ((rng.integers(-1, 2, size=(16 * NPIX, NPIX)) * (rng.random((16 * NPIX, NPIX)) < 0.2)) * 0.25, (np.arange(NPIX) % 9 - 4) * 0.25)
    return dict(vin=vin.astype(np.float64), pin=pin.astype(np.float64), vfc1=vfc1, vfc2=vfc2, pfc=pfc)


def _glorot(rng, *shape):
    rf = int(np.prod(shape[2:])) if len(shape) == 4 else 1
    fan_in, fan_out = (shape[1] * rf, shape[0] * rf) if len(shape) == 4 else (shape[0], shape[1])
    return ref64.bf16_round((rng.random(shape) * 2 - 1) * np.sqrt(6.0 / (fan_in + fan_out)))


def _bias(rng, n):
    return ref64.bf16_round(rng.standard_normal(n) * 0.1)


@functools.lru_cache(maxsize=None)
def rounded_block_case(iso):
    """The same three isolations on Glorot-scaled bf16 weights, randn * 0.5 inputs and randn * 0.1 biases (all bf16 values)."""
    rng = np.random.default_rng({"conv1": 71, "conv2": 72, "proj": 73}[iso])
    zero3, zero1, zb = np.zeros((W, W, 3, 3)), np.zeros((W, W, 1, 1)), np.zeros(W)
    if iso == "conv1":
        b2 = _bias(rng, W)
        case = dict(c1=(_glorot(rng, W, W, 3, 3), _bias(rng, W)), c2=(_identity3(), b2), res=(zero1, -b2))
    elif iso == "conv2":
        case = dict(c1=(_identity3(), zb), c2=(_glorot(rng, W, W, 3, 3), _bias(rng, W)), res=(zero1, _bias(rng, W)))
    else:
        case = dict(c1=(_glorot(rng, W, W, 3, 3), _bias(rng, W)), c2=(zero3, _bias(rng, W)), res=(_glorot(rng, W, W, 1, 1), _bias(rng, W)))
    case["h"] = ref64.bf16_round(rng.standard_normal((NROUND, W, S, S)) * 0.5)
    return case


@functools.lru_cache(maxsize=None)
def rounded_ends_case():
    rng = np.random.default_rng(74)
    return dict(planes=ref64.bf16_round(rng.standard_normal((NROUND, 3, S, S)) * 0.5), stem=(_glorot(rng, W, 3, 5, 5), _bias(rng, W)),
                h=ref64.bf16_round(rng.standard_normal((NROUND, W, S, S)) * 0.5),
                vconv=(_glorot(rng, 4, W, 1, 1), _bias(rng, 4)), pconv=(_glorot(rng, 16, W, 1, 1), _bias(rng, 16)))


def error_bound(ref, A, n):
    """The derived per-element bound of the rounded regime: one bf16 rounding of the stored value; the fp32 accumulation bound of
    an n-term dot product with absolute-term sum A, doubled because the MFMA's internal rounding is not documented; v_exp_f32 on
    the ELU's negative side."""
    return 2.0 ** -8 * np.abs(ref) + 2.0 * n * 2.0 ** -24 * A + 2.0 ** -22


# ------------------------------------------------------------------ the conditions ------------------------------------------------------------------
def _integers_in(a, lo, hi):
    return bool((a == np.rint(a)).all() and a.min() >= lo and a.max() <= hi)


@pytest.mark.parametrize("iso", ISOLATIONS)
def test_exact_block_generators_meet_the_exactness_conditions(iso):
    case = exact_block_case(iso)
    h = case["h"]
    g, A1, out, A2 = exact_block_reference(iso)
    assert A1.max() <= 256 and A2.max() <= 256                         # every partial sum, in any order, is an integer below 2^24
    assert _integers_in(g, 0, 256) and _integers_in(out, 0, 256) and _integers_in(h, 0, 256)
    # (the reference returns ELU(pre): a negative pre-activation would show as a non-integer in (-1, 0), so this is also "pre >= 0")
    first = h[:NPIX].reshape(NPIX, W, NPIX)
    assert ((first != 0).sum(axis=0) == 1).all()                      # every (cin, pixel) site is non-zero in exactly one of the first 225
    for c in range(0, W, 9):                                          # no two positions share an input plane
        assert len(np.unique(h[:, c].reshape(NPOS, NPIX), axis=0)) == NPOS
    for k in ("c1", "c2", "res"):
        assert set(np.unique(case[k][0])) <= {-1.0, 0.0, 1.0} and _integers_in(case[k][1], -256, 256)
    total = case["c2"][1] + case["res"][1]
    if iso == "conv1":
        assert len(set(case["c1"][1])) == W and not total.any() and case["res"][1].all() and np.array_equal(out, g)
    else:
        assert len(set(total)) == W and case["res"][1].all() and case["c2"][1].all()
        assert np.array_equal(g, h) if iso == "conv2" else not case["c2"][0].any()
    assert len(np.unique(out.reshape(NPOS, -1), axis=0)) == NPOS      # a stale buffer (another position's result) shows
    # the outputs are not just the biases — on the rows next to the seam in particular: a half that multiplied a row its sibling
    # had overwritten, or missed the neighbouring row, gives another integer there
    assert out.std() > 2 and out[:, :, 7].std() > 2 and out[:, :, 8].std() > 2
    bias_only = total if iso != "conv1" else case["c1"][1]
    for row in (6, 7, 8, 9):
        assert (out[:NPIX, :, row] != bias_only[None, :, None]).any(axis=0).all()      # every (cout, pixel) of those rows sees a stone in some position


def test_exact_stem_generator_meets_the_exactness_conditions():
    c = exact_stem_case()
    y, A = ref64.stem(c["planes"], c["w"], c["b"])
    assert A.max() <= 256 and _integers_in(y, 0, 256)
    assert set(np.unique(c["planes"])) == {0.0, 1.0} and set(np.unique(c["w"])) == {-1.0, 0.0, 1.0} and len(set(c["b"])) == W
    p = c["planes"]
    assert p[0].all() and not p[1].any() and len(np.unique(p.reshape(NDIST, -1), axis=0)) == NDIST
    single = p[p.reshape(NDIST, -1).sum(1) == 1]
    assert len(single) == 3 * len(STEM_STONES)
    for cin in range(3):                                             # a single stone at every listed cell of every plane
        for (yy, xx) in STEM_STONES:
            assert single[:, cin, yy, xx].any()
    assert (np.abs(c["w"]).sum(axis=0) > 0).all()                    # every one of the 75 taps carries weight for some cout


def test_exact_heads_generator_meets_the_exactness_conditions():
    c = exact_heads_case()
    vin, Av, pin, Ap = ref64.heads(c["h"], c["vconv"], c["pconv"])
    assert Av.max() <= 256 and Ap.max() <= 256 and _integers_in(vin, 0, 256) and _integers_in(pin, 0, 256)
    assert vin.shape == (NDIST, 4 * NPIX) and pin.shape == (NDIST, 16 * NPIX)
    assert _integers_in(c["h"], 0, 256) and (c["h"] != 0).any(axis=0).all()
    assert len(np.unique(c["h"].reshape(NDIST, -1), axis=0)) == NDIST
    assert len(set(c["vconv"][1]) | set(c["pconv"][1])) == 20         # 20 distinct biases over the two heads


def test_exact_dense_generator_meets_the_exactness_conditions():
    c = exact_dense_case()
    policy, value, logits, z = ref64.dense(c["vin"], c["pin"], c["vfc1"], c["vfc2"], c["pfc"])
    assert policy.shape == (NDIST, NPIX) and c["vfc1"][0].shape == (900, 64) and c["pfc"][0].shape == (3600, 225)
    assert _integers_in(c["vin"], 0, 256) and _integers_in(c["pin"], 0, 256)
    assert _integers_in(logits * 4, -64, 64)                         # multiples of 2^-2, |logit| <= 16
    assert (np.abs(z) < 3).mean() >= 0.9                             # tanh is not saturated
    v1 = c["vin"] @ c["vfc1"][0] + c["vfc1"][1]
    av1 = np.abs(c["vin"]) @ np.abs(c["vfc1"][0]) + np.abs(c["vfc1"][1])
    assert _integers_in(v1, 0, 2 ** 24) and av1.max() < 2 ** 24      # fc1 stays on the ELU's x >= 0 side and is exact in fp32
    assert v1.min() >= 64                                            # ... with room: the smallest of 4096 sums is far from the 900-term tail
    az = av1 @ np.abs(c["vfc2"][0])[:, 0] + abs(c["vfc2"][1][0])
    assert _integers_in(z * 2 ** 12, -2 ** 24, 2 ** 24) and az.max() * 2 ** 12 < 2 ** 24     # z: multiples of 2^-12 below 2^12
    al = np.abs(c["pin"]) @ np.abs(c["pfc"][0]) + np.abs(c["pfc"][1])
    assert al.max() * 4 < 2 ** 24
    assert set(np.unique(c["vfc2"][0] * 2 ** 12)) == {-1.0, 0.0, 1.0} and c["vfc2"][1][0] != 0
    assert set(np.unique(c["pfc"][0] * 4)) == {-1.0, 0.0, 1.0} and _integers_in(c["pfc"][1] * 4, -64, 64) and c["pfc"][1].any()
    for name in ("vin", "pin"):
        assert len(np.unique(c[name], axis=0)) == NDIST
    for w in (c["vfc1"], c["vfc2"], c["pfc"]):                       # the packers round to bf16: nothing may change
        assert np.array_equal(ref64.bf16_round(w[0]), w[0]) and np.array_equal(ref64.bf16_round(w[1]), w[1])
    assert len(np.unique(np.round(value, 6))) > NDIST // 2 and value.std() > 1e-3       # the positions do differ in value
    # 31 dead outputs: were their exp(0 - max) terms summed, every row sum would move by far more than the 1e-5 the GPU test allows
    stray = 31.0 * np.exp(-logits.max(axis=1)) / np.exp(logits - logits.max(axis=1, keepdims=True)).sum(axis=1)
    assert stray.min() > 1e-4
