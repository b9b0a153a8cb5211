"""Cases for the bf16 tower kernels (csrc/af_tower_bf16.hip) against oracle/tower_fp64.py, one layer at a time, on both board sizes
the library takes: the generators, the error bound of the rounded regime and — from the reference alone, without a GPU — the
conditions the exact-regime cases must meet.  Plain numpy; tests/test_gpu_tower_exact.py and tests/test_gpu_tower15_exact.py run the
kernels on these cases (helpers in tests/tower_gpu.py), tests/test_tower_reference_cpu.py and tests/test_tower15_reference_cpu.py
run the conditions.  Every function takes the board size first; what differs between the sizes is in SIZES.

EXACT REGIME.  Inputs, weights and biases are small integers (dyadic fractions in the dense layers) chosen so that every
partial sum, in any order, is exact in fp32 and every stored activation is an integer in [0, 256] — exactly representable
in bf16 and on the x >= 0 side of the kernels' ELU, which returns x itself there.  The kernels must then reproduce the
fp64 reference bit for bit: a mis-packed tap or weight row, a wrong zero neighbour at a board edge, a stale LDS buffer
or a dropped bias is a wrong integer.

ROUNDED REGIME.  Random bf16 data with negative pre-activations, per element, against the derived bound
    |out - ref| <= 2^-8 |ref| + 2 n 2^-24 A + 2^-22
(one bf16 rounding of the stored value; the fp32 accumulation bound of an n-term dot product with absolute-term sum A,
doubled because the MFMA's internal rounding is not documented; v_exp_f32 on the ELU's negative side).

A residual block's three weight sets are isolated through the public ABI:
    "conv1": c2 = centre-tap identity, projection 0, b2 + b_res = 0   ->  h' = ELU(g),  g = ELU(conv1(h) + b1)
    "conv2": c1 = centre-tap identity, b1 = 0 (g = ELU(h))            ->  h' = ELU(conv2(g) + b2 + b_res)
    "proj" : c2 = 0                                                   ->  h' = ELU(proj(h) + b_res + b2)

15x15.  The convolution runs every board as two half-board pseudo-positions (rows 0..7 and 8..14) that stage one row of their
sibling, so the stem planes carry single stones on both sides of the row-7 / row-8 seam and the block conditions look at the rows
next to it.  The block generators provide 232 positions: 225 put a stone on every (cin, pixel) site once (a stone stride of 37 is
coprime to 225 as it is to 121), 7 more carry a second stone, as at 11x11 (121 + 7).  The dense layers' fan-in grows: value fc1 sums
900 terms instead of 484 and the policy 3600 instead of 1936, so fc1's biases start higher and the policy weights are thinned."""
import collections
import functools

import numpy as np

from oracle import tower_fp64 as ref64

W = 128
ISOLATIONS = ("conv1", "conv2", "proj")
STRIDE = 37                      # pixel stride of the block input's stones: coprime to 121 and to 225, so (37 c + b) mod NPIX walks every pixel as b does
NDIST = 64                       # distinct positions of the stem / heads / dense generators (larger batches tile them)

Size = collections.namedtuple("Size", "NPIX NPOS NROUND second seed stones vfc1_bias pfc_density dead")
SIZES = {
    11: Size(NPIX=121,
             NPOS=128,           # positions the block generators provide (the tests take the first B): 121 cover every site, 7 more carry a second stone
             NROUND=300,         # rounded regime: more than one pass of 256 workgroups, ragged; its first 33 positions are the other batch
             second=60,          # the second stone of positions past NPIX lies this many pixels on
             seed=0,             # added to every generator's rng seed: blocks 11 / 12 / 13, stem / heads / dense 21 / 22 / 23, rounded 31 / 32 / 33, ends 34
             # single stones of the stem planes: the four corners, the four edge midpoints and the centre (together every one of
             # the 75 taps meets a stone at a corner, an edge and in the interior)
             stones=((0, 0), (0, 10), (10, 0), (10, 10), (0, 5), (5, 0), (10, 5), (5, 10), (5, 5)),
             vfc1_bias=(128, 1),  # vfc1's biases lo + step * permutation(64): above the 484-term sums, so its ELU stays on x >= 0
             pfc_density=0.375,  # share of pfc's draws kept (each then non-zero with probability 2/3): |logit| <= 16 over 1936 terms
             dead=7),            # policy outputs 121..127 of the dense kernel's padded row
    15: Size(NPIX=225,
             NPOS=232,           # 225 cover every (cin, pixel) site once, 7 more carry a second stone
             NROUND=140,         # rounded regime: 280 half boards, more than one pass of 256 workgroups; its first 33 are the other batch
             second=112,
             seed=40,            # blocks 51 / 52 / 53, stem / heads / dense 61 / 62 / 63, rounded 71 / 72 / 73, ends 74
             # corners, edge midpoints, centre, and both sides of the seam between board rows 7 and 8
             stones=((0, 0), (0, 14), (14, 0), (14, 14), (0, 7), (7, 0), (14, 7), (7, 14), (7, 7), (8, 7), (8, 0), (8, 14), (7, 3), (8, 3)),
             # fc1 sums 900 terms of standard deviation 0.91 (x in {0, 1, 2} with P(0) = 1/2, w in {-1, 0, 1}): sigma = 27.4, so the
             # biases 192, 194 .. 318 (even: bf16 values above 256) start at 7 sigma
             vfc1_bias=(192, 2),
             pfc_density=0.2,    # the policy sums 3600 terms: non-zero with probability 0.2 * 2/3, the logits keep the standard deviation (2.7) of 11x11
             dead=31),           # policy outputs 225..255
}


def _rng(S, seed):
    return np.random.default_rng(SIZES[S].seed + seed)


# ------------------------------------------------------------------ generators ------------------------------------------------------------------
def _identity3():
    w = np.zeros((W, W, 3, 3))
    w[np.arange(W), np.arange(W), 1, 1] = 1.0
    return w


def _distinct_bias(rng, lo):
    """128 distinct integers lo .. lo + 127, shuffled: a bias delivered to the wrong cout is a wrong integer."""
    return (lo + rng.permutation(W)).astype(np.float64)


def exact_block_input(S):
    """[NPOS, 128, S, S]: position b < NPIX holds one stone of value 1..3 per channel c, at pixel (37 c + b) mod NPIX — over the
    first NPIX positions every (cin, pixel) site is non-zero exactly once; the positions past them hold a second stone further on."""
    z = SIZES[S]
    h = np.zeros((z.NPOS, W, z.NPIX))
    c = np.arange(W)
    for b in range(z.NPOS):
        h[b, c, (STRIDE * c + b) % z.NPIX] = 1 + (c + b) % 3
        if b >= z.NPIX:
            h[b, c, (STRIDE * c + b + z.second) % z.NPIX] = 1 + (2 * c + b) % 3
    return h.reshape(z.NPOS, W, S, S)


def _split(total, rng):
    """total = b2 + b_res with both parts positive integers (the kernels see only their sum)."""
    b_res = 1.0 + rng.permutation(W) % 32
    return total - b_res, b_res


@functools.lru_cache(maxsize=None)
def exact_block_case(S, iso):
    """-> dict(h, c1, c2, res): weights in {-1, 0, 1}, integer biases distinct per cout."""
    rng = _rng(S, {"conv1": 11, "conv2": 12, "proj": 13}[iso])
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
    case["h"] = exact_block_input(S)
    return case


@functools.lru_cache(maxsize=None)
def exact_block_reference(S, iso):
    """-> (g, A1, h', A2) of oracle.tower_fp64.block on the NPOS positions of the case."""
    c = exact_block_case(S, iso)
    return ref64.block(c["h"], c["c1"], c["c2"], c["res"])


def _stone_planes(S, rng, n):
    """[n, 3, S, S] of 0 / 1: a full board, an empty one, a single stone in every plane at each of the size's `stones`, random fill."""
    x = np.zeros((n, 3, S, S))
    x[0] = 1.0
    k = 2
    for (yy, xx) in SIZES[S].stones:
        for c in range(3):
            x[k, c, yy, xx] = 1.0
            k += 1
    for b in range(k, n):
        x[b] = rng.random((3, S, S)) < (0.1 + 0.8 * (b - k) / (n - k))
    return x


@functools.lru_cache(maxsize=None)
def exact_stem_case(S):
    rng = _rng(S, 21)
    w = rng.integers(-1, 2, size=(W, 3, 5, 5)) * (rng.random((W, 3, 5, 5)) < 0.75)
    return dict(planes=_stone_planes(S, rng, NDIST), w=w.astype(np.float64), b=_distinct_bias(rng, 60))


@functools.lru_cache(maxsize=None)
def exact_heads_case(S):
    rng = _rng(S, 22)
    h = rng.integers(1, 3, size=(NDIST, W, S, S)) * (rng.random((NDIST, W, S, S)) < 0.5)
    wgt = lambda n: (rng.integers(-1, 2, size=(n, W, 1, 1)) * (rng.random((n, W, 1, 1)) < 0.75)).astype(np.float64)  # noqa: E731
    return dict(h=h.astype(np.float64), vconv=(wgt(4), 100.0 + rng.permutation(4)), pconv=(wgt(16), 104.0 + rng.permutation(16)))


@functools.lru_cache(maxsize=None)
def exact_dense_case(S):
    """vin / pin integers, vfc1 in {-1, 0, 1} under biases that keep its ELU on x >= 0, vfc2 in {0, +-2^-12} with bias 0.25,
    pfc in {0, +-2^-2} with biases that are multiples of 2^-2: logits and z are exact in fp32 in any summation order."""
    z, rng = SIZES[S], _rng(S, 23)
    NPIX, (lo, step) = z.NPIX, z.vfc1_bias
    vin = rng.integers(1, 3, size=(NDIST, 4 * NPIX)) * (rng.random((NDIST, 4 * NPIX)) < 0.5)
    pin = rng.integers(1, 3, size=(NDIST, 16 * NPIX)) * (rng.random((NDIST, 16 * NPIX)) < 0.1)
    vfc1 = (rng.integers(-1, 2, size=(4 * NPIX, 64)).astype(np.float64), float(lo) + float(step) * rng.permutation(64))
    vfc2 = (rng.choice([1.0, 1.0, -1.0, 0.0], size=(64, 1)) * 2.0 ** -12, np.array([0.25]))
    pfc = ((rng.integers(-1, 2, size=(16 * NPIX, NPIX)) * (rng.random((16 * NPIX, NPIX)) < z.pfc_density)) * 0.25, (np.arange(NPIX) % 9 - 4) * 0.25)
    return dict(vin=vin.astype(np.float64), pin=pin.astype(np.float64), vfc1=vfc1, vfc2=vfc2, pfc=pfc)


def _glorot(rng, *shape):
    rf = int(np.prod(shape[2:])) if len(shape) == 4 else 1
    fan_in, fan_out = (shape[1] * rf, shape[0] * rf) if len(shape) == 4 else (shape[0], shape[1])
    return ref64.bf16_round((rng.random(shape) * 2 - 1) * np.sqrt(6.0 / (fan_in + fan_out)))


def _bias(rng, n):
    return ref64.bf16_round(rng.standard_normal(n) * 0.1)


@functools.lru_cache(maxsize=None)
def rounded_block_case(S, iso):
    """The same three isolations on Glorot-scaled bf16 weights, randn * 0.5 inputs and randn * 0.1 biases (all bf16 values)."""
    rng = _rng(S, {"conv1": 31, "conv2": 32, "proj": 33}[iso])
    zero3, zero1, zb = np.zeros((W, W, 3, 3)), np.zeros((W, W, 1, 1)), np.zeros(W)
    if iso == "conv1":
        b2 = _bias(rng, W)
        case = dict(c1=(_glorot(rng, W, W, 3, 3), _bias(rng, W)), c2=(_identity3(), b2), res=(zero1, -b2))
    elif iso == "conv2":
        case = dict(c1=(_identity3(), zb), c2=(_glorot(rng, W, W, 3, 3), _bias(rng, W)), res=(zero1, _bias(rng, W)))
    else:
        case = dict(c1=(_glorot(rng, W, W, 3, 3), _bias(rng, W)), c2=(zero3, _bias(rng, W)), res=(_glorot(rng, W, W, 1, 1), _bias(rng, W)))
    case["h"] = ref64.bf16_round(rng.standard_normal((SIZES[S].NROUND, W, S, S)) * 0.5)
    return case


@functools.lru_cache(maxsize=None)
def rounded_ends_case(S):
    rng, n = _rng(S, 34), SIZES[S].NROUND
    return dict(planes=ref64.bf16_round(rng.standard_normal((n, 3, S, S)) * 0.5), stem=(_glorot(rng, W, 3, 5, 5), _bias(rng, W)),
                h=ref64.bf16_round(rng.standard_normal((n, W, S, S)) * 0.5),
                vconv=(_glorot(rng, 4, W, 1, 1), _bias(rng, 4)), pconv=(_glorot(rng, 16, W, 1, 1), _bias(rng, 16)))


def error_bound(ref, A, n):
    """The derived per-element bound of the rounded regime (module docstring)."""
    return 2.0 ** -8 * np.abs(ref) + 2.0 * n * 2.0 ** -24 * A + 2.0 ** -22


# ------------------------------------------------------------------ the conditions of the exact regime ------------------------------------------------------------------
def _integers_in(a, lo, hi):
    return bool((a == np.rint(a)).all() and a.min() >= lo and a.max() <= hi)


def check_exact_block_generator(S, iso):
    NPIX, NPOS = SIZES[S].NPIX, SIZES[S].NPOS
    case = exact_block_case(S, iso)
    h = case["h"]
    g, A1, out, A2 = exact_block_reference(S, iso)
    assert A1.max() <= 256 and A2.max() <= 256                         # every partial sum, in any order, is an integer below 2^24
    assert _integers_in(g, 0, 256) and _integers_in(out, 0, 256) and _integers_in(h, 0, 256)
    # (the reference returns ELU(pre): a negative pre-activation would show as a non-integer in (-1, 0), so this is also "pre >= 0")
    first = h[:NPIX].reshape(NPIX, W, NPIX)
    assert ((first != 0).sum(axis=0) == 1).all()                      # every (cin, pixel) site is non-zero in exactly one of the first NPIX
    for c in range(W):                                                # no two positions share an input plane
        assert len(np.unique(h[:, c].reshape(NPOS, NPIX), axis=0)) == NPOS
    for k in ("c1", "c2", "res"):
        assert set(np.unique(case[k][0])) <= {-1.0, 0.0, 1.0} and _integers_in(case[k][1], -256, 256)
    # what the isolation is for: distinct biases per cout on the convolution under test, and an output that depends on it
    total = case["c2"][1] + case["res"][1]
    if iso == "conv1":
        assert len(set(case["c1"][1])) == W and not total.any() and case["res"][1].all() and np.array_equal(out, g)
    else:
        assert len(set(total)) == W and case["res"][1].all() and case["c2"][1].all()
        assert np.array_equal(g, h) if iso == "conv2" else not case["c2"][0].any()
    assert len(np.unique(out.reshape(NPOS, -1), axis=0)) == NPOS      # a stale buffer (another position's result) shows
    assert out.std() > 5                                              # ... and the outputs are not just the biases
    if S == 15:
        # nor on the rows next to the seam: a half that multiplied a row its sibling had overwritten, or missed the neighbouring
        # row, gives another integer there
        assert out[:, :, 7].std() > 2 and out[:, :, 8].std() > 2
        bias_only = total if iso != "conv1" else case["c1"][1]
        for row in (6, 7, 8, 9):
            assert (out[:NPIX, :, row] != bias_only[None, :, None]).any(axis=0).all()      # every (cout, pixel) of those rows sees a stone in some position


def check_exact_stem_generator(S):
    stones = SIZES[S].stones
    c = exact_stem_case(S)
    y, A = ref64.stem(c["planes"], c["w"], c["b"])
    assert A.max() <= 256 and _integers_in(y, 0, 256)
    assert set(np.unique(c["planes"])) == {0.0, 1.0} and set(np.unique(c["w"])) == {-1.0, 0.0, 1.0} and len(set(c["b"])) == W
    p = c["planes"]
    assert p[0].all() and not p[1].any() and len(np.unique(p.reshape(NDIST, -1), axis=0)) == NDIST
    single = p[p.reshape(NDIST, -1).sum(1) == 1]
    assert len(single) == 3 * len(stones)
    for cin in range(3):                                             # a single stone at every listed cell of every plane
        for (yy, xx) in stones:
            assert single[:, cin, yy, xx].any()
    assert (np.abs(c["w"]).sum(axis=0) > 0).all()                    # every one of the 75 taps carries weight for some cout


def check_exact_heads_generator(S):
    NPIX = SIZES[S].NPIX
    c = exact_heads_case(S)
    vin, Av, pin, Ap = ref64.heads(c["h"], c["vconv"], c["pconv"])
    assert Av.max() <= 256 and Ap.max() <= 256 and _integers_in(vin, 0, 256) and _integers_in(pin, 0, 256)
    assert vin.shape == (NDIST, 4 * NPIX) and pin.shape == (NDIST, 16 * NPIX)
    assert _integers_in(c["h"], 0, 256) and (c["h"] != 0).any(axis=0).all()
    assert len(np.unique(c["h"].reshape(NDIST, -1), axis=0)) == NDIST
    assert len(set(c["vconv"][1]) | set(c["pconv"][1])) == 20         # 20 distinct biases over the two heads


def check_exact_dense_generator(S):
    NPIX = SIZES[S].NPIX
    c = exact_dense_case(S)
    policy, value, logits, z = ref64.dense(c["vin"], c["pin"], c["vfc1"], c["vfc2"], c["pfc"])
    assert policy.shape == (NDIST, NPIX) and c["vfc1"][0].shape == (4 * NPIX, 64) and c["pfc"][0].shape == (16 * NPIX, NPIX)
    assert _integers_in(c["vin"], 0, 256) and _integers_in(c["pin"], 0, 256)
    assert _integers_in(logits * 4, -64, 64)                         # multiples of 2^-2, |logit| <= 16
    assert (np.abs(z) < 3).mean() >= 0.9                             # tanh is not saturated
    v1 = c["vin"] @ c["vfc1"][0] + c["vfc1"][1]
    av1 = np.abs(c["vin"]) @ np.abs(c["vfc1"][0]) + np.abs(c["vfc1"][1])
    assert _integers_in(v1, 0, 2 ** 24) and av1.max() < 2 ** 24      # fc1 stays on the ELU's x >= 0 side and is exact in fp32
    assert v1.min() >= 64                                            # ... with room: the smallest of 4096 sums is far from the tail
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
    # the dead outputs: were their exp(0 - max) terms summed, every row sum would move by far more than the 1e-5 the GPU test allows
    stray = SIZES[S].dead * np.exp(-logits.max(axis=1)) / np.exp(logits - logits.max(axis=1, keepdims=True)).sum(axis=1)
    assert stray.min() > 1e-4
    assert (policy.max(axis=1) > 0.05).all()                         # ... and the rows are peaked
