"""The bf16 tower kernels (csrc/af_tower_bf16.hip) against oracle/tower_fp64.py, one layer at a time.

EXACT REGIME.  Inputs, weights and biases are small integers (dyadic fractions in the dense layers) chosen so that every
partial sum, in any order, is exact in fp32 and every stored activation is an integer in [0, 256] — exactly representable
in bf16 and on the x >= 0 side of the kernels' ELU, which returns x itself there.  The kernels must then reproduce the
fp64 reference bit for bit: a mis-packed tap or weight row, a wrong zero neighbour at a board edge, a stale LDS buffer
or a dropped bias is a wrong integer.  tests/test_tower_reference_cpu.py checks, from the reference alone, that the
generators below meet those conditions.

ROUNDED REGIME.  Random bf16 data with negative pre-activations, per element, against the derived bound
    |out - ref| <= 2^-8 |ref| + 2 n 2^-24 A + 2^-22
(one bf16 rounding of the stored value; the fp32 accumulation bound of an n-term dot product with absolute-term sum A,
doubled because the MFMA's internal rounding is not documented; v_exp_f32 on the ELU's negative side).

A residual block's three weight sets are isolated through the public ABI:
    "conv1": c2 = centre-tap identity, projection 0, b2 + b_res = 0   ->  h' = ELU(g),  g = ELU(conv1(h) + b1)
    "conv2": c1 = centre-tap identity, b1 = 0 (g = ELU(h))            ->  h' = ELU(conv2(g) + b2 + b_res)
    "proj" : c2 = 0                                                   ->  h' = ELU(proj(h) + b_res + b2)
"""
import functools

import numpy as np
import pytest

from oracle import tower_fp64 as ref64

S, W, NPIX = 11, 128, 121
NPOS = 128                       # positions the block generators provide (the tests take the first B)
NDIST = 64                       # distinct positions of the stem / heads / dense generators (larger batches tile them)
ISOLATIONS = ("conv1", "conv2", "proj")
# (engine = tune key 3, ring depth = tune key 0): af_tower_conv3 + af_tower_conv, af_tower_conv3 for both, af_tower_conv<*, depth>;
# engines 3 and 2 run at depth 8 whatever key 0 says: (3, 16) and (2, 12) pin that a depth is neither refused nor honoured there
ENGINES = ((3, 0), (2, 0), (0, 0), (0, 8), (0, 12), (0, 16), (3, 16), (2, 12))
# (batch, persistent workgroups = tune key 1).  Default grid min(batch, CUs): a multiple of 8 (XCD swizzle on) at 8 and 128 only.
# 121 positions on 3 / 8 / 16 workgroups: 41 / 16 / 8 iterations each, both LDS buffer parities, ragged last passes.
# 9 / 17 / 25 positions on 8 workgroups: workgroup 0 runs 2 / 3 / 4 positions, the others one fewer — af_tower_conv3's
# first-position form, its drain after the last position, and one steady-state position more.
CONFIGS = tuple((b, 0) for b in (1, 2, 8, 9, 121, 128)) + tuple((121, g) for g in (3, 8, 16)) + tuple((b, 8) for b in (9, 17, 25))


# ------------------------------------------------------------------ generators (numpy, no GPU) ------------------------------------------------------------------
def _identity3():
    w = np.zeros((W, W, 3, 3))
    w[np.arange(W), np.arange(W), 1, 1] = 1.0
    return w


def _distinct_bias(rng, lo):
    """128 distinct integers lo .. lo + 127, shuffled: a bias delivered to the wrong cout is a wrong integer."""
    return (lo + rng.permutation(W)).astype(np.float64)


def exact_block_input():
    """[NPOS, 128, 11, 11]: position b < 121 holds one stone of value 1..3 per channel c, at pixel (37 c + b) mod 121 — over the
    first 121 positions every (cin, pixel) site is non-zero exactly once; positions 121..127 hold a second stone 60 pixels on."""
    h = np.zeros((NPOS, W, NPIX))
    c = np.arange(W)
    for b in range(NPOS):
        h[b, c, (37 * c + b) % NPIX] = 1 + (c + b) % 3
        if b >= NPIX:
            h[b, c, (37 * c + b + 60) % NPIX] = 1 + (2 * c + b) % 3
    return h.reshape(NPOS, W, S, S)


def _split(total, rng):
    """total = b2 + b_res with both parts positive integers (the kernels see only their sum)."""
    b_res = 1.0 + rng.permutation(W) % 32
    return total - b_res, b_res


@functools.lru_cache(maxsize=None)
def exact_block_case(iso):
    """-> dict(h, c1, c2, res): weights in {-1, 0, 1}, integer biases distinct per cout."""
    rng = np.random.default_rng({"conv1": 11, "conv2": 12, "proj": 13}[iso])
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
    """[n, 3, 11, 11] of 0 / 1: a full board, an empty one, single stones in every plane at the four corners, the four edge
    midpoints and the centre (together every one of the 75 taps meets a stone at a corner, an edge and in the interior), random fill."""
    x = np.zeros((n, 3, S, S))
    x[0] = 1.0
    k = 2
    for (yy, xx) in ((0, 0), (0, S - 1), (S - 1, 0), (S - 1, S - 1), (0, 5), (5, 0), (S - 1, 5), (5, S - 1), (5, 5)):
        for c in range(3):
            x[k, c, yy, xx] = 1.0
            k += 1
    for b in range(k, n):
        x[b] = rng.random((3, S, S)) < (0.1 + 0.8 * (b - k) / (n - k))
    return x


@functools.lru_cache(maxsize=None)
def exact_stem_case():
    rng = np.random.default_rng(21)
    w = rng.integers(-1, 2, size=(W, 3, 5, 5)) * (rng.random((W, 3, 5, 5)) < 0.75)
    return dict(planes=_stone_planes(rng, NDIST), w=w.astype(np.float64), b=_distinct_bias(rng, 60))


@functools.lru_cache(maxsize=None)
def exact_heads_case():
    rng = np.random.default_rng(22)
    h = rng.integers(1, 3, size=(NDIST, W, S, S)) * (rng.random((NDIST, W, S, S)) < 0.5)
    wgt = lambda n: (rng.integers(-1, 2, size=(n, W, 1, 1)) * (rng.random((n, W, 1, 1)) < 0.75)).astype(np.float64)  # noqa: E731
    return dict(h=h.astype(np.float64), vconv=(wgt(4), 100.0 + rng.permutation(4)), pconv=(wgt(16), 104.0 + rng.permutation(16)))


@functools.lru_cache(maxsize=None)
def exact_dense_case():
    """vin / pin integers, vfc1 in {-1, 0, 1} under biases that keep its ELU on x >= 0, vfc2 in {0, +-2^-12} with bias 0.25,
    pfc in {0, +-2^-2} with biases that are multiples of 2^-2: logits and z are exact in fp32 in any summation order."""
    rng = np.random.default_rng(23)
    vin = rng.integers(1, 3, size=(NDIST, 4 * NPIX)) * (rng.random((NDIST, 4 * NPIX)) < 0.5)
    pin = rng.integers(1, 3, size=(NDIST, 16 * NPIX)) * (rng.random((NDIST, 16 * NPIX)) < 0.1)
    vfc1 = (rng.integers(-1, 2, size=(4 * NPIX, 64)).astype(np.float64), 128.0 + rng.permutation(64))
    vfc2 = (rng.choice([1.0, 1.0, -1.0, 0.0], size=(64, 1)) * 2.0 ** -12, np.array([0.25]))
    pfc = ((rng.integers(-1, 2, size=(16 * NPIX, NPIX)) * (rng.random((16 * NPIX, NPIX)) < 0.375)) * 0.25, (np.arange(NPIX) % 9 - 4) * 0.25)
    return dict(vin=vin.astype(np.float64), pin=pin.astype(np.float64), vfc1=vfc1, vfc2=vfc2, pfc=pfc)


def _glorot(rng, *shape):
    rf = int(np.prod(shape[2:])) if len(shape) == 4 else 1
    fan_in, fan_out = (shape[1] * rf, shape[0] * rf) if len(shape) == 4 else (shape[0], shape[1])
    return ref64.bf16_round((rng.random(shape) * 2 - 1) * np.sqrt(6.0 / (fan_in + fan_out)))


def _bias(rng, n):
    return ref64.bf16_round(rng.standard_normal(n) * 0.1)


NROUND = 300                     # rounded regime: more than one pass of 256 workgroups, ragged; its first 33 positions are the other batch


@functools.lru_cache(maxsize=None)
def rounded_block_case(iso):
    """The same three isolations on Glorot-scaled bf16 weights, randn * 0.5 inputs and randn * 0.1 biases (all bf16 values)."""
    rng = np.random.default_rng({"conv1": 31, "conv2": 32, "proj": 33}[iso])
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
    rng = np.random.default_rng(34)
    return dict(planes=ref64.bf16_round(rng.standard_normal((NROUND, 3, S, S)) * 0.5), stem=(_glorot(rng, W, 3, 5, 5), _bias(rng, W)),
                h=ref64.bf16_round(rng.standard_normal((NROUND, W, S, S)) * 0.5),
                vconv=(_glorot(rng, 4, W, 1, 1), _bias(rng, 4)), pconv=(_glorot(rng, 16, W, 1, 1), _bias(rng, 16)))


def error_bound(ref, A, n):
    """The derived per-element bound of the rounded regime (module docstring)."""
    return 2.0 ** -8 * np.abs(ref) + 2.0 * n * 2.0 ** -24 * A + 2.0 ** -22


# ------------------------------------------------------------------ GPU side ------------------------------------------------------------------
pytestmark = pytest.mark.gpu
SENT16 = 0x4B4B                  # bf16 bit pattern (a finite 1.3e7) no kernel here can produce
SENT32 = -777.25


def _t(a, dtype=None):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to("cuda", dtype or torch.float32)


def _tower(case, max_batch, **kw):
    import torch
    from alphafive_amd import tower_hip
    tt = lambda wb: (torch.from_numpy(np.asarray(wb[0], np.float32)), torch.from_numpy(np.asarray(wb[1], np.float32)))  # noqa: E731
    blocks = [dict(c1=tt(case["c1"]), c2=tt(case["c2"]), res=tt(case["res"]))] if "c1" in case else [_null_block()]
    for k in ("stem", "vconv", "pconv"):
        if k in kw:
            kw[k] = tt(kw[k])
    if "dense" in kw:
        kw["dense"] = tuple(torch.from_numpy(np.asarray(a, np.float32)) for a in kw["dense"])
    return tower_hip.HipTower(blocks, S, W, max_batch, "cuda:0", **kw)


def _null_block():
    import torch
    z3, z1, zb = torch.zeros(W, W, 3, 3), torch.zeros(W, W, 1, 1), torch.zeros(W)
    return dict(c1=(z3, zb), c2=(z3, zb), res=(z1, zb))


def _bits16(t):
    import torch
    return t.view(torch.int16)                       # same element size: a view of the very memory, whatever the strides


def _poison(tw, B):
    """Positions at or past B of every buffer a kernel writes hold a sentinel."""
    for buf in (tw.x, tw.g, tw.vin, tw.pin):
        _bits16(buf[B:]).fill_(SENT16)
    for buf in (tw.x, tw.g):                         # (the zero rows of a position an earlier, smaller batch had poisoned)
        buf[:B, :, :S] = 0
        buf[:B, :, S + NPIX:] = 0
    tw.policy[B:].fill_(SENT32)
    tw.value[B:].fill_(SENT32)


def _assert_untouched(tw, B):
    """... and still do, bit for bit; the two zero rows of the positions below B are still zero."""
    import torch
    torch.cuda.synchronize()
    for name in ("x", "g", "vin", "pin"):
        assert bool((_bits16(getattr(tw, name)[B:]) == SENT16).all()), f"{name}: a position at or past batch {B} was written"
    for name in ("policy", "value"):
        assert bool((getattr(tw, name)[B:] == SENT32).all()), f"{name}: a position at or past batch {B} was written"
    for name in ("x", "g"):
        buf = getattr(tw, name)[:B]
        assert not bool(_bits16(buf[:, :, :S]).any()) and not bool(_bits16(buf[:, :, S + NPIX:]).any()), f"{name}: a zero row was written"


def _g_nchw(tw, B):
    """The mid activation af_tower_forward leaves in the scratch buffer (one block), as NCHW."""
    gin = tw.g[:, :, S:S + NPIX, :].unflatten(2, (S, S))
    return gin[:B].permute(0, 1, 4, 2, 3).reshape(B, W, S, S)


class _Tune(object):
    """Tune keys set for one run; every key is put back to its default whatever happens."""

    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        from alphafive_amd import tower_hip
        try:
            for k, v in self.kv.items():
                tower_hip.tune(int(k[1:]), v)
        except Exception:
            self.__exit__()
            raise

    def __exit__(self, *exc):
        from alphafive_amd import tower_hip
        for k, v in ((0, 0), (1, 0), (2, 0), (3, 3), (4, 1)):
            tower_hip.tune(k, v)


def _run_block(tw, h_dev, B, engine, depth, grid):
    _poison(tw, B)
    tw.load_nchw(h_dev[:B])
    with _Tune(k3=engine, k0=depth, k1=grid):
        tw.forward(B)
    _assert_untouched(tw, B)
    return tw.store_nchw(B), _g_nchw(tw, B)


def _mismatch(out, ref):
    import torch
    bad = (out != ref).nonzero()
    return "%d of %d elements differ; first at (position, channel, y, x) = %s: got %s, expected %s" % (
        bad.shape[0], out.numel(), bad[0].tolist(), out[tuple(bad[0])].item(), ref[tuple(bad[0])].item()) if bad.shape[0] else "equal"


@pytest.fixture(scope="module")
def block_towers():
    """One single-block tower per isolation and regime, with its input on the device and — exact regime — the reference."""
    import torch
    made = {}

    def get(regime, iso):
        if (regime, iso) not in made:
            case = exact_block_case(iso) if regime == "exact" else rounded_block_case(iso)
            n = case["h"].shape[0]
            tw = _tower(case, n + 8)
            ref = None
            if regime == "exact":
                g, _, out, _ = exact_block_reference(iso)
                ref = (_t(ref64.bf16_round(out), torch.bfloat16), _t(ref64.bf16_round(g), torch.bfloat16))
            made[(regime, iso)] = (tw, _t(case["h"], torch.bfloat16), ref)
        return made[(regime, iso)]
    yield get
    for tw, _, _ in made.values():
        tw.close()


@pytest.mark.parametrize("engine, depth", ENGINES)
@pytest.mark.parametrize("iso", ISOLATIONS)
def test_block_convolutions_are_exact(block_towers, iso, engine, depth):
    """Every (cout, cin, tap, pixel, position) of one convolution, on every kernel, batch and grid: bit equality with fp64."""
    import torch
    tw, h_dev, (ref_out, ref_g) = block_towers("exact", iso)
    for B, grid in CONFIGS:
        out, g = _run_block(tw, h_dev, B, engine, depth, grid)
        assert torch.equal(g, ref_g[:B]), f"mid activation, batch {B}, grid {grid}: " + _mismatch(g, ref_g[:B])
        assert torch.equal(out, ref_out[:B]), f"block output, batch {B}, grid {grid}: " + _mismatch(out, ref_out[:B])


def test_tune_rejects_undocumented_values_and_keeps_the_setting(block_towers):
    """af_tower_tune: a rejected value leaves the previous setting in force — shown on key 2's "no stores" bit, whose
    effect is visible: af_tower_conv keeps storing nothing after the rejected call."""
    import torch
    from alphafive_amd import tower_hip
    tw, h_dev, (ref_out, _) = block_towers("exact", "conv1")
    B = 9
    try:
        tower_hip.tune(3, 0)
        tower_hip.tune(2, 2)
        for key, bad in ((0, 5), (0, 7), (0, 24), (0, -8), (1, -1), (2, 8), (2, -1), (3, 1), (4, 2), (4, -1), (5, 0), (-1, 0)):
            with pytest.raises(tower_hip.TowerError):
                tower_hip.tune(key, bad)
        tw.load_nchw(h_dev[:B])
        _bits16(tw.g[:B, :, S:S + NPIX]).fill_(SENT16)
        tw.forward(B)                                # the rejected tune(2, 8) did not clear the "no stores" bit ...
        torch.cuda.synchronize()
        assert bool((_bits16(tw.g[:B, :, S:S + NPIX]) == SENT16).all()) and torch.equal(tw.store_nchw(B), h_dev[:B])
    finally:
        for k, v in ((0, 0), (1, 0), (2, 0), (3, 3), (4, 1)):
            tower_hip.tune(k, v)
    tw.load_nchw(h_dev[:B])
    tw.forward(B)                                    # ... nor did any of them leave something else behind
    assert torch.equal(tw.store_nchw(B), ref_out[:B])


@pytest.fixture(scope="module")
def ends_tower():
    """Stem + heads of the exact regime on one tower (null block), 2048 + 5 positions + room for the sentinels."""
    st, hd = exact_stem_case(), exact_heads_case()
    tw = _tower({}, 2048 + 5 + 3, stem=(st["w"], st["b"]), vconv=hd["vconv"], pconv=hd["pconv"])
    yield tw
    tw.close()


@pytest.mark.parametrize("B", [1, 121, 1024 + 5])
def test_stem_is_exact(ends_tower, B):
    """All 75 taps at corners, edges and interior; 1024 + 5 wraps the stem's grid cap of 1024 (64 distinct positions, tiled)."""
    import torch
    tw, case = ends_tower, exact_stem_case()
    y, _ = ref64.stem(case["planes"], case["w"], case["b"])
    ref = _t(ref64.bf16_round(y), torch.bfloat16)
    idx = torch.arange(B, device="cuda") % NDIST
    planes = _t(case["planes"])[idx].contiguous()
    _poison(tw, B)
    tw.stem(planes)
    _assert_untouched(tw, B)
    out = tw.store_nchw(B)
    n = min(B, NDIST)
    assert torch.equal(out[:n], ref[:n]), _mismatch(out[:n], ref[:n])
    assert torch.equal(out, out[idx]), "a repeat of a position differs from its first occurrence"


@pytest.mark.parametrize("B", [1, 121, 2048 + 5])
def test_heads_are_exact_on_both_kernels(ends_tower, B):
    """The heads' 1x1 convolutions on an integer tower output: MFMA kernel = VALU kernel = fp64; 2048 + 5 wraps the grid cap."""
    import torch
    tw, case = ends_tower, exact_heads_case()
    vin, _, pin, _ = ref64.heads(case["h"], case["vconv"], case["pconv"])
    ref_v, ref_p = _t(ref64.bf16_round(vin), torch.bfloat16), _t(ref64.bf16_round(pin), torch.bfloat16)
    idx = torch.arange(B, device="cuda") % NDIST
    h = _t(case["h"], torch.bfloat16)[idx].contiguous()
    n = min(B, NDIST)
    for kernel in (1, 0):
        _poison(tw, B)
        tw.load_nchw(h)
        with _Tune(k4=kernel):
            v, p = tw.heads(B)
        _assert_untouched(tw, B)
        assert torch.equal(v[:n], ref_v[:n]), f"heads kernel {kernel}, value: " + _mismatch(v[:n], ref_v[:n])
        assert torch.equal(p[:n], ref_p[:n]), f"heads kernel {kernel}, policy: " + _mismatch(p[:n], ref_p[:n])
        assert torch.equal(v, v[idx]) and torch.equal(p, p[idx]), "a repeat of a position differs from its first occurrence"


@pytest.fixture(scope="module")
def dense_tower():
    """The one tower of the dense tests: 32768 + 5 positions reach the second trip of the kernel's loop over 32-position groups."""
    c = exact_dense_case()
    tw = _tower({}, 32768 + 5 + 3, dense=(c["vfc1"][0], c["vfc1"][1], c["vfc2"][0], c["vfc2"][1], c["pfc"][0], c["pfc"][1]))
    yield tw
    tw.close()


@pytest.mark.parametrize("B", [1, 31, 32, 33, 65, 32768 + 5])
def test_dense_matches_fp64_to_1e5(dense_tower, B):
    """Logits and z are exact in fp32 whatever the summation order, so what is left is __expf, tanhf and one division:
    policy and value within 1e-5 of fp64 (the project's fp32 bar), rows summing to 1; vfc2's bias is not zero."""
    import torch
    tw, c = dense_tower, exact_dense_case()
    policy, value, _, _ = ref64.dense(c["vin"], c["pin"], c["vfc1"], c["vfc2"], c["pfc"])
    idx = torch.arange(B, device="cuda") % NDIST
    _poison(tw, B)
    tw.vin[:B] = _t(c["vin"], torch.bfloat16)[idx]
    tw.pin[:B] = _t(c["pin"], torch.bfloat16)[idx]
    p, v = tw.dense(B)
    _assert_untouched(tw, B)
    n = min(B, NDIST)
    ep = np.abs(p[:n].double().cpu().numpy() - policy[:n]).max()
    ev = np.abs(v[:n].double().cpu().numpy() - value[:n]).max()
    es = float((p.double().sum(1) - 1).abs().max())
    print("dense B=%d: max |policy - fp64| %.3g, |value - fp64| %.3g, |row sum - 1| %.3g" % (B, ep, ev, es))
    assert ep <= 1e-5 and ev <= 1e-5 and es <= 1e-5
    assert torch.equal(p, p[idx]) and torch.equal(v, v[idx]), "a repeat of a position differs from its first occurrence"


# ------------------------------------------------------------------ rounded regime ------------------------------------------------------------------
def _worst_ratio(out, ref, A, n, what):
    """max over elements of |out - ref| / bound, printed (the headroom of the derived bound) and returned."""
    err = np.abs(out.double().cpu().numpy() - ref)
    ratio = float((err / error_bound(ref, A, n)).max())
    print("rounded regime, %s: worst |error| / bound = %.3f (max |error| %.3g)" % (what, ratio, err.max()))
    return ratio


@pytest.mark.parametrize("B", [33, NROUND])
@pytest.mark.parametrize("iso", ISOLATIONS)
def test_block_convolutions_meet_the_rounding_bound(block_towers, iso, B):
    """Per element, one convolution at a time: the stored mid activation against ELU(conv1) and the block output against the
    second convolution of the mid activation that was stored, so each comparison crosses exactly one rounding to bf16."""
    import torch
    tw, h_dev, _ = block_towers("rounded", iso)
    case = rounded_block_case(iso)
    h = case["h"][:B]
    got = {}
    for engine, depth in ENGINES:
        out, g = _run_block(tw, h_dev, B, engine, depth, 0)
        got[(engine, depth)] = (out.clone(), g.clone())
    for depth in (8, 12, 16):                        # the same MFMAs in the same order: the ring depth changes no bit
        assert torch.equal(got[(0, depth)][0], got[(0, 0)][0]) and torch.equal(got[(0, depth)][1], got[(0, 0)][1]), depth
    assert torch.equal(got[(3, 0)][0], got[(0, 0)][0]) and torch.equal(got[(3, 0)][1], got[(0, 0)][1])    # engine 3 = engine 0
    assert torch.isfinite(got[(2, 0)][0].float()).all() and torch.isfinite(got[(3, 0)][0].float()).all()
    refs = {}
    for engine in (3, 2):                            # engine 0 equals engine 3 by bits
        out, g = got[(engine, 0)]
        key = g.cpu().view(torch.int16).numpy().tobytes()
        if key not in refs:
            refs[key] = ref64.block(h, case["c1"], case["c2"], case["res"], mid=g.double().cpu().numpy())
        g_ref, A1, out_ref, A2 = refs[key]
        assert (g_ref < 0).any() and (out_ref < 0).any()             # the ELU's negative side is exercised
        assert _worst_ratio(g, g_ref, A1, 1152, f"{iso} B={B} engine {engine} first convolution") <= 1.0
        assert _worst_ratio(out, out_ref, A2, 1280, f"{iso} B={B} engine {engine} second convolution + projection") <= 1.0


@pytest.mark.parametrize("B", [33, NROUND])
def test_stem_and_heads_meet_the_rounding_bound(B):
    import torch
    c = rounded_ends_case()
    tw = _tower({}, B + 3, stem=c["stem"], vconv=c["vconv"], pconv=c["pconv"])
    try:
        y, A = ref64.stem(c["planes"][:B], *c["stem"])
        _poison(tw, B)
        tw.stem(_t(c["planes"][:B]))
        _assert_untouched(tw, B)
        assert (y < 0).any()
        assert _worst_ratio(tw.store_nchw(B), y, A, 75, f"stem B={B}") <= 1.0
        vin, Av, pin, Ap = ref64.heads(c["h"][:B], c["vconv"], c["pconv"])
        for kernel in (1, 0):
            _poison(tw, B)
            tw.load_nchw(_t(c["h"][:B], torch.bfloat16))
            with _Tune(k4=kernel):
                v, p = tw.heads(B)
            _assert_untouched(tw, B)
            assert _worst_ratio(v, vin, Av, 128, f"heads kernel {kernel} value B={B}") <= 1.0
            assert _worst_ratio(p, pin, Ap, 128, f"heads kernel {kernel} policy B={B}") <= 1.0
    finally:
        tw.close()
