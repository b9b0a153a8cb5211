"""Cases for the int8 tower kernels (csrc/af_tower_i8.hip) against alphafive_amd/tower_i8.py, one layer at a time: the generators,
the comparison rule and — from the reference alone, without a GPU — the conditions the cases must meet.  Plain numpy;
tests/test_gpu_tower_i8.py runs the kernels on these cases, tests/test_tower_i8_cpu.py runs the conditions.

A case is one residual block: Glorot weights, biases randn * 0.1, inputs randn * 0.5 (rounded to bf16, as the stem stores them)
pushed through the quantiser.  The layer under test is launched on its own (af_tower_conv_i8), and a block's three weight sets
are isolated as in tests/tower_cases.py:
    "conv1": the block's first convolution                              g  = Q(ELU(m1 * conv3x3(h) + b1))
    "conv2": its second, projection weights 0                           h' = Q(ELU(m2 * conv3x3(g) + b2 + b_res))
    "proj" : its second, 3x3 weights 0                                  h' = Q(ELU(m2 * proj(h) + b2 + b_res))
    "both" : its second as a net has it, 3x3 and projection together — the folded ratio and the joint absmax at work
The tower of a case has two blocks — the case, then an all-zero block (whose rows exercise the packers' "absmax = 0" branch) — so
that the second convolution of block 0 has an int8 output with a scale of its own: scales = (a_h0, a_g0, a_h1, 1).

SCALES.  Input scales are absmax / 127 of the real-valued input.  The scale of the tensor a case WRITES is the 99.7th percentile
of |ELU(pre)| of the real-valued (dequantised, fp64) layer over 127: the clamp at +-127 is exercised on about 0.3 % of the
outputs.  Every r = 1 / a stays below 128 (checked).

THE COMPARISON RULE (compare).  Integer accumulation is exact and fmaf, the multiply and rint are reproducible, so every element
whose reference pre-activation is >= 0 must equal the reference bit for bit.  On the negative side the kernels' v_exp_f32 is not
reproducible in numpy: an element whose real y * r_out lies within delta = r_out * 2^-20 of a half-integer ("near") may differ
by exactly one step, every other element is exact, and near elements may be at most 0.1 % of a layer's outputs (expected share
about 2 delta <= 2.5e-4 at r_out <= 128).  The bf16 form rounds y itself, on a step that shrinks with |y|, so its rule is stated
in y: the stored value must be a bf16 value between the roundings of y - 2^-22 and y + 2^-22 — 2^-22 being the derived absolute
error of the kernels' ELU (tower_i8.bf16_interval).  Where the two roundings agree that is bit equality; an element where they
differ is "near" (one step of room at ordinary magnitudes, more below |y| = 2^-13, where the bf16 step is smaller than the
error), under the same 0.1 % cap (expected: 0.8 * 2^-14 per binade of |y| from 1 down to 2^-13 and everything below: about 7e-4
at these cases' density of 0.8 per unit around pre = 0).
"""
import functools

import numpy as np

from alphafive_amd import tower_i8 as t8
from oracle import tower_fp64 as ref64

W, S, NPOS = 128, 11, 33
CASES = ("conv1", "conv2", "proj", "both")
NEAR_CAP = 1e-3


def _glorot(rng, *shape):
    rf = int(np.prod(shape[2:]))
    lim = np.sqrt(6.0 / ((shape[0] + shape[1]) * rf))
    return ((rng.random(shape) * 2 - 1) * lim).astype(np.float32)


def _bias(rng):
    return (rng.standard_normal(W) * 0.1).astype(np.float32)


def _acts(rng, n=NPOS):
    return ref64.bf16_round(rng.standard_normal((n, W, S, S)) * 0.5)


def _scale(x):
    return np.float32(np.abs(x).max() / 127.0)


def null_block():
    return dict(c1=(np.zeros((W, W, 3, 3), np.float32), np.zeros(W, np.float32)), c2=(np.zeros((W, W, 3, 3), np.float32), np.zeros(W, np.float32)),
                res=(np.zeros((W, W, 1, 1), np.float32), np.zeros(W, np.float32)))


@functools.lru_cache(maxsize=None)
def layer_case(name):
    """-> dict(c1, c2, res: (weight, bias) fp32; h, g: real-valued inputs; hq, gq: their int8 images; scales fp32 [4]; second)."""
    rng = np.random.default_rng(100 + CASES.index(name))
    zero3, zero1 = np.zeros((W, W, 3, 3), np.float32), np.zeros((W, W, 1, 1), np.float32)
    c1 = (_glorot(rng, W, W, 3, 3), _bias(rng))
    c2 = (zero3 if name == "proj" else _glorot(rng, W, W, 3, 3), _bias(rng))
    res = (zero1 if name == "conv2" else _glorot(rng, W, W, 1, 1), _bias(rng))
    h, g = _acts(rng), _acts(rng)
    a_h, a_g = _scale(h), _scale(g)
    hq, gq = t8.quantize_activation(h, t8.reciprocal(a_h)), t8.quantize_activation(g, t8.reciprocal(a_g))
    second = name != "conv1"
    # the real-valued layer over the dequantised inputs: where the output scale comes from
    if second:
        pre = ref64._conv2d(gq * np.float64(a_g), c2[0], c2[1])[0] + ref64._conv2d(hq * np.float64(a_h), res[0], res[1])[0]
    else:
        pre = ref64._conv2d(hq * np.float64(a_h), c1[0], c1[1])[0]
    a_out = np.float32(np.percentile(np.abs(ref64.elu(pre)), 99.7) / 127.0)
    scales = np.array([a_h, a_out, 1.0, 1.0] if not second else [a_h, a_g, a_out, 1.0], np.float32)
    return dict(c1=c1, c2=c2, res=res, h=h, g=g, hq=hq, gq=gq, scales=scales, second=second, real=ref64.elu(pre))


def case_blocks(name):
    c = layer_case(name)
    return [dict(c1=c["c1"], c2=c["c2"], res=c["res"]), null_block()]


@functools.lru_cache(maxsize=None)
def layer_reference(name, bf16_out):
    """-> (out, t64, pre, r_out) of tower_i8.conv_reference on the NPOS positions of the case; r_out None for the bf16 form."""
    c = layer_case(name)
    a = c["scales"]
    r = t8.reciprocal(a)
    qw = t8.quantize_weights(c["c1"], c["c2"], c["res"], a[0], a[1])
    if c["second"]:
        r_out = None if bf16_out else r[2]
        return t8.conv_reference(c["gq"], qw["q2"], qw["m2"], qw["b2"], r_out, c["hq"], qw["qp"]) + (r_out,)
    r_out = None if bf16_out else r[1]
    return t8.conv_reference(c["hq"], qw["q1"], qw["m1"], qw["b1"], r_out) + (r_out,)


def near_elements(t64, pre, r_out):
    """-> (near, lo, hi): the elements the rule leaves room on, and the values allowed there (int8: ref -+ 1 is handled by the
    caller, lo / hi are None; bf16 form: tower_i8.bf16_interval)."""
    if r_out is not None:
        return t8.near_boundary(t64, r_out) & (pre < 0), None, None
    lo, hi = t8.bf16_interval(t64)
    return (lo != hi) & (pre < 0), lo, hi


def compare(out, ref, t64, pre, r_out, what=""):
    """The comparison rule of the module docstring; out / ref int8, or bf16 values as fp32 (r_out None).  Returns the share of
    near elements and the number of them that differ from ref; raises AssertionError with the first offender otherwise."""
    out, ref = np.asarray(out), np.asarray(ref)
    assert out.shape == ref.shape, (out.shape, ref.shape)
    near, lo, hi = near_elements(t64, pre, r_out)
    if r_out is None:
        inside = (out.astype(np.float64) >= lo) & (out.astype(np.float64) <= hi)
    else:
        inside = np.abs(out.astype(np.int64) - ref.astype(np.int64)) <= 1
    share = float(near.mean())
    bad = np.where(near, ~inside, out != ref)
    flips = int((out[near] != ref[near]).sum())
    print("%s: %d elements, %.4f %% near a rounding boundary on the negative side, %d of them not the reference's value, %d wrong"
          % (what, out.size, 100 * share, flips, int(bad.sum())))
    if bad.any():
        i = tuple(int(v) for v in np.argwhere(bad)[0])
        raise AssertionError("%s: %d of %d elements wrong (%d on the side pre >= 0); first at (position, channel, y, x) = %s: got %s, expected %s, "
                             "pre %.6g; rows hit: %s" % (what, int(bad.sum()), out.size, int((bad & (pre >= 0)).sum()), i, out[i], ref[i], pre[i],
                                                         sorted(set(np.argwhere(bad)[:, 2].tolist()))))
    assert share <= NEAR_CAP, "%s: %.4f %% of the outputs are near a rounding boundary, cap 0.1 %%" % (what, 100 * share)
    return share, flips


# ------------------------------------------------------------------ the conditions, on the reference alone ------------------------------------------------------------------
def check_layer_generator(name):
    c = layer_case(name)
    r = t8.reciprocal(c["scales"])
    assert (r <= 128).all(), r                                        # every r_out <= 128: delta <= 2^-13
    for bf16_out in (False, True):
        out, t64, pre, r_out = layer_reference(name, bf16_out)
        neg = float((pre < 0).mean())
        assert 0.25 <= neg <= 0.75, neg                               # both ELU sides are well populated
        near = near_elements(t64, pre, r_out)[0]
        assert near.mean() <= NEAR_CAP, near.mean()                   # the near-boundary share is under its cap
        if not bf16_out:
            sat = float((np.abs(out.astype(np.int32)) == 127).mean())
            assert 0 < sat < 0.01, sat                                # the clamp is exercised without dominating
            assert (out == 127).any() and out.min() < -40             # (ELU >= -1: the negative side ends above -r_out; only +127 saturates)
            # the int8 image follows the real-valued layer: a mis-scaled multiplier or a dropped bias would not
            a_out = np.float64(c["scales"][2 if c["second"] else 1])
            err = np.abs(out.astype(np.float64) * a_out - np.clip(c["real"], -127 * a_out, 127 * a_out))
            assert np.median(err) < 0.05 and np.corrcoef(out.reshape(-1), c["real"].reshape(-1))[0, 1] > 0.99
    assert len(np.unique(layer_reference(name, False)[0].reshape(NPOS, -1), axis=0)) == NPOS     # a stale buffer shows
    if c["second"]:
        a = c["scales"]
        qw = t8.quantize_weights(c["c1"], c["c2"], c["res"], a[0], a[1])
        conv_part = np.abs(t8._accumulate(c["gq"], qw["q2"]))
        proj_part = np.abs(c["hq"].astype(np.float64).transpose(0, 2, 3, 1).reshape(-1, W) @ qw["qp"].astype(np.float64).T)
        if name in ("conv2", "both"):
            assert conv_part.mean() > 100
        if name in ("proj", "both"):
            assert proj_part.mean() > 100
        if name == "both":                                            # both terms carry weight in the shared accumulator
            ratio = proj_part.mean() / conv_part.mean()
            assert 0.1 < ratio < 10, ratio
            assert np.abs(qw["qp"]).max() > 16 and np.abs(qw["q2"]).max() > 16
        if name == "conv2":
            assert not qw["qp"].any()
        if name == "proj":
            assert not qw["q2"].any()


# ------------------------------------------------------------------ whole towers ------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def tower_case(blocks, n=9, seed=7):
    """A `blocks`-deep random tower, a stem-like bf16 input and scales calibrated on it with the fp64 reference.
    -> dict(blocks=[dict(c1, c2, res)], x [n,128,11,11] bf16 values, scales fp32 [2 * blocks])."""
    rng = np.random.default_rng(seed + blocks)
    blks = [dict(c1=(_glorot(rng, W, W, 3, 3), _bias(rng)), c2=(_glorot(rng, W, W, 3, 3), _bias(rng)), res=(_glorot(rng, W, W, 1, 1), _bias(rng)))
            for _ in range(blocks)]
    x = ref64.bf16_round(ref64.elu(rng.standard_normal((n, W, S, S)) * 0.7))
    scales, h = [], x
    for b in blks:
        g, _, out, _ = ref64.block(h, b["c1"], b["c2"], b["res"], mid=None)
        scales += [_scale(h), _scale(g)]
        h = out
    return dict(blocks=blks, x=x, scales=np.array(scales, np.float32), out64=h)
