"""The fp16 split-operand forward (csrc/af_conv_f16s.hip, conv path 5 on 11x11 and 15x15) against oracle/net_fp64.intermediates, one
layer at a time, through the per-layer read-back HipNet.debug_activation (af_net_debug_activation).  The generators of the cases
are generic in the board size and live in tests/net_cases.py.

EXACT REGIME.  One layer (the TARGET: the stem, conv1 / conv2 / the 1x1 projection of one of the five blocks, a head convolution)
carries random weights; every other layer is a centre-tap SELECTOR (cout c takes cin (c + 5 (c // Cin)) mod Cin where the net
widens, cin c where it narrows; conv2 = identity, projection = 0), so the target's input is the input planes fanned out over its
channels and its output reaches every buffer behind it unchanged.  Blocks 3 and 5 never store their output: there the head
convolution folds all 32 channels, vconv[c] = K + sum_j (-1)^j o3[4 j + c], pconv[c] = K + o5[c] - o5[c + 16] (K the smallest integer
that keeps the fold positive), so one wrong o3 / o5 value is one wrong head value.  Three data classes, in each of which the kernel
must equal fp64 BIT FOR BIT in every buffer the launch form writes:
    int     weights in {-1, 0, 1}, integer biases distinct per cout (a bias at the wrong cout is a wrong integer), integer inputs:
            every stored activation is an integer in [0, 2048] = fp16 hi with lo = 0, on the x >= 0 side of the ELU (which returns x)
    wsplit  the target's non-zero weights are +-1 or +-(1 + 2^-13): after the group's scale 4096 (pick_scale: max in [4096, 8192))
            hi = 4096, lo = 0.5.  A dropped W_lo X_hi product or a swapped hi | lo fragment half loses the 2^-13 parts.
    xsplit  the bias of the layer that PRODUCES the target's input is 1 + k 2^-12 (k = 1..3 by channel), so the stored input has a
            non-zero lo half everywhere.  A dropped W_hi X_lo product or a lo half from the wrong row loses the 2^-12 parts.
The kernel omits W_lo X_lo by design; in both split classes that product is zero everywhere (the weights that meet a split
activation are integers and vice versa).  tests/test_f16s_reference_cpu.py checks, from the reference and a numpy model of the
split alone, that the generators meet all of these conditions, and that the comparison would notice a swapped weight row, a row-end
neighbour that is not zeroed and a dropped lo half.

Inputs: position b of the S*S distinct ones holds one stone per plane p at pixel (37 p + b) mod S*S, and the stem selector gives
channel c the value 1 + (c // 3) mod 3 of plane c mod 3 — over the positions every (cin, pixel) site of every layer's input is
non-zero exactly once, so every tap meets every edge, every corner and, on 15x15, both sides of the half seam at pixel 128.
The stem's own case runs on 0 / 1 planes (full, empty, single stones at corners, edge midpoints and centre, random fill).  Larger
batches tile the distinct positions.  Before every checked forward one forward runs on the positions in reverse order, and a test
reads only what its launch form writes (READABLE), so a skipped store leaves wrong values, not yesterday's right ones.

Which buffers a forward writes (f16s_plan, include/af_net.h):
    f0 g1 o1 g2 o2 g4 o4 vconv pconv     every form (roles B <= 8, paired, branches; tile split or whole positions), both sizes
    g3 g5                                15x15 always; 11x11 only with af_net_tune(7, 256) — fused blocks keep them in LDS
    o3 o5                                never (registers -> head convolution)

Shapes (B, key-7 bits) and the kernel forms they reach — 11x11, ncu = CUs of the device (256):
    (1 | 2 | 8, 0)   af_small_forward_f16s: ONE launch of dataflow roles, tile-split bodies, fused blocks 3 / 5 + af_policy_fc_f16s
    (9, 0)           smallest whole-position form: af_stem_mfma_f16s, af_conv_f16s, af_big_pair_f16s / af_big_l7v_f16s, af_block_f16s
    (121, 0)         every site once
    (1025, 0)        the largest grid of any layer is layer 0's (bone/block1 conv1: two workgroups per CU, 2 x 256 = 512), so at
                     1025 positions its workgroup 0 walks positions 0, 512, 1024: both LDS ring parities and the drain; every other
                     layer's workgroups walk 4 or more (the digests use 600, which gives layer 0 two at most)
    (8 | 9, 256)     two launches per 32-wide block: g3 / g5 observed, tile-split af_conv_f16s_sb / whole positions
    (8, 2048)        the nine dependent launches instead of the roles
    (9, 16) VALU stem; (121, 32) one workgroup per CU in the 32-channel-input layers; (8, 128) one workgroup per position
15x15: (3, 0) two-halves launch; (127, 0) / (128, 0) either side of half_classes (af_conv_f16s_h15 + af_corner_f16s from 128);
    (225, 0) every site once on the class split; (128, 64) the two-halves launch at 128.

DENSE LAYERS.  Softmax and tanh cannot be bit-exact; selector weights put one integer head-convolution value on each logit and
an integer in [-8, 8] on the value's pre-activation x, and log p_j - log p_0 and 2 atanh(v) are compared with the fp64 logits / x.
Tolerance: a probability is exp (<= 2 ulp on v_exp_f32 plus 2^-24 |t| from the argument's rounding, |t| <= 8 log2 e) over a sum
of S*S terms and a division: relative error <= (S*S + 16) 2^-24, twice for the difference of two logs, doubled because the
order of the reduction is not specified: 4 (S*S + 16) 2^-24 <= 5.8e-5.  v = tanh(x / 2) with absolute error <= 8 2^-24 (a
quotient of two exponentials), d(2 atanh v) = 2 dv / (1 - v^2): 16 2^-24 / (1 - tanh(x/2)^2) <= 7.1e-4 at |x| = 8.  Neighbouring
integers are 1 apart: both are more than 1000x below that.

ROUNDED REGIME.  Random fp32 weights (Glorot), biases of order 1, one scale group (bone/block2 conv1) whose members span 2^12, on
0 / 1 boards; and the ENVELOPE: the shipped checkpoint with one layer's group scaled by a power of two so that its largest
activation lies in [2^15, 65504) (its consumer's kernel scaled back, so that nothing behind it leaves the range), or all of its
activations below 2^-14 (hi a fp16 subnormal), for a trunk layer (g2) and a branch layer (g4).  Every layer L is compared per
element with fp64 OF THE INPUT THE KERNEL ACTUALLY READ (the read-back of L's input buffers, which is exactly hi + lo), so no
error propagates between layers; where an input is not stored (o3 / o5, fused g3 / g5) its own bound E is carried through |w|.
    |got - ref| <= conv(|x|, dW) + 2 2^-22 A + 2^-25 sum|w| + 2 n 2^-24 A + 2^-22 |ref| + 2^-25 + 2^-22 + conv(E, |w|)
    dW = |w - (hi + lo) / scale| elementwise from the numpy model of the packer's split (exact: it covers small members of a
         wide group, whose lo half is subnormal);  2^-22 A: the split of an input formed in registers, again 2^-22 A: the dropped
         W_lo X_lo (2^-11 2^-11 per product);  2^-25 sum|w|: the absolute floor of that split, lo being a fp16 subnormal below
         2^-3 — this is the term that carries the small side of the envelope;  2 n 2^-24 A: fp32 accumulation of n terms with
         absolute-term sum A, doubled because the MFMA's internal order is undocumented;  2^-22 |ref| + 2^-25: the split of the
         stored value;  2^-22: v_exp_f32 (1 ulp of a value <= 1) and the rounding of its argument on the ELU's negative side, as
         the comment above elu1 bounds it.  No constant is fitted.
The end-to-end 1e-5 bar on policy and value is asserted only where PyTorch's own fp32 evaluation of the same weights meets it.
No case drives an activation past 65504: beyond it the outputs are undefined (include/af_net.h).
"""
import functools
import os

import numpy as np
import pytest

from conftest import GOLDEN
from net_cases import BLOCKS, CASES, LAYERS, board_positions, dense_case, exact_reference, exact_variables, rounded_variables
from oracle import net_fp64

W6960 = os.path.join(GOLDEN, "alphaFive-6960.weights.npz")
# scale groups of the packer (f16s_update_absmax): kernels that share one power-of-two scale
FOLDED = (1, 2, 4)                               # blocks whose projection rides conv2 as extra k-steps; 3 and 5 produce it separately
CONFIGS11 = ((1, 0), (2, 0), (8, 0), (9, 0), (121, 0), (1025, 0), (8, 256), (9, 256), (8, 2048), (9, 16), (121, 32), (8, 128))
CONFIGS15 = ((3, 0), (127, 0), (128, 0), (225, 0), (128, 64))
MAX_BATCH = {11: 1025, 15: 225}


def readable(S, bits):
    """The keys a forward with these key-7 bits writes (module docstring)."""
    keys = ["f0", "g1", "o1", "g2", "o2", "g4", "o4", "vconv", "pconv"]
    return tuple(keys + ["g3", "g5"]) if S == 15 or (bits & 256) else tuple(keys)


# ------------------------------------------------------------------ numpy model of the split ------------------------------------------------------------------
def pick_scale(mx):
    """pick_scale of af_conv_f16s.hip: the power of two that puts a group's max|w| into [4096, 8192)."""
    mx = float(np.float32(mx))
    if not (mx > 0.0) or not np.isfinite(mx):
        return 1.0
    return 2.0 ** (13 - np.frexp(mx)[1])


def split16(x):
    """hi = fp16(x), lo = fp16(x - hi) of fp32 values, as the packer and the epilogues compute them -> (hi, lo) in float64."""
    x = np.asarray(x, np.float32)
    hi = x.astype(np.float16)
    lo = (x - hi.astype(np.float32)).astype(np.float16)
    return hi.astype(np.float64), lo.astype(np.float64)


def scale_groups(v):
    """-> {kernel name: the power-of-two scale of its group}, the convolutions' groups only."""
    out = {}

    def group(*names):
        s = pick_scale(max(np.abs(v[n]).max() for n in names))
        for n in names:
            out[n] = s
    group("bone/conv1/kernel")
    for k, (name, _, _, _) in enumerate(BLOCKS, 1):
        group(name + "_conv1/kernel")
        if k in FOLDED:
            group(name + "_conv2/kernel", name + "_res/kernel")
        else:
            group(name + "_conv2/kernel")
            group(name + "_res/kernel")
    group("value/conv/kernel")
    group("policy/conv/kernel")
    return out


# ---- rounded regime (the generators of the cases, generic in the board size: tests/net_cases.py) ----
ENVELOPE = (("large", "trunk"), ("large", "branch"), ("small", "trunk"), ("small", "branch"))
ENVELOPE_LAYER = {"trunk": ("bone/block2", "g2"), "branch": ("policy/block4", "g4")}


@functools.lru_cache(maxsize=None)
def envelope_variables(side, where):
    """The shipped checkpoint with `where`'s conv1 (kernel and bias: the layer's pre-activation) scaled by a power of two:
    large — its largest activation on the 64 positions of board_positions(11, 64) moves into [2^15, 2^16) (the generator's CPU test
    holds it below 65504), and the block's conv2 kernel, the layer's only consumer, is scaled back by the same power;
    small — every activation of the layer falls below 2^-14 (one group rescaled, nothing else)."""
    with np.load(W6960) as z:
        v = {k: z[k].astype(np.float32) for k in z.files}
    name, key = ENVELOPE_LAYER[where]
    x = board_positions(11, 64, seed=0)
    out = net_fp64.intermediates(v, x, sums=True)
    if side == "large":
        e = int(np.ceil(np.log2(2.0 ** 15 / out[key].max())))
        v[name + "_conv2/kernel"] = v[name + "_conv2/kernel"] * np.float32(2.0 ** -e)
    else:
        e = -(int(np.ceil(np.log2(np.abs(out["pre:" + key]).max() / 2.0 ** -14))) + 1)
    v[name + "_conv1/kernel"] = v[name + "_conv1/kernel"] * np.float32(2.0 ** e)
    v[name + "_conv1/bias"] = v[name + "_conv1/bias"] * np.float32(2.0 ** e)
    return v, x, key


def layer_bounds(v, planes, got, keys):
    """The rounded regime's comparison (module docstring): every convolution recomputed in fp64 from the input the kernel read.
    got: {key: float64 [B, C, S, S]} read back; keys: what the launch form wrote.  -> {key: (|got - ref|, bound, ref)} for those keys."""
    scales = scale_groups(v)
    state, report = {"planes": (np.asarray(planes, np.float64), None)}, {}
    for key, conv, proj, src, src2 in LAYERS:
        pre = A = W = dW = E = 0.0
        n = 1
        for cname, skey in ((conv, src), (proj, src2)):
            if cname is None:
                continue
            x, Ein = state[skey]
            k32 = v[cname + "/kernel"].astype(np.float32)
            k, b = k32.astype(np.float64), v[cname + "/bias"].astype(np.float64)
            s = scales[cname + "/kernel"]
            hi, lo = split16(k32 * np.float32(s))
            zero = np.zeros_like(b)
            pre = pre + net_fp64._conv2d_flat(x, k, b)
            A = A + net_fp64._conv2d_flat(np.abs(x), np.abs(k), np.abs(b))
            dW = dW + net_fp64._conv2d_flat(np.abs(x), np.abs(k - (hi + lo) / s), zero)
            W = W + np.abs(k).sum(axis=(0, 1, 2))[None, :, None, None]
            n += int(np.prod(k.shape[:3]))
            if Ein is not None:
                E = E + net_fp64._conv2d_flat(Ein, np.abs(k), zero)
        ref = net_fp64._elu(pre)
        bound = dW + 2.0 * 2.0 ** -22 * A + 2.0 ** -25 * W + 2.0 * n * 2.0 ** -24 * A + 2.0 ** -22 * np.abs(ref) + 2.0 ** -25 + 2.0 ** -22 + E
        if key in keys:
            report[key] = (np.abs(got[key] - ref), bound, ref)
            state[key] = (got[key], None)
        else:
            state[key] = (ref, bound)
    return report


# ------------------------------------------------------------------ GPU side ------------------------------------------------------------------
_gpu = pytest.mark.gpu
_handles = {}


@pytest.fixture(scope="module", autouse=True)
def _close_handles():
    """frees the device memory the module's handles hold when its last test has run"""
    yield
    while _handles:
        _handles.popitem()[1].close()


def _net(S, v):
    """One handle per board size for the whole module (af_net_create allocates for the largest batch), reloaded per case."""
    from alphafive_amd import net_hip
    v32 = {k: np.ascontiguousarray(a, np.float32) for k, a in v.items()}
    if S not in _handles:
        _handles[S] = net_hip.HipNet(v32, S, MAX_BATCH[S], "cuda:0")
    else:
        _handles[S].load(v32)
    return _handles[S]


def _forward(net, planes, bits):
    """One forward on the positions in reverse order, then the checked one -> (policy, value) as numpy; restores key 7."""
    import torch
    from alphafive_amd import net_hip
    x = torch.from_numpy(np.ascontiguousarray(planes, np.float32)).cuda()
    try:
        net_hip.tune(7, bits)
        net(torch.flip(x, dims=(0, 1)).contiguous())
        p, v = net(x)
        p, v = p.cpu().numpy().copy(), v.cpu().numpy().copy()
    finally:
        net_hip.tune(7, 0)
    if planes.shape[0] <= 8 and net.S == 11:
        assert net.small_forward_error() == 0
    return p, v


def _read(net, keys, B):
    S = net.S
    return {k: net.debug_activation(k, B).astype(np.float64).reshape(B, -1, S, S) for k in keys}


_EXACT_PARAMS = [pytest.param(S, B, bits, t, c, id="%d-B%d-bits%d-%s-%s" % (S, B, bits, t, c))
                 for S, configs in ((11, CONFIGS11), (15, CONFIGS15)) for (t, c) in CASES for (B, bits) in configs]


@_gpu
@pytest.mark.parametrize("S,B,bits,target,cls", _EXACT_PARAMS)
def test_exact_regime_every_written_buffer_equals_fp64_bit_for_bit(S, B, bits, target, cls):
    """Every buffer the launch form writes, not only the target's: the selectors behind the target must hand its values on unchanged
    (a wrong one there is a wrong copy), and the ones in front of it must deliver the sites."""
    v, planes, _ = exact_variables(S, target, cls)
    ref = exact_reference(S, target, cls)
    net = _net(S, v)
    idx = np.arange(B) % (S * S)
    _forward(net, planes[idx], bits)
    for k in readable(S, bits):
        got = net.debug_activation(k, B)
        want = ref[k][idx]
        bad = got.view(np.uint32) != want.view(np.uint32)
        assert not bad.any(), "%s (target %s, %s): %d of %d elements differ, first at [b, c, pixel] = %s: got %r, fp64 %r" % (
            k, target, cls, int(bad.sum()), bad.size, tuple(np.argwhere(bad)[0]), got[bad][0], want[bad][0])


@_gpu
@pytest.mark.parametrize("S,B,bits", [(11, 8, 0), (11, 64, 0), (11, 8, 2048), (15, 3, 0), (15, 130, 0)])
def test_dense_layers_put_each_integer_on_its_logit(S, B, bits):
    v, planes, ref = dense_case(S)
    idx = np.arange(B) % planes.shape[0]
    net = _net(S, v)
    p, val = _forward(net, planes[idx], bits)
    p, val = p.astype(np.float64), val.astype(np.float64)
    n = S * S
    logits, x = ref["logits"][idx], ref["vpre"][idx]
    assert (logits == np.round(logits)).all() and (x == np.round(x)).all() and np.abs(x).max() <= 8 and np.ptp(logits, axis=1).max() <= 8
    tol_p = 4.0 * (n + 16) * 2.0 ** -24
    dl = np.abs((np.log(p) - np.log(p[:, :1])) - (logits - logits[:, :1]))
    tol_v = 16.0 * 2.0 ** -24 / (1.0 - np.tanh(x / 2.0) ** 2)
    dx = np.abs(2.0 * np.arctanh(val) - x)
    print("dense S=%d B=%d bits=%d: |d log-ratio| max %.3g (tolerance %.3g), |d 2 atanh v| / tolerance max %.3g" % (S, B, bits, dl.max(), tol_p, (dx / tol_v).max()))
    assert tol_p < 1e-2 and tol_v.max() < 1e-2
    assert (dl <= tol_p).all()
    assert (dx <= tol_v).all()
    assert np.abs(p.sum(axis=1) - 1.0).max() < 1e-5


def _report(tag, report):
    worst = 0.0
    for key, (err, bound, ref) in report.items():
        r = float((err / bound).max())
        worst = max(worst, r)
        print("%s %-5s max|err| %.3g  max|ref| %.3g  max err/bound %.3g" % (tag, key, err.max(), np.abs(ref).max(), r))
    return worst


def _end_to_end(tag, v, x, p, val):
    """Asserts the 1e-5 bar where PyTorch's fp32 evaluation of the same weights meets it; prints both."""
    import torch
    from alphafive_amd.network import ResNet
    S = x.shape[-1]
    out = net_fp64.intermediates(v, x)
    net = ResNet(S, device="cuda")
    net.set_variables({k: np.asarray(a, np.float32) for k, a in v.items()})
    pt, vt = net.eval_torch(torch.from_numpy(np.ascontiguousarray(x, np.float32)).cuda())
    dpt, dvt = np.abs(pt.cpu().numpy() - out["prob"]).max(), np.abs(vt.cpu().numpy() - out["value"]).max()
    dp, dv = np.abs(p - out["prob"]).max(), np.abs(val - out["value"]).max()
    print("%s end to end: kernel |dp| %.3g |dv| %.3g; PyTorch fp32 |dp| %.3g |dv| %.3g" % (tag, dp, dv, dpt, dvt))
    if dpt < 1e-5:
        assert dp < 1e-5
    if dvt < 1e-5:
        assert dv < 1e-5


@_gpu
@pytest.mark.parametrize("S,B,bits", [(11, 8, 0), (11, 200, 0), (11, 9, 256), (15, 3, 0), (15, 130, 0)])
def test_rounded_regime_every_layer_within_the_derived_bound(S, B, bits):
    v = rounded_variables(S, seed=50 + S)
    x = board_positions(S, B, seed=3)
    net = _net(S, v)
    p, val = _forward(net, x, bits)
    keys = readable(S, bits)
    report = layer_bounds(v, x, _read(net, keys, B), keys)
    worst = _report("rounded S=%d B=%d bits=%d" % (S, B, bits), report)
    _end_to_end("rounded S=%d B=%d bits=%d" % (S, B, bits), v, x, p, val)
    for key, (err, bound, ref) in report.items():
        assert np.isfinite(err).all() and (err <= bound).all(), key
    assert worst <= 1.0


@_gpu
@pytest.mark.parametrize("side,where", ENVELOPE)
def test_range_envelope_layer_and_its_consumers_within_the_derived_bound(side, where):
    v, x, key = envelope_variables(side, where)
    net = _net(11, v)
    for bits in (0, 256):                                        # fused blocks, and the form that stores g3 / g5
        p, val = _forward(net, x, bits)
        keys = readable(11, bits)
        got = _read(net, keys, x.shape[0])
        top = np.abs(got[key]).max()
        assert (2.0 ** 15 <= top < 65504.0) if side == "large" else (0.0 < top < 2.0 ** -14)
        report = layer_bounds(v, x, got, keys)
        tag = "envelope %s %s bits=%d" % (side, where, bits)
        _report(tag, report)
        _end_to_end(tag, v, x, p, val)
        for k, (err, bound, ref) in report.items():
            assert np.isfinite(got[k]).all() and np.abs(got[k]).max() < 65504.0, k
            assert (err <= bound).all(), k
