"""The fp32 Winograd forward (csrc/af_net.hip: af_stem_conv, af_conv_wino with the folded 1x1 projection, af_value_head,
af_policy_head<8> / <4>, af_policy_head_mfma, the packer af_update_wino) against oracle/net_fp64.py one layer at a time, on every
board size af_net_create accepts (3..16), through the read-back of the path's eleven fp32 planes (HipNet.debug_activation_fp32,
af_net_debug_activation's which = 16 + i / 32 + i).  It is the path of every size but 11x11 and 15x15, and there af_net_tune(0, 1)
selects it.  Generators, the numpy model and the comparisons: tests/net_cases.py; tests/test_wino_reference_cpu.py checks them
without a GPU.

EXACT REGIME.  The cases of tests/test_gpu_f16s_exact.py (one TARGET layer with random weights in {-1, 0, 1}, 1 + 2^-13 parts in
class wsplit, 1 + k 2^-12 inputs in class xsplit, behind and in front of centre-tap selectors; inputs that put a non-zero value on
every (cin, pixel) site once over S*S positions).  In the Winograd domain U = G g G^T is a multiple of 1/4 of the weights' unit and
V = B^T d B a sum of four inputs, and every sum stays below 2^24 units, so af_conv_wino must equal fp64 BIT FOR BIT in all eleven
planes — this path stores g3, o3, g5 and o5 too — whatever the order of its sums (the CPU module shows both orders).
    full matrix      all 18 targets x {int, wsplit, xsplit} (no xsplit for the stem) at S = 3, 4 (smallest odd / even board),
                     7 (odd, MFMA policy head), 11 (bench.py's size), 16 (largest)
    reduced matrix   class int, targets stem, b1.conv1, b2.conv2, b2.proj, b3.conv2, b5.proj, vconv, pconv at every other size
    batches          1;  S*S: every site once, and a ragged last wave wherever T^2 is no multiple of 32;  1024 // T^2 + 1: the
                     first batch past 1024 tiles, where wino_task's 8-way workgroup interleave starts its second round (257 at
                     S = 3, 17 at S = 16); larger batches tile the case's distinct positions
    side stream      S = 7 and 11, every target once more with af_net_tune(4, 0): the value branch on the caller's stream
Before every checked forward one forward runs on the same positions in reverse order (planes reversed too), so a skipped store
leaves wrong values, not yesterday's right ones.  No (size, class) pair is left out.

BORDERS AND NEIGHBOURS, after the exact forward of every case at B = S*S, through the planes as stored: every element outside the
S x S interior (border rows and columns, the pad behind WP^2) of positions below B is +0.0 by its bits — the planes are zero-filled
once and a store into row or column S of an odd board would corrupt the next layer's taps for good; positions B .. max_batch - 1
(the handles are three positions larger than their largest batch) keep, bit for bit, what a preceding forward at max_batch on other
planes left there; policy and value rows from B on keep a sentinel.

HEADS.  dense_case(S) at every S = 3..16 and batches 1, 7, 8, 9, 15, 16, 17 (either side of the 8 and 16 positions a workgroup of
af_value_head / af_policy_head<8> / af_policy_head_mfma takes, and of the 4 of af_policy_head<4>): integer logits of spread <= 8,
|x| <= 8, tolerances 4 (S*S + 16) 2^-24 on log p_j - log p_0 and 16 2^-24 / (1 - tanh(x/2)^2) on 2 atanh v, as derived in
tests/test_gpu_f16s_exact.py (net_cases.dense_check).  Default heads (af_policy_head_mfma up to 11x11, af_policy_head<4> above),
af_policy_head<8> with af_net_tune(5, 0) up to 11x11, and on 15x15 the split-operand branches followed by these heads
(af_net_tune(9, 0)).  At 16x16 af_policy_head<4> asks for (16 256 4 + 512 + 16) 4 = 67,648 bytes of dynamic LDS, above 64 KiB:
measured on an MI355X, the launch is accepted as it stands (af_net_forward returns 0 without the kernel's dynamic-LDS attribute
raised; allocate() raises it for af_policy_head_mfma only) and the head meets both tolerances at all seven batches
(|d log-ratio| <= 1.2e-7 against 6.5e-5).

ROUNDED REGIME.  rounded_variables(S, 50 + S) on board_positions(S, B, 3), S in {3, 7, 12, 16} x B in {1, 9} and S = 11 (tune(0, 1)),
B = 9.  Every layer is recomputed in fp64 from the planes the kernel actually read (the read-back of its sources), so no error passes
between layers, and per element
    |got - ref| <= (2 n + 8) 2^-24 (A_w + |b|) + 2^-22
    A_w = |A^T| (sum_c |U| (.) |B^T| |d| |B|) |A|, the absolute-term sum of the layer in the Winograd domain, plus the folded
          projection's;  n = cin, plus the projection's cin.  The roundings a term passes, counted from the kernel: U (one, fp64 sum
          rounded to fp32), V (two levels of adds), the accumulation over n terms — n roundings, doubled because the MFMA's internal
          order is undocumented —, the output transform (s0 / s1: two adds, y: two more) and the bias (one): 1 + 2 + 2 n + 5.  First
          order in 2^-24; the doubling covers the second-order terms ((2 n + 8) 2^-24 <= 1.6e-5) many times over.
    2^-22   the ELU's __expf - 1 on the negative side, as the comment above elu1 bounds it; the ELU itself is 1-Lipschitz.
    stem    the same formula with the direct convolution's absolute-term sum and n = 75 (its 76 fma roundings are fewer).
No constant is fitted.  The worst-case bound is loose, so there is a yardstick next to it: per layer the kernel's largest error is at
most 4x the largest error of the numpy model (wino_layer, cin forwards) on the same input — the margin the project gives the loss
head for a different but legitimate summation order.  Measured (err / bound, kernel / model), worst layer per case:
    S = 3: (0.021, 1.00) at B = 1, (0.032, 1.00) at B = 9;  S = 7: (0.019, 1.00), (0.067, 1.00);  S = 12: (0.026, 1.00), (0.038, 1.00);
    S = 16: (0.019, 1.00), (0.038, 1.00);  S = 11: (0.038, 1.00).  The worst err / bound is the stem's everywhere; the Winograd layers
    lie between 0.001 and 0.012.  kernel / model is 1.00 on all 99 (case, layer) pairs: the largest error of the kernel is the
    model's to every printed digit — the MFMA evidently accumulates its k-steps in order, as the model does.
The end-to-end 1e-5 bar on policy and value is asserted where PyTorch's fp32 evaluation of the same weights meets it.

ALL SIZES END TO END.  S = 3..16, random-init weights, B = 5: policy and value within 1e-5 of net_fp64.forward, rows sum to 1 within
1e-5, the last position evaluated alone gives the bits it has inside the batch.
"""
import contextlib

import numpy as np
import pytest

import net_cases as nc
from net_cases import CASES, PLANES, TARGETS, exact_reference, exact_variables
from oracle import net_fp64

FULL_SIZES = (3, 4, 7, 11, 16)
REDUCED_SIZES = (5, 6, 8, 9, 10, 12, 13, 14, 15)
REDUCED_TARGETS = ("stem", "b1.conv1", "b2.conv2", "b2.proj", "b3.conv2", "b5.proj", "vconv", "pconv")
EXACT_TRIPLES = tuple((S, t, c) for S in FULL_SIZES for (t, c) in CASES) + tuple((S, t, "int") for S in REDUCED_SIZES for t in REDUCED_TARGETS)
SPARE = 3                                        # positions of a handle behind its largest batch: the neighbours the border test watches
HEAD_BATCHES = (1, 7, 8, 9, 15, 16, 17)
SENTINEL = -7.0

pytestmark = pytest.mark.gpu
_handles, _loaded = {}, {}


def max_batch(S):
    return max(nc.wino_batches(S) + HEAD_BATCHES) + SPARE


@pytest.fixture(scope="module", autouse=True)
def _close_handles():
    """frees the device memory the module's handles hold when its last test has run"""
    yield
    while _handles:
        _handles.popitem()[1].close()
    _loaded.clear()


def _net(S, v, case):
    """One handle per board size for the whole module, reloaded when the case changes."""
    from alphafive_amd import net_hip
    if S in _handles and _loaded.get(S) == case:
        return _handles[S]
    v32 = {k: np.ascontiguousarray(a, np.float32) for k, a in v.items()}
    if S not in _handles:
        _handles[S] = net_hip.HipNet(v32, S, max_batch(S), "cuda:0")
    else:
        _handles[S].load(v32)
    _loaded[S] = case
    return _handles[S]


@contextlib.contextmanager
def _tuned(S, *pairs, fp32=True):
    """The fp32 path (af_net_tune(0, 1) where the split-operand path is the default) plus `pairs` of (key, value); all put back."""
    from alphafive_amd import net_hip
    try:
        if fp32 and S in (11, 15):
            net_hip.tune(0, 1)
        for key, value in pairs:
            net_hip.tune(key, value)
        yield
    finally:
        net_hip.tune(0, 5)
        net_hip.tune(4, 1)
        net_hip.tune(5, 1)
        net_hip.tune(9, 1)


def _run(net, planes):
    import torch
    x = torch.from_numpy(np.ascontiguousarray(planes, np.float32)).cuda()
    p, v = net(x)
    torch.cuda.synchronize()
    return p.cpu().numpy().copy(), v.cpu().numpy().copy()


def _forward(net, planes):
    """One forward on the positions in reverse order (and the planes of each reversed), then the checked one -> (policy, value)."""
    _run(net, np.ascontiguousarray(np.asarray(planes)[::-1, ::-1]))
    return _run(net, planes)


def _stored(net, B):
    return {k: net.debug_activation_fp32(k, B, padded=True) for k in PLANES}


def _check_planes(net, S, B, ref, idx, tag):
    for k in PLANES:
        nc.assert_same_bits(net.debug_activation_fp32(k, B), ref[k][idx], "%s plane %s" % (tag, k))


def _check_borders_and_neighbours(net, S, planes, idx, ref, tag):
    """The exact forward at B = len(idx) between a forward at max_batch on other planes and a look at everything the handle holds."""
    import torch
    B, MB, N = len(idx), net.max_batch, planes.shape[0]
    assert MB > B
    other = np.ascontiguousarray(planes[(7 * np.arange(MB) + 3) % N][:, ::-1])
    _run(net, other)
    before = _stored(net, MB)
    net.policy.fill_(SENTINEL)
    net.value.fill_(SENTINEL)
    _forward(net, planes[idx])
    after = _stored(net, MB)
    for k in PLANES:
        nc.assert_same_bits(nc.interior(after[k][:B], S), ref[k][idx], "%s plane %s" % (tag, k))
        nc.assert_border_zero(after[k][:B], S, "%s plane %s" % (tag, k))
        nc.assert_same_bits(after[k][B:], before[k][B:], "%s plane %s, positions %d..%d of the handle" % (tag, k, B, MB - 1))
        assert (before[k][B:] != 0).any(), k                     # (the neighbours hold something a stray store would change)
    torch.cuda.synchronize()
    sentinel = np.float32(SENTINEL)
    nc.assert_same_bits(net.policy[B:MB].cpu().numpy(), np.full((MB - B, S * S), sentinel), tag + " policy rows from B on")
    nc.assert_same_bits(net.value[B:MB].cpu().numpy(), np.full(MB - B, sentinel), tag + " value rows from B on")
    assert (net.policy[:B].cpu().numpy() != sentinel).all() and (net.value[:B].cpu().numpy() != sentinel).all()


_EXACT_PARAMS = [pytest.param(S, t, c, B, id="%d-%s-%s-B%d" % (S, t, c, B)) for (S, t, c) in EXACT_TRIPLES for B in dict.fromkeys(nc.wino_batches(S))]


@pytest.mark.parametrize("S,target,cls,B", _EXACT_PARAMS)
def test_exact_regime_every_plane_equals_fp64_bit_for_bit(S, target, cls, B):
    """All eleven planes, not only the target's: the selectors behind the target must hand its values on unchanged and the ones in
    front of it must deliver the sites.  At B = S*S also the borders, the pad, the handle's further positions and the outputs' rows."""
    v, planes, _ = exact_variables(S, target, cls)
    ref = exact_reference(S, target, cls)
    idx = np.arange(B) % planes.shape[0]
    net = _net(S, v, (target, cls))
    tag = "S=%d %s %s B=%d" % (S, target, cls, B)
    with _tuned(S):
        if B == S * S:
            _check_borders_and_neighbours(net, S, planes, idx, ref, tag)
        else:
            _forward(net, planes[idx])
            _check_planes(net, S, B, ref, idx, tag)


@pytest.mark.parametrize("S,target", [(S, t) for S in (7, 11) for t in TARGETS])
def test_exact_regime_value_branch_on_the_callers_stream(S, target):
    v, planes, _ = exact_variables(S, target, "int")
    ref = exact_reference(S, target, "int")
    B = S * S
    idx = np.arange(B) % planes.shape[0]
    net = _net(S, v, (target, "int"))
    with _tuned(S):
        p1, v1 = _forward(net, planes[idx])
    with _tuned(S, (4, 0)):
        p0, v0 = _forward(net, planes[idx])
        _check_planes(net, S, B, ref, idx, "S=%d %s side stream off" % (S, target))
    nc.assert_same_bits(p0, p1, "policy with and without the side stream")
    nc.assert_same_bits(v0, v1, "value with and without the side stream")


_HEAD_PARAMS = [(S, "default") for S in range(3, 17)] + [(S, "valu8") for S in range(3, 12)] + [(15, "split-operand branches")]


@pytest.mark.parametrize("S,heads", _HEAD_PARAMS)
def test_dense_layers_put_each_integer_on_its_logit(S, heads):
    v, planes, ref = nc.dense_case(S)
    net = _net(S, v, "dense")
    tune = {"default": dict(), "valu8": dict(pairs=((5, 0),)), "split-operand branches": dict(pairs=((9, 0),), fp32=False)}[heads]
    with _tuned(S, *tune.get("pairs", ()), fp32=tune.get("fp32", True)):
        for B in HEAD_BATCHES:
            idx = np.arange(B) % planes.shape[0]
            p, val = _forward(net, planes[idx])
            nc.dense_check("dense S=%d %s B=%d" % (S, heads, B), S, p, val, ref["logits"][idx], ref["vpre"][idx])


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


@pytest.mark.parametrize("S,B", [(S, B) for S in (3, 7, 12, 16) for B in (1, 9)] + [(11, 9)])
def test_rounded_regime_every_layer_within_the_derived_bound_and_the_models_error_class(S, B):
    v = nc.rounded_variables(S, seed=50 + S)
    x = nc.board_positions(S, B, seed=3)
    net = _net(S, v, "rounded")
    with _tuned(S):
        p, val = _forward(net, x)
        got = _stored(net, B)
    report = nc.wino_bounds(S, v, x, got)
    tag = "rounded S=%d B=%d" % (S, B)
    worst = [0.0, 0.0]
    for key, (err, bound, ref, model_err) in report.items():
        r, m = float((err / bound).max()), float(err.max() / model_err.max())
        worst = [max(worst[0], r), max(worst[1], m)]
        print("%s %-3s max|ref| %.3g  kernel max|err| %.3g  model max|err| %.3g  kernel / model %.3g  max err/bound %.3g" % (
            tag, key, np.abs(ref).max(), err.max(), model_err.max(), m, r))
    print("%s worst err/bound %.3g, worst kernel / model %.3g" % (tag, worst[0], worst[1]))
    _end_to_end(tag, v, x, p, val)
    for key, (err, bound, ref, model_err) in report.items():
        assert np.isfinite(got[key]).all() and np.isfinite(err).all(), key
        assert (err <= bound).all(), key
        assert err.max() <= 4.0 * model_err.max(), key
        nc.assert_border_zero(got[key], S, "%s plane %s" % (tag, key))


@pytest.mark.parametrize("S", range(3, 17))
def test_every_board_size_end_to_end(S):
    from alphafive_amd.network import random_variables
    B = 5
    v = random_variables(S, seed=S)
    x = nc.board_positions(S, B, seed=S)
    net = _net(S, v, "random-init")
    with _tuned(S):
        p, val = _forward(net, x)
        p1, val1 = _run(net, x[B - 1:])
    p64, v64 = net_fp64.forward(v, x)
    dp, dv = np.abs(p - p64).max(), np.abs(val - v64).max()
    print("end to end S=%d: |dp| %.3g |dv| %.3g" % (S, dp, dv))
    assert np.isfinite(p).all() and np.isfinite(val).all()
    assert dp < 1e-5 and dv < 1e-5
    assert np.abs(p.astype(np.float64).sum(axis=1) - 1.0).max() < 1e-5
    nc.assert_same_bits(p1[0], p[B - 1], "policy of the last position alone")
    nc.assert_same_bits(val1[0], val[B - 1], "value of the last position alone")
