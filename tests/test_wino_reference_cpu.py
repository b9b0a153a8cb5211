"""No GPU: the numpy fp32 model of the fp32 Winograd path (tests/net_cases.py: wino_u, wino_v, wino_layer, stem_layer — U = fp32(G g G^T)
summed in fp64 as af_update_wino does, the 1x1 projection a centre-tap 3x3, V = B^T d B in two levels of fp32 adds, exact products and
fp32 accumulation over cin, Y = A^T M A in fp32 on planes padded to WP) against oracle/net_fp64.py, and the comparisons of
tests/test_gpu_wino_exact.py against planted faults.

EXACTNESS.  For every (S, target, class) of the GPU module's exact regime the model's eleven planes equal net_fp64.intermediates bit
for bit with cin accumulated forwards and backwards (the projection's segment after / before the 3x3 one), so the equality the GPU
module demands does not hang on the MFMA's order.  The sequential model costs a pass over all accumulators per cin, so it runs on six
positions of each case (three from 11x11 up) spread evenly over its planes, first and last among them; every (size, class) pair was
exact in both orders, none is left out.  (Over ALL positions of the full matrix at S = 3, 4, 7 and 11 a sufficient condition was
checked once, outside the suite: in the input transform, the accumulation per (xi, nu) and the output transform of every layer every
addend is a multiple of 2^-q and the absolute-term sum lies below 2^(24 - q) — at most 0.68 of that limit, b2.conv2 in class wsplit.
On the MI355X the GPU module's matrix, which runs all positions, is bit-equal throughout.)

PLANTED FAULTS.  assert_same_bits and assert_border_zero, the functions the GPU module calls, raise for: two U rows swapped; the
projection's four Winograd positions dropped; one (xi, nu) of the 16 taken from the neighbouring cin; a value in board row S or
column S of an odd board's padded plane; a tile of position b written into position b + 1.

ROUNDED REGIME.  On random weights the model stays within the GPU module's derived bound on every layer; the worst err / bound is
printed (0.02 to 0.07 over the sizes below, the stem's; the Winograd layers 0.001 to 0.008)."""
import numpy as np
import pytest

import net_cases as nc
import test_gpu_wino_exact as gpu
from oracle import net_fp64


def _spread(n, k=6):
    return np.unique(np.linspace(0, n - 1, k).astype(int))


@pytest.mark.parametrize("S,target,cls", gpu.EXACT_TRIPLES, ids=["%d-%s-%s" % t for t in gpu.EXACT_TRIPLES])
def test_model_equals_fp64_bit_for_bit_in_both_orders(S, target, cls):
    v, planes, key = nc.exact_variables(S, target, cls)
    idx = _spread(planes.shape[0], 6 if S < 11 else 3)
    ref = net_fp64.intermediates(v, planes[idx], flat=True)
    for name, a in v.items():
        assert (np.asarray(a, np.float32) == a).all(), name
    for backwards in (False, True):
        got = nc.wino_forward(S, v, planes[idx], backwards=backwards)
        for k in nc.PLANES:
            want = ref[k].astype(np.float32)
            assert (want == ref[k]).all(), k
            nc.assert_same_bits(nc.interior(got[k], S), want.reshape(len(idx), -1, S * S), "%s, cin %s" % (k, "backwards" if backwards else "forwards"))
            nc.assert_border_zero(got[k], S, k)


@pytest.mark.parametrize("S", [3, 4, 5, 6, 16])
def test_stone_planes_hold_the_special_boards_on_every_size(S):
    x = nc.stone_planes(S, np.random.default_rng(0))
    m = S // 2
    assert x.shape == (max(S * S, 32), 3, S, S) and set(np.unique(x)) == {0.0, 1.0} and x[0].all() and not x[1].any()
    singles = x[2:29]
    assert (singles.sum(axis=(1, 2, 3)) == 1).all()
    for (yy, xx) in ((0, 0), (0, S - 1), (S - 1, 0), (S - 1, S - 1), (0, m), (m, 0), (S - 1, m), (m, S - 1), (m, m)):
        assert (singles[:, :, yy, xx].sum(axis=0) >= 1).all()          # (on 3x3 / 4x4 some of the nine places coincide)
    assert x[29:].any()
    v, planes, key = nc.exact_variables(S, "stem", "int")
    assert planes.shape[0] == max(S * S, 32) and nc.exact_reference(S, "stem", "int")["f0"].shape == (planes.shape[0], 32, S * S)


@pytest.mark.parametrize("S", range(3, 17))
def test_plane_layout_helpers(S):
    T, WP, PP = nc.geometry(S)
    assert WP == 2 * ((S + 1) // 2) + 2 and PP % 16 == 0 and WP * WP <= PP < WP * WP + 16
    assert nc.outside_mask(S).sum() == PP - S * S
    x = np.arange(2 * 3 * S * S, dtype=np.float32).reshape(2, 3, S, S) + 1
    st = nc.to_stored(x, S)
    assert st.shape == (2, 3, PP) and (nc.interior(st, S).reshape(x.shape) == x).all() and st[0, 0, (0 + 1) * WP + 1] == x[0, 0, 0, 0]
    nc.assert_border_zero(st, S, "layout")
    B1, B2, B3 = nc.wino_batches(S)
    assert (B1, B2) == (1, S * S) and (B3 - 1) * T * T <= 1024 < B3 * T * T
    assert {3: 257, 16: 17}.get(S, B3) == B3


def _target_layer(S, target, cls):
    """-> (reference planes of the case, what wino_layer needs for the target's launch, the reference's output as stored bits)"""
    v, planes, key = nc.exact_variables(S, target, cls)
    ref = nc.exact_reference(S, target, cls)
    _, conv, proj, src, src2 = next(lay for lay in nc.LAYERS if lay[0] == key)
    U, bias = nc.wino_weights(v)
    n = planes.shape[0]
    stored = lambda k: nc.to_stored(ref[k].reshape(n, -1, S, S), S)
    args = dict(src=stored(src), u=U[conv], bias=bias[key], src2=stored(src2), u2=U[proj])
    return args, ref[key]


def _raises(fn):
    try:
        fn()
    except AssertionError:
        return True
    return False


def test_the_comparisons_notice_every_planted_fault():
    S = 7
    # ---- a 3x3 layer: U rows swapped, one (xi, nu) from the neighbouring cin, a tile in the next position ----
    args, want = _target_layer(S, "b2.conv2", "wsplit")
    same = lambda out: nc.assert_same_bits(nc.interior(out, S), want, "o2")
    same(nc.wino_layer(S, **args))                                                       # the unperturbed model passes
    u = args["u"]
    c = next(c for c in range(u.shape[1] - 1) if (u[:, c] != u[:, c + 1]).any())
    swapped = u.copy()
    swapped[:, [c, c + 1]] = u[:, [c + 1, c]]
    assert _raises(lambda: same(nc.wino_layer(S, **dict(args, u=swapped))))
    for x in range(16):                                                                  # each of the 16 positions on its own
        c = next(c for c in range(u.shape[1] - 1) if (u[x, c] != u[x, c + 1]).any())
        one = u.copy()
        one[x, c] = u[x, c + 1]
        assert _raises(lambda: same(nc.wino_layer(S, **dict(args, u=one)))), x
    assert _raises(lambda: same(nc.wino_layer(S, faults=("tile_to_next_position",), **args)))
    # ---- the folded projection dropped ----
    args, want = _target_layer(S, "b2.proj", "int")
    same = lambda out: nc.assert_same_bits(nc.interior(out, S), want, "o2")
    same(nc.wino_layer(S, **args))
    assert (args["u2"][[i for i in range(16) if i not in nc._CENTRE]] == 0).all() and (args["u2"][list(nc._CENTRE)] != 0).any()
    assert _raises(lambda: same(nc.wino_layer(S, **dict(args, u2=np.zeros_like(args["u2"])))))
    # ---- a store into board row S / column S of an odd board: the interior still equals the reference, the border check raises ----
    T, WP, PP = nc.geometry(S)
    good = nc.wino_layer(S, **args)
    nc.assert_border_zero(good, S, "o2")
    for off in ((S + 1) * WP + 1, (S + 1) * WP + S, 1 * WP + S + 1, S * WP + S + 1, (S + 1) * WP + S + 1):
        for val in (1.0, -0.0):
            bad = good.copy()
            bad[3, 5, off] = val
            same(bad)
            assert _raises(lambda: nc.assert_border_zero(bad, S, "o2")), (off, val)
    pad = good.copy()
    pad[0, 0, PP - 1] = 1.0                                                              # the pad behind WP * WP
    assert PP > WP * WP and _raises(lambda: nc.assert_border_zero(pad, S, "o2"))


@pytest.mark.parametrize("S,B", [(3, 3), (7, 3), (12, 3), (16, 2)])
def test_model_within_the_derived_bound_on_random_weights(S, B):
    v = nc.rounded_variables(S, seed=50 + S)
    x = nc.board_positions(S, B, seed=3)
    got = nc.wino_forward(S, v, x)
    report = nc.wino_bounds(S, v, x, got)
    worst = 0.0
    for key, (err, bound, ref, model_err) in report.items():
        assert (err == model_err).all(), key                       # the model recomputed from its own planes is the model
        assert np.isfinite(err).all() and (err <= bound).all(), key
        assert ((ref < 0).any() and (ref > 0).any()), key          # both sides of the ELU
        worst = max(worst, float((err / bound).max()))
        print("model S=%d B=%d %-3s max|err| %.3g  max|ref| %.3g  max err/bound %.3g" % (S, B, key, err.max(), np.abs(ref).max(), (err / bound).max()))
    print("model S=%d B=%d worst err/bound %.3g" % (S, B, worst))
    assert 0.0 < worst <= 1.0
