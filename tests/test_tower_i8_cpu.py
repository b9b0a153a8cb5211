"""The int8 tower's numpy specification (alphafive_amd/tower_i8.py) on its own, the conditions the GPU cases of
tests/tower_i8_cases.py must meet, and the Python surface's refusals.  No GPU."""
import numpy as np
import pytest

import tower_i8_cases as gen
from alphafive_amd import tower_i8 as t8
from oracle import tower_fp64 as ref64

W, S = 128, 11


def _slow_accumulate(xq, q3, xq2=None, qp=None):
    """The integer convolution written out: int64 sums, one output pixel and tap at a time, the zero padding by bounds checks."""
    B = xq.shape[0]
    x, w = xq.astype(np.int64), q3.astype(np.int64)
    acc = np.zeros((B, W, S, S), np.int64)
    for y in range(S):
        for xx in range(S):
            for ky in range(3):
                for kx in range(3):
                    yy, xs = y + ky - 1, xx + kx - 1
                    if 0 <= yy < S and 0 <= xs < S:
                        acc[:, :, y, xx] += x[:, :, yy, xs] @ w[:, :, ky, kx].T
            if qp is not None:
                acc[:, :, y, xx] += xq2[:, :, y, xx].astype(np.int64) @ qp.astype(np.int64).T
    return acc


@pytest.mark.parametrize("name", ["conv1", "both"])
def test_conv_reference_agrees_with_a_direct_integer_convolution(name):
    c = gen.layer_case(name)
    a = c["scales"]
    r = t8.reciprocal(a)
    qw = t8.quantize_weights(c["c1"], c["c2"], c["res"], a[0], a[1])
    hq, gq = c["hq"][:2], c["gq"][:2]
    if c["second"]:
        acc = _slow_accumulate(gq, qw["q2"], hq, qw["qp"])
        m, b, r_out = qw["m2"], qw["b2"], r[2]
        out, t64, pre = t8.conv_reference(gq, qw["q2"], m, b, r_out, hq, qw["qp"])
    else:
        acc = _slow_accumulate(hq, qw["q1"])
        m, b, r_out = qw["m1"], qw["b1"], r[1]
        out, t64, pre = t8.conv_reference(hq, qw["q1"], m, b, r_out)
    assert np.abs(acc).max() < 2 ** 24 and np.abs(acc).max() > 2 ** 12
    # the epilogue again, element by element in Python floats (fp64 holds acc * m exactly; math.fma is not assumed)
    from fractions import Fraction
    idx = np.random.default_rng(0).integers(0, acc.size, size=400)
    for i in idx:
        p, ch, y, x = np.unravel_index(i, acc.shape)
        exact = Fraction(int(acc[p, ch, y, x])) * Fraction(float(m[ch])) + Fraction(float(b[ch]))
        lo = np.float32(float(exact))
        cand = [np.nextafter(lo, np.float32(-np.inf)), lo, np.nextafter(lo, np.float32(np.inf))]
        best = min(cand, key=lambda v: abs(Fraction(float(v)) - exact))
        assert best == pre[p, ch, y, x]
    y32 = np.where(pre >= 0, pre, np.expm1(np.minimum(pre.astype(np.float64), 0)).astype(np.float32)).astype(np.float32)
    want = np.clip(np.rint(y32 * np.float32(r_out)), -127, 127).astype(np.int8)
    assert np.array_equal(out, want)
    # and the accumulator itself, through the one place the module exposes it
    acc_mod = t8._accumulate(gq, qw["q2"]) if c["second"] else t8._accumulate(hq, qw["q1"])
    if c["second"]:
        acc_mod = acc_mod + (hq.astype(np.float64).transpose(0, 2, 3, 1).reshape(-1, W) @ qw["qp"].astype(np.float64).T).reshape(2, S, S, W).transpose(0, 3, 1, 2)
    assert np.array_equal(acc_mod, acc.astype(np.float64))


def test_forward_reference_against_fp64():
    """forward_reference against oracle.tower_fp64 on a 2-block random net, 16 positions, calibrated on the same data: the
    dequantised error of the block output (bf16 values against fp64).  Measured here: max |error| 0.0935, mean |error| 0.01204,
    on outputs of absmax 4.16 and mean |value| 0.520; asserted at twice those: 0.187 and 0.0241."""
    tc = gen.tower_case(2, n=16)
    h, trace = t8.forward_reference(tc["x"], tc["blocks"], tc["scales"])
    err = np.abs(h.astype(np.float64) - tc["out64"])
    print("int8 forward_reference against fp64: max |error| %.4g, mean |error| %.4g (outputs: absmax %.3g, mean |value| %.3g)"
          % (err.max(), err.mean(), np.abs(tc["out64"]).max(), np.abs(tc["out64"]).mean()))
    assert err.max() <= 0.187 and err.mean() <= 0.0241
    assert len(trace) == 2 and trace[0]["h"].dtype == np.int8 and trace[1]["g"].shape == tc["x"].shape
    assert np.array_equal(ref64.bf16_round(h), h)                     # the output is bf16-valued


@pytest.mark.parametrize("name", gen.CASES)
def test_case_generators_meet_their_conditions(name):
    gen.check_layer_generator(name)


def test_fragment_map_and_c16_are_bijections():
    rng = np.random.default_rng(1)
    q3 = np.arange(W * W * 9, dtype=np.int64).reshape(W, W, 3, 3)
    qp = -1 - np.arange(W * W, dtype=np.int64).reshape(W, W)
    # (pack_fragments stores int8: run it on each byte of the index separately)
    seen = np.zeros((2, 80, 64, 16), np.int64)
    for k in range(3):
        f = t8.pack_fragments(((q3 >> (8 * k)) & 255).astype(np.uint8).view(np.int8), ((qp >> (8 * k)) & 255).astype(np.uint8).view(np.int8))
        seen |= f.astype(np.int64) << (8 * k)
    seen = np.where(seen >= 1 << 23, seen - (1 << 24), seen)
    assert sorted(seen.reshape(-1).tolist()) == sorted(q3.reshape(-1).tolist() + qp.reshape(-1).tolist())
    assert t8.pack_fragments(q3.astype(np.int8)).shape == (2, 72, 64, 16)
    x = rng.integers(-127, 128, size=(3, W, S, S)).astype(np.int8)
    c = t8.to_c16(x)
    assert c.shape == (3, 8, 144, 16) and not c[:, :, :S].any() and not c[:, :, S + S * S:].any()
    assert np.array_equal(t8.from_c16(c), x)
    assert c[1, 2, S * (4 + 1) + 7, 5] == x[1, 16 * 2 + 5, 4, 7]


def test_quantizers_edge_cases():
    r = np.float32(2.0)
    x = np.array([0.25, 0.75, 1.25, -0.25, -0.75, 63.5, 100.0, -100.0, 63.25, -63.75], np.float32)     # ties go to even; saturation
    assert t8.quantize_activation(x, r).tolist() == [0, 2, 2, 0, -2, 127, 127, -127, 126, -127]
    qw = t8.quantize_weights(*[(w, np.zeros(W, np.float32)) for w in (np.zeros((W, W, 3, 3), np.float32),) * 2], (np.zeros((W, W, 1, 1), np.float32), np.ones(W, np.float32)), 0.5, 0.25)
    assert (qw["s1"] == 1).all() and not qw["q1"].any() and (qw["m1"] == 0.5).all() and (qw["m2"] == 0.25).all() and (qw["b2"] == 1).all()
    with pytest.raises(ValueError):
        t8.check_scales([1.0, 2.0, 3.0], 2)
    with pytest.raises(ValueError):
        t8.check_scales([1.0, 0.0, 3.0, 1.0], 2)
    with pytest.raises(ValueError):
        t8.check_scales([1.0, np.inf, 3.0, 1.0], 2)


# ------------------------------------------------------------------ Python surface ------------------------------------------------------------------
def _cpu_net(S, blocks=2):
    import torch
    from alphafive_amd.network_deep import DeepResNet
    return DeepResNet(S, blocks=blocks, device="cpu", dtype=torch.bfloat16, seed=0)


def _planes(n, S, seed=3):
    rng = np.random.default_rng(seed)
    x = np.zeros((n, 3, S, S), np.float32)
    stones = rng.integers(0, 3, size=(n, S, S))
    x[:, 0], x[:, 1] = stones == 1, stones == 2
    x[:, 2] = rng.integers(0, 2, size=(n, 1, 1))
    return x


def test_calibrate_int8_returns_positive_scales_deterministically():
    net = _cpu_net(11, blocks=3)
    x = _planes(6, 11)
    a = net.calibrate_int8(x)
    assert a.dtype == np.float32 and a.shape == (6,) and np.isfinite(a).all() and (a > 0).all()
    assert np.array_equal(a, net.calibrate_int8(x))
    assert np.allclose(net.calibrate_int8(x, margin=1.5), a * 1.5, rtol=1e-6)
    t8.check_scales(a, 3)


def test_int8_is_refused_where_it_does_not_exist():
    with pytest.raises(ValueError, match="11x11"):
        _cpu_net(15).select_backend("hip", 8, precision="int8", act_scales=np.ones(4, np.float32))
    with pytest.raises(ValueError, match="unknown precision"):
        _cpu_net(11).select_backend("hip", 8, precision="fp8")
    with pytest.raises(ValueError, match="act_scales"):
        _cpu_net(11).evaluator(8, precision="int8")
    with pytest.raises(ValueError, match="2 \\* blocks"):
        _cpu_net(11).evaluator(8, precision="int8", act_scales=np.ones(3, np.float32))
