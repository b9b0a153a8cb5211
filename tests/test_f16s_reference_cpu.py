"""No GPU: the generators of tests/net_cases.py, as tests/test_gpu_f16s_exact.py uses them, checked from oracle/net_fp64.py and a
numpy model of the fp16 split alone — the conditions under which the split-operand kernels must reproduce fp64 bit for bit hold
for every exact case, the envelope cases sit in the binades they claim, the shipped checkpoint keeps its headroom below fp16's maximum, and the exact comparison is sharp:
a swapped weight row, a row-end neighbour that is not zeroed and a dropped lo half each change a compared value."""
import numpy as np
import pytest

import net_cases as gen
import test_gpu_f16s_exact as f16s
from oracle import net_fp64


def _gran(a):
    """smallest q with a * 2^q integral everywhere"""
    a = np.asarray(a, np.float64)
    for q in range(0, 40):
        s = a * 2.0 ** q
        if (s == np.round(s)).all():
            return q
    raise AssertionError("not a dyadic fraction of 40 bits")


def _integral(a, q):
    s = np.asarray(a, np.float64) * 2.0 ** q
    return bool((s == np.round(s)).all())


def test_intermediates_end_in_the_bits_of_forward():
    with np.load(f16s.W6960) as z:
        v = {k: z[k] for k in z.files}
    x = gen.board_positions(11, 6, seed=1)
    p, val = net_fp64.forward(v, x)
    for sums in (False, True):
        out = net_fp64.intermediates(v, x, sums=sums)
        assert (out["prob"].view(np.uint64) == p.view(np.uint64)).all() and (out["value"].view(np.uint64) == val.view(np.uint64)).all()
        assert [k for k in net_fp64.INTERMEDIATES if k not in out] == []
    assert out["f0"].shape == (6, 32, 11, 11) and out["o2"].shape == (6, 128, 11, 11) and out["vconv"].shape == (6, 4, 11, 11)
    assert out["pconv"].shape == (6, 16, 11, 11) and out["logits"].shape == (6, 121) and out["vpre"].shape == (6,)
    assert np.allclose(np.tanh(out["vpre"] / 2), val, rtol=0, atol=1e-15)
    # A and n of a block output cover conv2, the projection and both biases
    assert out["n:o1"] == 9 * 64 + 1 + 32 + 1 and out["n:f0"] == 76 and (out["A:o1"] >= np.abs(out["pre:o1"])).all()
    # the device's names are a subset of the reference's
    from alphafive_amd.net_hip import HipNet
    assert set(HipNet.ACTIVATIONS) <= set(net_fp64.INTERMEDIATES) and set(HipNet.ACTIVATIONS) <= set(gen.STORED)


def test_pick_scale_restatement():
    for mx, want in ((1.0, 4096.0), (1.0 + 2.0 ** -13, 4096.0), (3.0, 2048.0), (0.99, 8192.0), (0.0, 1.0), (np.inf, 1.0), (4096.0, 1.0), (8191.0, 1.0)):
        assert f16s.pick_scale(mx) == want
        if 0 < mx < np.inf:
            assert 4096.0 <= mx * f16s.pick_scale(mx) < 8192.0


@pytest.mark.parametrize("S", [11, 15])
def test_site_planes_cover_every_site_of_every_layer_exactly_once(S):
    n = S * S
    planes = gen.site_planes(S)
    assert planes.shape == (n, 3, S, S) and set(np.unique(planes)) == {0.0, 1.0}
    out = net_fp64.intermediates(gen.base_variables(S), planes, flat=True)
    for key in gen.STORED[:-2]:                       # the input of every convolution
        a = out[key].reshape(n, -1, n)
        hits = (a != 0).sum(axis=0)                   # [C, pixel]
        assert (hits == 1).all(), key
        assert set(np.unique(a)) <= {0.0, 1.0, 2.0, 3.0}
        assert len(np.unique(a.max(axis=(0, 2)))) == 3, key      # the values are keyed to the channel
        if S == 15:                                   # both halves of the board, both sides of the seam at pixel 128 and its whole row
            assert (hits[:, :128] == 1).all() and (hits[:, 128:] == 1).all() and (hits[:, 120:135] == 1).all()
    # neighbouring channels of a 32-slab, of the two halves of a k-step and of the slabs see different planes or values somewhere
    f = out["o2"].reshape(n, 128, n)
    for d in (1, 8, 16, 32, 64):
        assert sum((f[:, c] != f[:, c + d]).any() for c in range(128 - d)) >= (128 - d) * 0.6, d


@pytest.mark.parametrize("S", [11, 15])
def test_stone_planes_hold_the_special_boards(S):
    x = gen.stone_planes(S, np.random.default_rng(0))
    m = S // 2
    assert x.shape == (S * S, 3, S, S) and set(np.unique(x)) == {0.0, 1.0} and x[0].all() and not x[1].any()
    singles = x[2:29]
    assert (singles.sum(axis=(1, 2, 3)) == 1).all()
    for (yy, xx) in ((0, 0), (0, S - 1), (S - 1, 0), (S - 1, S - 1), (0, m), (m, 0), (S - 1, m), (m, S - 1), (m, m)):
        assert (singles[:, :, yy, xx].sum(axis=0) == 1).all()
    # the bytes the function produced before it grew to max(S*S, 32) positions for boards below 6x6 (sha256 of the float64 array)
    import hashlib
    assert hashlib.sha256(x.tobytes()).hexdigest() == {11: "8a3cb13d605e51fd85991330f03942892e3b4f53e98489166d0990da03edd63f",
                                                       15: "8e576f0b21765ad3a4b824cf76aaafd2613937472ad6da6d16bc6fc31079a314"}[S]


def _check_exact_case(S, target, cls):
    v, planes, key = gen.exact_variables(S, target, cls)
    out = net_fp64.intermediates(v, planes, sums=True, flat=True)
    q = gen.Q[cls]
    kname, bnames, key2, producer = gen.target_names(target)
    assert key == key2
    # every weight, after its group's scale, is hi + lo exactly
    wlo = {}
    scales = f16s.scale_groups(v)
    for name, s in scales.items():
        w32 = v[name].astype(np.float32)
        assert (w32 == v[name]).all(), name
        hi, lo = f16s.split16(w32 * np.float32(s))
        assert (hi + lo == v[name] * s).all(), name
        assert np.abs(hi).max() < 8192.0
        wlo[name] = bool((lo != 0).any())
    for name, a in v.items():
        assert (a.astype(np.float32) == a).all(), name
    bias = sum(v[b] for b in bnames)
    assert len(np.unique(bias)) == bias.size and (bias == np.round(bias)).all()          # distinct integers per cout
    # every stored activation is hi + lo exactly, in [0, 2048]; integers with lo = 0 in the integer class
    xlo = {"planes": False}
    assert set(np.unique(planes)) <= {0.0, 1.0}
    for k in gen.STORED:
        a = out[k]
        a32 = a.astype(np.float32)
        assert (a32 == a).all(), k
        hi, lo = f16s.split16(a32)
        assert (hi + lo == a).all(), k
        assert a.min() >= 0.0 and a.max() <= 2048.0, (k, a.min(), a.max())
        if cls == "int":
            assert (lo == 0).all() and (a == np.round(a)).all(), k
        xlo[k] = bool((lo != 0).any())
    # W_lo X_lo is zero everywhere; every product is a multiple of 2^-q and the absolute-term sums stay below 2^(24 - q)
    for okey, conv, proj, src, src2 in gen.LAYERS:
        for cname, skey in ((conv, src), (proj, src2)):
            if cname is None:
                continue
            assert not (wlo[cname + "/kernel"] and xlo[skey]), (okey, cname)
            x = planes if skey == "planes" else out[skey]
            qw = _gran(v[cname + "/kernel"])
            assert qw <= q and _integral(x, q - qw) and _gran(v[cname + "/bias"]) <= q, (okey, cname)
        assert out["A:" + okey].max() < 2.0 ** (24 - q), okey
        assert (out["pre:" + okey] >= 0).all(), okey             # the ELU is the identity on every stored value
    # the class exercises what it claims
    src = {lay[0]: (lay[3], lay[4]) for lay in gen.LAYERS}[key]
    tin = src[1] if target.endswith("proj") else src[0]
    if cls == "wsplit":
        assert wlo[kname] and not xlo[tin] and _integral(out["pre:" + key], 13) and not _integral(out["pre:" + key], 12)
    if cls == "xsplit":
        assert xlo[tin] and not wlo[kname] and _integral(out["pre:" + key], 12) and not _integral(out["pre:" + key], 11)
        assert (f16s.split16(out[tin].astype(np.float32))[1] != 0).all()                  # a lo half at every site
    if target not in ("stem", "vconv", "pconv"):
        assert (v[kname] != 0).any(axis=(0, 1, 3)).all() and (v[kname] != 0).any(axis=(2, 3)).all()      # every cin, every tap
    return v, planes, key, out, tin


@pytest.mark.parametrize("target,cls", gen.CASES)
def test_exact_generators_meet_the_exactness_conditions_11(target, cls):
    v, planes, key, out, tin = _check_exact_case(11, target, cls)
    # ---- sensitivity: the reference perturbed the way a kernel bug would changes a compared value of the target's output ----
    kname = gen.target_names(target)[0]
    k = v[kname]
    x = planes if tin == "planes" else out[tin]
    zero = np.zeros(k.shape[-1])
    good = net_fp64._conv2d_flat(x, k, zero)
    # one tap's weight row swapped with its neighbour's
    ty, tx, ci = next((a, b, c) for a in range(k.shape[0]) for b in range(k.shape[1]) for c in range(k.shape[2] - 1) if (k[a, b, c] != k[a, b, c + 1]).any())
    k2 = k.copy()
    k2[ty, tx, [ci, ci + 1]] = k[ty, tx, [ci + 1, ci]]
    assert (net_fp64._conv2d_flat(x, k2, zero) != good).any()
    # one row-end neighbour not zeroed: the right-hand tap of pixel (4, S-1) reads pixel (5, 0), its neighbour in memory
    if k.shape[0] == 3:
        leak = np.einsum("bc,cd->bd", x[:, :, 5, 0], k[1, 2])
        assert (leak != 0).any()
    # one lo half dropped
    if cls == "wsplit":
        s = f16s.scale_groups(v)[kname]
        assert (net_fp64._conv2d_flat(x, f16s.split16((k * s).astype(np.float32))[0] / s, zero) != good).any()
    if cls == "xsplit":
        assert (net_fp64._conv2d_flat(f16s.split16(x.astype(np.float32))[0], k, zero) != good).any()


@pytest.mark.parametrize("target,cls", gen.CASES)
def test_exact_generators_meet_the_exactness_conditions_15(target, cls):
    _check_exact_case(15, target, cls)


@pytest.mark.parametrize("S", [11, 15])
def test_dense_case_is_integral_and_small(S):
    v, planes, ref = gen.dense_case(S)
    logits, x = ref["logits"], ref["vpre"]
    assert (logits == np.round(logits)).all() and np.ptp(logits, axis=1).max() <= 8 and len(np.unique(logits)) >= 6
    assert (x == np.round(x)).all() and np.abs(x).max() <= 8 and len(np.unique(x)) >= 4
    for k in ("vconv", "pconv", "fc1"):
        assert (ref[k] == np.round(ref[k])).all() and ref[k].min() >= 0 and ref[k].max() <= 2048
    # each logit reads one head-convolution value of its own pixel
    n = S * S
    j = np.arange(n)
    assert (logits == ref["pconv"].reshape(-1, 16, n)[:, j % 16, j] + j % 3).all()
    assert 4.0 * (n + 16) * 2.0 ** -24 < 1e-2 and 16.0 * 2.0 ** -24 / (1.0 - np.tanh(4.0) ** 2) < 1e-2


def test_rounded_weights_span_twelve_binades_and_both_signs():
    v = gen.rounded_variables(11, seed=61)
    k = np.abs(v["bone/block2_conv1/kernel"])
    assert k.max() / k[k > 0].min() >= 2.0 ** 12
    assert max(np.abs(v[n]).max() for n in v if n.endswith("bias")) > 1.0
    out = net_fp64.intermediates(v, gen.board_positions(11, 8, seed=3), sums=True)
    for key in ("f0", "g1", "o1", "g2", "o2", "g3", "o3", "g4", "o4", "g5", "o5", "vconv", "pconv"):
        pre = out["pre:" + key]
        assert (pre > 0).mean() > 0.01 and (pre < 0).mean() > 0.01, key
        assert np.abs(out[key]).max() < 65504.0


@pytest.mark.parametrize("side,where", f16s.ENVELOPE)
def test_envelope_cases_lie_in_the_binades_they_claim(side, where):
    v, x, key = f16s.envelope_variables(side, where)
    out = net_fp64.intermediates(v, x)
    top = np.abs(out[key]).max()
    if side == "large":
        assert 2.0 ** 15 <= top < 65504.0
    else:
        assert 0.0 < top < 2.0 ** -14
    for k in gen.STORED:                              # nothing anywhere leaves the stated range
        assert np.abs(out[k]).max() < 65504.0, k


def test_shipped_checkpoint_keeps_its_headroom():
    """Largest |activation| per stage of the shipped checkpoint on the 64 positions of board_positions(11, 64, seed=0): 174x below
    fp16's maximum.  A retrained fixture that fails this is a finding, not a tolerance to widen."""
    with np.load(f16s.W6960) as z:
        v = {k: z[k] for k in z.files}
    out = net_fp64.intermediates(v, gen.board_positions(11, 64, seed=0))
    stage = {"stem": ("f0",), "bone/block1": ("g1", "o1"), "bone/block2": ("g2", "o2"), "value/block3": ("g3", "o3"),
             "policy/block4": ("g4", "o4"), "policy/block5": ("g5", "o5"), "heads": ("vconv", "pconv")}
    top = {s: max(np.abs(out[k]).max() for k in keys) for s, keys in stage.items()}
    print(top)
    for s, want in (("stem", 2.3), ("bone/block1", 20.5), ("bone/block2", 144.0), ("value/block3", 230.0), ("policy/block4", 376.0)):
        assert abs(top[s] - want) <= 0.005 * want + 0.05, (s, top[s])
    for s, t in top.items():
        assert t < 2.0 ** 13, (s, t)                  # the factor of 8 below fp16's maximum that pick_scale keeps for the weights
