"""Cases for the policy / value network's forward kernels against oracle/net_fp64.py, one layer at a time, generic in the board size
S (3..16): the generators of the exact, dense and rounded regimes, and a numpy fp32 model of the fp32 Winograd path's arithmetic
(csrc/af_net.hip) with that path's comparisons.  Plain numpy, no GPU.  tests/test_gpu_f16s_exact.py (fp16 split-operand path, 11x11
and 15x15) and tests/test_gpu_wino_exact.py (fp32 Winograd path, every size) run the kernels on these cases;
tests/test_f16s_reference_cpu.py and tests/test_wino_reference_cpu.py check the generators, the model and the comparisons from the
reference alone.  The regimes are described in the docstrings of the two GPU modules.
"""
import functools
import zlib

import numpy as np

from oracle import net_fp64

# (name, cin, cout, key of the block's input)
BLOCKS = (("bone/block1", 32, 64, "f0"), ("bone/block2", 64, 128, "o1"), ("value/block3", 128, 32, "o2"),
          ("policy/block4", 128, 64, "o2"), ("policy/block5", 64, 32, "o4"))
STORED = ("f0", "g1", "o1", "g2", "o2", "g3", "o3", "g4", "o4", "g5", "o5", "vconv", "pconv")      # every activation the kernels split
PLANES = STORED[:11]                             # the fp32 path's planes, in af_net_debug_activation's order (which = 16 + i, 32 + i)
TARGETS = ("stem",) + tuple("b%d.%s" % (k, part) for k in range(1, 6) for part in ("conv1", "conv2", "proj")) + ("vconv", "pconv")
CLASSES = ("int", "wsplit", "xsplit")
CASES = tuple((t, c) for t in TARGETS for c in CLASSES if not (t == "stem" and c == "xsplit"))     # (the stem's input is the planes)
Q = {"int": 0, "wsplit": 13, "xsplit": 12}      # every product of a case is a multiple of 2^-Q
# the convolutions in graph order: (output key, variable prefix, projection prefix joined to the sum, input key, projection's input key)
LAYERS = (("f0", "bone/conv1", None, "planes", None),) + tuple(
    lay for k, (name, _, _, src) in enumerate(BLOCKS, 1)
    for lay in (("g%d" % k, name + "_conv1", None, src, None), ("o%d" % k, name + "_conv2", name + "_res", "g%d" % k, src))
) + (("vconv", "value/conv", None, "o3", None), ("pconv", "policy/conv", None, "o5", None))


# ------------------------------------------------------------------ generators ------------------------------------------------------------------
def _sel3(cin, cout):
    k = np.zeros((3, 3, cin, cout))
    c = np.arange(cout)
    k[1, 1, c if cout <= cin else (c + 5 * (c // cin)) % cin, c] = 1.0
    return k


def base_variables(S):
    """All 42 variables (float64, TF layout) of the selector network: nothing but copies of the planes, dense layers zero."""
    n = S * S
    v = {"bone/conv1/kernel": np.zeros((5, 5, 3, 32)), "bone/conv1/bias": np.zeros(32)}
    c = np.arange(32)
    v["bone/conv1/kernel"][2, 2, c % 3, c] = 1.0 + (c // 3) % 3
    for name, cin, cout, _ in BLOCKS:
        v[name + "_conv1/kernel"], v[name + "_conv1/bias"] = _sel3(cin, cout), np.zeros(cout)
        v[name + "_conv2/kernel"], v[name + "_conv2/bias"] = _sel3(cout, cout), np.zeros(cout)
        v[name + "_res/kernel"], v[name + "_res/bias"] = np.zeros((1, 1, cin, cout)), np.zeros(cout)
    for head, nc in (("value", 4), ("policy", 16)):
        v[head + "/conv/kernel"], v[head + "/conv/bias"] = np.zeros((1, 1, 32, nc)), np.zeros(nc)
        v[head + "/conv/kernel"][0, 0, np.arange(nc), np.arange(nc)] = 1.0
    v["value/fc1/kernel"], v["value/fc1/bias"] = np.zeros((4 * n, 64)), np.zeros(64)
    v["value/fc2/kernel"], v["value/fc2/bias"] = np.zeros((64, 1)), np.zeros(1)
    v["policy/fc/kernel"], v["policy/fc/bias"] = np.zeros((16 * n, n)), np.zeros(n)
    return v


def fold_head(v, head):
    """The value / policy head convolution as a fold of all 32 channels of o3 / o5 (which the split-operand path never stores);
    exact_variables sets its bias."""
    nc = 4 if head == "value" else 16
    k = np.zeros((1, 1, 32, nc))
    for ci in range(32):
        k[0, 0, ci, ci % nc] = (-1.0) ** (ci // nc)
    v[head + "/conv/kernel"], v[head + "/conv/bias"] = k, np.zeros(nc)


def site_planes(S):
    """[S*S, 3, S, S] of 0 / 1: position b holds one stone per plane p, at pixel (37 p + b) mod S*S."""
    n = S * S
    x = np.zeros((n, 3, n))
    for p in range(3):
        x[np.arange(n), p, (37 * p + np.arange(n)) % n] = 1.0
    return x.reshape(n, 3, S, S)


def stone_planes(S, rng):
    """[max(S*S, 32), 3, S, S] of 0 / 1: a full board, an empty one, single stones in every plane at the four corners, the four edge
    midpoints and the centre (29 positions, so boards below 6x6 get 32), then random fill of rising density."""
    n, m = max(S * S, 32), S // 2
    x = np.zeros((n, 3, S, S))
    x[0] = 1.0
    k = 2
    for (yy, xx) in ((0, 0), (0, S - 1), (S - 1, 0), (S - 1, S - 1), (0, m), (m, 0), (S - 1, m), (m, S - 1), (m, m)):
        for c in range(3):
            x[k, c, yy, xx] = 1.0
            k += 1
    for b in range(k, n):
        x[b] = rng.random((3, S, S)) < (0.1 + 0.8 * (b - k) / (n - k))
    return x


def target_names(target):
    """-> (kernel variable, bias variables that sum to its bias, output key, the variable whose bias produces its input)."""
    if target == "stem":
        return "bone/conv1/kernel", ("bone/conv1/bias",), "f0", None
    producer = {"f0": "bone/conv1/bias", "o1": "bone/block1_conv2/bias", "o2": "bone/block2_conv2/bias", "o4": "policy/block4_conv2/bias"}
    if target in ("vconv", "pconv"):
        head, blk = ("value", "value/block3") if target == "vconv" else ("policy", "policy/block5")
        return head + "/conv/kernel", (head + "/conv/bias",), target, blk + "_conv2/bias"
    k, part = int(target[1]), target[3:]
    name, _, _, src = BLOCKS[k - 1]
    if part == "conv1":
        return name + "_conv1/kernel", (name + "_conv1/bias",), "g%d" % k, producer[src]
    if part == "conv2":
        return name + "_conv2/kernel", (name + "_conv2/bias", name + "_res/bias"), "o%d" % k, name + "_conv1/bias"
    return name + "_res/kernel", (name + "_conv2/bias", name + "_res/bias"), "o%d" % k, producer[src]


@functools.lru_cache(maxsize=4)
def exact_variables(S, target, cls):
    """-> (variables, planes [N, 3, S, S], output key of the target) of one exact case; N = S*S, the stem's max(S*S, 32)."""
    rng = np.random.default_rng(zlib.crc32(("%d %s %s" % (S, target, cls)).encode()))
    v = base_variables(S)
    planes = stone_planes(S, rng) if target == "stem" else site_planes(S)
    kname, bnames, key, producer = target_names(target)
    folded = target[0] == "b" and target[1] in "35"
    if folded:
        fold_head(v, "value" if target[1] == "3" else "policy")
    if target.endswith("proj"):
        v[kname.replace("_res/", "_conv2/")][:] = 0.0
    if cls == "xsplit":
        nb = v[producer].shape[0]
        v[producer] = 1.0 + (1.0 + np.arange(nb) % 3) * 2.0 ** -12
    shape = v[kname].shape
    w = rng.integers(-1, 2, size=shape) * (rng.random(shape) < 0.75)
    if cls == "wsplit":
        w = w * (1.0 + 2.0 ** -13 * rng.integers(0, 2, size=shape))
    v[kname] = w.astype(np.float64)
    # integer biases, distinct per cout, above the most negative sum of the case: every stored activation stays on the ELU's x >= 0 side
    pre = net_fp64.intermediates(v, planes, flat=True)["pre:" + key]
    cout = shape[-1]
    total = np.ceil(max(0.0, -pre.min())) + 1.0 + rng.permutation(cout)
    if folded:                                                   # the fold's bias keeps the head convolution on the x >= 0 side as well
        head = "value" if target[1] == "3" else "policy"
        o = pre + total[None, :, None, None]                     # = o3 / o5: everything behind the target is a selector
        fold = np.einsum("bchw,cd->bdhw", o, v[head + "/conv/kernel"][0, 0])
        v[head + "/conv/bias"] = np.full(fold.shape[1], np.ceil(max(0.0, -fold.min())) + 1.0)
    if len(bnames) == 2:                                         # the kernels see only conv2 bias + projection bias
        v[bnames[1]] = 1.0 + rng.permutation(cout) % 7
        total = total - v[bnames[1]]
    v[bnames[0]] = v[bnames[0]] + total
    return v, planes, key


@functools.lru_cache(maxsize=2)
def exact_reference(S, target, cls):
    """-> {key: float32 [N, C, S*S]} of every stored activation of the case's N positions; the conversion from fp64 is checked to be
    exact."""
    v, planes, _ = exact_variables(S, target, cls)
    ref = net_fp64.intermediates(v, planes, flat=True)
    out = {}
    for key in STORED:
        a32 = ref[key].astype(np.float32)
        assert (a32.astype(np.float64) == ref[key]).all(), key
        out[key] = a32.reshape(a32.shape[0], a32.shape[1], -1)
    return out


DENSE_KEYS = ("vconv", "pconv", "fc1", "vpre", "logits", "prob", "value")


@functools.lru_cache(maxsize=2)
def dense_case(S):
    """Selector dense layers on 0 / 1 boards: logit j = pconv[j mod 16, pixel j] + (j mod 3) with pconv[c] = 1 + 2 o5[c] in {1, 3, 5, 7};
    x = sum of eight vconv values, four with weight +1 and four with -1 (vconv[c] = o3[c] in {0, 1, 2}): an integer in [-8, 8].
    -> (variables, planes [64, 3, S, S], the reference's DENSE_KEYS)."""
    n = S * S
    rng = np.random.default_rng(40 + S)
    v = base_variables(S)
    v["policy/conv/kernel"] *= 2.0
    v["policy/conv/bias"] += 1.0
    j = np.arange(n)
    v["policy/fc/kernel"][(j % 16) * n + j, j] = 1.0
    v["policy/fc/bias"] = (j % 3).astype(np.float64)
    pix = rng.permutation(n)[:8]
    for i in range(8):
        v["value/fc1/kernel"][(i % 4) * n + pix[i], i] = 1.0
        v["value/fc2/kernel"][i, 0] = 1.0 if i < 4 else -1.0
    planes = (rng.random((64, 3, S, S)) < 0.5).astype(np.float64)
    ref = net_fp64.intermediates(v, planes)
    return v, planes, {k: ref[k] for k in DENSE_KEYS}


def dense_check(tag, S, p, val, logits, x):
    """The dense layers' comparison of both paths: log p_j - log p_0 and 2 atanh(v) against the integer logits / x of dense_case
    (derivation of the tolerances: docstring of tests/test_gpu_f16s_exact.py)."""
    p, val = np.asarray(p, np.float64), np.asarray(val, np.float64)
    n = S * S
    assert (logits == np.round(logits)).all() and (x == np.round(x)).all() and np.abs(x).max() <= 8 and np.ptp(logits, axis=1).max() <= 8
    tol_p = 4.0 * (n + 16) * 2.0 ** -24
    dl = np.abs((np.log(p) - np.log(p[:, :1])) - (logits - logits[:, :1]))
    tol_v = 16.0 * 2.0 ** -24 / (1.0 - np.tanh(x / 2.0) ** 2)
    dx = np.abs(2.0 * np.arctanh(val) - x)
    print("%s: |d log-ratio| max %.3g (tolerance %.3g), |d 2 atanh v| / tolerance max %.3g" % (tag, dl.max(), tol_p, (dx / tol_v).max()))
    assert tol_p < 1e-2 and tol_v.max() < 1e-2
    assert (dl <= tol_p).all()
    assert (dx <= tol_v).all()
    assert np.abs(p.sum(axis=1) - 1.0).max() < 1e-5


# ---- rounded regime ----
def rounded_variables(S, seed):
    """Glorot kernels, biases of order 1, and bone/block2 conv1's members spread over 2^12 in magnitude (float32 values)."""
    from alphafive_amd.network import random_variables
    rng = np.random.default_rng(seed)
    v = random_variables(S, seed=seed)
    for name in v:
        if name.endswith("bias"):
            v[name] = (0.75 * rng.standard_normal(v[name].shape)).astype(np.float32)
    k = v["bone/block2_conv1/kernel"]
    v["bone/block2_conv1/kernel"] = (k * 2.0 ** -rng.integers(0, 13, size=k.shape)).astype(np.float32)
    return v


def board_positions(S, B, seed=0):
    """The 0 / 1 boards of tests/test_gpu_net.py::_positions."""
    rng = np.random.RandomState(seed)
    x = np.zeros((B, 3, S, S), np.float32)
    for b in range(B):
        n = rng.randint(0, S * S - 1)
        cells = rng.permutation(S * S)[:n + 1]
        x[b, 0].reshape(-1)[cells[0:n:2]] = 1
        x[b, 1].reshape(-1)[cells[1:n:2]] = 1
        if b % 7:
            x[b, 2].reshape(-1)[cells[n]] = 1
    return x


# ------------------------------------------------------------------ the fp32 Winograd path: geometry, model, comparisons ------------------------------------------------------------------
def geometry(S):
    """-> (T, WP, PP) of af_net_create: 2x2 output tiles per board side, padded plane width, plane stride."""
    T = (S + 1) // 2
    WP = 2 * T + 2
    return T, WP, (WP * WP + 15) // 16 * 16


def wino_batches(S):
    """The exact regime's batches: 1; S*S = every site once; the first batch whose B T^2 tiles pass 1024, where wino_task's 8-way
    workgroup interleave starts its second round."""
    return (1, S * S, 1024 // geometry(S)[0] ** 2 + 1)


def to_stored(x, S):
    """[B, C, S, S] -> float32 [B, C, PP] in the kernels' plane layout: pixel (y, x) at (y + 1) WP + x + 1, zero elsewhere."""
    T, WP, PP = geometry(S)
    B, C = x.shape[:2]
    out = np.zeros((B, C, PP), np.float32)
    out[:, :, :WP * WP].reshape(B, C, WP, WP)[:, :, 1:S + 1, 1:S + 1] = x
    return out


def interior(stored, S):
    """float [B, C, PP] -> [B, C, S*S] (a copy)."""
    T, WP, PP = geometry(S)
    B, C = stored.shape[:2]
    return np.ascontiguousarray(stored[:, :, :WP * WP].reshape(B, C, WP, WP)[:, :, 1:S + 1, 1:S + 1]).reshape(B, C, S * S)


def outside_mask(S):
    """bool [PP]: True on everything that is not a board pixel — the border of the padded plane and the pad behind WP*WP."""
    T, WP, PP = geometry(S)
    m = np.ones(PP, bool)
    m[:WP * WP].reshape(WP, WP)[1:S + 1, 1:S + 1] = False
    return m


def bit_differences(got, want):
    """bool array: where two float32 arrays differ in their bits (so -0.0 differs from +0.0 and a NaN equals only itself)."""
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    assert got.shape == want.shape, (got.shape, want.shape)
    return got.view(np.uint32) != want.view(np.uint32)


def assert_same_bits(got, want, what):
    bad = bit_differences(got, want)
    if bad.any():
        at = tuple(np.argwhere(bad)[0])
        raise AssertionError("%s: %d of %d elements differ, first at %s: got %r, expected %r" % (
            what, int(bad.sum()), bad.size, at, np.asarray(got)[at], np.asarray(want)[at]))


def assert_border_zero(stored, S, what):
    """Every element of float32 [B, C, PP] outside the S x S interior is +0.0 by its bits."""
    out = np.ascontiguousarray(stored, np.float32).view(np.uint32)[:, :, outside_mask(S)]
    if out.any():
        b, c, i = np.argwhere(out != 0)[0]
        at = int(np.flatnonzero(outside_mask(S))[i])
        WP = geometry(S)[1]
        raise AssertionError("%s: %d border / pad elements are not +0.0, first at [b, c] = [%d, %d], plane offset %d (row %d, column %d)" % (
            what, int((out != 0).sum()), b, c, at, at // WP, at % WP))


# Winograd F(2x2, 3x3): Y = A^T [ (G g G^T) (.) (B^T d B) ] A
_G = np.array([[1, 0, 0], [0.5, 0.5, 0.5], [0.5, -0.5, 0.5], [0, 0, 1]], np.float64)
_BT = np.array([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]], np.float64)
_AT = np.array([[1, 1, 1, 0], [0, 1, -1, -1]], np.float64)
_CENTRE = (5, 6, 9, 10)                          # the (xi, nu) = {1, 2}^2 a centre-tap kernel occupies


def wino_u(kernel):
    """af_update_wino: U = fp32(G g G^T) of a HWIO kernel (3x3, or 1x1 = the centre tap of a 3x3), the sum over i then j in fp64 as
    written, -> float32 [16, cin, cout], index xi * 4 + nu."""
    k = np.asarray(kernel, np.float32).astype(np.float64)
    g = np.zeros((3, 3) + k.shape[2:])
    if k.shape[0] == 3:
        g[:] = k
    else:
        g[1, 1] = k[0, 0]
    u = np.zeros((16,) + k.shape[2:])
    for xi in range(4):
        for nu in range(4):
            for i in range(3):
                for j in range(3):
                    u[xi * 4 + nu] += _G[xi, i] * g[i, j] * _G[nu, j]
    return u.astype(np.float32)


def _patches(stored, S):
    """[B, C, PP] -> view [B, C, T, T, 4, 4]: tile (ty, tx) reads rows 2 ty .. 2 ty + 3, columns 2 tx .. 2 tx + 3 of the padded plane."""
    T, WP, PP = geometry(S)
    B, C = stored.shape[:2]
    p = stored[:, :, :WP * WP].reshape(B, C, WP, WP)
    return np.lib.stride_tricks.sliding_window_view(p, (4, 4), axis=(2, 3))[:, :, ::2, ::2]


def wino_v(stored, S):
    """The kernel's input transform V = B^T d B in two levels of fp32 adds -> float32 [B, C, T, T, 16] (xi * 4 + nu).  The
    projection's four values are positions 5, 6, 9, 10 of the same transform: compute_ph forms them with the same two additions."""
    d = _patches(np.asarray(stored, np.float32), S)
    r = [d[..., i, :] for i in range(4)]
    t = (r[0] - r[2], r[1] + r[2], r[2] - r[1], r[1] - r[3])                    # rows of B^T d: [.., 4 columns]
    v = [f(ti) for ti in t for f in (lambda a: a[..., 0] - a[..., 2], lambda a: a[..., 1] + a[..., 2],
                                     lambda a: a[..., 2] - a[..., 1], lambda a: a[..., 1] - a[..., 3])]
    return np.stack(v, axis=-1)


def _mfma_chain(M, V, U, order):
    """M[p, x, co] = fp32(M + U[x, c, co] V[c, p, x]) one cin at a time (the fp32 products are exact, as the MFMA's), c in `order`."""
    V64, U64 = V.astype(np.float64), U.astype(np.float64)
    acc, term = M.astype(np.float64), np.empty(M.shape, np.float64)
    for c in order:
        np.multiply(V64[c][:, :, None], U64[:, c, :][None], out=term)
        term += acc
        M[...] = term                            # the one rounding of the step
        acc[...] = M


def native_exp(x):
    """__expf of a float32 array as the hardware forms it: exp2 of the fp32 product x log2(e) (the exp2 itself correctly rounded)."""
    t = np.asarray(x, np.float32) * np.float32(1.4426950408889634)
    return np.exp2(t.astype(np.float64)).astype(np.float32)


def elu32(x):
    x = np.asarray(x, np.float32)
    return np.where(x > 0, x, native_exp(np.minimum(x, np.float32(0))) - np.float32(1)).astype(np.float32)


def wino_layer(S, src, u, bias, src2=None, u2=None, backwards=False, out=None, faults=()):
    """One af_conv_wino launch in numpy fp32.  src [B, cin, PP] stored planes, u = wino_u(3x3 kernel), bias float32 [cout];
    src2 / u2: the folded 1x1 projection's input planes and wino_u of its kernel.  cin is accumulated forwards (3x3 segment, then the
    projection's, as the kernel runs them) or, backwards=True, in the exact reverse.  -> stored planes [B, cout, PP]: `out`
    (which keeps whatever the tiles do not write) or fresh zeros.  faults: planted kernel faults for the tests of the comparisons —
    "tile_to_next_position" stores tile (0, 0) of position 0 into position 1."""
    T, WP, PP = geometry(S)
    B, cin = src.shape[:2]
    cout = u.shape[2]
    M = np.zeros((B * T * T, 16, cout), np.float32)
    V = np.ascontiguousarray(wino_v(src, S).transpose(1, 0, 2, 3, 4)).reshape(cin, B * T * T, 16)
    steps = [(M, V, u, range(cin))]
    if src2 is not None:
        cin2 = src2.shape[1]
        V2 = np.ascontiguousarray(wino_v(src2, S).transpose(1, 0, 2, 3, 4)).reshape(cin2, B * T * T, 16)[:, :, _CENTRE]
        steps.append((None, V2, u2[_CENTRE, :, :], range(cin2)))
    for _, Vs, Us, order in (steps[::-1] if backwards else steps):
        order = list(order)[::-1] if backwards else order
        if Vs.shape[2] == 16:
            _mfma_chain(M, Vs, Us, order)
        else:
            Mc = np.ascontiguousarray(M[:, _CENTRE, :])
            _mfma_chain(Mc, Vs, Us, order)
            M[:, _CENTRE, :] = Mc
    m = [M[:, x, :] for x in range(16)]
    s0 = [m[0 + j] + m[4 + j] + m[8 + j] for j in range(4)]
    s1 = [m[4 + j] - m[8 + j] - m[12 + j] for j in range(4)]
    b = np.asarray(bias, np.float32)[None, :]
    y = np.stack([elu32(s0[0] + s0[1] + s0[2] + b), elu32(s0[1] - s0[2] - s0[3] + b),
                  elu32(s1[0] + s1[1] + s1[2] + b), elu32(s1[1] - s1[2] - s1[3] + b)], axis=-1)     # [B T T, cout, 4]
    y = y.reshape(B, T, T, cout, 2, 2).transpose(0, 3, 1, 4, 2, 5).reshape(B, cout, 2 * T, 2 * T)
    if out is None:
        out = np.zeros((B, cout, PP), np.float32)
    o = out[:, :, :WP * WP].reshape(B, cout, WP, WP)
    o[:, :, 1:S + 1, 1:S + 1] = y[:, :, :S, :S]           # ok1y / ok1x: the last tile row / column of an odd board stores one pixel only
    if "tile_to_next_position" in faults:
        o[1, :, 1:3, 1:3] = y[0, :, 0:2, 0:2]
    return out


def stem_layer(S, planes, kernel, bias):
    """af_stem_conv in numpy: acc = bias, then fma(x, w, acc) over ky, kx, c in that order (each fma one rounding) -> stored [B, 32, PP]."""
    x = np.asarray(planes, np.float64)
    B = x.shape[0]
    k = np.asarray(kernel, np.float32).astype(np.float64)
    xp = np.zeros((B, 3, S + 4, S + 4))
    xp[:, :, 2:S + 2, 2:S + 2] = x
    acc = np.broadcast_to(np.asarray(bias, np.float32)[None, :, None, None], (B, 32, S, S)).astype(np.float32)
    for ky in range(5):
        for kx in range(5):
            for c in range(3):
                acc = (acc.astype(np.float64) + xp[:, c, None, ky:ky + S, kx:kx + S] * k[ky, kx, c][None, :, None, None]).astype(np.float32)
    return to_stored(elu32(acc), S)


def wino_weights(v):
    """The weight-derived tensors of the fp32 path as pack_from_device makes them: {conv prefix: U}, {output key: float32 bias}."""
    U, bias = {}, {}
    for key, conv, proj, _, _ in LAYERS[1:11]:
        U[conv] = wino_u(v[conv + "/kernel"])
        bias[key] = np.asarray(v[conv + "/bias"], np.float32)
        if proj is not None:
            U[proj] = wino_u(v[proj + "/kernel"])
            bias[key] = bias[key] + np.asarray(v[proj + "/bias"], np.float32)         # one fp32 addition (af_update_copy)
    return U, bias


def wino_forward(S, v, planes, backwards=False, U=None):
    """The fp32 path's eleven planes on `planes` [B, 3, S, S], every layer fed by the model's own previous one ->
    {key: float32 [B, C, PP]}.  U: replaces wino_weights' (planted faults)."""
    U0, bias = wino_weights(v)
    U = U0 if U is None else U
    out = {"planes": None, "f0": stem_layer(S, planes, v["bone/conv1/kernel"], v["bone/conv1/bias"])}
    for key, conv, proj, src, src2 in LAYERS[1:11]:
        out[key] = wino_layer(S, out[src], U[conv], bias[key], out[src2] if proj else None, U[proj] if proj else None, backwards)
    del out["planes"]
    return out


def wino_bounds(S, v, planes, got):
    """The rounded regime's comparison of the fp32 path (docstring of tests/test_gpu_wino_exact.py).  got: {key: float32 [B, C, PP]}
    read back as stored.  Every layer is recomputed in fp64, and by the fp32 model, from the input planes the kernel actually read.
    -> {key: (|got - ref|, bound, ref, |model - ref|)}, all [B, C, S*S]."""
    T, WP, PP = geometry(S)
    B = planes.shape[0]
    U, bias = wino_weights(v)
    report = {}
    x = np.asarray(planes, np.float64)
    k, b = np.asarray(v["bone/conv1/kernel"], np.float32).astype(np.float64), np.asarray(v["bone/conv1/bias"], np.float32).astype(np.float64)
    ref = net_fp64._elu(net_fp64._conv2d(x, k, b))
    A = net_fp64._conv2d(np.abs(x), np.abs(k), np.abs(b))
    n = 75
    model = stem_layer(S, planes, v["bone/conv1/kernel"], v["bone/conv1/bias"])
    for key, conv, proj, src, src2 in LAYERS[:11]:
        if key != "f0":
            ref = A = 0.0
            n = 0
            model = wino_layer(S, got[src], U[conv], bias[key], got[src2] if proj else None, U[proj] if proj else None)
            for cname, skey in ((conv, src), (proj, src2)):
                if cname is None:
                    continue
                xin = interior(got[skey], S).astype(np.float64).reshape(B, -1, S, S)
                k = np.asarray(v[cname + "/kernel"], np.float32).astype(np.float64)
                ref = ref + net_fp64._conv2d(xin, k, np.zeros(k.shape[-1]), same=k.shape[0] == 3)
                # A_w = |A^T| (sum_c |U| (.) |B^T| |d| |B|) |A|, on the stored planes (their borders are part of the patches)
                d = np.abs(_patches(got[skey].astype(np.float64), S))
                absV = np.einsum("xi,bctuij,nj->btuxnc", np.abs(_BT), d, np.abs(_BT), optimize=True).reshape(B, T, T, 16, -1)
                absM = np.einsum("btuxc,xco->btuxo", absV, np.abs(U[cname].astype(np.float64)), optimize=True).reshape(B, T, T, 4, 4, -1)
                Y = np.einsum("yx,btuxno,zn->botyuz", np.abs(_AT), absM, np.abs(_AT), optimize=True)
                A = A + Y.reshape(B, -1, 2 * T, 2 * T)[:, :, :S, :S]
                n += k.shape[2]
            b = bias[key].astype(np.float64)[None, :, None, None]
            ref, A = net_fp64._elu(ref + b), A + np.abs(b)
        bound = (2 * n + 8) * 2.0 ** -24 * A + 2.0 ** -22
        g = interior(got[key], S).astype(np.float64)
        sh = g.shape
        report[key] = (np.abs(g - ref.reshape(sh)), bound.reshape(sh), ref.reshape(sh), np.abs(interior(model, S).astype(np.float64) - ref.reshape(sh)))
    return report
