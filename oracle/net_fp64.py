"""fp64 numpy restatement of the reference network's forward pass (genData/network.py:52-97,
163-165) — the checker for "value within 1e-5 fp32".  TEST INFRASTRUCTURE ONLY.

PARITY UNPINNED against real TensorFlow: the arithmetic lives in TF 1.x (un-vendored, no
version pinned in the reference, not installable here) and the reference holds no stored
network outputs.  What is pinned: the checkpoint weights (ckpt/alphaFive-6960, read without TF)
and the graph definition restated here line by line: NCHW, HWIO kernels, SAME/VALID padding,
ELU(alpha=1), flatten in NCHW order, tanh(x/2), softmax.
"""
import numpy as np


def _elu(x):
    return np.where(x > 0, x, np.expm1(np.minimum(x, 0)))


def _conv2d(x, kernel, bias, same=True):
    """x [B,Cin,H,W] f64, kernel HWIO -> [B,Cout,H,W]; SAME zero padding (odd kernels) or VALID 1x1."""
    kh, kw, cin, cout = kernel.shape
    B, _, H, W = x.shape
    ph, pw = (kh // 2, kw // 2) if same else (0, 0)
    xp = np.zeros((B, H + 2 * ph, W + 2 * pw, cin), np.float64)       # NHWC: every tap is one fp64 matrix product
    xp[:, ph:ph + H, pw:pw + W, :] = x.transpose(0, 2, 3, 1)
    k64 = kernel.astype(np.float64)
    out = np.zeros((B, H, W, cout), np.float64)
    for a in range(kh):
        for b in range(kw):
            out += xp[:, a:a + H, b:b + W, :] @ k64[a, b]
    return out.transpose(0, 3, 1, 2) + bias.astype(np.float64)[None, :, None, None]


def _conv2d_flat(x, kernel, bias, same=True):
    """_conv2d as one GEMM per non-zero tap over all pixels of all positions (contiguous operands: an order of magnitude faster on
    hundreds of positions, and a selector kernel costs one tap).  The same sums in another order: equal to _conv2d bit for bit
    wherever every partial sum is exact (the exact regime of tests/test_gpu_f16s_exact.py), within fp64 rounding otherwise."""
    kh, kw, cin, cout = kernel.shape
    B, _, H, W = x.shape
    ph, pw = (kh // 2, kw // 2) if same else (0, 0)
    k64 = kernel.astype(np.float64)
    taps = [(a, b) for a in range(kh) for b in range(kw) if k64[a, b].any()]
    nhwc = np.ascontiguousarray(x.transpose(0, 2, 3, 1))
    out = np.zeros((B * H * W, cout), np.float64)
    if taps == [(ph, pw)]:                                            # a 1x1 kernel or a centre-tap selector: no padding needed
        out += nhwc.reshape(-1, cin) @ k64[ph, pw]
    elif taps:
        xp = np.zeros((B, H + 2 * ph, W + 2 * pw, cin), np.float64)
        xp[:, ph:ph + H, pw:pw + W, :] = nhwc
        for a, b in taps:
            out += np.ascontiguousarray(xp[:, a:a + H, b:b + W, :]).reshape(-1, cin) @ k64[a, b]
    out += bias.astype(np.float64)[None, :]
    return np.ascontiguousarray(out.reshape(B, H, W, cout).transpose(0, 3, 1, 2))


def _residual(f, v, name):                                        # network.py:52-56
    res = _conv2d(f, v[name + "_res/kernel"], v[name + "_res/bias"], same=False)
    g = _elu(_conv2d(f, v[name + "_conv1/kernel"], v[name + "_conv1/bias"]))
    g = _conv2d(g, v[name + "_conv2/kernel"], v[name + "_conv2/bias"])
    return _elu(res + g)


def forward(variables, inputs):
    """variables: {tf name: ndarray}; inputs [B,3,S,S] -> (prob [B,S*S], value [B]) in float64."""
    v = variables
    x = np.asarray(inputs, np.float64)
    B = x.shape[0]
    f = _elu(_conv2d(x, v["bone/conv1/kernel"], v["bone/conv1/bias"]))           # :63
    f = _residual(f, v, "bone/block1")                                          # :64
    f = _residual(f, v, "bone/block2")                                          # :65
    val = _residual(f, v, "value/block3")                                       # :68
    val = _elu(_conv2d(val, v["value/conv/kernel"], v["value/conv/bias"]))      # :70
    val = val.reshape(B, -1)                                                    # :71-72 (NCHW flatten)
    val = _elu(val @ v["value/fc1/kernel"].astype(np.float64) + v["value/fc1/bias"])   # :73
    val = np.tanh((val @ v["value/fc2/kernel"].astype(np.float64) + v["value/fc2/bias"]) / 2)[:, 0]   # :76,163
    pol = _residual(f, v, "policy/block4")                                      # :79
    pol = _residual(pol, v, "policy/block5")                                    # :80
    pol = _elu(_conv2d(pol, v["policy/conv/kernel"], v["policy/conv/bias"]))    # :82
    logits = pol.reshape(B, -1) @ v["policy/fc/kernel"].astype(np.float64) + v["policy/fc/bias"]   # :85
    logits = logits - logits.max(axis=1, keepdims=True)
    e = np.exp(logits)
    return e / e.sum(axis=1, keepdims=True), val                                # :88


# every stored tensor of the forward, in graph order; alphafive_amd.net_hip.HipNet.ACTIVATIONS reads the device's copy of the conv ones
INTERMEDIATES = ("f0", "g1", "o1", "g2", "o2", "g3", "o3", "g4", "o4", "g5", "o5", "vconv", "pconv", "fc1", "vpre", "logits")


def intermediates(variables, inputs, sums=False, flat=False):
    """Every intermediate of `forward` on inputs [B,3,S,S], in float64: {name: array}, names as in INTERMEDIATES — f0 the stem,
    g<k> / o<k> block k's conv1 output / block output (after their ELUs), vconv / pconv the head convolutions' outputs [B,4|16,S,S],
    fc1 [B,64], vpre the value before tanh(x/2) [B], logits [B,S*S] (before the max is subtracted) — plus "prob" and "value", computed
    by the statements of `forward` (the same bits).  sums=True adds, for each convolution output X, "A:X" = sum |w x| + |bias|
    per element (the absolute-term sum of its dot product, as oracle.tower_fp64.block returns A1 / A2) and "n:X" = its term count;
    "pre:X" = its value before the ELU is always there.  X also runs over res1..res5, the projections alone (pre:o<k>, A:o<k> and
    n:o<k> include them).  flat=True computes the convolutions with _conv2d_flat (exact cases: the same bits, much faster)."""
    v = variables
    x = np.asarray(inputs, np.float64)
    B = x.shape[0]
    out = {}
    c2d = _conv2d_flat if flat else _conv2d

    def conv(name, key, src, same=True, extra=None):
        """pre-activation of conv `name` on src (+ `extra` = (pre, A, n) of a second convolution that joins the sum)"""
        k, b = v[name + "/kernel"], v[name + "/bias"]
        part = pre = c2d(src, k, b, same=same)
        if extra is not None:
            pre = extra[0] + pre
        out["pre:" + key] = pre
        A = n = None
        if sums:
            # (non-negative operands — the selector layers of the exact regime: the absolute terms are the terms, the same sum)
            same_sum = (np.asarray(k) >= 0).all() and (np.asarray(b) >= 0).all() and (src >= 0).all()
            A = (part if same_sum else c2d(np.abs(src), np.abs(k), np.abs(b), same=same)) + (extra[1] if extra is not None else 0.0)
            n = int(np.prod(k.shape[:3])) + 1 + (extra[2] if extra is not None else 0)
            out["A:" + key], out["n:" + key] = A, n
        return pre, A, n

    def residual(f, name, k):                                     # the statements of _residual, its intermediates kept
        res = conv(name + "_res", "res%d" % k, f, same=False)
        g = out["g%d" % k] = _elu(conv(name + "_conv1", "g%d" % k, f)[0])
        o = out["o%d" % k] = _elu(conv(name + "_conv2", "o%d" % k, g, extra=res)[0])
        return o

    f = out["f0"] = _elu(conv("bone/conv1", "f0", x)[0])
    f = residual(f, "bone/block1", 1)
    f = residual(f, "bone/block2", 2)
    val = residual(f, "value/block3", 3)
    val = out["vconv"] = _elu(conv("value/conv", "vconv", val)[0])
    val = val.reshape(B, -1)
    val = out["fc1"] = _elu(val @ v["value/fc1/kernel"].astype(np.float64) + v["value/fc1/bias"])
    out["vpre"] = (val @ v["value/fc2/kernel"].astype(np.float64) + v["value/fc2/bias"])[:, 0]
    out["value"] = np.tanh((val @ v["value/fc2/kernel"].astype(np.float64) + v["value/fc2/bias"]) / 2)[:, 0]
    pol = residual(f, "policy/block4", 4)
    pol = residual(pol, "policy/block5", 5)
    pol = out["pconv"] = _elu(conv("policy/conv", "pconv", pol)[0])
    logits = out["logits"] = pol.reshape(B, -1) @ v["policy/fc/kernel"].astype(np.float64) + v["policy/fc/bias"]
    logits = logits - logits.max(axis=1, keepdims=True)
    e = np.exp(logits)
    out["prob"] = e / e.sum(axis=1, keepdims=True)
    return out


def loss_terms(variables, boards, distrib, winner, weights):
    """fp64 restatement of the loss graph (network.py:40-50): total, cross_entropy, value_loss, entropy."""
    v = variables
    x = np.asarray(boards, np.float64)
    B = x.shape[0]
    f = _elu(_conv2d(x, v["bone/conv1/kernel"], v["bone/conv1/bias"]))
    f = _residual(f, v, "bone/block1")
    f = _residual(f, v, "bone/block2")
    val = _residual(f, v, "value/block3")
    val = _elu(_conv2d(val, v["value/conv/kernel"], v["value/conv/bias"])).reshape(B, -1)
    val = _elu(val @ v["value/fc1/kernel"].astype(np.float64) + v["value/fc1/bias"])
    val = np.tanh((val @ v["value/fc2/kernel"].astype(np.float64) + v["value/fc2/bias"]) / 2)[:, 0]
    pol = _residual(f, v, "policy/block4")
    pol = _residual(pol, v, "policy/block5")
    pol = _elu(_conv2d(pol, v["policy/conv/kernel"], v["policy/conv/bias"]))
    logits = pol.reshape(B, -1) @ v["policy/fc/kernel"].astype(np.float64) + v["policy/fc/bias"]
    z = logits - logits.max(axis=1, keepdims=True)
    logsm = z - np.log(np.exp(z).sum(axis=1, keepdims=True))
    x_entropy = (np.asarray(distrib, np.float64) * logsm).sum(axis=1)                       # :41
    w = np.asarray(weights, np.float64)
    value_sq = (val - np.asarray(winner, np.float64)) ** 2                                  # :44
    l2 = sum((np.asarray(a, np.float64) ** 2).sum() / 2 for n, a in v.items() if "bias" not in n and "bn" not in n)  # :47-48
    total = -(x_entropy * w).mean() + 2.0 * (value_sq * w).mean() + 4e-5 * l2               # :50
    entropy = -(np.exp(logsm) * logsm).sum(axis=1).mean()
    return dict(total=total, cross_entropy=-x_entropy.mean(), value_loss=value_sq.mean(), entropy=entropy)
