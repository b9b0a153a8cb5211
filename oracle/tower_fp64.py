"""fp64 numpy restatement of the bf16 residual tower (BASELINE configs[4]), layer by layer, written from
include/af_tower_bf16.h and alphafive_amd/network_deep.py — the per-element checker of csrc/af_tower_bf16.hip.
TEST INFRASTRUCTURE ONLY.

Layouts are the ABI's: activations NCHW, convolution weights PyTorch OIHW, dense weights [in][out].  Every layer
returns its fp64 value BEFORE the rounding to bf16 that the kernels apply to what they store, together with the
absolute-term sum  A = sum |w * x| + |bias|  of every output's pre-activation: the quantity a floating-point error
bound of an n-term dot product is proportional to.  Callers round with bf16_round where the kernels do.
"""
import numpy as np


def bf16_round(a):
    """Round to the nearest bfloat16 (8 significant bits), ties to even, straight from fp64 (no detour through fp32);
    the result is returned as fp64.  Values below bf16's normal range are not treated specially."""
    a = np.asarray(a, np.float64)
    m, e = np.frexp(a)                                   # a = m * 2**e, 0.5 <= |m| < 1
    return np.ldexp(np.rint(m * 256.0), e - 8)           # np.rint rounds half to even


def elu(x):
    return np.where(x > 0, x, np.expm1(np.minimum(x, 0)))


def _conv2d(x, w, b):
    """x [B,Cin,H,W], w OIHW (odd kernel, SAME zero padding), b [Cout] -> (pre-activation [B,Cout,H,W], A), fp64."""
    x, w, b = np.asarray(x, np.float64), np.asarray(w, np.float64), np.asarray(b, np.float64)
    cout, cin, kh, kw = w.shape
    B, _, H, W = x.shape
    ph, pw = kh // 2, kw // 2
    xp = np.zeros((B, H + 2 * ph, W + 2 * pw, cin), np.float64)      # NHWC: every tap is one fp64 matrix product
    xp[:, ph:ph + H, pw:pw + W, :] = x.transpose(0, 2, 3, 1)
    xa, wa = np.abs(xp), np.abs(w)
    out = np.zeros((B * H * W, cout), np.float64)
    absum = np.zeros((B * H * W, cout), np.float64)
    for a in range(kh):
        for c in range(kw):
            if not w[:, :, a, c].any():
                continue
            win = (slice(None), slice(a, a + H), slice(c, c + W))        # (contiguous 2-D operands: one BLAS call per tap)
            out += np.ascontiguousarray(xp[win]).reshape(-1, cin) @ np.ascontiguousarray(w[:, :, a, c].T)
            absum += np.ascontiguousarray(xa[win]).reshape(-1, cin) @ np.ascontiguousarray(wa[:, :, a, c].T)
    nchw = lambda y: y.reshape(B, H, W, cout).transpose(0, 3, 1, 2)  # noqa: E731
    bias = b[None, :, None, None]
    return nchw(out) + bias, nchw(absum) + np.abs(bias)


def stem(planes, w, b):
    """5x5 SAME convolution 3 -> W + bias + ELU (network_deep.py eval_device, first line).  -> (y, A)."""
    pre, A = _conv2d(planes, w, b)
    return elu(pre), A


def block(h, c1, c2, res, mid=None):
    """One residual block (af_tower_bf16.h):  r = conv1x1(h) + b_res;  g = ELU(conv3x3(h) + b1);  h' = ELU(r + conv3x3(g) + b2).
    c1 / c2 / res = (weight OIHW, bias).  -> (g, A1, h', A2): both convolutions' fp64 values before rounding and their
    absolute-term sums.  The second convolution reads the mid activation as the kernels store it: g rounded to bf16 —
    or `mid`, when the caller passes the mid activation that was actually stored."""
    pre1, A1 = _conv2d(h, *c1)
    g = elu(pre1)
    gin = bf16_round(g) if mid is None else np.asarray(mid, np.float64)
    pre2, A2 = _conv2d(gin, *c2)
    r, Ar = _conv2d(h, *res)
    return g, A1, elu(pre2 + r), A2 + Ar


def heads(h, vconv, pconv):
    """The heads' 1x1 convolutions + bias + ELU, flattened in NCHW order as the dense layers take them.
    -> (vin [B, 4*S*S], Av, pin [B, 16*S*S], Ap)."""
    B = np.asarray(h).shape[0]
    pv, Av = _conv2d(h, *vconv)
    pp, Ap = _conv2d(h, *pconv)
    return elu(pv).reshape(B, -1), Av.reshape(B, -1), elu(pp).reshape(B, -1), Ap.reshape(B, -1)


def dense(vin, pin, vfc1, vfc2, pfc):
    """The three dense layers behind the heads (weights [in][out]): value = tanh((ELU(vin @ vfc1 + b) @ vfc2 + b) / 2),
    policy = softmax(pin @ pfc + b).  -> (policy [B, S*S], value [B], logits [B, S*S], z [B])."""
    f = lambda a: np.asarray(a, np.float64)  # noqa: E731
    v1 = elu(f(vin) @ f(vfc1[0]) + f(vfc1[1]))
    z = (v1 @ f(vfc2[0]).reshape(-1, 1))[:, 0] + float(f(vfc2[1]).reshape(-1)[0])
    logits = f(pin) @ f(pfc[0]) + f(pfc[1])
    e = np.exp(logits - logits.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True), np.tanh(z / 2), logits, z
