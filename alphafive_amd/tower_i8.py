"""The int8 (W8A8) residual tower, stated once in numpy: the specification csrc/af_tower_i8.hip — kernels and packers — is held
to, as replay.draw_reference and train_hip.adam_reference are for their kernels.  Plain numpy, no GPU, no torch.

Every operation and its order is fixed here; "fp32" means one IEEE single-precision operation, round to nearest even.

ACTIVATION SCALES.  One fp32 scale `a` per stored int8 tensor, 2 * blocks of them in the order h_0, g_0, h_1, g_1, ...,
g_{blocks-1}: h_b is the input of block b, g_b the output of its first convolution.  The last block's output stays bf16 and has
none.  The kernels multiply by r = fp32(1 / a) (one fp32 division).

SCALES FROM ACTIVATIONS (scales_from_absmax, calibration_ok).  A scale comes from the absmax of the tensor it belongs to, over all
board pixels of all positions of a calibration batch:  a = fp32(fp32(absmax * margin) / 127), a = 1 for an absmax of exactly 0,
r = fp32(1 / a).  A set of 2 * blocks scales is usable iff every absmax is finite and every a finite and positive.  The DEVICE
calibration (af_tower_i8_calibrate, HipTower.calibrate_i8) measures the bf16 kernels' own stored activations — the h_b and g_b
the bf16 tower (csrc/af_tower_bf16.hip) writes for the same planes, exact bf16 values, so their absmax is exact — and applies
these operations in a kernel, held to them bit for bit.  DeepResNet.calibrate_int8 measures the fp32 PyTorch path instead and
does its arithmetic in fp64 on the host: the two agree to about the bf16 path's own distance from fp32, not to the bit.

ENTRY.  The stem's bf16 output x becomes int8 by  q = clamp(rint(fp32(x) * r_h0), -127, 127), rint = round half to even.

WEIGHTS of a block's first convolution, per cout c over its 1152 weights w (fp32):
    absmax = max |w|;  s[c] = absmax / 127;  inv = 127 / absmax;  q = clamp(rint(w * inv), -127, 127)
an all-zero row gets s = 1, q = 0.  Its multiplier is m[c] = s[c] * a_h, its bias b[c] = c1_b[c].

WEIGHTS of the second convolution and the 1x1 projection, which share an int32 accumulator over tensors of different scales
(g_b, h_b): the ratio goes into the projection first, ratio = a_h / a_g, wp' = wp * ratio, then ONE absmax per cout over the 1152
conv2 weights and the 128 wp' together, s / inv / q as above for all 1280.  m[c] = s[c] * a_g, b[c] = c2_b[c] + res_b[c].

EPILOGUE of a convolution with int32 accumulator acc (exact: |acc| <= 1280 * 127 * 127 < 2^25):
    pre = fmaf(float(acc), m[c], b[c])                 (float(acc): int32 -> fp32, exact below 2^24; the fmaf rounds ONCE)
    y   = ELU(pre) = pre if pre >= 0 else exp(pre) - 1
    out = clamp(rint(y * r_out), -127, 127)            int8, r_out the reciprocal scale of the tensor written
    out = bf16(y), round to nearest even               the last block's second convolution
The kernels' exponential (v_exp_f32) is not reproducible in numpy: on the side pre < 0 a kernel may land one step away from
this module where the real y * r_out is within r_out * 2^-20 of a rounding boundary; conv_reference returns that real value
in fp64 so that a test can tell (near_boundary; bf16_interval for the bf16 form).

FRAGMENT MAP (pack_fragments).  v_mfma_i32_32x32x32_i8 contracts 32 channels per k-step: lane l of the A operand holds row l % 32
and the 16 consecutive channels 32 * cc + 16 * (l / 32) + e of k-step cc.  A wave owns TWO cout tiles of 32, so the stream is
    uint8 [2 cout halves][NS][64 lanes][16],  fragment f = 2 * s + ct,  s = 4 * tap + cc (tap row-major, 36 steps), then the
    projection's four steps s = 36 + cc;  NS = 72 (first convolution) or 80
and the lane's row is cout 64 * half + 32 * ct + perm(l % 32), perm the row permutation of the bf16 streams (oracle/tower_pack.py)
that leaves a lane's 16 accumulator rows 16 consecutive couts.

ACTIVATION LAYOUT "C16": int8 [batch][8][PIX = 144][16], pixel (y, x) of channel 16 * k + e at [k][11 * (y + 1) + x][e]: the C8
layout of include/af_tower_bf16.h with 16 one-byte channels per 16-byte unit.
"""
import numpy as np

W, S, NPIX, PIX = 128, 11, 121, 144
QMAX = 127.0
f32 = np.float32


def _perm(m):
    return 16 * ((m >> 2) & 1) + 8 * (m >> 4) + 4 * ((m >> 3) & 1) + (m & 3)


PERM = np.array([_perm(m) for m in range(32)])


def bf16_round(a):
    """fp64 -> nearest bf16 value (ties to even), returned as fp64 (as oracle.tower_fp64.bf16_round; restated: the package does
    not import the test oracle)."""
    a = np.asarray(a, np.float64)
    m, e = np.frexp(a)
    return np.ldexp(np.rint(m * 256.0), e - 8)


def check_scales(act_scales, blocks):
    a = np.asarray(act_scales, np.float32).reshape(-1)
    if a.shape[0] != 2 * blocks:
        raise ValueError("int8 tower: %d activation scales, expected 2 * blocks = %d" % (a.shape[0], 2 * blocks))
    if not (np.isfinite(a).all() and (a > 0).all()):
        raise ValueError("int8 tower: activation scales must be finite and positive")
    return a


def reciprocal(a):
    """r = fp32(1 / a)."""
    return f32(1.0) / np.asarray(a, np.float32)


def scales_from_absmax(absmax, margin):
    """absmax [n] (any float dtype; bf16 values on the device route) -> (a, r), float32 [n] each: a = fdiv(fmul(absmax, margin), 127),
    1 where absmax is exactly 0; r = fdiv(1, a).  Every step one fp32 operation.  Values that calibration_ok refuses (NaN,
    infinities) pass through as IEEE arithmetic makes them."""
    x = np.asarray(absmax, np.float32).reshape(-1)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        a = ((x * f32(margin)).astype(np.float32) / f32(QMAX)).astype(np.float32)
        a = np.where(x == 0, f32(1.0), a).astype(np.float32)
        r = (f32(1.0) / a).astype(np.float32)
    return a, r


def calibration_ok(absmax, margin):
    """True iff every absmax is finite and every scale scales_from_absmax makes of it is finite and positive: the condition under
    which the device calibration installs its scales (all of them, or none)."""
    x = np.asarray(absmax, np.float32).reshape(-1)
    a, _ = scales_from_absmax(x, margin)
    return bool(np.isfinite(x).all() and np.isfinite(a).all() and (a > 0).all())


def quantize_activation(x, r):
    """x (bf16 values, any float dtype) -> int8: clamp(rint(fp32(x) * r), -127, 127)."""
    t = np.asarray(x, np.float32) * f32(r)
    return np.clip(np.rint(t), -QMAX, QMAX).astype(np.int8)


def _quantize_rows(rows):
    """rows fp32 [128][n] -> (q int8 [128][n], s fp32 [128])."""
    absmax = np.abs(rows).max(axis=1).astype(np.float32)
    zero = absmax == 0
    safe = np.where(zero, f32(1.0), absmax).astype(np.float32)
    s = np.where(zero, f32(1.0), safe / f32(QMAX)).astype(np.float32)
    inv = (f32(QMAX) / safe).astype(np.float32)
    q = np.clip(np.rint((rows * inv[:, None]).astype(np.float32)), -QMAX, QMAX).astype(np.int8)
    q[zero] = 0
    return q, s


def quantize_weights(c1, c2, res, a_h, a_g):
    """One block.  c1 / c2 / res = (weight OIHW, bias) in fp32 (converted if not); a_h / a_g the scales of the block's input and
    of its mid activation.  -> dict(q1 int8 [128,128,3,3], m1, b1, q2 int8 [128,128,3,3], qp int8 [128,128], m2, b2, s1, s2)."""
    a_h, a_g = f32(a_h), f32(a_g)
    w1, w2 = np.asarray(c1[0], np.float32).reshape(W, W * 9), np.asarray(c2[0], np.float32).reshape(W, W * 9)
    wp = np.asarray(res[0], np.float32).reshape(W, W)
    q1, s1 = _quantize_rows(w1)
    ratio = f32(a_h / a_g)
    wpf = (wp * ratio).astype(np.float32)
    q2p, s2 = _quantize_rows(np.concatenate([w2, wpf], axis=1))
    return dict(q1=q1.reshape(W, W, 3, 3), s1=s1, m1=(s1 * a_h).astype(np.float32), b1=np.asarray(c1[1], np.float32).copy(),
                q2=q2p[:, :W * 9].reshape(W, W, 3, 3), qp=q2p[:, W * 9:].copy(), s2=s2, m2=(s2 * a_g).astype(np.float32),
                b2=(np.asarray(c2[1], np.float32) + np.asarray(res[1], np.float32)).astype(np.float32))


def pack_fragments(q3, qp=None):
    """The A-fragment stream of one convolution: uint8 [2][NS][64][16] (module docstring), NS = 72, or 80 with the projection."""
    NS = 72 if qp is None else 80
    out = np.zeros((2, NS, 64, 16), np.int8)
    lane = np.arange(64)
    for half in range(2):
        for s in range(NS // 2):
            for ct in range(2):
                co = 64 * half + 32 * ct + PERM[lane & 31]                      # [64]
                ci = 32 * (s % 4 if s < 36 else s - 36) + 16 * (lane >> 5)      # [64]
                idx = ci[:, None] + np.arange(16)[None, :]
                if s < 36:
                    t = s // 4
                    out[half, 2 * s + ct] = q3[co[:, None], idx, t // 3, t % 3]
                else:
                    out[half, 2 * s + ct] = qp[co[:, None], idx]
    return out.view(np.uint8)


def to_c16(q):
    """int8 NCHW [B,128,11,11] -> C16 [B][8][144][16] with zero rows."""
    B = q.shape[0]
    out = np.zeros((B, 8, PIX, 16), np.int8)
    out[:, :, S:S + NPIX, :] = q.reshape(B, 8, 16, NPIX).transpose(0, 1, 3, 2)
    return out


def from_c16(c):
    B = c.shape[0]
    return np.ascontiguousarray(c[:, :, S:S + NPIX, :].transpose(0, 1, 3, 2)).reshape(B, W, S, S)


def _fmaf32(acc, m, b):
    """fp32 fmaf(float(acc), m, b) with ONE rounding: the product of two fp32 values is exact in fp64; the fp64 sum is
    made sticky (round to odd) with the error term of the addition, so that the final rounding to fp32 sees the exact value."""
    p = np.asarray(acc).astype(np.float32).astype(np.float64) * np.asarray(m, np.float64)     # float(acc): one rounding above 2^24
    b = np.broadcast_to(np.asarray(b, np.float64), p.shape)
    s = p + b
    bb = s - p
    err = (p - (s - bb)) + (b - bb)
    even = (s.view(np.int64) & 1) == 0
    nudged = np.nextafter(s, np.where(err > 0, np.inf, -np.inf))
    s = np.where((err != 0) & even, nudged, s)
    return s.astype(np.float32)


def _accumulate(xq, q3):
    """Integer 3x3 SAME convolution as fp64 matrix products (exact: every sum is an integer below 2^25).  -> [B,128,11,11] fp64."""
    B = xq.shape[0]
    xp = np.zeros((B, S + 2, S + 2, W), np.float64)
    xp[:, 1:S + 1, 1:S + 1, :] = np.asarray(xq, np.float64).transpose(0, 2, 3, 1)
    acc = np.zeros((B * NPIX, W), np.float64)
    w = np.asarray(q3, np.float64)
    for a in range(3):
        for c in range(3):
            acc += np.ascontiguousarray(xp[:, a:a + S, c:c + S, :]).reshape(-1, W) @ np.ascontiguousarray(w[:, :, a, c].T)
    return acc.reshape(B, S, S, W).transpose(0, 3, 1, 2)


def conv_reference(xq, q3, m, b, r_out=None, xq2=None, qp=None):
    """One layer.  xq int8 [B,128,11,11] through the int8 3x3 weights q3 (plus, with xq2 / qp, the int8 1x1 projection of xq2 into
    the same accumulator), multipliers m, biases b.  r_out: reciprocal scale of the int8 output, or None for the bf16 form.
    -> (out, t64, pre): out int8, or the bf16 values as fp32; t64 the real value in front of the final rounding in fp64 —
    ELU(pre) * r_out, or ELU(pre) for the bf16 form — and pre the fp32 pre-activation."""
    acc = _accumulate(xq, q3)
    if qp is not None:
        x2 = np.asarray(xq2, np.float64).transpose(0, 2, 3, 1).reshape(-1, W)
        acc = acc + (x2 @ np.asarray(qp, np.float64).T).reshape(-1, S, S, W).transpose(0, 3, 1, 2)
    pre = _fmaf32(acc, np.asarray(m, np.float32)[None, :, None, None], np.asarray(b, np.float32)[None, :, None, None])
    p64 = pre.astype(np.float64)
    y64 = np.where(p64 >= 0, p64, np.expm1(np.minimum(p64, 0)))
    y32 = np.where(pre >= 0, pre, y64.astype(np.float32)).astype(np.float32)
    if r_out is None:
        return bf16_round(y32.astype(np.float64)).astype(np.float32), y64, pre
    t32 = (y32 * f32(r_out)).astype(np.float32)
    return np.clip(np.rint(t32), -QMAX, QMAX).astype(np.int8), y64 * np.float64(f32(r_out)), pre


ELU_ERR = 2.0 ** -22


def near_boundary(t64, r_out):
    """int8 form: the elements whose final rounding the kernels' exponential may decide the other way (module docstring): t64 =
    y * r_out within r_out * 2^-20 of a half-integer."""
    return np.abs((t64 - np.floor(t64)) - 0.5) < float(r_out) * 2.0 ** -20


def bf16_interval(y64):
    """bf16 form: the bf16 values the kernels may store for a NEGATIVE pre-activation whose real ELU is y64 -> (lo, hi), the
    roundings of y64 -+ ELU_ERR.  The bf16 form rounds y itself, on a step that shrinks with |y| while the error of the kernels'
    ELU does not: y = e - 1 with e = v_exp_f32(fl(x * log2 e)); the rounded argument moves e by at most |x| e 2^-24 <= 0.37 * 2^-24,
    v_exp_f32 is good to one ulp of e <= 1, i.e. 2^-23, the subtraction is exact for e >= 1/2 (2^-25 below), and the max(x, .)
    form returns x instead for -3e-4 < x < 0, within x^2 / 2 < 2^-24: |error of y| < ELU_ERR = 2^-22, absolute.  Where lo == hi
    the stored value is determined; where they differ (y within 2^-22 of the midpoint of two bf16 values: one step apart at
    ordinary magnitudes, more below |y| = 2^-13, where the step is smaller than the error) any bf16 value in [lo, hi] may appear."""
    y64 = np.asarray(y64, np.float64)
    return bf16_round(y64 - ELU_ERR), bf16_round(y64 + ELU_ERR)


def forward_reference(x, blocks, act_scales):
    """x: the stem's output (bf16 values) [B,128,11,11]; blocks: list of dict(c1, c2, res) of (weight, bias); act_scales as the
    module docstring orders them.  -> (h bf16 values as fp32 [B,128,11,11], trace): trace[b] = dict(h int8, g int8) of block b."""
    a = check_scales(act_scales, len(blocks))
    r = reciprocal(a)
    h = quantize_activation(x, r[0])
    trace = []
    for i, blk in enumerate(blocks):
        qw = quantize_weights(blk["c1"], blk["c2"], blk["res"], a[2 * i], a[2 * i + 1])
        g, _, _ = conv_reference(h, qw["q1"], qw["m1"], qw["b1"], r[2 * i + 1])
        trace.append(dict(h=h, g=g))
        last = i == len(blocks) - 1
        h, _, _ = conv_reference(g, qw["q2"], qw["m2"], qw["b2"], None if last else r[2 * i + 2], h, qw["qp"])
    return h, trace
