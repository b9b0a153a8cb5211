"""The trainer's fused kernels (libaf_train.so, include/af_train.h) on torch device tensors, and their specifications.

    loss_head   logits, value, pi, winner, weight -> dlogits, dvalue, row_terms      one launch, one wavefront per row
    adam        every variable's (p, g, m, v) updated in place + the L2 partial sums  one launch per 64 variables
    finalize    row_terms + L2 partials -> (total, cross_entropy, value_loss, entropy) on the device

All three run on torch's current stream and never wait for the device.  The specifications, in numpy:
    adam_reference          the Adam element in float32, one operation per line                        the kernel: bit for bit
    l2_partials_reference   a chunk's sum of p * p in the header's order (strided, butterfly, waves)   the kernel: bit for bit
    finalize_reference      the six fp64 sums in that order and the header's four expressions          the kernel: bit for bit
    loss_head_reference     the loss head in float64 (loss_head_parts: with logsm and sum(pi)); dvalue, vsq and w * vsq bit for
                            bit, dlogits inside the fp32 interval around ref +- 2^-40 * (w / B) * (|pi| + s * sum(pi))
terms_reference() is finalize in float64 without an order.  tests/train_cases.py holds the cases and the comparison rules,
tests/test_gpu_train_fused.py runs the kernels on them.  train.Trainer(fused=True) is the caller.
"""
import ctypes as C
import os

import numpy as np
import torch

_PKG = os.path.dirname(os.path.abspath(__file__))
_LIBPATH = os.environ.get("AF_TRAIN_LIB") or os.path.join(_PKG, "_lib", "libaf_train.so")
_lib = None

MAX_C = 1024            # AF_TRAIN_MAX_C
ROW_TERMS = 5           # AF_TRAIN_ROW_TERMS: (w * xent, w * vsq, xent, vsq, ent), float64
MAX_VARS = 64           # AF_TRAIN_MAX_VARS
ADAM_CHUNK = 2048       # AF_TRAIN_ADAM_CHUNK
ERR_ARG, ERR_HIP, ERR_RANGE = -1, -2, -3
L2_COEF = 4e-5          # network.py:47-50


class TrainError(RuntimeError):
    pass


class Var(C.Structure):
    """af_train_var"""
    _fields_ = [("p", C.c_void_p), ("g", C.c_void_p), ("m", C.c_void_p), ("v", C.c_void_p), ("n", C.c_int64),
                ("decay", C.c_int32), ("reserved", C.c_int32)]


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(_LIBPATH):
            raise ImportError(f"{_LIBPATH} not built (python -m alphafive_amd.build)")
        L = C.CDLL(_LIBPATH)            # torch (imported above) first: one HIP runtime per process, see replay.lib
        vp, f = C.c_void_p, C.c_float
        L.af_train_loss_head.argtypes = [vp, C.c_int32, C.c_int32, vp, vp, vp, vp, vp, vp, vp, vp]
        L.af_train_adam.argtypes = [vp, C.c_int32, C.POINTER(Var), f, f, f, f, f, vp]
        L.af_train_adam_partials.argtypes = [C.c_int32, C.POINTER(C.c_int64)]
        L.af_train_finalize.argtypes = [vp, C.c_int32, vp, C.c_int32, vp, f, vp]
        L.af_train_strerror.argtypes = [C.c_int]
        L.af_train_strerror.restype = C.c_char_p
        _lib = L
    return _lib


def _check(rc, what):
    if rc < 0:
        raise TrainError(f"{what}: {lib().af_train_strerror(rc).decode()} (code {rc})")
    return rc


def _stream(device):
    return torch.cuda.current_stream(device).cuda_stream


def _dev32(t, what, device=None, dtype=torch.float32):
    """A contiguous fp32 device tensor as it is; anything else is the caller's mistake, not something to convert quietly."""
    if not (torch.is_tensor(t) and t.is_cuda and t.dtype == dtype and t.is_contiguous()):
        raise TrainError(f"{what}: expected a contiguous {dtype} device tensor")
    if device is not None and t.device != device:
        raise TrainError(f"{what}: on {t.device}, expected {device}")
    return t


def loss_head(logits, value, pi, winner, weight):
    """-> (dlogits[B][C], dvalue[B], row_terms[B][ROW_TERMS] float64): the gradient of `total` with respect to logits and value, and
    the per-row terms finalize() reduces (af_train_loss_head).  None of the inputs needs to be detached; none is written."""
    logits, value = _dev32(logits.detach(), "logits"), _dev32(value.detach(), "value", logits.device)
    B, Cn = logits.shape
    for name, t, shape in (("pi", pi, (B, Cn)), ("winner", winner, (B,)), ("weight", weight, (B,)), ("value", value, (B,))):
        if tuple(_dev32(t, name, logits.device).shape) != shape:
            raise TrainError(f"{name}: shape {tuple(t.shape)}, expected {shape}")
    dlogits, dvalue = torch.empty_like(logits), torch.empty_like(value)
    rows = torch.empty((B, ROW_TERMS), dtype=torch.float64, device=logits.device)
    _check(lib().af_train_loss_head(_stream(logits.device), B, Cn, logits.data_ptr(), value.data_ptr(), pi.data_ptr(),
                                    winner.data_ptr(), weight.data_ptr(), dlogits.data_ptr(), dvalue.data_ptr(),
                                    rows.data_ptr()), "af_train_loss_head")
    return dlogits, dvalue, rows


def adam_partials(sizes):
    """Length of the l2_partials an adam() over variables of these sizes writes: sum of ceil(n / ADAM_CHUNK)."""
    a = (C.c_int64 * len(sizes))(*[int(n) for n in sizes])
    return _check(lib().af_train_adam_partials(len(sizes), a), "af_train_adam_partials")


class VarTable(object):
    """The (p, m, v, decay) side of adam()'s table, built once: ctypes arrays of at most MAX_VARS entries each, one launch per
    array.  set_grads() fills in the side that changes every step (autograd hands out fresh gradient tensors).  An empty
    variable is allowed: torch gives it a null pointer, which the library accepts for n = 0 and never reads."""

    def __init__(self, ps, ms, vs, decay):
        self.device = ps[0].device
        self.keep = (list(ps), list(ms), list(vs))
        self.groups = []
        for i0 in range(0, len(ps), MAX_VARS):
            arr = (Var * len(ps[i0:i0 + MAX_VARS]))()
            for j, (p, m, v, d) in enumerate(zip(ps[i0:i0 + MAX_VARS], ms[i0:], vs[i0:], decay[i0:])):
                for name, t in (("p", p), ("m", m), ("v", v)):
                    if _dev32(t.detach(), name, self.device).numel() != p.numel():
                        raise TrainError(f"{name} of variable {i0 + j}: {t.numel()} elements, expected {p.numel()}")
                arr[j].p, arr[j].m, arr[j].v = p.data_ptr(), m.data_ptr(), v.data_ptr()
                arr[j].n, arr[j].decay = p.numel(), int(bool(d))
            self.groups.append(arr)
        self.n_partials = adam_partials([p.numel() for p in ps])
        self.grads = None

    def set_grads(self, grads):
        """Gradients in the variables' order.  A gradient that is not laid out like its variable (the 42-variable net's
        convolution kernels: autograd returns the permuted view of an OIHW gradient) is copied into that layout first."""
        grads = [g if g.is_contiguous() else g.contiguous() for g in grads]
        if len(grads) != len(self.keep[0]):
            raise TrainError(f"{len(grads)} gradients for {len(self.keep[0])} variables")
        it = iter(grads)
        for arr in self.groups:
            for e in arr:
                g = _dev32(next(it), "g", self.device)
                if g.numel() != e.n:
                    raise TrainError(f"gradient of {g.numel()} elements for a variable of {e.n}")
                e.g = g.data_ptr()
        self.grads = grads          # alive until the launch that reads them is queued


def adam(vars, lr_t, beta1, beta2, eps, l2_coef, l2_partials):
    """tf.train.AdamOptimizer's update of every variable in place (af_train_adam; adam_reference is its element).  `vars`: a
    VarTable after set_grads(), or a list of (p, g, m, v, decay).  One launch per MAX_VARS variables.  l2_partials: float32
    device buffer of at least adam_partials(sizes) elements; -> how many of them were written."""
    if not isinstance(vars, VarTable):
        vars = list(vars)
        table = VarTable([x[0] for x in vars], [x[2] for x in vars], [x[3] for x in vars], [x[4] for x in vars])
        table.set_grads([x[1] for x in vars])
        vars = table
    if vars.grads is None:
        raise TrainError("adam: VarTable without gradients (set_grads)")
    if _dev32(l2_partials, "l2_partials", vars.device).numel() < vars.n_partials:
        raise TrainError(f"l2_partials holds {l2_partials.numel()} elements, {vars.n_partials} needed")
    st, done, base = _stream(vars.device), 0, l2_partials.data_ptr()
    for arr in vars.groups:
        done += _check(lib().af_train_adam(st, len(arr), arr, lr_t, beta1, beta2, eps, l2_coef, base + 4 * done),
                       "af_train_adam")
    vars.grads = None
    return done


def finalize(row_terms, l2_partials, n_partials, l2_coef, out=None):
    """-> float32[4] on the device: (total, cross_entropy, value_loss, entropy) (af_train_finalize)."""
    rows = _dev32(row_terms, "row_terms", dtype=torch.float64)
    if rows.dim() != 2 or rows.shape[1] != ROW_TERMS:
        raise TrainError(f"row_terms: shape {tuple(rows.shape)}, expected (B, {ROW_TERMS})")
    if n_partials and _dev32(l2_partials, "l2_partials", rows.device).numel() < n_partials:
        raise TrainError(f"l2_partials holds {l2_partials.numel()} elements, n_partials = {n_partials}")
    out = torch.empty(4, dtype=torch.float32, device=rows.device) if out is None else _dev32(out, "out", rows.device)
    _check(lib().af_train_finalize(_stream(rows.device), rows.shape[0], rows.data_ptr(), int(n_partials),
                                   l2_partials.data_ptr() if n_partials else None, l2_coef, out.data_ptr()),
           "af_train_finalize")
    return out


# ---- specifications ----
def adam_reference(p, g, m, v, decay, lr_t, beta1, beta2, eps, l2_coef):
    """One Adam step of one variable in numpy float32 -> (p, m, v), new arrays.  Every line is one rounded fp32 operation per
    operator, in the order af_train_adam_kernel performs them; numpy's float32 divide and square root are correctly rounded."""
    f = np.float32
    p, g, m, v = (np.asarray(a, f) for a in (p, g, m, v))
    lr_t, beta1, beta2, eps, l2_coef = f(lr_t), f(beta1), f(beta2), f(eps), f(l2_coef)
    c1 = f(1) - beta1
    c2 = f(1) - beta2
    if decay:
        g = g + l2_coef * p
    m = m * beta1 + g * c1
    v = v * beta2 + (g * g) * c2
    p = p - (lr_t * m) / (np.sqrt(v) + eps)
    assert p.dtype == m.dtype == v.dtype == np.float32
    return p, m, v


def _tree_sum(acc):
    """The fixed tree every block reduction of af_train.hip ends with (block_sum): acc[..., 256] holds the 256 threads' own
    sums; a butterfly over the 64 lanes of each wave (x = x + x[lane ^ o], o = 32 .. 1: every lane ends with the same bits),
    then the four waves as ((w0 + w1) + w2) + w3.  In acc's dtype, one IEEE add per step."""
    x = acc.reshape(acc.shape[:-1] + (4, 64))
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        x = x + x[..., lane ^ o]
    w = x[..., 0]
    return ((w[..., 0] + w[..., 1]) + w[..., 2]) + w[..., 3]


def _strided_sum(x, dtype):
    """Thread t of 256 adds entries t, t + 256, ... of x (one dimension) in index order, from 0; then _tree_sum.  A thread's
    sum never is -0 (it starts at +0), so padding the tail with +0 adds nothing."""
    x = np.asarray(x, dtype).reshape(-1)
    pad = np.zeros(-(-max(x.size, 1) // 256) * 256, dtype)
    pad[:x.size] = x
    acc = np.zeros(256, dtype)
    for row in pad.reshape(-1, 256):
        acc = acc + row
    return _tree_sum(acc)


def l2_partials_reference(p, decay):
    """af_train_adam's l2_partials of one variable (p BEFORE the update) -> float32[ceil(n / ADAM_CHUNK)], in the order
    include/af_train.h states: per chunk, thread t of 256 adds p * p of elements t, t + 256, ... in fp32, then the butterfly
    over the 64 lanes, then the four waves in order.  0 per chunk for a variable without decay; empty for n = 0.
    The kernel equals it bit for bit."""
    p = np.asarray(p, np.float32).reshape(-1)
    chunks = -(-p.size // ADAM_CHUNK)
    if not decay or chunks == 0:
        return np.zeros(chunks, np.float32)
    pad = np.zeros(chunks * ADAM_CHUNK, np.float32)
    pad[:p.size] = p
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        sq = (pad * pad).reshape(chunks, ADAM_CHUNK // 256, 256)
        acc = np.zeros((chunks, 256), np.float32)
        for j in range(sq.shape[1]):
            acc = acc + sq[:, j, :]
        out = _tree_sum(acc)
    assert out.dtype == np.float32
    return out


def finalize_reference(row_terms, l2_partials, l2_coef):
    """af_train_finalize -> float32[4] (total, cross_entropy, value_loss, entropy), bit for bit: the five column sums S_j of
    row_terms float64[B][ROW_TERMS] and L, the sum of the fp32 partials converted to fp64, each in the strided, butterfly and
    four-wave order of include/af_train.h in fp64; then the header's four expressions as written, each rounded to fp32 once."""
    rows = np.asarray(row_terms, np.float64).reshape(-1, ROW_TERMS)
    dB = np.float64(rows.shape[0])
    with np.errstate(over="ignore", invalid="ignore"):
        s = [_strided_sum(rows[:, j], np.float64) for j in range(ROW_TERMS)]
        L = _strided_sum(np.asarray(l2_partials, np.float32).astype(np.float64), np.float64)
        total = (-(s[0] / dB) + np.float64(2.0) * (s[1] / dB)) + np.float64(np.float32(l2_coef)) * (L / np.float64(2.0))
        return np.array([total, -(s[2] / dB), s[3] / dB, s[4] / dB], np.float64).astype(np.float32)


def loss_head_parts(logits, value, pi, winner, weight):
    """The float64 statement of af_train_loss_head with its intermediates -> dict(dlogits, dvalue, rows, logsm, psum)."""
    z, v, pi, zv, w = (np.asarray(a, np.float64) for a in (logits, value, pi, winner, weight))
    B = z.shape[0]
    z = z - z.max(axis=1, keepdims=True)
    logsm = z - np.log(np.exp(z).sum(axis=1, keepdims=True))
    xent = (pi * logsm).sum(axis=1)
    vsq = (v - zv) ** 2
    ent = -(np.exp(logsm) * logsm).sum(axis=1)
    rows = np.stack([w * xent, w * vsq, xent, vsq, ent], axis=1)
    psum = pi.sum(axis=1, keepdims=True)
    dlogits = -(w / B)[:, None] * (pi - np.exp(logsm) * psum)
    dvalue = (4 * w / B) * (v - zv)
    return dict(dlogits=dlogits, dvalue=dvalue, rows=rows, logsm=logsm, psum=psum[:, 0])


def loss_head_reference(logits, value, pi, winner, weight):
    """af_train_loss_head in float64 -> (dlogits[B][C], dvalue[B], row_terms[B][ROW_TERMS])."""
    r = loss_head_parts(logits, value, pi, winner, weight)
    return r["dlogits"], r["dvalue"], r["rows"]


def terms_reference(row_terms, l2_sum, l2_coef=L2_COEF):
    """af_train_finalize in float64: rows of loss_head_reference and sum(p^2) over the decay variables -> dict of the four."""
    s = np.asarray(row_terms, np.float64).mean(axis=0)
    return dict(total=-s[0] + 2.0 * s[1] + l2_coef * float(l2_sum) / 2.0, cross_entropy=-s[2], value_loss=s[3], entropy=s[4])
