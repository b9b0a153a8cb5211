"""Cases for the trainer's fused kernels (csrc/af_train.hip, include/af_train.h) against the specifications of
alphafive_amd/train_hip.py: the generators, the comparison rules and — from the references alone, without a GPU — numpy models
of the kernels that a planted fault can be put into.  Plain numpy; tests/test_gpu_train_fused.py runs the kernels on these
cases and calls the check_* functions below, tests/test_train_fused_cpu.py runs the generators' conditions and shows that the same
check_* functions reject every planted fault.

THE LOSS HEAD.  HEAD_CASES reaches all five kernels (K = 1, 2, 4, 8, 16 logits per lane) with both sides of every lane-count
boundary, B = 9 (two full four-row blocks and a block with one live wave) and B = 1 .. 5 at two widths.  Rows are N(0, 3) logits
and a normalised exp(randn) target, except (by row index, where B reaches it):
    0  largest |z| is 40, one-hot pi                  5  pi with exact zeros, sum 0.5
    1  all logits equal                               6  pi all zero
    2  N(0, 3) - 1000: every logit far below zero     7  weight 0
    3  N(0, 3) * 300: beyond fp32 exp on both sides   8  pi sums to 2
    4  the maximum at c = C - 1, every other logit 90 .. 103 below it, every second pi zero (subnormal fp32 gradients)

THE RULE FOR dlogits (check_loss_head).  With ref, s_c = exp(logsm_c) and psum of train_hip.loss_head_parts in fp64 and
    e_c = 2^-40 * (w / B) * (|pi_c| + s_c * psum)
the stored fp32 value must lie in the closed interval [float32(ref - e), float32(ref + e)]; where the two ends are the same fp32
value that is bit equality.  Why 2^-40: the kernel shifts the row by its max exactly; its sums differ from numpy's only in the
order of at most 22 fp64 adds; the device's fp64 exp and log differ from libm's by a couple of ulp; so logsm carries at most
|logsm| * 2^-52 + 2^-48 of absolute error, which is the relative error of s_c wherever s_c is not zero (|logsm| < 745).  That is
below 2^-42 relative on s_c * psum and 2^-50 on pi_c; 2^-40 leaves a factor of four and is still 2^16 below an fp32 ulp of the
larger operand.  Subnormal results are not exempt.  C = 1 is stated on its own: s = 1 exactly, so every element is the
reference's signed zero, bit for bit.
Elements whose interval has two different ends are "near"; over all cases together (C = 1 aside) they may be at most 0.1 % of
the elements (near_share: a condition on the generator).
dvalue, row_terms[:, 3] (vsq) and row_terms[:, 1] (w * vsq) are the reference's IEEE operations in its order: bit for bit.
ROW TERMS.  row_terms[:, 2] (xent = sum_c pi_c * logsm_c) and [:, 4] (ent = -sum_c s_c * logsm_c) must lie within
    2^-40 * sum_c |term_c|  +  2^-48 * sum_c |coefficient_c|          (coefficient: pi_c for xent, s_c for ent)
of the reference, [:, 0] (w * xent) within |w| times xent's bound plus 2^-40 * |w * xent|.  The second term is the absolute
part, 2^-48, of logsm's error as stated above: the rounding of sum_c exp(z_c - max) >= 1 (2^-53 of it, at most 22 times over two
summation orders) passes through the log as an ABSOLUTE error of logsm, which a bound relative to |coefficient_c * logsm_c| cannot
cover where logsm_c is near 0 — the largest element of a peaked row.  Row 0 has such an element (s = 1 - 1e-5, logsm = -1e-5,
ent = 1.8e-4): two correct fp64 evaluations of the header's formula differ by 2.2e-16 there, 1.3 times 2^-40 * sum |term|.
For an ordinary row (|logsm| about 5) the second term adds 0.1 % to the first.

ADAM.  adam_case(): eleven variables (every size around the wave, the workgroup and the chunk, mixed decay flags), four steps,
one variable of 4,096 elements carrying planted values in blocks of 256 (PLANTED).  Everything is train_hip.adam_reference's and
train_hip.l2_partials_reference's bits, signed zeros included; where the reference is NaN the kernel's value must be NaN.

FINALIZE.  finalize_case(B, P): row terms of mixed sign over twelve decades, most of them in pairs that cancel exactly, so that
the order of the fp64 adds shows in the fp32 results; partials positive over the same decades.  Bit for bit against
train_hip.finalize_reference.
"""
import functools

import numpy as np

from alphafive_amd import train_hip

E_REL = 2.0 ** -40
LOGSM_ABS = 2.0 ** -48                                                    # the absolute part of logsm's error, see ROW TERMS above
NEAR_CAP = 1e-3
BETA1, BETA2, EPS, L2 = 0.9, 0.999, 1e-8, 4e-5

HEAD_C = (1, 36, 63, 64, 65, 121, 127, 128, 129, 225, 255, 256, 257, 511, 512, 513, 1023, 1024)
HEAD_CASES = tuple((9, c) for c in HEAD_C) + tuple((b, c) for c in (121, 513) for b in (1, 2, 3, 4, 5))


def lr_t(t, lr=1e-3):
    return float(lr * np.sqrt(1.0 - BETA2 ** t) / (1.0 - BETA1 ** t))      # Trainer.step


def per_lane(C):
    """K of the af_train_loss_head_kernel<K> a row of C logits runs."""
    return next(k for k in (1, 2, 4, 8, 16) if C <= 64 * k)


def bits32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def bits64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


# ------------------------------------------------------------------ the loss head ------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def head_case(B, C):
    """-> (logits, value, pi, winner, weight), float32, read-only; the planted rows of the module docstring where B reaches."""
    rng = np.random.RandomState(7000 + 37 * B + C)
    z = (rng.randn(B, C) * 3).astype(np.float32)
    pi = np.exp(rng.randn(B, C))
    pi /= pi.sum(axis=1, keepdims=True)
    value = np.tanh(rng.randn(B)).astype(np.float32)
    winner = rng.choice([-1.0, 1.0], size=B).astype(np.float32)
    weight = (0.5 + rng.rand(B)).astype(np.float32)
    if B > 0:
        z[0] *= np.float32(39.0) / np.abs(z[0]).max()
        i = int(np.abs(z[0]).argmax())
        z[0, i] = np.copysign(np.float32(40.0), z[0, i])
        pi[0] = 0.0
        pi[0, C // 2] = 1.0
    if B > 1:
        z[1] = np.float32(1.25)
    if B > 2:
        z[2] = (rng.randn(C) * 3 - 1000.0).astype(np.float32)
    if B > 3:
        z[3] = (rng.randn(C) * 3 * 300.0).astype(np.float32)
    if B > 4:
        z[4] = (np.clip(rng.randn(C) * 3, -6.5, 6.5) - 96.5).astype(np.float32)
        z[4, C - 1] = 0.0
        pi[4, ::2] = 0.0
    if B > 5:
        pi[5, rng.rand(C) < 0.5] = 0.0
        pi[5, 0] = max(pi[5, 0], 1e-3)
        pi[5] *= 0.5 / pi[5].sum()
    if B > 6:
        pi[6] = 0.0
    if B > 7:
        weight[7] = 0.0
    pi = pi.astype(np.float32)
    if B > 8:
        pi[8] *= np.float32(2.0)
    out = (z, value, pi, winner, weight)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def head_reference(B, C):
    """train_hip.loss_head_parts of head_case(B, C), computed once and shared."""
    with np.errstate(all="ignore"):
        return train_hip.loss_head_parts(*head_case(B, C))


def dlogits_interval(parts, pi, weight):
    """-> (lo, hi) float32 [B][C] of the rule, and e."""
    B = parts["dlogits"].shape[0]
    w, pi = np.asarray(weight, np.float64), np.asarray(pi, np.float64)
    e = E_REL * (w / B)[:, None] * (np.abs(pi) + np.exp(parts["logsm"]) * parts["psum"][:, None])
    ref = parts["dlogits"]
    with np.errstate(under="ignore"):                                   # (e = 0: the reference's own signed zero, not -0 + 0)
        return np.where(e > 0, ref - e, ref).astype(np.float32), np.where(e > 0, ref + e, ref).astype(np.float32), e


def _step_ratio(got, ref, e):
    """How far outside ref the kernel's fp64 result must have been for `got` to be its rounding, in units of e: 0 where got is
    float32(ref); otherwise the distance from ref to the rounding boundary on got's side of float32(ref), over e."""
    got64 = got.astype(np.float64)
    up = got > ref.astype(np.float32)
    other = np.nextafter(got, np.where(up, -np.inf, np.inf).astype(np.float32)).astype(np.float64)
    boundary = (got64 + other) / 2
    d = np.where(up, boundary - ref, ref - boundary)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(d <= 0, 0.0, np.where(e > 0, d / e, np.inf))


def check_loss_head(inputs, dlogits, dvalue, rows, what="", parts=None):
    """The rules of the module docstring on one case.  inputs: (logits, value, pi, winner, weight); dlogits [B][C] and dvalue
    [B] float32, rows [B][5] float64 as the kernel stored them.  -> dict(n, near, flips, worst, worst_rows, relative_only):
    elements, near elements, near elements that are not float32(ref), the worst _step_ratio, the worst |got - ref| / bound over
    the three bounded row terms, and the same over xent and ent against 2^-40 * sum |term| alone.  Raises AssertionError naming
    the first offender."""
    z, value, pi, winner, weight = inputs
    B, C = z.shape
    if parts is None:
        with np.errstate(all="ignore"):
            parts = train_hip.loss_head_parts(*inputs)
    dlogits, dvalue, rows = np.asarray(dlogits), np.asarray(dvalue), np.asarray(rows)
    assert dlogits.dtype == np.float32 and dvalue.dtype == np.float32 and rows.dtype == np.float64, what
    assert dlogits.shape == (B, C) and dvalue.shape == (B,) and rows.shape == (B, train_hip.ROW_TERMS), what
    ref = parts["dlogits"]
    r32 = ref.astype(np.float32)
    if C == 1:
        assert not r32.any(), what
        bad = bits32(dlogits) != bits32(r32)
        near = np.zeros_like(bad)
        worst = 0.0 if not bad.any() else np.inf
    else:
        lo, hi, e = dlogits_interval(parts, pi, weight)
        near = bits32(lo) != bits32(hi)
        bad = np.where(near, ~((dlogits >= lo) & (dlogits <= hi)), bits32(dlogits) != bits32(lo))
        off = bits32(dlogits) != bits32(r32)
        worst = float(_step_ratio(dlogits[off], ref[off], e[off]).max()) if off.any() else 0.0
    if bad.any():
        b, c = (int(v) for v in np.argwhere(bad)[0])
        raise AssertionError("%s dlogits: %d of %d elements outside their interval (rows %s); first at (%d, %d): got %r, reference %r"
                             % (what, int(bad.sum()), bad.size, sorted(set(np.argwhere(bad)[:, 0].tolist())), b, c,
                                float(dlogits[b, c]), float(ref[b, c])))
    flips = int((bits32(dlogits) != bits32(r32))[near].sum())
    # the exact quantities
    for name, got, want in (("dvalue", bits32(dvalue), bits32(parts["dvalue"].astype(np.float32))),
                            ("row_terms[:, 3] (vsq)", bits64(rows[:, 3]), bits64(parts["rows"][:, 3])),
                            ("row_terms[:, 1] (w * vsq)", bits64(rows[:, 1]), bits64(parts["rows"][:, 1]))):
        assert np.array_equal(got, want), "%s %s: rows %s differ from the reference's bits" % (what, name, np.flatnonzero(got != want).tolist())
    # the bounded ones
    p64, w = np.asarray(pi, np.float64), np.asarray(weight, np.float64)
    logsm = parts["logsm"]
    tol_x = E_REL * np.abs(p64 * logsm).sum(axis=1) + LOGSM_ABS * np.abs(p64).sum(axis=1)
    tol_e = E_REL * np.abs(np.exp(logsm) * logsm).sum(axis=1) + LOGSM_ABS * np.exp(logsm).sum(axis=1)
    tol_wx = np.abs(w) * tol_x + E_REL * np.abs(parts["rows"][:, 0])
    worst_rows = relative_only = 0.0
    for j, name, tol in ((2, "xent", tol_x), (4, "ent", tol_e), (0, "w * xent", tol_wx)):
        err = np.abs(rows[:, j] - parts["rows"][:, j])
        ok = err <= tol                                                 # a NaN is not ok
        assert ok.all(), "%s row_terms[:, %d] (%s): rows %s off by %s, bound %s" % (
            what, j, name, np.flatnonzero(~ok).tolist(), err[~ok].tolist(), tol[~ok].tolist())
        with np.errstate(divide="ignore", invalid="ignore"):
            worst_rows = max(worst_rows, float(np.where(err > 0, err / tol, 0.0).max()))
            if j:                                                       # reported, not asserted: the bound without its 2^-48 term
                rel = E_REL * np.abs((p64 if j == 2 else np.exp(logsm)) * logsm).sum(axis=1)
                relative_only = max(relative_only, float(np.where(err > 0, err / rel, 0.0).max()))
    return dict(n=int(bad.size) if C > 1 else 0, near=int(near.sum()), flips=flips, worst=worst, worst_rows=worst_rows,
                relative_only=relative_only)


def near_share():
    """Near elements over all HEAD_CASES (C = 1 aside) -> (near, elements)."""
    near = n = 0
    for B, C in HEAD_CASES:
        if C > 1:
            z, value, pi, winner, weight = head_case(B, C)
            lo, hi, _ = dlogits_interval(head_reference(B, C), pi, weight)
            near += int((bits32(lo) != bits32(hi)).sum())
            n += lo.size
    return near, n


def _lane_sum(x, valid):
    """Lane l adds its elements k = 0, 1, ... in that order (valid ones only), then the butterfly: x [B][K][64] -> [B]."""
    acc = np.zeros((x.shape[0], 64), x.dtype)
    for k in range(x.shape[1]):
        acc = np.where(valid[k], acc + x[:, k], acc)
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[:, lane ^ o]
    return acc[:, 0]


HEAD_FAULTS = ("fp32", "max0", "nomax", "psum1", "b4", "swap", "lane")


def head_model(inputs, fault=None, ulps=None):
    """A numpy model of af_train_loss_head_kernel<K> in the kernel's order -> (dlogits float32, dvalue float32, rows float64).
    fault: None, or one of HEAD_FAULTS —
        fp32   the softmax (exp, log, the sums) in fp32               max0   masked lanes contribute 0 to the row max
        nomax  no max subtraction                                     psum1  sum_c pi_c taken as 1
        b4     w / B with B rounded up to a multiple of 4             swap   the entropy and vsq slots exchanged
        lane   lane l's second element read from lane l + 1
    ulps: a RandomState; every exp and log result is then moved by up to +-2 ulp (the device's are not libm's)."""
    z, value, pi, winner, weight = inputs
    B, C = z.shape
    K = per_lane(C)
    T = np.float32 if fault == "fp32" else np.float64

    def lanes(a, fill):
        out = np.full((B, K * 64), fill, a.dtype)
        out[:, :C] = a
        return out.reshape(B, K, 64)

    def wobble(a):
        if ulps is None:
            return a
        return a + np.spacing(a) * ulps.randint(-2, 3, size=a.shape)

    valid = (np.arange(K * 64) < C).reshape(K, 64)
    with np.errstate(all="ignore"):
        zl, pr = lanes(z, np.float32(0)), lanes(pi, np.float32(0)).astype(T)
        mx = np.where(valid, zl, np.float32(0 if fault == "max0" else -np.inf)).max(axis=(1, 2))
        zr = zl.astype(T) - (T(0) if fault == "nomax" else mx.astype(T)[:, None, None])
        lse = wobble(np.log(_lane_sum(wobble(np.exp(zr)), valid)))
        logsm = zr - lse[:, None, None]
        sr = wobble(np.exp(logsm))
        xent, ent, psum = _lane_sum(pr * logsm, valid), _lane_sum(sr * logsm, valid), _lane_sum(pr, valid)
        xent, ent, psum = (a.astype(np.float64) for a in (xent, ent, psum))
        if fault == "psum1":
            psum = np.ones(B)
        w = np.asarray(weight, np.float64)
        dB = np.float64(-(-B // 4) * 4 if fault == "b4" else B)
        pd, sd = pr.astype(np.float64), sr.astype(np.float64)
        if fault == "lane" and K > 1:
            pd, sd = pd.copy(), sd.copy()
            pd[:, 1] = np.roll(np.where(valid[1], pd[:, 1], 0.0), -1, axis=1)       # a masked lane's registers hold 0
            sd[:, 1] = np.roll(np.where(valid[1], sd[:, 1], 0.0), -1, axis=1)
        dl = (-(w / dB)[:, None, None] * (pd - sd * psum[:, None, None])).astype(np.float32).reshape(B, K * 64)[:, :C]
        d = np.asarray(value, np.float64) - np.asarray(winner, np.float64)
        vsq = d * d
        dv = (((4.0 * w) / dB) * d).astype(np.float32)
        rows = np.stack([w * xent, w * vsq, xent, vsq, -ent], axis=1)
        if fault == "swap":
            rows[:, [3, 4]] = rows[:, [4, 3]]
    return np.ascontiguousarray(dl), dv, rows


# ------------------------------------------------------------------ Adam ------------------------------------------------------------------
ADAM_SIZES = (1, 63, 64, 65, 2047, 2048, 2049, 4096, 4097, 147456, 4096)
ADAM_DECAY = (True, False, True, True, False, True, True, False, True, True, True)
ADAM_STEPS = 4
PLANTED_VAR = 10                                                          # the last variable, under decay
# blocks of 256 elements of the planted variable: name -> what it holds (g is planted again at every step; p, m, v at the start)
PLANTED = ("g=1e-20,p=0", "g=1e-23,p=0", "g=3e19", "g=1e30", "g=+inf", "g=-inf", "g=nan", "p=-0,g=-0", "p=+0,g=+0", "p=-0,g=+0",
           "p=+0,g=-0", "p=1e-38,g~1e-42", "m,v subnormal,p=g=0", "m subnormal,v=1e4,p=g=0", "p=3e38", "ordinary")


def planted_block(name):
    i = PLANTED.index(name)
    return slice(256 * i, 256 * (i + 1))


def _plant_g(g, rng):
    sign = rng.choice([-1.0, 1.0], size=256).astype(np.float32)
    for name, val in (("g=1e-20,p=0", 1e-20), ("g=1e-23,p=0", 1e-23), ("g=3e19", 3e19), ("g=1e30", 1e30)):
        g[planted_block(name)] = np.float32(val) * sign
    g[planted_block("g=+inf")] = np.inf
    g[planted_block("g=-inf")] = -np.inf
    g[planted_block("g=nan")] = np.nan
    g[planted_block("p=-0,g=-0")] = -0.0
    g[planted_block("p=+0,g=+0")] = 0.0
    g[planted_block("p=-0,g=+0")] = 0.0
    g[planted_block("p=+0,g=-0")] = -0.0
    g[planted_block("p=1e-38,g~1e-42")] = np.float32(1e-42) * rng.randint(-3, 4, size=256).astype(np.float32)
    g[planted_block("m,v subnormal,p=g=0")] = 0.0
    g[planted_block("m subnormal,v=1e4,p=g=0")] = 0.0


@functools.lru_cache(maxsize=None)
def adam_case():
    """-> dict(sizes, decay, p, m, v: the state before step 1 (lists of float32 arrays), g: [step][variable], lr_t: [step])."""
    rng = np.random.RandomState(11)
    p = [(rng.randn(n) * 0.1).astype(np.float32) for n in ADAM_SIZES]
    m = [np.zeros(n, np.float32) for n in ADAM_SIZES]
    v = [np.zeros(n, np.float32) for n in ADAM_SIZES]
    pp, pm, pv = p[PLANTED_VAR], m[PLANTED_VAR], v[PLANTED_VAR]
    for name in ("g=1e-20,p=0", "g=1e-23,p=0", "p=+0,g=+0", "p=+0,g=-0", "m,v subnormal,p=g=0", "m subnormal,v=1e4,p=g=0"):
        pp[planted_block(name)] = 0.0
    pp[planted_block("p=-0,g=-0")] = -0.0
    pp[planted_block("p=-0,g=+0")] = -0.0
    pp[planted_block("p=1e-38,g~1e-42")] = np.float32(1e-38) * rng.choice([-1.0, 1.0], size=256).astype(np.float32)
    pp[planted_block("p=3e38")] = np.float32(3e38) * rng.choice([-1.0, 1.0], size=256).astype(np.float32)
    pm[planted_block("m,v subnormal,p=g=0")] = np.float32(1e-40) * rng.randint(-9, 10, size=256).astype(np.float32)
    pv[planted_block("m,v subnormal,p=g=0")] = np.float32(1e-41) * rng.randint(0, 10, size=256).astype(np.float32)
    pm[planted_block("m subnormal,v=1e4,p=g=0")] = np.float32(1e-40) * rng.randint(-9, 10, size=256).astype(np.float32)
    pv[planted_block("m subnormal,v=1e4,p=g=0")] = np.float32(1e4)
    grads = []
    for _ in range(ADAM_STEPS):
        gs = []
        for n in ADAM_SIZES:
            g = (rng.randn(n) * 1e-2).astype(np.float32)
            g[rng.rand(n) < 0.25] = 0.0                                   # with v = 0: m / eps, and 0 / eps
            gs.append(g)
        _plant_g(gs[PLANTED_VAR], rng)
        grads.append(gs)
    for a in p + m + v + [g for gs in grads for g in gs]:
        a.setflags(write=False)
    return dict(sizes=ADAM_SIZES, decay=ADAM_DECAY, p=p, m=m, v=v, g=grads, lr_t=[lr_t(t + 1) for t in range(ADAM_STEPS)])


def adam_step_reference(p, g, m, v, decay, lr_t_, fault=None, flip=None):
    """train_hip.adam_reference and l2_partials_reference over a list of variables -> (p, m, v, partials), or, with fault one of
    ADAM_FAULTS, a model of a kernel that has it: "eps" (eps inside the root), "decay" (variable `flip`'s flag flipped),
    "beta" (beta1 used for v), "order" (a chunk's p * p summed in index order)."""
    f = np.float32
    out_p, out_m, out_v, parts = [], [], [], []
    with np.errstate(all="ignore"):
        for i in range(len(p)):
            dec = bool(decay[i]) != (fault == "decay" and i == flip)
            if fault in ("eps", "beta"):
                gi = g[i] + f(L2) * p[i] if dec else g[i]
                mi = m[i] * f(BETA1) + gi * (f(1) - f(BETA1))
                b2 = f(BETA1) if fault == "beta" else f(BETA2)
                vi = v[i] * b2 + (gi * gi) * (f(1) - b2)
                den = np.sqrt(vi + f(EPS)) if fault == "eps" else np.sqrt(vi) + f(EPS)
                a = (p[i] - (f(lr_t_) * mi) / den, mi, vi)
            else:
                a = train_hip.adam_reference(p[i], g[i], m[i], v[i], dec, lr_t_, BETA1, BETA2, EPS, L2)
            out_p.append(a[0]), out_m.append(a[1]), out_v.append(a[2])
            if fault == "order" and dec:
                sq = p[i] * p[i]
                parts.append(np.array([np.cumsum(sq[c:c + train_hip.ADAM_CHUNK], dtype=f)[-1]
                                       for c in range(0, sq.size, train_hip.ADAM_CHUNK)], f))
            else:
                parts.append(train_hip.l2_partials_reference(p[i], dec))
    return out_p, out_m, out_v, np.concatenate(parts) if parts else np.zeros(0, f)


ADAM_FAULTS = ("eps", "decay", "beta", "order")


def check_bits(got, ref, what=""):
    """Bit for bit, signed zeros included; where the reference is NaN the value must be NaN (any NaN)."""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.dtype == ref.dtype == np.float32 and got.shape == ref.shape, (what, got.dtype, got.shape, ref.shape)
    nan = np.isnan(ref)
    bad = np.where(nan, ~np.isnan(got), bits32(got) != bits32(ref))
    if bad.any():
        i = np.flatnonzero(bad.reshape(-1))
        raise AssertionError("%s: %d of %d elements differ; first at %d: got %r, reference %r" %
                             (what, i.size, bad.size, int(i[0]), float(got.reshape(-1)[i[0]]), float(ref.reshape(-1)[i[0]])))
    return int(bad.size)


def check_adam(got, ref, what=""):
    """got, ref: (p, m, v, partials) as adam_step_reference returns them -> elements compared."""
    n = 0
    for name, gs, rs in zip("pmv", got[:3], ref[:3]):
        assert len(gs) == len(rs), what
        for i, (a, b) in enumerate(zip(gs, rs)):
            n += check_bits(a, b, "%s variable %d (%d elements) %s" % (what, i, b.size, name))
    return n + check_bits(got[3], ref[3], "%s l2_partials" % what)


def table_case(nvars):
    """nvars variables of 5 elements (the 64-variable table exactly full, one over, and three launches): (p, g, m, v, decay)."""
    rng = np.random.RandomState(500 + nvars)
    mk = lambda s: [(rng.randn(5) * s).astype(np.float32) for _ in range(nvars)]  # noqa: E731
    p, g, m = mk(0.1), mk(1e-2), mk(1e-3)
    v = [np.abs(a) for a in mk(1e-4)]
    return p, g, m, v, [i % 3 != 0 for i in range(nvars)]


# ------------------------------------------------------------------ finalize ------------------------------------------------------------------
FIN_B = (1, 255, 256, 257, 1000)
FIN_P = (0, 1, 255, 256, 257, 1500)
FIN_CASES = tuple((b, p) for b in FIN_B for p in FIN_P)


@functools.lru_cache(maxsize=None)
def finalize_case(B, P):
    """-> (row_terms float64 [B][5], l2_partials float32 [P]).  Per column: two thirds of the rows are pairs (x, -x) at random
    places, |x| = 10^U(-6, 6); the rest, of either sign, lie in the lowest decade.  The sum is that of the rest, about 1e-4,
    and the rounding errors of adds at 1e6, which depend on their order, are 1e-6 of it: they show in the fp32 results."""
    rng = np.random.RandomState(900 + 7 * B + P)
    rows = np.empty((B, train_hip.ROW_TERMS), np.float64)
    for j in range(train_hip.ROW_TERMS):
        x = 10.0 ** rng.uniform(-6, 6, size=B) * rng.choice([-1.0, 1.0], size=B)
        h = B // 3
        x[h:2 * h] = -x[:h]
        x[2 * h:] = 10.0 ** rng.uniform(-6, -5, size=B - 2 * h) * rng.choice([-1.0, 1.0], size=B - 2 * h)
        rows[:, j] = x[rng.permutation(B)]
    partials = (10.0 ** rng.uniform(-6, 6, size=P)).astype(np.float32)
    rows.setflags(write=False)
    partials.setflags(write=False)
    return rows, partials


def finalize_model(rows, partials, l2_coef, fault=None):
    """train_hip.finalize_reference, or a model of a kernel with a fault: "order" (every sum in index order), "half" (L not halved)."""
    if fault is None:
        return train_hip.finalize_reference(rows, partials, l2_coef)
    seq = lambda a: np.cumsum(np.concatenate([[0.0], np.asarray(a, np.float64)]))[-1]  # noqa: E731
    tree = lambda a: train_hip._strided_sum(a, np.float64)  # noqa: E731
    s_of = seq if fault == "order" else tree
    s = [s_of(rows[:, j]) for j in range(train_hip.ROW_TERMS)]
    L = s_of(np.asarray(partials, np.float32).astype(np.float64))
    dB = np.float64(rows.shape[0])
    l2 = np.float64(np.float32(l2_coef)) * (L if fault == "half" else L / 2.0)
    return np.array([(-(s[0] / dB) + 2.0 * (s[1] / dB)) + l2, -(s[2] / dB), s[3] / dB, s[4] / dB], np.float64).astype(np.float32)


FINALIZE_FAULTS = ("order", "half")


def check_finalize(got, rows, partials, l2_coef, what=""):
    check_bits(np.asarray(got), train_hip.finalize_reference(rows, partials, l2_coef), "%s terms" % what)
