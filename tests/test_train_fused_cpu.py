"""Trainer(fused=True), the parts that need no GPU: the guard, and the two numpy specifications the HIP kernels are held to on
the device (tests/test_gpu_train_fused.py) against what the eager Trainer and the fp64 restatement compute."""
import numpy as np
import pytest
import torch

from alphafive_amd import train, train_hip
from alphafive_amd.network import ResNet
from oracle import net_fp64
import train_cases as tc
from test_train_cpu import _batch

S, B, LR = 6, 32, 1e-3
BETA1, BETA2, EPS = 0.9, 0.999, 1e-8
LR_T1 = float(LR * np.sqrt(1.0 - BETA2) / (1.0 - BETA1))          # Trainer.step's lr_t at t = 1


def _decay(name):
    return "bias" not in name and "bn" not in name


def _l2(params):
    return sum((p ** 2).sum() / 2 for n, p in params.items() if _decay(n))


@pytest.fixture(scope="module")
def eager_step():
    """One eager CPU step from ResNet(6, seed=4): the state before, both gradients, the variables after."""
    net = ResNet(S, device="cpu", seed=4)
    tr = train.Trainer(net.variables, S, device="cpu")
    batch = _batch(S, B, seed=1)
    boards, weights, winner, pol = batch
    before = tr.variables()
    ps = list(tr.params.values())
    terms = train.loss_terms(tr.params, *(torch.from_numpy(a) for a in (boards, pol, winner, weights)))
    g_total = [g.numpy().copy() for g in torch.autograd.grad(terms["total"], ps, retain_graph=True)]
    g_data = [g.numpy().copy() for g in torch.autograd.grad(terms["total"] - 4e-5 * _l2(tr.params), ps)]
    metrics = tr.step(boards, weights, winner, pol, lr=LR)
    names = list(tr.params)
    return dict(net=net, batch=batch, before=before, after=tr.variables(), metrics=metrics,
                g_total=dict(zip(names, g_total)), g_data=dict(zip(names, g_data)))


def _spec_step(e, grads, decay):
    out = {}
    for k, p0 in e["before"].items():
        z = np.zeros_like(p0)
        out[k] = train_hip.adam_reference(p0, grads[k], z, z, decay(k), LR_T1, BETA1, BETA2, EPS, 4e-5)[0]
    return out


def test_fused_on_a_cpu_device_is_a_value_error():
    net = ResNet(S, device="cpu", seed=4)
    with pytest.raises(ValueError, match="CUDA/ROCm device"):
        train.Trainer(net.variables, S, device="cpu", fused=True)


def test_adam_reference_reproduces_the_eager_step(eager_step):
    """g from autograd of the eager total (the L2 gradient is in it), no decay in the specification."""
    got = _spec_step(eager_step, eager_step["g_total"], lambda k: False)
    for k, ref in eager_step["after"].items():
        assert got[k].dtype == np.float32 and got[k].shape == ref.shape
        np.testing.assert_allclose(got[k], ref, rtol=2e-5, atol=1e-8, err_msg=k)


def test_adam_reference_adds_the_l2_gradient_itself(eager_step):
    """g of the data terms alone (total - 4e-5 * l2), decay by the name rule: g' = g + l2_coef * p is the eager gradient."""
    assert any(np.abs(eager_step["g_total"][k] - eager_step["g_data"][k]).max() > 0 for k in eager_step["before"] if _decay(k))
    got = _spec_step(eager_step, eager_step["g_data"], _decay)
    for k, ref in eager_step["after"].items():
        np.testing.assert_allclose(got[k], ref, rtol=2e-5, atol=1e-8, err_msg=k)


def test_loss_head_reference_matches_the_fp64_restatement(eager_step):
    net = eager_step["net"]
    boards, weights, winner, pol = eager_step["batch"]
    params = {k: torch.from_numpy(v) for k, v in net.variables.items()}
    with torch.no_grad():
        logits, value = train.forward_train(params, torch.from_numpy(boards))
    dlogits, dvalue, rows = train_hip.loss_head_reference(logits.numpy(), value.numpy(), pol, winner, weights)
    assert dlogits.shape == (B, S * S) and dvalue.shape == (B,) and rows.shape == (B, train_hip.ROW_TERMS)
    l2_sum = sum((np.asarray(a, np.float64) ** 2).sum() for n, a in net.variables.items() if _decay(n))
    got = train_hip.terms_reference(rows, l2_sum)
    ref = net_fp64.loss_terms(net.variables, boards, pol, winner, weights)
    for k in ("total", "cross_entropy", "value_loss", "entropy"):
        assert abs(got[k] - ref[k]) < 2e-5 * max(1.0, abs(ref[k])), k
    # and the eager step logged the same four
    for k in ref:
        assert abs(eager_step["metrics"][k] - ref[k]) < 2e-5 * max(1.0, abs(ref[k])), k


def test_loss_head_reference_gradients_are_autograds(eager_step):
    """dlogits / dvalue of the specification = autograd of the data terms of train.loss_terms on two leaf tensors."""
    boards, weights, winner, pol = eager_step["batch"]
    rng = np.random.RandomState(3)
    logits = torch.tensor(rng.randn(B, S * S) * 3, dtype=torch.float64, requires_grad=True)
    value = torch.tensor(np.tanh(rng.randn(B)), dtype=torch.float64, requires_grad=True)
    t = train.loss_terms({}, None, *(torch.from_numpy(a).double() for a in (pol, winner, weights)),
                         forward=lambda params, x: (logits, value))
    gl, gv = torch.autograd.grad(t["total"], [logits, value])
    dlogits, dvalue, _ = train_hip.loss_head_reference(logits.detach().numpy(), value.detach().numpy(), pol, winner, weights)
    assert np.abs(dlogits - gl.numpy()).max() < 1e-14 and np.abs(dvalue - gv.numpy()).max() < 1e-14


def test_first_step_of_the_specification_lands_on_the_eager_one(eager_step):
    """The first step moves every element by about lr * sign(g) whatever |g| is, so where g is rounding noise the sign, and
    the step, is arbitrary: compare the elements whose eager |g| exceeds 1e-4 of their variable's largest."""
    got = _spec_step(eager_step, eager_step["g_data"], _decay)
    left_out = total = 0
    for k, ref in eager_step["after"].items():
        g = np.abs(eager_step["g_total"][k])
        keep = g > 1e-4 * g.max()
        left_out += int((~keep).sum())
        total += keep.size
        assert np.abs(got[k] - ref)[keep].max() <= 1e-3 * LR, k
    print("left out: %d of %d elements (%.3f %%)" % (left_out, total, 100.0 * left_out / total))
    assert left_out < 0.05 * total


# ---------------------------------------------------------------- the cases of tests/train_cases.py, on the references alone
def test_head_cases_reach_every_kernel_and_the_near_share_is_under_its_cap():
    assert {tc.per_lane(C) for _, C in tc.HEAD_CASES} == {1, 2, 4, 8, 16}
    for k in (1, 2, 4, 8):                                              # both sides of every lane-count boundary
        assert {64 * k - 1, 64 * k, 64 * k + 1} <= set(tc.HEAD_C)
    assert {1, 1023, 1024} <= set(tc.HEAD_C) and max(tc.HEAD_C) == train_hip.MAX_C
    near, n = tc.near_share()
    print("loss head cases: %d of %d dlogits elements near a rounding boundary (%.4f %%)" % (near, n, 100.0 * near / n))
    assert n == sum(B * C for B, C in tc.HEAD_CASES if C > 1) and near <= tc.NEAR_CAP * n


@pytest.mark.parametrize("C", [36, 129, 1024])
def test_every_planted_row_is_what_it_claims_to_be(C):
    z, value, pi, winner, weight = tc.head_case(9, C)
    z64, p64 = z.astype(np.float64), pi.astype(np.float64)
    assert np.abs(z[0]).max() == 40 and (pi[0] != 0).sum() == 1 and pi[0].sum() == 1
    assert (z[1] == z[1, 0]).all()
    assert z[2].max() < -980                                            # a row max of 0 underflows every exp
    assert z[3].max() > 89 * 3 and z[3].min() < -104 * 3                # fp32 exp overflows above 88.7 and is 0 below -103.9
    assert z[4].argmax() == C - 1 and (np.delete(z64[4], C - 1) <= z64[4, C - 1] - 90).all()
    assert (pi[5] == 0).any() and abs(p64[5].sum() - 0.5) < 1e-6
    assert not pi[6].any() and weight[7] == 0 and abs(p64[8].sum() - 2.0) < 1e-5
    assert set(np.unique(winner)) <= {-1.0, 1.0} and (np.abs(value) < 1).all() and (np.delete(weight, 7) >= 0.5).all()
    ref = tc.head_reference(9, C)
    assert np.isfinite(ref["dlogits"]).all() and np.isfinite(ref["rows"]).all()
    sub = np.abs(ref["dlogits"][4].astype(np.float32))
    assert ((sub > 0) & (sub < np.finfo(np.float32).tiny)).any()        # row 4 stores subnormal fp32 gradients


def test_the_kernel_order_model_meets_the_rule_with_exp_and_log_two_ulp_off():
    """The derivation of 2^-40 on the cases themselves: a numpy model in the kernel's summation order, every exp and log
    moved by up to +-2 ulp, stays inside every interval and bound."""
    rng = np.random.RandomState(5)
    total = dict(n=0, near=0, flips=0)
    worst = worst_rows = 0.0
    for B, C in tc.HEAD_CASES:
        for ulps in (None, rng) if C > 1 else (None,):                  # C = 1 rests on exp(0) = 1 and log(1) = 0 exactly
            r = tc.check_loss_head(tc.head_case(B, C), *tc.head_model(tc.head_case(B, C), ulps=ulps), what="model (%d, %d)" % (B, C),
                                   parts=tc.head_reference(B, C))
            worst, worst_rows = max(worst, r["worst"]), max(worst_rows, r["worst_rows"])
        for k in total:
            total[k] += r[k]
    print("kernel-order model, exp/log +-2 ulp: %(n)d elements, %(near)d near, %(flips)d of them not float32(ref)" % total,
          "worst step ratio %.3g, worst row-term ratio %.3g" % (worst, worst_rows))
    assert worst <= 1 and worst_rows <= 1


@pytest.mark.parametrize("fault,case", [("fp32", (9, 121)), ("max0", (9, 121)), ("nomax", (9, 121)), ("psum1", (9, 121)),
                                        ("b4", (9, 121)), ("swap", (9, 121)), ("lane", (9, 129)), ("b4", (5, 513)),
                                        ("max0", (3, 513)), ("psum1", (9, 1024))])
def test_check_loss_head_rejects_a_planted_fault(fault, case):
    inputs = tc.head_case(*case)
    tc.check_loss_head(inputs, *tc.head_model(inputs), what="sound", parts=tc.head_reference(*case))
    with pytest.raises(AssertionError) as e:
        tc.check_loss_head(inputs, *tc.head_model(inputs, fault=fault), what=fault, parts=tc.head_reference(*case))
    print(str(e.value)[:300])


@pytest.mark.parametrize("fault,rows", [("max0", [2]), ("nomax", [2, 3]),("psum1", [5, 6, 8])])
def test_a_fault_of_the_inputs_shows_on_the_rows_planted_for_it(fault, rows):
    """The planted rows are what catches these three: with only those rows taken from the faulty model, the check still fails;
    with them taken from the sound one, it passes (N(0, 3) rows with a normalised target cannot see the fault)."""
    inputs, parts = tc.head_case(9, 121), tc.head_reference(9, 121)
    good, bad = tc.head_model(inputs), tc.head_model(inputs, fault=fault)
    for r in rows:
        mixed = [g.copy() for g in good]
        for a, b in zip(mixed, bad):
            a[r] = b[r]
        with pytest.raises(AssertionError):
            tc.check_loss_head(inputs, *mixed, what="%s, row %d" % (fault, r), parts=parts)
    healed = [b.copy() for b in bad]
    for a, g in zip(healed, good):
        a[rows] = g[rows]
    if fault != "psum1":                                                # (sum pi = 1 only to fp32 rounding elsewhere: 1e-8 shows too)
        tc.check_loss_head(inputs, *healed, what="%s healed" % fault, parts=parts)


def test_adam_cases_hold_what_they_claim_and_numpy_keeps_subnormals():
    f = np.float32
    tiny = np.finfo(f).tiny
    assert 0 < f(1e-20) * f(1e-20) < tiny and f(4e-5) * f(1e-38) != 0   # no flush to zero on this host
    c = tc.adam_case()
    assert set(c["sizes"]) >= {1, 63, 64, 65, 2047, 2048, 2049, 4096, 4097, 147456} and len(set(c["decay"])) == 2
    p, m, v = c["p"], c["m"], c["v"]
    seen_sub_v = seen_inf_v = seen_nan = seen_sub_l2 = False
    with np.errstate(all="ignore"):
        for t in range(tc.ADAM_STEPS):
            g = c["g"][t][tc.PLANTED_VAR]
            gg = g * g
            assert ((gg > 0) & (gg < tiny)).any() and np.isinf(gg[tc.planted_block("g=3e19")]).all() and np.isnan(g).any()
            assert np.signbit(g[tc.planted_block("p=-0,g=-0")]).all() and not g[tc.planted_block("p=-0,g=-0")].any()
            l2p = f(tc.L2) * p[tc.PLANTED_VAR]
            seen_sub_l2 |= bool(((np.abs(l2p) > 0) & (np.abs(l2p) < tiny)).any())
            p, m, v, parts = tc.adam_step_reference(p, c["g"][t], m, v, c["decay"], c["lr_t"][t])
            pv = v[tc.PLANTED_VAR]
            seen_sub_v |= bool(((pv > 0) & (pv < tiny)).any())
            seen_inf_v |= bool(np.isinf(pv).any())
            seen_nan |= bool(np.isnan(p[tc.PLANTED_VAR]).any())
            assert parts.size == sum(-(-n // train_hip.ADAM_CHUNK) for n in c["sizes"])
            assert not np.isfinite(parts[-2:]).all() and np.isfinite(parts[:-2]).all()   # only the planted variable's
            if t == 0:                                                  # signed zeros survive a step
                for name in ("p=-0,g=-0", "p=-0,g=+0"):
                    assert np.signbit(p[tc.PLANTED_VAR][tc.planted_block(name)]).all()
                for name in ("p=+0,g=+0", "p=+0,g=-0"):
                    assert not np.signbit(p[tc.PLANTED_VAR][tc.planted_block(name)]).any()
                q = p[tc.PLANTED_VAR][tc.planted_block("m subnormal,v=1e4,p=g=0")]
                assert ((np.abs(q) > 0) & (np.abs(q) < tiny)).any()     # a subnormal quotient
    assert seen_sub_v and seen_inf_v and seen_nan and seen_sub_l2
    assert all(np.isfinite(a).all() for a in p[:tc.PLANTED_VAR])


def test_the_reduction_references_agree_with_fsum_within_the_blocking_bound():
    """l2_partials_reference: no term passes through more than 8 + 6 + 3 adds and its own square, far inside the bound
    tests/test_gpu_train_fused.py:_check_l2 derives for any blocking of a chunk (2048 + 1 roundings of fp32).
    finalize_reference: the same for fp64 sums of B (P) entries, against sum |x| because the cases cancel, plus the one fp32
    rounding of each result."""
    import math
    U = 2.0 ** -24
    rng = np.random.RandomState(8)
    for n in (1, 255, 2048, 2049, 10000):
        p = (rng.randn(n) * 10.0 ** rng.uniform(-3, 3, size=n)).astype(np.float32)
        got = train_hip.l2_partials_reference(p, True)
        assert got.dtype == np.float32 and got.shape == (-(-n // 2048),) and not train_hip.l2_partials_reference(p, False).any()
        d = train_hip.ADAM_CHUNK + 1
        for k, c in enumerate(range(0, n, 2048)):
            exact = math.fsum(float(x) ** 2 for x in p[c:c + 2048])
            assert abs(float(got[k]) - exact) <= d * U / (1 - d * U) * exact, (n, k)
    assert train_hip.l2_partials_reference(np.zeros(0, np.float32), True).shape == (0,)
    u64, differs = 2.0 ** -53, 0
    for B, P in tc.FIN_CASES:
        rows, partials = tc.finalize_case(B, P)
        got = train_hip.finalize_reference(rows, partials, tc.L2)
        assert got.dtype == np.float32 and got.shape == (4,)
        s = [math.fsum(rows[:, j]) for j in range(5)]
        a = [math.fsum(np.abs(rows[:, j])) for j in range(5)]
        L = math.fsum(float(x) for x in partials)
        l2 = float(np.float32(tc.L2))
        exact = [-s[0] / B + 2 * s[1] / B + l2 * L / 2, -s[2] / B, s[3] / B, s[4] / B]
        slack = [(a[0] + 2 * a[1]) / B + l2 * L / 2, a[2] / B, a[3] / B, a[4] / B]
        d = max(B, P) + 8
        for k in range(4):
            assert abs(float(got[k]) - exact[k]) <= U * abs(exact[k]) + d * u64 * slack[k] * 1.001, (B, P, k)
        # the order matters: numpy's own (pairwise) sum of the same columns gives other bits
        plain = np.array([(-(rows[:, 0].sum() / B) + 2.0 * (rows[:, 1].sum() / B)) + l2 * (partials.astype(np.float64).sum() / 2.0),
                          -(rows[:, 2].sum() / B), rows[:, 3].sum() / B, rows[:, 4].sum() / B]).astype(np.float32)
        differs += int((tc.bits32(plain) != tc.bits32(got)).any())
    print("finalize cases on which a plain np.sum gives other bits: %d of %d" % (differs, len(tc.FIN_CASES)))
    assert differs >= 1


@pytest.mark.parametrize("fault", tc.ADAM_FAULTS)
def test_check_adam_rejects_a_planted_fault(fault):
    c = tc.adam_case()
    ref = tc.adam_step_reference(c["p"], c["g"][0], c["m"], c["v"], c["decay"], c["lr_t"][0])
    assert tc.check_adam(ref, ref, "sound") == 3 * sum(c["sizes"]) + ref[3].size
    for flip in ((0, 4, tc.PLANTED_VAR) if fault == "decay" else (None,)):   # a one-element variable's flag is enough
        with pytest.raises(AssertionError):
            tc.check_adam(tc.adam_step_reference(c["p"], c["g"][0], c["m"], c["v"], c["decay"], c["lr_t"][0], fault=fault, flip=flip),
                          ref, fault)


@pytest.mark.parametrize("fault", tc.FINALIZE_FAULTS)
def test_check_finalize_rejects_a_planted_fault(fault):
    caught = 0
    for B, P in tc.FIN_CASES:
        rows, partials = tc.finalize_case(B, P)
        tc.check_finalize(tc.finalize_model(rows, partials, tc.L2), rows, partials, tc.L2, "sound")
        try:
            tc.check_finalize(tc.finalize_model(rows, partials, tc.L2, fault=fault), rows, partials, tc.L2, fault)
        except AssertionError:
            caught += 1
    print("finalize fault %r: rejected on %d of %d cases" % (fault, caught, len(tc.FIN_CASES)))
    # the order shows wherever a thread adds more than one entry or the tree pairs other entries than a chain: B > 2;
    # the halving wherever there are partials
    assert caught >= (len(tc.FIN_B) - 1) * len(tc.FIN_P) if fault == "order" else caught == len(tc.FIN_B) * (len(tc.FIN_P) - 1)


def test_the_library_refuses_bad_arguments_before_any_hip_call():
    """Checked before anything touches the device, so it holds on a host without one."""
    import ctypes as C
    L = train_hip.lib()
    arr = (train_hip.Var * 65)()
    for e in arr:
        e.p = e.g = e.m = e.v = 64                                   # never dereferenced: every call below is refused
        e.n = 8
    args = (0.1, BETA1, BETA2, EPS, 4e-5)
    assert L.af_train_adam(None, 65, arr, *args, 64) == train_hip.ERR_ARG
    assert L.af_train_adam(None, 0, arr, *args, 64) == train_hip.ERR_ARG
    assert L.af_train_adam(None, 1, None, *args, 64) == train_hip.ERR_ARG
    assert L.af_train_adam(None, 1, arr, *args, None) == train_hip.ERR_ARG
    arr[0].m = None
    assert L.af_train_adam(None, 1, arr, *args, 64) == train_hip.ERR_ARG
    arr[0].m, arr[0].n = 64, -1
    assert L.af_train_adam(None, 1, arr, *args, 64) == train_hip.ERR_ARG
    arr[0].n = 2 ** 31
    assert L.af_train_adam(None, 1, arr, *args, 64) == train_hip.ERR_RANGE
    assert L.af_train_loss_head(None, 1, 1025, 64, 64, 64, 64, 64, 64, 64, 64) == train_hip.ERR_RANGE
    assert L.af_train_loss_head(None, 1, 4, 64, None, 64, 64, 64, 64, 64, 64) == train_hip.ERR_ARG
    assert L.af_train_finalize(None, 0, 64, 0, None, 0.0, 64) == train_hip.ERR_ARG
    assert L.af_train_adam_partials(3, (C.c_int64 * 3)(1, 2048, 2049)) == 4
    assert train_hip.adam_partials([128 * 128 * 9, 0, 5]) == 73
    assert L.af_train_strerror(train_hip.ERR_RANGE) == b"size out of range"
