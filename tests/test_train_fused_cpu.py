"""Trainer(fused=True), the parts that need no GPU: the guard, and the two numpy specifications the HIP kernels are held to on
the device (tests/test_gpu_train_fused.py) against what the eager Trainer and the fp64 restatement compute."""
import numpy as np
import pytest
import torch

from alphafive_amd import train, train_hip
from alphafive_amd.network import ResNet
from oracle import net_fp64
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
