"""The deep net (network_deep.DeepResNet, BASELINE configs[4]) as a net one can train and checkpoint: the parts that need no GPU.
Names, shapes and their order are the ABI of af_tower_update_device (include/af_tower_bf16.h); the training forward is the
evaluator's op sequence; Trainer and loss_terms take it without changing what their default callers get."""
import os

import numpy as np
import pytest
import torch

from alphafive_amd import network, network_deep, train

S, BLOCKS = 11, 2


def _net(seed=0, dtype=torch.float32):
    return network_deep.DeepResNet(S, blocks=BLOCKS, width=128, device="cpu", dtype=dtype, seed=seed)


def _perturbed(net, seed):
    """The net's variables with non-zero biases (the initialiser's are all zero) and shifted kernels."""
    rng = np.random.RandomState(seed)
    return {k: (v + rng.standard_normal(v.shape).astype(np.float32) * 0.05) for k, v in net.variables.items()}


def _planes(n, seed):
    rng = np.random.RandomState(seed)
    x = np.zeros((n, 3, S, S), np.float32)
    stones = rng.randint(0, 3, size=(n, S, S))
    x[:, 0], x[:, 1], x[:, 2] = stones == 1, stones == 2, 1.0
    return torch.from_numpy(x)


def test_variable_shapes_follow_the_update_abi():
    """12 + 6 * blocks entries in the order and with the element counts include/af_tower_bf16.h states for af_tower_update_device."""
    from alphafive_amd import tower_hip
    net = _net()
    shapes = net.variable_shapes()
    assert len(shapes) == 12 + 6 * BLOCKS
    names = list(shapes)
    assert names == tower_hip.update_names(BLOCKS)
    assert names[:2] == ["stem/kernel", "stem/bias"]
    assert names[2:8] == ["tower/block0_conv1/kernel", "tower/block0_conv1/bias", "tower/block0_conv2/kernel", "tower/block0_conv2/bias",
                          "tower/block0_res/kernel", "tower/block0_res/bias"]
    assert names[8:14] == [n.replace("block0", "block1") for n in names[2:8]]
    assert names[14:] == ["value/conv/kernel", "value/conv/bias", "policy/conv/kernel", "policy/conv/bias", "value/fc1/kernel",
                          "value/fc1/bias", "value/fc2/kernel", "value/fc2/bias", "policy/fc/kernel", "policy/fc/bias"]
    counts = [int(np.prod(s)) for s in shapes.values()]
    assert counts == [9600, 128] + [147456, 128, 147456, 128, 16384, 128] * BLOCKS + [512, 4, 2048, 16, 30976, 64, 64, 1, 234256, 121]
    assert shapes["stem/kernel"] == (128, 3, 5, 5) and shapes["tower/block1_res/kernel"] == (128, 128, 1, 1)       # OIHW
    assert shapes["value/fc1/kernel"] == (4 * S * S, 64) and shapes["policy/fc/kernel"] == (16 * S * S, S * S)     # [in][out]
    assert all(("bias" in n) == (len(s) == 1) for n, s in shapes.items())
    got = net.variables
    assert list(got) == names and all(got[n].shape == tuple(shapes[n]) and got[n].dtype == np.float32 for n in names)
    h = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "af_tower_bf16.h")).read()
    assert "af_tower_update_device(" in h and "af_tower_debug_weights(" in h


def test_training_forward_is_the_evaluators_op_sequence():
    """On a cpu fp32 net forward_train_deep gives eval_device(dtype=float32) exactly: value and softmax(logits) bit for bit."""
    net = _net(seed=3)
    net.set_variables(_perturbed(net, 1))
    x = _planes(5, 2)
    policy, value = net.eval_device(x, dtype=torch.float32)
    params = {k: torch.from_numpy(v) for k, v in net.variables.items()}
    with torch.no_grad():
        logits, v = train.forward_train_deep(params, x)
    assert logits.shape == (5, S * S) and v.shape == (5,)
    assert torch.equal(v, value)
    assert torch.equal(torch.softmax(logits, dim=1), policy)
    assert float(value.abs().max()) > 0 and float(policy.std()) > 0


def test_deep_trainer_lowers_the_loss_on_a_fixed_batch():
    net = _net(seed=4)
    tr = train.Trainer(net.variables, S, device="cpu", forward=train.forward_train_deep, shapes=net.variable_shapes())
    assert list(tr.params) == list(net.variable_shapes())
    rng = np.random.RandomState(7)
    n = 8
    boards = _planes(n, 8)
    pi = rng.dirichlet(np.ones(S * S) * 0.3, size=n).astype(np.float32)
    z = rng.choice([-1.0, 1.0], size=n).astype(np.float32)
    w = np.ones(n, np.float32)
    totals = []
    for _ in range(20):
        tr.step(boards, w, z, pi, 1e-3)
        with torch.no_grad():
            terms = train.loss_terms(tr.params, boards, torch.from_numpy(pi), torch.from_numpy(z), torch.from_numpy(w),
                                     forward=train.forward_train_deep)
        totals.append(float(terms["total"]))
    assert totals[-1] < totals[0] and np.isfinite(totals).all()
    # the L2 term leaves the biases out: exactly the kernels' half sums of squares
    l2 = sum(float((p.detach() ** 2).sum()) / 2 for k, p in tr.params.items() if "bias" not in k)
    with torch.no_grad():
        ce = -(torch.from_numpy(pi) * torch.log_softmax(train.forward_train_deep(tr.params, boards)[0], 1)).sum(1).mean()
    assert abs(float(terms["total"]) - (float(ce) + 2.0 * float(terms["value_loss"]) + 4e-5 * l2)) < 1e-4


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_npz_round_trip_is_bit_exact(tmp_path, dtype):
    a = _net(seed=5, dtype=dtype)
    a.set_variables(_perturbed(a, 2))
    path = str(tmp_path / "deep.npz")
    a.save_npz(path)
    b = _net(seed=6, dtype=dtype)
    assert any(not np.array_equal(x, y) for x, y in zip(a.variables.values(), b.variables.values()))
    b.load_npz(path)
    va, vb = a.variables, b.variables
    assert list(va) == list(vb)
    for k in va:
        assert va[k].dtype == np.float32 and np.array_equal(va[k].view(np.uint32), vb[k].view(np.uint32)), k
    x = _planes(3, 9)
    for got, ref in zip(b.eval_device(x), a.eval_device(x)):
        assert torch.equal(got, ref)


def test_set_variables_checks_names_and_shapes():
    net = _net()
    v = dict(net.variables)
    del v["tower/block1_res/bias"]
    with pytest.raises(KeyError):
        net.set_variables(v)
    v = dict(net.variables)
    v["value/fc2/kernel"] = v["value/fc2/kernel"].reshape(1, 64)
    with pytest.raises(ValueError):
        net.set_variables(v)


def test_set_variables_device_on_a_cpu_net_is_set_variables():
    a, b = _net(seed=1, dtype=torch.bfloat16), _net(seed=2, dtype=torch.bfloat16)
    new = _perturbed(a, 3)
    a.set_variables(new)
    b.set_variables_device({k: torch.from_numpy(v) for k, v in new.items()})
    for k, v in a.variables.items():
        assert np.array_equal(v.view(np.uint32), b.variables[k].view(np.uint32)), k
        assert np.array_equal(v.view(np.uint32) & 0xFFFF, np.zeros_like(v, np.uint32)), k      # a bf16 net holds bf16 values
    x = _planes(2, 4)
    for got, ref in zip(b.eval_device(x), a.eval_device(x)):
        assert torch.equal(got, ref)


def test_default_trainer_is_the_42_variable_net():
    shapes = network.variable_shapes(S)
    tr = train.Trainer(network.random_variables(S, seed=1), S, device="cpu")
    assert len(tr.params) == 42 and list(tr.params) == list(shapes)
    assert tr.forward is train.forward_train
    assert train.loss_terms.__defaults__ == (train.forward_train,)


def test_update_abi_refuses_null_arguments_before_any_hip_call():
    """af_tower_update_device / af_tower_debug_weights are exported and return AF_TOWER_ERR_ARG for a null handle or table: checked
    before anything touches the device, so it holds on a host without one."""
    import ctypes
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    L = ctypes.CDLL(os.path.join(repo, "alphafive_amd", "_lib", "libaf_tower.so"))
    vp = ctypes.c_void_p
    L.af_tower_update_device.argtypes = [vp, vp, ctypes.POINTER(vp), ctypes.POINTER(ctypes.c_int64), ctypes.c_int32]
    L.af_tower_debug_weights.argtypes = [vp, ctypes.c_int32, vp, ctypes.c_int64]
    L.af_tower_debug_weights.restype = ctypes.c_int64
    n = 12 + 6 * BLOCKS
    ptrs, counts = (vp * n)(), (ctypes.c_int64 * n)()
    assert L.af_tower_update_device(None, None, ptrs, counts, n) == -1
    assert L.af_tower_update_device(None, None, None, None, n) == -1
    assert L.af_tower_debug_weights(None, 0, None, 0) == -1
