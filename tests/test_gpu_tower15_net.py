"""DeepResNet(15) on the hand-written bf16 tower (csrc/af_tower_bf16.hip, Geo<15>): both ways of handing it weights write the
same bytes, the whole net meets the bar the 11x11 net is held to, and it plugs into the self-play engine and the training loop."""
import functools

import numpy as np
import pytest

import tower_gpu
from conftest import make_cfg
from tower_gpu import same_bits

pytestmark = pytest.mark.gpu
S, W, NPIX = 15, 128, 225
planes = functools.partial(tower_gpu.planes, S=S)    # random-stone positions [n, 3, 15, 15]


def weight_set(net, seed):
    """The net's variable shapes filled with bf16 values: Glorot-sized kernels and biases that are not zero."""
    import torch
    rng = np.random.default_rng(seed)
    out = {}
    for name, shape in net.variable_shapes().items():
        if name.endswith("bias"):
            a = rng.standard_normal(shape) * 0.1
        else:
            fan = int(np.prod(shape[1:])) if len(shape) == 4 else shape[0]
            a = (rng.random(shape) * 2 - 1) * np.sqrt(3.0 / fan)
        out[name] = torch.from_numpy(a.astype(np.float32)).bfloat16().float().numpy()
    return out


def test_host_setters_and_device_update_write_the_same_bytes():
    """A 2-block DeepResNet(15) packed through the host setters, and another — packed from other weights first — re-packed by
    set_variables_device from fp32 tensors holding the same values: byte-equal buffers, bit-equal eval_hip; a forward graph captured
    before the device update replays with the new weights (no address and no by-value kernel argument depends on a weight)."""
    import torch
    from alphafive_amd.network_deep import DeepResNet
    B = 33
    x = planes(B, seed=2)
    host = DeepResNet(S, blocks=2, width=W, device="cuda", seed=1)
    V0, V1 = weight_set(host, 40), weight_set(host, 41)
    assert V1["value/fc1/kernel"].shape == (900, 64) and V1["policy/fc/kernel"].shape == (3600, 225) and V1["policy/fc/bias"].shape == (225,)
    host.set_variables(V1)
    pv_host = host.select_backend("hip", B)
    want = tuple(t.clone() for t in pv_host(x))
    dev = DeepResNet(S, blocks=2, width=W, device="cuda", seed=2)
    dev.set_variables(V0)
    pv_dev = dev.select_backend("hip", B)
    try:
        tw = dev._tower
        old = tuple(t.clone() for t in dev.eval_hip(x))
        assert not same_bits(old, want)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, capture_error_mode="thread_local"):
            dev.eval_hip(x)
        g.replay()
        torch.cuda.synchronize()
        assert same_bits((tw.policy[:B], tw.value[:B]), old)
        before = tw.debug_weights()
        version = pv_dev.weights_version()
        dev.set_variables_device({k: torch.from_numpy(v).cuda() for k, v in V1.items()})
        assert pv_dev.weights_version() == version + 1
        a, b = tw.debug_weights(), host._tower.debug_weights()
        assert len(a) == len(b) == 4 * 2 + 12
        for i, (p, q, r) in enumerate(zip(a, b, before)):
            assert p is not None and q is not None and p.shape == q.shape and np.array_equal(p, q), f"buffer {i} differs between the two paths"
            assert p.shape == r.shape
        assert a[8 + 6].size == 225 * 8 * 64 * 16 and a[8 + 7].size == 57 * 2 * 64 * 16 and a[8 + 8].size == 256 * 4      # dense_wp, dense_wv, dense_pb
        assert np.array_equal(a[8 + 8].view(np.float32)[225:], np.full(31, -1.0e30, np.float32))     # the dead policy outputs' bias survives both
        assert same_bits(tuple(t.clone() for t in dev.eval_hip(x)), want)
        tw.policy.zero_()
        tw.value.zero_()
        g.replay()                                   # captured before the update: the new weights' outputs
        torch.cuda.synchronize()
        assert same_bits((tw.policy[:B], tw.value[:B]), want)
        del g
    finally:
        dev._tower.close()
        host._tower.close()


def _assert_no_worse_than_torch_bf16(net, x, p, v):
    """The bar of the deep bf16 net (tests/test_gpu_realnet.py, restated): there is no bit parity between two bf16 evaluations; per
    output, the hand-written path's error against an fp32 evaluation of the same bf16-valued weights is bounded by the error of the
    all-PyTorch bf16 path it replaces on the very same positions — mean <= 1.25x, max <= 2x (+ one bf16 ulp of the output range)."""
    import torch
    p32, v32 = net.eval_device(x, dtype=torch.float32)
    pt, vt = net.eval_device(x)
    for name, got, ref, tor, ulp in (("policy", p, p32, pt, 2.0 ** -9 * float(p32.max())), ("value", v, v32, vt, 2.0 ** -9)):
        e_hip, e_tor = (got.float() - ref).abs(), (tor.float() - ref).abs()
        print("deep 15x15 %s: |hip - fp32| mean %.3g max %.3g; |torch bf16 - fp32| mean %.3g max %.3g"
              % (name, e_hip.mean().item(), e_hip.max().item(), e_tor.mean().item(), e_tor.max().item()))
        assert e_hip.mean().item() <= 1.25 * e_tor.mean().item() + 1e-7, name
        assert e_hip.max().item() <= 2.0 * e_tor.max().item() + ulp, name
    assert p.argmax(1).eq(p32.argmax(1)).float().mean().item() >= pt.argmax(1).eq(p32.argmax(1)).float().mean().item() - 0.02


def test_whole_net_is_no_worse_than_the_pytorch_bf16_path():
    """The 8-block net end to end on 140 random-stone positions (280 half boards: more than one pass of the persistent grid), and
    batches 1 and 33 reproduce their rows of the 140-batch result bit for bit."""
    import torch
    from alphafive_amd.network_deep import DeepResNet
    net = DeepResNet(S, blocks=8, width=W, device="cuda", seed=5)
    net.set_variables(weight_set(net, 42))
    pv = net.select_backend("hip", 140)
    try:
        x = planes(140, seed=3)
        p, v = (t.clone() for t in pv(x))
        assert p.shape == (140, NPIX) and torch.isfinite(p).all() and torch.isfinite(v).all()
        assert (p.sum(1) - 1).abs().max().item() < 1e-5
        _assert_no_worse_than_torch_bf16(net, x, p, v)
        p33, v33 = (t.clone() for t in pv(x[:33].contiguous()))
        assert same_bits((p33, v33), (p[:33], v[:33]))
        for i in (0, 77, 139):
            p1, v1 = pv(x[i:i + 1].contiguous())
            assert same_bits((p1, v1), (p[i:i + 1], v[i:i + 1])), i
        for other in (net.eval_hip_torch_dense, net.eval_hip_torch_ends):        # the A/B pipelines run at this size too
            po, vo = other(x)
            assert po.shape == (140, NPIX) and (po.float() - p).abs().max().item() < 0.05 and (vo.float() - v).abs().max().item() < 0.1
    finally:
        net._tower.close()


def _engine(net, seed=2):
    from alphafive_amd.engine import SelfPlayEngine
    cfg = make_cfg(board_size=S, goal=5, simulation_per_step=30, upper_simulation_per_step=40)
    pv = net.select_backend("hip", 64)
    return SelfPlayEngine(cfg, 64, pv, device=0, seed=seed), pv


def test_deep15_evaluator_plugs_into_the_engine_eager_and_captured():
    """64 games of 15x15, 40 ticks eagerly, then the same 40 from a fresh engine as one eager tick + three replays of a 13-tick graph."""
    import torch
    from alphafive_amd.network_deep import DeepResNet
    net = DeepResNet(S, blocks=2, width=W, device="cuda", seed=6)
    counters = []
    for graph in (False, True):
        sp, pv = _engine(net)
        try:
            if graph:
                for _ in range(3):
                    sp.run_ticks_graph(13)
            else:
                sp.run_ticks(40)
            sp.check()
            assert sp.ticks == 40
            ct = sp.counters()
            assert ct["sims"] == ct["expands"] + ct["terminals"] and ct["plies"] == 64          # 30 sims -> one move each
            p, v = pv(sp.planes)
            assert p.dtype == torch.float32 and p.shape == (64, NPIX) and torch.isfinite(p).all() and torch.isfinite(v).all()
            assert (p.sum(1) - 1).abs().max().item() < 1e-3 and p.min().item() >= 0 and v.abs().max().item() <= 1.0
            counters.append(ct)
        finally:
            sp.close()
            net._tower.close()
    assert counters[0] == counters[1]


def test_closed_loop_trains_a_deep15_net_on_the_device(capsys, tmp_path):
    """train_loop(net=DeepResNet(15), weights_on_device=True): self-play on the tower, a Trainer on forward_train_deep, the new
    weights re-packed in place after every step."""
    import random
    from alphafive_amd import replay, train
    from alphafive_amd.engine import SelfPlayEngine
    from alphafive_amd.network_deep import DeepResNet
    random.seed(3)
    np.random.seed(3)
    cfg = make_cfg(board_size=S, goal=5, simulation_per_step=8, upper_simulation_per_step=12, batch_size=32)
    cfg.get_lr = lambda step: 1e-3
    cfg.ckpt_path = str(tmp_path / "ckpt")
    deep = DeepResNet(S, blocks=2, width=W, device="cuda", seed=7)
    before = {k: v.copy() for k, v in deep.variables.items()}
    pv = deep.select_backend("hip", 64)
    first, version = deep._tower, pv.weights_version()
    sp = SelfPlayEngine(cfg, 64, pv, device=0, seed=1)
    stack = replay.DeviceRandomStack(S, 60, device=0, draw_seed=21)
    tr = train.Trainer(deep.variables, S, device="cuda", forward=train.forward_train_deep, shapes=deep.variable_shapes())
    logs = []
    try:
        steps = train.train_loop(cfg, sp, deep, stack, tr, steps=2, log=logs.append, weights_on_device=True)
        capsys.readouterr()
        assert steps == 2 and len(logs) >= 1
        assert deep._tower is first and pv.weights_version() > version                      # re-packed in place
        after = deep.variables
        assert any(np.abs(after[k] - before[k]).max() > 0 for k in before)
        assert all(np.isfinite(v).all() for v in after.values())
        p, v = pv(sp.planes)
        assert p.shape == (64, NPIX) and bool(np.isfinite(p.cpu().numpy()).all())
    finally:
        sp.close()
        stack.close()
        first.close()
