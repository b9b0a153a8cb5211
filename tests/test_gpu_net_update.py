"""af_net_update_device: weights re-packed on the device, in place, must be the bytes af_net_set_variable + af_net_finalize make of
the same values — every weight-derived buffer of both conv paths and every scale — and therefore the same forward, bit for bit;
the update is ordered on its stream, all or nothing, refused under capture, and is what train_loop(weights_on_device=True) hands
the evaluator through ResNet.set_variables_device / net_hip.make_eval.

Both entry points end in the same device packers, so their agreement alone would say little: what pins the bytes is
tests/golden/packed_weight_digests.json, the digests of every buffer as the host packers those kernels replaced produced them
(tests/golden/make_packed_weight_digests.py)."""
import hashlib
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN

pytestmark = pytest.mark.gpu
W = os.path.join(GOLDEN, "alphaFive-6960.weights.npz")
N_FP32_BUFFERS, N_SPLIT_BUFFERS, N_SCALES = 37, 35, 25          # include/af_net.h: af_net_debug_weights / af_net_debug_scales
DIGESTS = os.path.join(GOLDEN, "packed_weight_digests.json")
_recorded = {}


def _assert_recorded_state(H, key, what):
    """every buffer of H and every scale is what the host packers made of weight set `key` (packed_weight_digests.json)"""
    if not _recorded:
        with open(DIGESTS) as f:
            _recorded.update(json.load(f))
    rec = _recorded[key]
    got = [hashlib.sha256(b.tobytes()).hexdigest() for b in H.debug_weights()]
    assert len(got) == len(rec["buffers"]), (what, len(got), len(rec["buffers"]))
    for i, (g, r) in enumerate(zip(got, rec["buffers"])):
        assert g == r, "%s: buffer %d is not the recorded one of %s" % (what, i, key)
    scales = [int(u) for u in H.debug_scales().view(np.uint32)]
    assert scales == rec["scales"], (what, key, scales, rec["scales"])


def _positions(S, B, seed=0):
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


def _random_weights(S, seed):
    """glorot kernels as a fresh net has them, and biases that are not zero (so that the bias buffers are told apart too)"""
    from alphafive_amd.network import random_variables
    v = random_variables(S, seed)
    rng = np.random.RandomState(1000 + seed)
    for k in v:
        if k.endswith("bias"):
            v[k] = (0.1 * rng.randn(*v[k].shape)).astype(np.float32)
    return v


def _weights(case):
    S, kind = case
    if kind == "ckpt":
        with np.load(W) as z:
            return {k: np.ascontiguousarray(z[k], np.float32) for k in z.files}
    return _random_weights(S, 1)


def _variant(v, variant):
    v = {k: a.copy() for k, a in v.items()}
    if variant == "scaled":             # power-of-two factors: the scale exponents of two groups move by +-3
        v["bone/block2_conv1/kernel"] *= np.float32(8.0)
        v["policy/block5_res/kernel"] *= np.float32(0.125)
    elif variant == "zero":             # an all-zero group: pick_scale's scale 1.0
        v["value/block3_conv2/kernel"][...] = 0.0
    return v


def _dev(v):
    import torch
    return {k: torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda() for k, a in v.items()}


def _pair(S, V, max_batch, check_changed=False, other=None):
    """A: V through the host path.  B: other weights through the host path, then V through the device update."""
    import torch
    from alphafive_amd import net_hip
    A = net_hip.HipNet(V, S, max_batch, "cuda")
    B = net_hip.HipNet(other if other is not None else _random_weights(S, 99), S, max_batch, "cuda")
    before = B.debug_weights() if check_changed else None
    src = _dev(V)
    ver = B.weights_version()
    B.load_device(src)
    assert B.weights_version() == ver + 1
    torch.cuda.synchronize()
    if check_changed:                           # (what is compared afterwards is not two untouched copies of one weight set)
        assert sum(int((a != b).any()) for a, b in zip(before, B.debug_weights())) > 30
    return A, B, src


def _assert_same_state(A, B, S):
    wa, wb = A.debug_weights(), B.debug_weights()
    split = S in (11, 15)
    assert len(wa) == len(wb) == N_FP32_BUFFERS + (N_SPLIT_BUFFERS if split else 0)
    for i, (a, b) in enumerate(zip(wa, wb)):
        assert a.size == b.size and a.size > 0, i
        diff = np.flatnonzero(a != b)
        assert diff.size == 0, "buffer %d: %d of %d bytes differ, first at %d" % (i, diff.size, a.size, diff[0])
    sa, sb = A.debug_scales(), B.debug_scales()
    assert sa.size == sb.size == (N_SCALES if split else 0)
    assert np.array_equal(sa.view(np.uint32), sb.view(np.uint32)), (sa, sb)
    return sa


CASES = [(11, "ckpt"), (11, "random"), (15, "random"), (9, "random")]


@pytest.mark.parametrize("variant", ["plain", "scaled", "zero"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "%dx%d-%s" % (c[0], c[0], c[1]))
def test_device_update_packs_the_bytes_of_the_host_path(case, variant):
    """A (host load), B (device update over other weights) and C (a second host load over other weights) hold the same, recorded
    bytes.  af_net_finalize packs in place into the buffers af_net_create made: C is where a byte that no packer rewrites would show."""
    from alphafive_amd import net_hip
    S = case[0]
    V = _variant(_weights(case), variant)
    other = _random_weights(S, 99)
    A, B, _ = _pair(S, V, 8, check_changed=True, other=other)
    C = net_hip.HipNet(other, S, 8, "cuda")
    key = "%dx%d-%s-%s" % (S, S, case[1], variant)
    try:
        C.load(V)
        scales = _assert_same_state(A, B, S)
        _assert_same_state(A, C, S)
        _assert_recorded_state(A, key, "A (af_net_finalize)")
        _assert_recorded_state(B, key, "B (af_net_update_device)")
        _assert_recorded_state(C, key, "C (af_net_finalize over other weights)")
        if variant == "zero" and scales.size:
            assert scales[1 + 5] == 1.0         # layer 5 = value/block3 conv2, its projection produced separately: an all-zero group
    finally:
        A.close()
        B.close()
        C.close()


def _forward(h, xt):
    p, v = h(xt)
    return p.cpu().numpy().copy(), v.cpu().numpy().copy()


def _assert_same_forward(A, B, xt, what):
    pa, va = _forward(A, xt)
    pb, vb = _forward(B, xt)
    assert np.isfinite(pa).all() and np.isfinite(va).all(), what
    assert np.array_equal(pa.view(np.uint32), pb.view(np.uint32)) and np.array_equal(va.view(np.uint32), vb.view(np.uint32)), what


@pytest.mark.parametrize("case", [(11, "ckpt"), (15, "random"), (9, "random")], ids=lambda c: "%dx%d-%s" % (c[0], c[0], c[1]))
def test_forward_after_device_update_equals_forward_after_host_load(case):
    import torch
    from alphafive_amd import net_hip
    S = case[0]
    A, B, _ = _pair(S, _variant(_weights(case), "scaled"), 512)
    try:
        x = torch.from_numpy(_positions(S, 512, seed=3)).cuda()
        for batch in (512, 1, 3, 8):            # 1, 3, 8 on 11x11: the single-launch small forward
            _assert_same_forward(A, B, x[:batch].contiguous(), "batch %d" % batch)
        if S == 11:
            assert A.small_forward_error() == 0 and B.small_forward_error() == 0
        try:
            net_hip.tune(0, 1)                  # the fp32 Winograd path reads the other set of buffers of the same handles
            for batch in (512, 3):
                _assert_same_forward(A, B, x[:batch].contiguous(), "fp32 path, batch %d" % batch)
        finally:
            net_hip.tune(0, 5)
        _assert_same_forward(A, B, x, "back on the default path")
    finally:
        A.close()
        B.close()


def test_update_is_ordered_on_its_stream_between_two_forwards():
    import torch
    from alphafive_amd import net_hip
    S, nb = 11, 64
    V0, V1 = _weights((11, "ckpt")), _random_weights(11, 5)
    H0, H1 = net_hip.HipNet(V0, S, nb, "cuda"), net_hip.HipNet(V1, S, nb, "cuda")
    H = net_hip.HipNet(V0, S, nb, "cuda")
    try:
        x = torch.from_numpy(_positions(S, nb, seed=4)).cuda()
        src = _dev(V1)
        outs = [(torch.zeros(nb, S * S, device="cuda"), torch.zeros(nb, device="cuda")) for _ in range(2)]
        torch.cuda.synchronize()
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):              # forward(V0), update to V1, forward(V1): queued back to back, no wait of ours between
            H.bind_outputs(*outs[0])
            H(x)
            H.load_device(src)
            H.bind_outputs(*outs[1])
            H(x)
        s.synchronize()
        for h, (p, v), what in ((H0, outs[0], "before"), (H1, outs[1], "after")):
            pr, vr = _forward(h, x)
            assert np.array_equal(p.cpu().numpy().view(np.uint32), pr.view(np.uint32)), what
            assert np.array_equal(v.cpu().numpy().view(np.uint32), vr.view(np.uint32)), what
        assert not np.array_equal(outs[0][1].cpu().numpy(), outs[1][1].cpu().numpy())
    finally:
        for h in (H, H0, H1):
            h.close()


def test_host_load_after_a_device_update_restores_the_first_weights_for_any_stream():
    """load(V0) -> load_device(V1) -> load(V0) on one handle: the recorded bytes of V0 again and V0's forward bit for bit — also for
    a forward queued on a fresh non-default stream right behind load(), with no wait of the test's own: af_net_finalize packs
    with kernels on the null stream out of the handle's staging area, and has to have finished them before it returns."""
    import torch
    from alphafive_amd import net_hip
    S, nb = 11, 8
    V0, V1 = _weights((11, "ckpt")), _random_weights(11, 5)
    H0 = net_hip.HipNet(V0, S, nb, "cuda")          # only ever sees V0
    H = net_hip.HipNet(V0, S, nb, "cuda")
    try:
        x = torch.from_numpy(_positions(S, nb, seed=9)).cuda()
        p0, v0 = _forward(H0, x)
        pa, va = _forward(H, x)
        assert np.array_equal(p0.view(np.uint32), pa.view(np.uint32)) and np.array_equal(v0.view(np.uint32), va.view(np.uint32))
        H.load_device(_dev(V1))
        p1, v1 = _forward(H, x)
        assert not np.array_equal(p0, p1) and not np.array_equal(v0, v1)
        out = (torch.zeros(nb, S * S, device="cuda"), torch.zeros(nb, device="cuda"))
        s = torch.cuda.Stream()
        torch.cuda.synchronize()                    # (x, out and the stream exist; nothing of ours waits from here to the forward)
        H.load(V0)
        with torch.cuda.stream(s):
            H.bind_outputs(*out)
            H(x)
        s.synchronize()
        p2, v2 = out[0].cpu().numpy(), out[1].cpu().numpy()
        assert np.array_equal(p0.view(np.uint32), p2.view(np.uint32)) and np.array_equal(v0.view(np.uint32), v2.view(np.uint32))
        _assert_recorded_state(H, "11x11-ckpt-plain", "load, load_device, load")
        p3, v3 = _forward(H, x)                     # ... and on the default stream
        assert np.array_equal(p0.view(np.uint32), p3.view(np.uint32)) and np.array_equal(v0.view(np.uint32), v3.view(np.uint32))
    finally:
        H.close()
        H0.close()


def test_host_load_waits_for_the_forwards_in_flight():
    """Four forwards with V0 queued on a fresh non-default stream, load(V1) from the host at once — no wait of the test's own —,
    then a fifth forward: the first four are V0's bit for bit, the fifth V1's.  af_net_finalize rewrites the packed weights in
    place, so it is the library that has to wait for what still reads them."""
    import torch
    from alphafive_amd import net_hip
    S, nb = 11, 64
    V0, V1 = _weights((11, "ckpt")), _random_weights(11, 5)
    H0, H1 = net_hip.HipNet(V0, S, nb, "cuda"), net_hip.HipNet(V1, S, nb, "cuda")
    H = net_hip.HipNet(V0, S, nb, "cuda")
    try:
        x = torch.from_numpy(_positions(S, nb, seed=4)).cuda()
        refs = [_forward(h, x) for h in (H0, H1)]
        outs = [(torch.zeros(nb, S * S, device="cuda"), torch.zeros(nb, device="cuda")) for _ in range(5)]
        s = torch.cuda.Stream()
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            for out in outs[:4]:
                H.bind_outputs(*out)
                H(x)
            H.load(V1)
            H.bind_outputs(*outs[4])
            H(x)
        s.synchronize()
        for i, (p, v) in enumerate(outs):
            pr, vr = refs[i // 4]
            assert np.array_equal(p.cpu().numpy().view(np.uint32), pr.view(np.uint32)), i
            assert np.array_equal(v.cpu().numpy().view(np.uint32), vr.view(np.uint32)), i
        assert not np.array_equal(refs[0][1], refs[1][1])
    finally:
        for h in (H, H0, H1):
            h.close()


def _synthetic_batch(rng, S, n=64):
    boards = (rng.rand(n, 3, S, S) < 0.2).astype(np.float32)
    pol = rng.rand(n, S * S).astype(np.float32)
    pol /= pol.sum(axis=1, keepdims=True)
    return boards, (0.5 + rng.rand(n)).astype(np.float32), np.sign(rng.randn(n)).astype(np.float32), pol


def test_hand_off_from_a_live_trainer_equals_a_fresh_handle(monkeypatch):
    import torch
    from alphafive_amd import net_hip
    from alphafive_amd.network import ResNet
    from alphafive_amd.train import Trainer
    S, nb = 11, 32
    net = ResNet(S, device="cuda")
    net.load_npz(W)
    trainer = Trainer(net.variables, S, device="cuda")
    pv = net.select_backend("hip")
    x = torch.from_numpy(_positions(S, nb, seed=6)).cuda()
    pv(x)                                       # builds the evaluator's handle (host path, once)
    calls = {"load": 0, "load_device": 0}
    for name in calls:
        real = getattr(net_hip.HipNet, name)
        monkeypatch.setattr(net_hip.HipNet, name, lambda self, t, _r=real, _n=name: (calls.__setitem__(_n, calls[_n] + 1), _r(self, t))[1])
    rng = np.random.RandomState(7)
    last = None
    try:
        for step in range(3):
            trainer.step(*_synthetic_batch(rng, S), lr=1e-3)
            net.set_variables_device(trainer.device_variables())
            trainer_now = trainer.variables()
            p, v = pv(x)
            p, v = p.cpu().numpy().copy(), v.cpu().numpy().copy()
            assert calls == {"load": 0, "load_device": step + 1}       # the evaluator took the device path, and only it
            fresh = net_hip.HipNet(trainer_now, S, nb, "cuda")
            calls["load"] -= 1                                           # (the fresh handle's own)
            try:
                pr, vr = _forward(fresh, x)
            finally:
                fresh.close()
            assert np.array_equal(p.view(np.uint32), pr.view(np.uint32)) and np.array_equal(v.view(np.uint32), vr.view(np.uint32)), step
            assert last is None or not np.array_equal(last, v)           # the weights moved
            last = v
            got = net.variables                                          # materialised from the device snapshot
            assert set(got) == set(trainer_now)
            for k, a in trainer_now.items():
                assert np.array_equal(a.view(np.uint32), got[k].view(np.uint32)), (step, k)
            # the torch-op evaluation follows too
            pt, vt = net.eval_torch(x)
            assert np.abs(pt.cpu().numpy() - pr).max() < 5e-5 and np.abs(vt.cpu().numpy() - vr).max() < 5e-5
    finally:
        net.close()


def test_refused_updates_change_nothing_and_capture_is_a_state_error():
    import torch
    from alphafive_amd import net_hip
    S, nb = 11, 8
    V0, V1 = _weights((11, "ckpt")), _random_weights(11, 5)
    H = net_hip.HipNet(V0, S, nb, "cuda")
    try:
        x = torch.from_numpy(_positions(S, nb, seed=8)).cuda()
        p0, v0 = _forward(H, x)
        w0, ver = H.debug_weights(), H.weights_version()
        src = _dev(V1)
        spare = torch.zeros(64, device="cuda")                          # a live tensor whose size is not value/conv/bias's
        missing = {k: t for k, t in src.items() if k != "policy/block4_conv2/kernel"}
        renamed = dict(missing, **{"policy/block4_conv2/kernel_": src["policy/block4_conv2/kernel"]})
        wrong_count = dict(src, **{"value/conv/bias": spare})
        for bad, code in ((missing, -1), (renamed, -3), (wrong_count, -3)):
            with pytest.raises(net_hip.NetError) as ei:
                H.load_device(bad)
            assert "code %d" % code in str(ei.value)
        g = torch.cuda.CUDAGraph()
        y = torch.zeros(4, device="cuda")
        torch.cuda.synchronize()
        with torch.cuda.graph(g, capture_error_mode="thread_local"):
            y.add_(1.0)
            with pytest.raises(net_hip.NetError) as ei:
                H.load_device(src)                                      # the call would wait for the stream: not capturable
            assert "code -4" in str(ei.value)
        torch.cuda.synchronize()
        assert H.weights_version() == ver
        p1, v1 = _forward(H, x)
        assert np.array_equal(p0.view(np.uint32), p1.view(np.uint32)) and np.array_equal(v0.view(np.uint32), v1.view(np.uint32))
        assert all(np.array_equal(a, b) for a, b in zip(w0, H.debug_weights()))
        # a good update goes through, and the host path still works on the same handle afterwards (load sets all 42 again)
        H.load_device(src)
        p2, _ = _forward(H, x)
        assert not np.array_equal(p0, p2)
        H.load(V0)
        p3, v3 = _forward(H, x)
        assert np.array_equal(p0.view(np.uint32), p3.view(np.uint32)) and np.array_equal(v0.view(np.uint32), v3.view(np.uint32))
    finally:
        H.close()
