"""Device-drawn minibatches on the GPU: af_replay_draw_kernel against its numpy specification (replay.draw_reference) bit for
bit — sizes off every tile, the cap, the tie at the selection threshold, a wrapped ring — the gather behind it against
af_replay_sample on the same triples, the call surface of DeviceRandomStack.draw_batches / get_data_device, and
train_loop(device_draws=True) end to end."""
import ctypes as C
import random

import numpy as np
import pytest

from alphafive_amd import replay
from alphafive_amd.replay import draw_reference

pytestmark = pytest.mark.gpu


def _positions(S, n, seed):
    """n random positions as af_replay_append takes them; values carry the position's serial number."""
    rng = np.random.RandomState(seed)
    boards = rng.randint(-1, 2, size=(n, S * S)).astype(np.int8)
    pol = rng.rand(n, S * S).astype(np.float32)
    last = rng.randint(-1, S * S, size=n).astype(np.int32)
    val = np.arange(n, dtype=np.float32)
    wts = rng.rand(n).astype(np.float32)
    return boards, pol, last, val, wts


def _append(st, pos, lo=0, hi=None):
    import torch
    boards, pol, last, val, wts = (np.ascontiguousarray(a[lo:hi]) for a in pos)
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int32)
    stream = torch.cuda.current_stream(st.device).cuda_stream
    replay._check(replay.lib().af_replay_append(st._h, stream, len(val), boards.ctypes.data_as(C.POINTER(C.c_int8)),
                                                pol.ctypes.data_as(fp), last.ctypes.data_as(ip), val.ctypes.data_as(fp),
                                                wts.ctypes.data_as(fp)), "af_replay_append")


def _stack(S, n, seed=0, draw_seed=0):
    st = replay.DeviceRandomStack(S, max(n, 1), device=0, draw_seed=draw_seed)
    pos = _positions(S, n, seed)
    if n:
        _append(st, pos)
    assert st._size() == n
    return st, pos


def _spec(n, num, batches, seed, draw):
    return np.stack(draw_reference(n, num, batches, seed, draw))          # int32[3][batches][k]


def _sample(st, idx, turns, flip):
    """af_replay_sample (the host-drawn path) on given triples -> the four tensors."""
    import torch
    S, num = st.board_size, len(idx)
    f32 = dict(dtype=torch.float32, device=st.device)
    out = (torch.empty((num, 3, S, S), **f32), torch.empty((num,), **f32), torch.empty((num,), **f32),
           torch.empty((num, S * S), **f32))
    ip = C.POINTER(C.c_int32)
    a = [np.ascontiguousarray(x, np.int32) for x in (idx, turns, flip)]
    replay._check(replay.lib().af_replay_sample(st._h, torch.cuda.current_stream(st.device).cuda_stream, num,
                                                a[0].ctypes.data_as(ip), a[1].ctypes.data_as(ip), a[2].ctypes.data_as(ip),
                                                *[t.data_ptr() for t in out]), "af_replay_sample")
    return out


def _same_bits(a, b):
    import torch
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.mark.parametrize("n, num, batches", [(1, 1, 1), (3, 8, 2), (64, 64, 1), (65, 64, 1), (200, 1, 3), (257, 100, 4),
                                             (300, 299, 1), (5000, 512, 4), (5000, 4096, 1)])
def test_draws_equal_the_specification(n, num, batches):
    S, seed = 5, 0x1234ABCD5678
    st, pos = _stack(S, n, seed=n, draw_seed=seed)
    st.draw_counter = 3
    boards, weights, values, policies, draws = st.draw_batches(num, batches, return_draws=True)
    k = min(n, num)
    assert boards.shape == (batches, k, 3, S, S) and weights.shape == values.shape == (batches, k)
    assert policies.shape == (batches, k, S * S) and draws.shape == (3, batches, k)
    want = _spec(n, num, batches, seed, 3)
    got = draws.cpu().numpy()
    assert got.dtype == np.int32 and np.array_equal(got, want)
    # ... and the gather took those positions (values carry the serial number, weights the position's own)
    assert np.array_equal(values.cpu().numpy(), want[0].astype(np.float32))
    assert np.array_equal(weights.cpu().numpy(), pos[4][want[0]])
    st.close()


@pytest.mark.parametrize("num, tail", [(1917, [18275, 9262, 1782]), (1918, [9262, 1782, 9966])])
def test_equal_words_at_the_threshold_go_to_the_lower_index(num, tail):
    """seed 0, draw 141, 20000 positions: the words of ranks 1916 and 1917 (positions 1782, 9966) are equal.  num = 1917 cuts
    between them: the kernel's rank-ordered tie branch."""
    st, _ = _stack(5, 20000)
    st.draw_counter = 141
    draws = st.draw_batches(num, 1, return_draws=True)[4].cpu().numpy()
    assert np.array_equal(draws, _spec(20000, num, 1, 0, 141))
    assert draws[0, 0, -3:].tolist() == tail and (num == 1918) == (9966 in draws[0, 0].tolist())
    assert st.draw_counter == 142
    st.close()


def test_wrapped_ring():
    """head > 0 and head + idx crosses the end of the ring: draws are on logical indices, the gather follows them round."""
    S = 5
    st = replay.DeviceRandomStack(S, 100, device=0, max_episode=10, draw_seed=9)          # ring of 120
    pos = _positions(S, 190, seed=4)
    _append(st, pos, 0, 120)
    st._drop_front(90)
    _append(st, pos, 120, 190)                              # the tail passes the end: slots 0..69
    assert st._size() == 100
    logical = [a[90:190] for a in pos]                      # what the ring holds, oldest first
    boards, weights, values, policies, draws = st.draw_batches(64, 2, return_draws=True)
    want = _spec(100, 64, 2, 9, 0)
    d = draws.cpu().numpy()
    assert np.array_equal(d, want)
    assert np.array_equal(values.cpu().numpy(), logical[3][want[0]]) and np.array_equal(weights.cpu().numpy(), logical[4][want[0]])
    for b in range(2):
        ref = _sample(st, d[0, b], d[1, b], d[2, b])
        assert all(_same_bits(x[b], y) for x, y in zip((boards, weights, values, policies), ref))
    st.close()


@pytest.mark.parametrize("S", [5, 11, 15, 3, 16])
def test_gather_is_af_replay_samples(S):
    """The returned (idx, turns, flip) fed to af_replay_sample give the very tensors draw_batches returned: the kernel against
    itself behind its two front ends, on the smallest board and on C = 256 = the workgroup size too (what af_replay_sample's
    tensors must be is tests/test_gpu_replay_exact.py's business)."""
    st, _ = _stack(S, 300, seed=S, draw_seed=S)
    for batches, num in ((1, 64), (4, 37)):
        got = st.draw_batches(num, batches, return_draws=True)
        d = got[4].cpu().numpy()
        assert ((d[1] >= 0) & (d[1] <= 3)).all() and set(np.unique(d[1]).tolist()) == {0, 1, 2, 3} and set(np.unique(d[2]).tolist()) == {0, 1}
        for b in range(batches):
            ref = _sample(st, d[0, b], d[1, b], d[2, b])
            assert all(_same_bits(x[b], y) for x, y in zip(got[:4], ref))
    st.close()


def test_counter_shapes_and_empty_stack():
    import torch
    S = 5
    random.seed(2)
    np.random.seed(2)
    st, _ = _stack(S, 80, draw_seed=5)
    assert st.draw_counter == 0
    a = st.draw_batches(16, 4)
    assert st.draw_counter == 1 and len(a) == 4
    b = st.get_data_device(16)
    assert st.draw_counter == 2
    host = st.get_data(16)                                  # the host-drawn path: untouched, and it does not move the counter
    assert st.draw_counter == 2
    assert [(t.shape, t.dtype, t.device) for t in b] == [(t.shape, t.dtype, t.device) for t in host]
    c = st.get_data_device(200)                             # more than the buffer holds: all 80, once each
    assert c[0].shape == (80, 3, S, S) and sorted(c[2].cpu().tolist()) == list(range(80))
    # a call is a function of (draw_seed, draw_counter): the same address draws the same minibatch, the next one another
    st.draw_counter = 1                                     # `b` was the second call
    assert all(_same_bits(x, y) for x, y in zip(st.get_data_device(16), b))
    assert not _same_bits(st.get_data_device(16)[2], b[2])  # counter 2
    st.draw_counter = 0                                     # ... and minibatch 0 of a call is what a call for one minibatch draws
    assert all(_same_bits(x, y[0]) for x, y in zip(st.get_data_device(16), a))
    with pytest.raises(ValueError):
        st.draw_batches(replay.MAX_DRAW + 1, 1)
    st.close()
    empty = replay.DeviceRandomStack(S, 10, device=0)
    e = empty.draw_batches(16, 4, return_draws=True)
    assert [tuple(t.shape) for t in e] == [(4, 0, 3, S, S), (4, 0), (4, 0), (4, 0, S * S), (3, 4, 0)]
    g = empty.get_data_device(16)
    assert [tuple(t.shape) for t in g] == [(0, 3, S, S), (0,), (0,), (0, S * S)] and all(t.dtype == torch.float32 for t in g)
    empty.close()


def test_outputs_stay_inside_their_arrays():
    """Through the C ABI, every output inside a larger poisoned tensor: the words before and behind it are untouched."""
    import torch
    S, n, num, batches, pad, poison = 5, 257, 100, 3, 512, 0x7FC0DEAD
    st, _ = _stack(S, n, seed=1)
    total = batches * num
    sizes = [total * 3 * S * S, total, total, total * S * S, 3 * total]
    bufs = [torch.full((sz + 2 * pad,), poison, dtype=torch.int32, device="cuda") for sz in sizes]
    ptrs = [b.data_ptr() + 4 * pad for b in bufs]
    stream = torch.cuda.current_stream(st.device).cuda_stream
    replay._check(replay.lib().af_replay_sample_device(st._h, stream, num, batches, 77, 5, *ptrs), "af_replay_sample_device")
    torch.cuda.synchronize()
    for b, sz in zip(bufs, sizes):
        assert bool((b[:pad] == poison).all()) and bool((b[pad + sz:] == poison).all())
        assert not bool((b[pad:pad + sz] == poison).any())                 # ... and every word inside was written
    assert np.array_equal(bufs[4][pad:pad + 3 * total].cpu().numpy().reshape(3, batches, num), _spec(n, num, batches, 77, 5))
    # a request the buffer cannot serve is refused, not clamped, at this level
    assert replay.lib().af_replay_sample_device(st._h, stream, n + 1, 1, 0, 0, *ptrs) == -4
    st.close()


def test_closed_loop_with_device_draws(capsys, tmp_path):
    """train_loop(device_draws=True, weights_on_device=True): self-play -> ring -> device-drawn minibatches -> trainer ->
    evaluator, the host only launching."""
    from alphafive_amd.engine import SelfPlayEngine
    from alphafive_amd.network import ResNet
    from alphafive_amd.train import Trainer, train_loop
    from conftest import make_cfg
    random.seed(3)
    np.random.seed(3)
    S = 6
    cfg = make_cfg(board_size=S, goal=4, simulation_per_step=16, upper_simulation_per_step=24, batch_size=64)
    cfg.get_lr = lambda step: 1e-3
    cfg.ckpt_path = str(tmp_path / "ckpt")
    net = ResNet(S, device="cuda", seed=0)
    before = {k: v.copy() for k, v in net.variables.items()}
    sp = SelfPlayEngine(cfg, 64, net.select_backend("hip"), device=0, seed=1)
    stack = replay.DeviceRandomStack(S, 120, device=0, draw_seed=21)
    tr = Trainer(net.variables, S, device="cuda")
    logs = []
    steps = train_loop(cfg, sp, net, stack, tr, steps=4, log=logs.append, device_draws=True, weights_on_device=True)
    capsys.readouterr()
    assert steps == 4 and len(logs) == 3 and all("xcross_loss" in s for s in logs)
    assert stack.draw_counter == 3 and tr.t == 12           # one draw of four minibatches per accepted episode on a full buffer
    stack.check()
    assert stack.is_full() and stack._size() <= 120
    after = tr.variables()
    assert any(np.abs(after[k] - before[k]).max() > 0 for k in before)
    assert all(np.isfinite(v).all() for v in after.values())
    sp.close()
    stack.close()
