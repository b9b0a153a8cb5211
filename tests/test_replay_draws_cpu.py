"""Device-drawn minibatches, the parts that need no GPU: the numpy specification replay.draw_reference (Philox known answer,
invariants, the draw counter, the tie at the selection threshold, uniformity), the C ABI of af_replay_sample_device (declared,
exported, bad arguments refused before any HIP call) and train_loop(device_draws=True)'s plumbing on a host-side stack."""
import ctypes
import os
import random
import re

import numpy as np
import pytest

from alphafive_amd import replay, utils
from alphafive_amd.network import ResNet
from alphafive_amd.replay import draw_reference, philox4x32_10
from alphafive_amd.train import Trainer, train_loop
from conftest import REPO
from test_net_update_cpu import S, _cfg, _StubEngine


def test_philox_known_answer():
    assert [int(w) for w in philox4x32_10(0, 0, 0, 0, 0, 0)] == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    # arrays broadcast, and every word of counter and key matters
    base = philox4x32_10(np.arange(4), 1, 2, 3, 4, 5)
    assert all(w.dtype == np.uint32 and w.shape == (4,) for w in base)
    for pos in range(1, 6):
        args = [np.arange(4), 1, 2, 3, 4, 5]
        args[pos] += 1
        assert not np.array_equal(philox4x32_10(*args)[0], base[0])
    assert np.array_equal(philox4x32_10(np.arange(4) + 2 ** 32, 1, 2, 3, 4 + 2 ** 32, 5)[0], base[0])     # 32-bit words


@pytest.mark.parametrize("n, num, batches", [(1, 1, 1), (3, 8, 2), (64, 64, 1), (300, 299, 3), (5000, 512, 4), (0, 4, 2)])
def test_draw_invariants(n, num, batches):
    idx, turns, flip = draw_reference(n, num, batches, seed=11, draw=5)
    k = min(n, num)
    for a in (idx, turns, flip):
        assert a.shape == (batches, k) and a.dtype == np.int32
    for b in range(batches):
        assert len(set(idx[b].tolist())) == k and (idx[b] >= 0).all() and (idx[b] < n).all()
    assert ((turns >= 0) & (turns <= 3)).all() and ((flip == 0) | (flip == 1)).all()
    if n and n <= num:                                       # fewer positions than asked for: all of them, once each
        assert all(sorted(idx[b].tolist()) == list(range(n)) for b in range(batches))
    # the definition itself, position by position, on the first minibatch
    if n:
        v = philox4x32_10(np.arange(n), 0, 5, replay.DRAW_TAG, 11, 0)
        key = [(int(w) << 32) | i for i, w in enumerate(v[0])]
        want = sorted(range(n), key=key.__getitem__)[:k]
        assert idx[0].tolist() == want
        assert turns[0].tolist() == [int(v[1][i]) >> 30 for i in want] and flip[0].tolist() == [int(v[2][i]) >> 31 for i in want]


def test_draw_counter_seed_and_batch_address_the_draw():
    a = draw_reference(500, 64, 3, seed=7, draw=9)
    b = draw_reference(500, 64, 3, seed=7, draw=9)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    assert not np.array_equal(a[0], draw_reference(500, 64, 3, seed=7, draw=10)[0])
    assert not np.array_equal(a[0], draw_reference(500, 64, 3, seed=8, draw=9)[0])
    assert not np.array_equal(a[0], draw_reference(500, 64, 3, seed=7 + (1 << 32), draw=9)[0])        # the key's second word
    assert not np.array_equal(a[0][0], a[0][1]) and not np.array_equal(a[0][1], a[0][2])
    # minibatch b does not depend on how many minibatches are drawn with it, nor sample j on how many samples
    assert np.array_equal(draw_reference(500, 64, 1, seed=7, draw=9)[0][0], a[0][0])
    assert np.array_equal(draw_reference(500, 10, 3, seed=7, draw=9)[0], a[0][:, :10])


def test_tie_at_the_selection_threshold_goes_to_the_lower_index():
    """seed 0, draw 141, 20000 positions, minibatch 0: positions 1782 and 9966 share the word 0x195ba320 and hold the sorted
    ranks 1916 and 1917 (found by search once; asserted here)."""
    w = philox4x32_10(np.array([1782, 9966]), 0, 141, replay.DRAW_TAG, 0, 0)[0]
    assert [int(x) for x in w] == [0x195BA320, 0x195BA320]
    idx = draw_reference(20000, 1917, 1, seed=0, draw=141)[0][0]
    assert idx[-3:].tolist() == [18275, 9262, 1782] and 9966 not in idx.tolist()
    idx = draw_reference(20000, 1918, 1, seed=0, draw=141)[0][0]
    assert idx[-3:].tolist() == [9262, 1782, 9966]


def test_draws_are_uniform():
    """25,600 minibatches of 7 out of 50 (deterministic: the figures are 50.76, 56.28 and 6.54), each chi-square below the
    p = 0.001 quantile of its distribution: 85.35 at 49 degrees of freedom, 24.32 at 7."""
    n, num = 50, 7
    counts, first, cells = np.zeros(n), np.zeros(n), np.zeros(8)
    for draw in range(400):
        idx, turns, flip = draw_reference(n, num, 64, seed=2026, draw=draw)
        counts += np.bincount(idx.ravel(), minlength=n)
        first += np.bincount(idx[:, 0], minlength=n)
        cells += np.bincount((turns * 2 + flip).ravel(), minlength=8)

    def chi2(c):
        e = c.sum() / len(c)
        return float(((c - e) ** 2 / e).sum())
    assert counts.sum() == 25600 * num and first.sum() == 25600
    assert chi2(counts) < 85.35 and chi2(first) < 85.35 and chi2(cells) < 24.32
    assert abs(chi2(counts) - 50.76) < 0.01 and abs(chi2(first) - 56.28) < 0.01 and abs(chi2(cells) - 6.54) < 0.01


# ---- C ABI ----
def test_header_declares_and_library_exports_the_device_draw():
    hdr = open(os.path.join(REPO, "include", "af_replay.h")).read()
    L = ctypes.CDLL(os.path.join(REPO, "alphafive_amd", "_lib", "libaf_replay.so"))
    assert re.search(r"\baf_replay_sample_device\s*\(", hdr) and hasattr(L, "af_replay_sample_device")
    assert re.search(r"#define\s+AF_REPLAY_MAX_DRAW\s+4096\b", hdr) and replay.MAX_DRAW == 4096
    assert re.search(r"#define\s+AF_REPLAY_DRAW_TAG\s+0x52504C59u", hdr) and replay.DRAW_TAG == 0x52504C59
    assert re.search(r"not meant for\s+(\*\s+)?stream capture", hdr)         # the ring state travels by value: part of the contract


def test_bad_arguments_are_refused_without_a_gpu():
    L = replay.lib()
    ERR_ARG, ERR_RANGE = -1, -4
    fake, out = ctypes.c_void_p(1), ctypes.c_void_p(64)     # never dereferenced: every call below is refused first
    call = L.af_replay_sample_device
    assert call(None, None, 8, 1, 0, 0, out, out, out, out, None) == ERR_ARG                  # null handle
    for hole in range(4):                                                                     # null outputs
        outs = [out] * 4
        outs[hole] = None
        assert call(fake, None, 8, 1, 0, 0, *outs, None) == ERR_ARG
    assert call(fake, None, 0, 1, 0, 0, out, out, out, out, None) == ERR_ARG                  # num 0
    assert call(fake, None, -3, 1, 0, 0, out, out, out, out, None) == ERR_ARG
    assert call(fake, None, 4097, 1, 0, 0, out, out, out, out, None) == ERR_RANGE             # num above AF_REPLAY_MAX_DRAW
    assert call(fake, None, 8, 0, 0, 0, out, out, out, out, None) == ERR_ARG                  # batches 0
    assert call(fake, None, 8, -1, 0, 0, out, out, out, out, None) == ERR_ARG


# ---- train_loop plumbing ----
class _HostDrawStack(utils.RandomStack):
    """The host RandomStack with draw_batches stated on draw_reference and get_data's augmentation (utils.py:127-145)."""

    def __init__(self, board_size, length, draw_seed=0):
        super().__init__(board_size, length)
        self.draw_seed, self.draw_counter, self.calls = draw_seed, 0, []

    def draw_batches(self, batch_size, batches, return_draws=False):
        Sz = self.board_size
        idx, turns, flip = draw_reference(len(self.data), batch_size, batches, self.draw_seed, self.draw_counter)
        self.draw_counter += 1
        self.calls.append((batch_size, batches, len(self.data)))
        num = idx.shape[1]
        boards = np.empty((batches, num, 3, Sz, Sz), np.float32)
        weights = np.empty((batches, num), np.float32)
        values = np.empty((batches, num), np.float32)
        policies = np.empty((batches, num, Sz * Sz), np.float32)
        for b in range(batches):
            for j in range(num):
                state, p, la, v, w = self.data[idx[b, j]]
                k = int(turns[b, j])
                board = np.rot90(utils.state_to_board(state, Sz), k=k)
                p = np.rot90(p, k=k)
                for _ in range(k if la is not None else 0):
                    la = (Sz - 1 - la[1], la[0])
                if flip[b, j]:
                    board, p = np.flip(board, axis=0), np.flip(p, axis=0)
                    la = None if la is None else (Sz - 1 - la[0], la[1])
                boards[b, j] = utils.board_to_inputs(board, last_action=la)
                weights[b, j], values[b, j], policies[b, j] = w, v, p.reshape(-1)
        return boards, weights, values, policies

    def get_data(self, batch_size=1):
        raise AssertionError("get_data called in a device_draws loop")


def _loop(tmp_path, stack, **kw):
    random.seed(4)
    np.random.seed(4)
    net = ResNet(S, device="cpu", seed=0)
    tr = Trainer(net.variables, S, device="cpu")
    seen = []
    real = tr.step
    tr.step = lambda boards, *a, **k: (seen.append(np.asarray(boards).copy()), real(boards, *a, **k))[1]
    step = train_loop(_cfg(tmp_path), _StubEngine(1), net, stack, tr, steps=4, log=lambda s: None, ckpt_every=1000, **kw)
    return step, tr, seen


def test_train_loop_device_draws_one_call_four_steps_per_episode(tmp_path, monkeypatch, capsys):
    monkeypatch.chdir(tmp_path)
    stack = _HostDrawStack(S, 60, draw_seed=3)
    step, tr, seen = _loop(tmp_path, stack, device_draws=True)
    capsys.readouterr()
    assert step == 4 and tr.t == 12                          # steps 2..4: three accepted episodes on a full buffer
    assert stack.draw_counter == 3 and [c[:2] for c in stack.calls] == [(16, 4)] * 3
    assert len(seen) == 12 and all(x.shape == (16, 3, S, S) for x in seen)
    # the four steps of an episode took the four slices of its one draw, in order: distinct minibatches of one buffer state
    assert all(not np.array_equal(seen[0], seen[i]) for i in (1, 2, 3))
    before = ResNet(S, device="cpu", seed=0).variables
    assert any(np.abs(tr.variables()[k] - before[k]).max() > 0 for k in before)


def test_train_loop_device_draws_needs_a_stack_that_draws(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    with pytest.raises(ValueError, match="draw_batches"):
        _loop(tmp_path, utils.RandomStack(S, 60), device_draws=True)


def test_train_loop_default_never_touches_draw_batches(tmp_path, monkeypatch, capsys):
    monkeypatch.chdir(tmp_path)

    class Stack(utils.RandomStack):
        def draw_batches(self, *a, **k):
            raise AssertionError("draw_batches called without device_draws")
    step, tr, seen = _loop(tmp_path, Stack(S, 60))
    capsys.readouterr()
    assert step == 4 and tr.t == 12 and len(seen) == 12
