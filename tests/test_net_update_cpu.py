"""Weights handed to the evaluator on the device, the parts that need no GPU: af_net.h declares af_net_update_device and its two
read-backs and libaf_net.so exports them, null arguments are refused before any HIP call, and train_loop(weights_on_device=True)
on a cpu net walks the same path as the default loop — same step, same trainer bits, net.variables equal to the trainer's —
without ever calling Trainer.variables()."""
import ctypes
import os
import random
import re

import numpy as np

from alphafive_amd import utils
from alphafive_amd.network import ResNet, random_variables, variable_shapes
from alphafive_amd.train import Trainer, train_loop
from conftest import REPO, make_cfg

S = 6


def _lib():
    L = ctypes.CDLL(os.path.join(REPO, "alphafive_amd", "_lib", "libaf_net.so"))
    vp = ctypes.c_void_p
    L.af_net_update_device.argtypes = [vp, vp, ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(vp), ctypes.POINTER(ctypes.c_int64),
                                       ctypes.c_int32]
    L.af_net_update_device.restype = ctypes.c_int
    L.af_net_debug_weights.argtypes = [vp, ctypes.c_int32, vp, ctypes.c_int64]
    L.af_net_debug_weights.restype = ctypes.c_int64
    L.af_net_debug_scales.argtypes = [vp, ctypes.POINTER(ctypes.c_float), ctypes.c_int32]
    L.af_net_debug_scales.restype = ctypes.c_int32
    return L


def test_header_declares_and_library_exports_the_device_update():
    hdr = open(os.path.join(REPO, "include", "af_net.h")).read()
    L = ctypes.CDLL(os.path.join(REPO, "alphafive_amd", "_lib", "libaf_net.so"))
    for name in ("af_net_update_device", "af_net_debug_weights", "af_net_debug_scales"):
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
        assert hasattr(L, name), name
    # the one host wait and the capture rule are part of the contract
    assert re.search(r"synchronises\s+`stream`\s+once", hdr) and "captured" in hdr


def test_null_arguments_are_refused_without_a_gpu():
    L = _lib()
    ERR_ARG = -1
    names = (ctypes.c_char_p * 1)(b"bone/conv1/bias")
    ptrs = (ctypes.c_void_p * 1)(None)
    counts = (ctypes.c_int64 * 1)(32)
    assert L.af_net_update_device(None, None, names, ptrs, counts, 1) == ERR_ARG            # null handle
    assert L.af_net_update_device(None, None, None, None, None, 42) == ERR_ARG
    fake = ctypes.c_void_p(1)           # a non-null handle is never dereferenced when an array is null
    assert L.af_net_update_device(fake, None, None, ptrs, counts, 1) == ERR_ARG
    assert L.af_net_update_device(fake, None, names, None, counts, 1) == ERR_ARG
    assert L.af_net_update_device(fake, None, names, ptrs, None, 1) == ERR_ARG
    assert L.af_net_debug_weights(None, 0, None, 0) == ERR_ARG
    assert L.af_net_debug_scales(None, None, 0) == ERR_ARG


class _StubEngine(object):
    """pop_episodes() of random 6x6 episodes in the record format: what train_loop needs of an engine on the host path."""

    def __init__(self, seed):
        self.rng = np.random.RandomState(seed)

    def run_ticks(self, n):
        pass

    def check(self):
        pass

    def _episode(self):
        rng = self.rng
        T = int(rng.randint(20, 34))
        board = np.zeros((S, S), np.int8)
        rec, la = [], None
        w = utils.construct_weights(T, 0.94)
        for t in range(T):
            p = rng.rand(S, S).astype(np.float32)
            p /= p.sum()
            rec.append((utils.board_to_state(board), p, la, float((-1.0) ** (T - t)), w[t]))
            empt = np.argwhere(board == 0)
            la = tuple(int(v) for v in empt[rng.randint(len(empt))])
            board = utils.step(board, la)
        return rec, (utils.BLACK_WIN if T % 2 == 1 else utils.WHITE_WIN)

    def pop_episodes(self):
        return [self._episode() for _ in range(3)]


def _cfg(tmp_path):
    cfg = make_cfg(board_size=S, goal=4, batch_size=16)
    cfg.get_lr = lambda step: 1e-3
    cfg.ckpt_path = str(tmp_path / "ckpt")
    return cfg


def _bits(d):
    return {k: np.asarray(a, np.float32).view(np.uint32).copy() for k, a in d.items()}


def _same(a, b):
    a, b = _bits(a), _bits(b)
    return a.keys() == b.keys() and all(np.array_equal(a[k], b[k]) for k in a)


def _run(tmp_path, on_device, **kw):
    random.seed(4)
    np.random.seed(4)
    net = ResNet(S, device="cpu", seed=0)
    tr = Trainer(net.variables, S, device="cpu")
    extra = dict(weights_on_device=True) if on_device else {}
    step = train_loop(_cfg(tmp_path), _StubEngine(1), net, utils.RandomStack(S, 60), tr, steps=4, log=lambda s: None, **extra, **kw)
    return step, net, tr


def test_train_loop_on_device_hand_off_equals_the_default_loop_on_cpu(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    step_a, net_a, tr_a = _run(tmp_path, False)
    start = _bits(random_variables(S, 0))

    calls = []
    real = Trainer.variables
    monkeypatch.setattr(Trainer, "variables", lambda self: (calls.append(1), real(self))[1])
    step_b, net_b, tr_b = _run(tmp_path, True, ckpt_every=1000)
    n_calls = len(calls)                                    # (the comparisons below call it themselves)
    monkeypatch.setattr(Trainer, "variables", real)

    assert step_a == step_b == 4 and tr_a.t == tr_b.t == 12         # 4 minibatches per step, steps 2..4
    assert _same(tr_a.variables(), tr_b.variables())        # the hand-off does not touch the training arithmetic
    assert not _same(tr_b.variables(), {k: v.view(np.float32) for k, v in start.items()})       # ... and the weights did move
    assert _same(net_b.variables, tr_b.variables())         # the evaluator's net follows the trainer
    assert _same(net_a.variables, net_b.variables)
    assert n_calls == 0                                     # no parameter left the trainer's device on the way


def test_set_variables_device_checks_names_and_shapes_like_set_variables():
    import pytest
    import torch
    net = ResNet(S, device="cpu", seed=0)
    v0 = net.version
    good = {k: torch.from_numpy(v) for k, v in random_variables(S, 3).items()}
    net.set_variables_device(good)
    assert net.version == v0 + 1 and _same(net.variables, random_variables(S, 3))
    x = torch.rand(2, 3, S, S)
    ref = ResNet(S, device="cpu", seed=3)
    assert all(torch.equal(a, b) for a, b in zip(net.eval_torch(x), ref.eval_torch(x)))
    missing = dict(good)
    del missing["policy/fc/bias"]
    with pytest.raises(KeyError):
        net.set_variables_device(missing)
    bad = dict(good)
    bad["value/fc2/kernel"] = torch.zeros(64)
    with pytest.raises(ValueError):
        net.set_variables_device(bad)
    assert net.version == v0 + 1 and set(net.variables) == set(variable_shapes(S))
    # Trainer.device_variables: the parameters themselves, detached, not copies
    tr = Trainer(random_variables(S, 0), S, device="cpu")
    dv = tr.device_variables()
    assert set(dv) == set(tr.params)
    assert all(dv[k].data_ptr() == tr.params[k].data_ptr() and not dv[k].requires_grad for k in dv)
