"""Stop and continue without a GPU: Trainer.state_dict / save_state / load_state put Adam back to the bit, train_loop(resumable=True)
writes what train.resume() reads (bundle + optimiser sidecar + the reference's data_buffer/*.pkl, main.py:73-75), and the replay
library declares and exports its read-out / state-string entry points."""
import ctypes
import os
import random
import re

import numpy as np
import torch

from alphafive_amd import utils
from alphafive_amd.network import ResNet, random_variables
from alphafive_amd.train import Trainer, resume, train_loop
from conftest import REPO, make_cfg

S = 6


def _batch(rng, n=32):
    boards = (rng.rand(n, 3, S, S) < 0.3).astype(np.float32)
    pol = rng.rand(n, S * S).astype(np.float32)
    pol /= pol.sum(axis=1, keepdims=True)
    return boards, (0.5 + rng.rand(n)).astype(np.float32), np.sign(rng.randn(n)).astype(np.float32), pol


def _bits(d):
    return {k: np.asarray(a, np.float32).view(np.uint32).copy() for k, a in d.items()}


def _same(a, b):
    a, b = _bits(a), _bits(b)
    return a.keys() == b.keys() and all(np.array_equal(a[k], b[k]) for k in a)


def test_trainer_state_round_trip_continues_to_the_bit(tmp_path):
    rng = np.random.RandomState(0)
    tr = Trainer(random_variables(S, 0), S, device="cpu")
    for _ in range(3):
        tr.step(*_batch(rng), lr=1e-3)
    ckpt = str(tmp_path / "ckpt")
    tr.save(ckpt, 3)
    tr.save_state(ckpt, 3)
    assert os.path.exists(os.path.join(ckpt, "alphaFive-3.opt.npz"))
    saved = tr.state_dict()
    assert saved["t"] == 3 and any(np.abs(a).max() > 0 for a in saved["m"].values())

    back = Trainer(random_variables(S, 1), S, device="cpu")            # other variables: everything must come from the files
    back.load_state(ckpt, 3)
    got = back.state_dict()
    assert got["t"] == 3
    for key in ("params", "m", "v"):
        assert _same(saved[key], got[key]), key

    fresh = Trainer(saved["params"], S, device="cpu")                  # the same variables, Adam from zero
    fourth = _batch(rng)
    for t in (tr, back, fresh):
        t.step(*fourth, lr=1e-3)
    assert _same(tr.variables(), back.variables())                     # resumed == uninterrupted, bit for bit
    assert not _same(tr.variables(), fresh.variables())                # what the sidecar is for

    other = Trainer(random_variables(S, 2), S, device="cpu")           # and without files, through the dicts
    other.load_state_dict(tr.state_dict())
    assert other.t == 4 and all(_same(tr.state_dict()[k], other.state_dict()[k]) for k in ("params", "m", "v"))


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


class _RecordingStack(utils.RandomStack):
    """Remembers what it and the trainer held at each save()."""
    trainer = None

    def save(self, s=""):
        super().save(s)
        self.saved = dict(step=s, data_len=list(self.data_len), result=list(self.result), n=len(self.data),
                          first=self.data[0], last=self.data[-1], trainer=self.trainer.state_dict())


def _cfg(tmp_path):
    cfg = make_cfg(board_size=S, goal=4, batch_size=16)
    cfg.get_lr = lambda step: 1e-3
    cfg.ckpt_path = str(tmp_path / "ckpt")
    return cfg


def test_train_loop_defaults_write_no_resume_files(tmp_path, monkeypatch, capsys):
    monkeypatch.chdir(tmp_path)
    random.seed(2)
    np.random.seed(2)
    cfg = _cfg(tmp_path)
    net = ResNet(S, device="cpu", seed=0)
    tr = Trainer(net.variables, S, device="cpu")
    assert train_loop(cfg, _StubEngine(1), net, utils.RandomStack(S, 60), tr, steps=3, log=lambda s: None) == 3
    assert not os.path.exists("data_buffer") and not os.path.exists(cfg.ckpt_path)      # step 60 is far away
    # a checkpoint that is not resumable is the bundle alone
    assert train_loop(cfg, _StubEngine(2), net, utils.RandomStack(S, 60), tr, steps=3, log=lambda s: None, ckpt_every=2) == 3
    capsys.readouterr()
    names = sorted(os.listdir(cfg.ckpt_path))
    assert "alphaFive-2.index" in names and "checkpoint" in names
    assert not any(n.endswith(".opt.npz") for n in names) and not os.path.exists("data_buffer")


def test_resumable_train_loop_and_resume(tmp_path, monkeypatch, capsys):
    monkeypatch.chdir(tmp_path)
    random.seed(3)
    np.random.seed(3)
    cfg = _cfg(tmp_path)
    net = ResNet(S, device="cpu", seed=0)
    tr = Trainer(net.variables, S, device="cpu")
    stack = _RecordingStack(S, 60)
    stack.trainer = tr
    assert train_loop(cfg, _StubEngine(1), net, stack, tr, steps=4, log=lambda s: None, resumable=True, ckpt_every=2) == 4
    for f in ("alphaFive-2.opt.npz", "alphaFive-4.opt.npz", "alphaFive-4.index"):
        assert os.path.exists(os.path.join(cfg.ckpt_path, f)), f
    for stem in ("data", "data_len", "result"):
        assert os.path.exists("data_buffer/%s2.pkl" % stem) and os.path.exists("data_buffer/%s4.pkl" % stem)
    saved = stack.saved
    assert saved["step"] == 4 and saved["trainer"]["t"] == 12           # 4 minibatches per step, steps 2..4

    net2 = ResNet(S, device="cpu", seed=5)
    tr2 = Trainer(net2.variables, S, device="cpu")
    stack2 = utils.RandomStack(S, 60)
    logs = []
    step = resume(cfg, net2, stack2, tr2, log=logs.append)
    capsys.readouterr()
    assert step == 4 and tr2.t == 12
    got = tr2.state_dict()
    for key in ("params", "m", "v"):
        assert _same(saved["trainer"][key], got[key]), key
    assert _same(net2.variables, saved["trainer"]["params"])
    assert stack2.data_len == saved["data_len"] and stack2.result == saved["result"] and len(stack2.data) == saved["n"]
    assert stack2.black_win == saved["result"].count(utils.BLACK_WIN)
    for x, y in ((stack2.data[0], saved["first"]), (stack2.data[-1], saved["last"])):
        assert x[0] == y[0] and np.array_equal(x[1], y[1]) and x[2:] == y[2:]
    # and the loop goes on from there
    assert train_loop(cfg, _StubEngine(7), net2, stack2, tr2, steps=6, log=logs.append, start_step=step, resumable=True,
                      ckpt_every=2) == 6
    capsys.readouterr()
    assert tr2.t == 20 and os.path.exists(os.path.join(cfg.ckpt_path, "alphaFive-6.opt.npz"))
    assert sum("step: " in s for s in logs) == 2

    # a bundle without a sidecar (what the reference writes): variables restored, Adam fresh, and resume() says so
    os.remove(os.path.join(cfg.ckpt_path, "alphaFive-6.opt.npz"))
    for stem in ("data", "data_len", "result"):
        os.remove("data_buffer/%s6.pkl" % stem)
    tr3 = Trainer(random_variables(S, 8), S, device="cpu")
    stack3 = utils.RandomStack(S, 60)
    logs = []
    assert resume(cfg, ResNet(S, device="cpu", seed=8), stack3, tr3, log=logs.append) == 6
    assert tr3.t == 0 and _same(tr3.variables(), tr2.variables()) and stack3.isEmpty()
    assert not any(np.abs(a).max() > 0 for a in tr3.state_dict()["m"].values())
    assert any("Adam starts fresh" in s for s in logs) and any("no replay buffer" in s for s in logs)


def test_replay_header_declares_and_library_exports_the_persistence_calls():
    hdr = open(os.path.join(REPO, "include", "af_replay.h")).read()
    assert re.search(r"#define\s+AF_REPLAY_ERR_FORMAT\s+\(-5\)", hdr)
    nl = ctypes.CDLL(os.path.join(REPO, "alphafive_amd", "_lib", "libaf_replay.so"))
    for name in ("af_replay_export", "af_replay_append_states", "af_replay_state_stride"):
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
        assert hasattr(nl, name), name
    nl.af_replay_strerror.restype = ctypes.c_char_p
    assert nl.af_replay_strerror(-5) == b"malformed state string"
    nl.af_replay_state_stride.restype = ctypes.c_int32
    nl.af_replay_state_stride.argtypes = [ctypes.c_void_p]
    assert nl.af_replay_state_stride(None) == 0
