"""The way out of the device replay ring and back: af_replay_export / af_replay_append_states (the state-string codec of
utils.py:156-196 on the device), DeviceRandomStack.to_host / from_host / save_pickles / load_pickles against the host class and
against files the unmodified reference wrote, and a closed-loop run that is stopped and continued (train.resume)."""
import ctypes as C
import os
import pickle
import random

import numpy as np
import pytest

from alphafive_amd import utils

pytestmark = pytest.mark.gpu

ERR_FORMAT = -5


# ---------------------------------------------------------------------------------------------------------------------------
# 4. the codec through the C ABI, all sizes
# ---------------------------------------------------------------------------------------------------------------------------
class _Ring(object):
    """A bare af_replay handle driven through ctypes."""

    def __init__(self, S, cap):
        from alphafive_amd import replay
        self.L, self.S, self.h = replay.lib(), S, C.c_void_p()
        assert self.L.af_replay_create(S, cap, 0, C.byref(self.h)) == 0
        self.stride = self.L.af_replay_state_stride(self.h)

    def size(self):
        return self.L.af_replay_size(self.h)

    def append(self, boards, pol, last, val, wts):
        fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int32)
        return self.L.af_replay_append(self.h, None, len(boards), boards.ctypes.data_as(C.POINTER(C.c_int8)),
                                       pol.ctypes.data_as(fp), last.ctypes.data_as(ip), val.ctypes.data_as(fp),
                                       wts.ctypes.data_as(fp))

    def append_states(self, raw, stride, pol, last, val, wts):
        """raw: bytes of n * stride characters."""
        n = len(raw) // stride
        buf = np.frombuffer(raw, np.uint8).copy()
        return self.L.af_replay_append_states(self.h, None, n, buf.ctypes.data, stride, pol.ctypes.data, last.ctypes.data,
                                              val.ctypes.data, wts.ctypes.data)

    def export(self, first, n, states=True, boards=True):
        Cc = self.S * self.S
        st = np.full(n * self.stride, 0x7f, np.uint8)                  # not NUL: the padding must be written
        bo = np.full((n, Cc), 9, np.int8)
        pol, last = np.empty((n, Cc), np.float32), np.empty(n, np.int32)
        val, wts = np.empty(n, np.float32), np.empty(n, np.float32)
        rc = self.L.af_replay_export(self.h, None, first, n, st.ctypes.data if states else None,
                                     bo.ctypes.data if boards else None, pol.ctypes.data, last.ctypes.data, val.ctypes.data,
                                     wts.ctypes.data)
        return rc, st.reshape(n, self.stride), bo, pol, last, val, wts

    def close(self):
        self.L.af_replay_destroy(self.h)


def _pad(strings, stride):
    return b"".join(s.encode().ljust(stride, b"\0") for s in strings)


def _codec_boards(S, rng):
    boards = [rng.randint(-1, 2, (S, S)).astype(np.int8) for _ in range(6)]
    boards.append(np.zeros((S, S), np.int8))                                       # empty
    boards.append(rng.choice(np.array([-1, 1], np.int8), (S, S)))                  # full: no runs at all, the longest string
    for i, j in ((0, 0), (0, S - 1), (S - 1, 0), (S - 1, S - 1)):                  # one stone in each corner
        b = np.zeros((S, S), np.int8)
        b[i, j] = 1 if (i + j) % 2 == 0 else -1
        boards.append(b)
    b = np.zeros((S, S), np.int8)
    b[S // 2] = [1 if j % 2 == 0 else -1 for j in range(S)]                         # an alternating row of stones
    b[S - 1] = [1 if j % 2 == 0 else 0 for j in range(S)]                           # and one of stone / empty
    boards.append(b)
    return np.stack(boards)


def _records(S, n, rng):
    pol = rng.rand(n, S * S).astype(np.float32)
    last = rng.randint(-1, S * S, n).astype(np.int32)
    return pol, last, rng.randn(n).astype(np.float32), rng.rand(n).astype(np.float32)


def _text(row):
    return bytes(row).split(b"\0", 1)[0].decode()


@pytest.mark.parametrize("S", [3, 5, 11, 15, 16])
def test_state_codec_on_the_device(S):
    rng = np.random.RandomState(S)
    boards = _codec_boards(S, rng)
    n, Cc = len(boards), S * S
    pol, last, val, wts = _records(S, n, rng)
    want = [utils.board_to_state(b) for b in boards]
    ring = _Ring(S, 3 * n)
    assert ring.stride == S * (S + 1) + 1
    assert max(len(s) for s in want) == S * (S + 1) == ring.stride - 1            # the full board fills the stride to its NUL
    flat = np.ascontiguousarray(boards.reshape(n, Cc))

    def exported_equals(first, count, b, p, la, v, w, strings):
        rc, st, bo, po, lo, vo, wo = ring.export(first, count)
        assert rc == 0
        for k in range(count):
            assert _text(st[k]) == strings[k]
            assert not st[k][len(strings[k]):].any()                              # NUL-terminated and NUL-padded
        assert np.array_equal(bo, b)
        assert np.array_equal(po.view(np.uint32), p.view(np.uint32)) and np.array_equal(lo, la)
        assert np.array_equal(vo.view(np.uint32), v.view(np.uint32)) and np.array_equal(wo.view(np.uint32), w.view(np.uint32))

    assert ring.append(flat, pol, last, val, wts) == 0
    exported_equals(0, n, flat, pol, last, val, wts, want)
    exported_equals(3, n - 5, flat[3:n - 2], pol[3:n - 2], last[3:n - 2], val[3:n - 2], wts[3:n - 2], want[3:n - 2])
    rc, st, bo = ring.export(0, n, states=False)[:3]                              # either text or boards may be left out
    assert rc == 0 and (st == 0x7f).all() and np.array_equal(bo, flat)
    rc, st, bo = ring.export(0, n, boards=False)[:3]
    assert rc == 0 and (bo == 9).all() and [_text(r) for r in st] == want
    assert ring.export(1, n)[0] == -4 and ring.export(n, 1)[0] == -4 and ring.export(n, 0)[0] == 0   # AF_REPLAY_ERR_RANGE
    assert ring.size() == n                                                       # the ring is not modified

    # the same records appended as text, in a caller's own stride
    stride = ring.stride + 7
    assert ring.append_states(_pad(want, stride), stride, pol, last, val, wts) == 0
    assert ring.size() == 2 * n
    exported_equals(n, n, flat, pol, last, val, wts, want)

    # one malformed string of each kind, between good ones: the whole call appends nothing
    good = want[0]
    rows = want[1].split("/")[:-1]
    empty_row, a = chr(97 + S), ord("a")
    bad = {
        "character 'a' (a run of 0)": "/".join(["a" + rows[0]] + rows[1:]) + "/",
        "character past 'a'+S": "/".join([chr(a + S + 1)] + rows[1:]) + "/",
        "character '2'": "/".join(["2" + chr(a + S - 1) if S > 1 else "2"] + rows[1:]) + "/",
        "upper case": "/".join([empty_row.upper()] + rows[1:]) + "/",
        "row past S cells (run)": "/".join(["3" + empty_row] + rows[1:]) + "/",
        "row past S cells (stone)": "/".join([empty_row + "1"] + rows[1:]) + "/",
        "row short of S cells": "/".join([chr(a + S - 1)] + rows[1:]) + "/",
        "S-1 rows": "/".join(rows[:-1]) + "/",
        "S+1 rows": "/".join(rows + [empty_row]) + "/",
        "last row not closed": "/".join(rows),
    }
    three = (pol[:3], last[:3], val[:3], wts[:3])
    for kind, s in bad.items():
        assert len(s) < stride, kind
        assert ring.append_states(_pad([good, s, good], stride), stride, *three) == ERR_FORMAT, kind
        assert ring.size() == 2 * n, kind
    # no NUL inside the stride: a good string that exactly fills it
    tight = len(want[7])
    assert ring.append_states(want[7].encode(), tight, pol[:1], last[:1], val[:1], wts[:1]) == ERR_FORMAT
    assert ring.append_states(_pad([want[7]], tight + 1), tight + 1, pol[7:8], last[7:8], val[7:8], wts[7:8]) == 0
    assert ring.size() == 2 * n + 1
    from alphafive_amd import replay
    assert b"state string" in replay.lib().af_replay_strerror(ERR_FORMAT)
    # ... and the ring is as good as before: what was there, and a valid append after the rejected ones
    exported_equals(2 * n, 1, flat[7:8], pol[7:8], last[7:8], val[7:8], wts[7:8], want[7:8])
    exported_equals(0, n, flat, pol, last, val, wts, want)
    exported_equals(n, n, flat, pol, last, val, wts, want)
    ring.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 5. against the host twin, across the wrap
# ---------------------------------------------------------------------------------------------------------------------------
def _episodes(S, n_ep, seed):
    """Random legal-looking episodes in the replay record format (utils.py:127: state, p[S,S], la, v, w)."""
    rng = np.random.RandomState(seed)
    eps = []
    for _ in range(n_ep):
        T = int(rng.randint(9, min(40, S * S)))
        board = np.zeros((S, S), np.int8)
        rec, la = [], None
        w = utils.construct_weights(T, 0.94)
        for t in range(T):
            p = rng.rand(S, S).astype(np.float32)
            p /= p.sum()
            rec.append((utils.board_to_state(board), p, la, float((-1.0) ** (T - t)), w[t]))
            empt = np.argwhere(board == 0)
            a = tuple(int(v) for v in empt[rng.randint(len(empt))])
            board = utils.step(board, a)
            la = a
        result = utils.DRAW if rng.rand() < 0.1 else (utils.BLACK_WIN if T % 2 == 1 else utils.WHITE_WIN)
        eps.append((rec, result))
    return eps


def _assert_same_stack(host, got):
    """`got` (a utils.RandomStack read out of the device) equals `host` record for record, types included."""
    S = host.board_size
    assert type(got) is utils.RandomStack and got.board_size == S and got.length == host.length
    assert got.data_len == host.data_len and got.result == host.result
    assert (got.black_win, got.white_win) == (host.black_win, host.white_win)
    assert len(got.data) == len(host.data)
    for x, y in zip(host.data, got.data):
        assert type(y) is tuple and len(y) == 5
        assert type(y[0]) is str and y[0] == x[0]
        assert type(y[1]) is np.ndarray and y[1].dtype == np.float32 == x[1].dtype and y[1].shape == (S, S) == x[1].shape
        assert np.array_equal(x[1].view(np.uint32), y[1].view(np.uint32))
        if x[2] is None:
            assert y[2] is None
        else:
            assert type(y[2]) is tuple and y[2] == tuple(x[2]) and all(type(v) is int for v in y[2])
        assert type(y[3]) is float and y[3] == x[3]
        assert type(y[4]) is np.float32 and y[4] == x[4]


class _CountingStack(utils.RandomStack):
    appended = 0

    def _store(self, data):
        self.appended += len(data)
        super()._store(data)


@pytest.mark.parametrize("S, length, n_ep, max_episode", [(11, 300, 40, None), (5, 60, 25, None), (15, 500, 40, 40)])
def test_to_host_equals_the_host_twin_across_the_wrap(S, length, n_ep, max_episode, capsys):
    from alphafive_amd.replay import DeviceRandomStack
    eps = _episodes(S, n_ep, seed=S)
    random.seed(7)
    np.random.seed(7)
    host = _CountingStack(S, length)
    host_mid = None
    for k, (rec, res) in enumerate(eps):
        host.push(rec, res)
        if k == n_ep // 2:
            host_mid = (list(host.data), list(host.data_len), list(host.result), host.black_win, host.white_win)
    capacity = length + 2 * (max_episode or S * S)
    assert host.appended > capacity                   # the ring's physical end has been passed: the export crosses it
    random.seed(7)
    np.random.seed(7)
    dev = DeviceRandomStack(S, length, device=0, max_episode=max_episode)
    for k, (rec, res) in enumerate(eps):
        dev.push(rec, res)
        if k == n_ep // 2:
            mid = utils.RandomStack(S, length)
            mid.data, mid.data_len, mid.result, mid.black_win, mid.white_win = host_mid
            _assert_same_stack(mid, dev.to_host())
    capsys.readouterr()
    got = dev.to_host()
    _assert_same_stack(host, got)
    assert dev._size() == len(host.data) and dev.data is None          # reading out changes nothing
    # and the way back: a second device stack built from the records, read out again, and sampled like the first
    back = DeviceRandomStack.from_host(got, device=0, max_episode=max_episode)
    _assert_same_stack(host, back.to_host())
    batches = []
    for st in (dev, back):
        random.seed(11)
        np.random.seed(11)
        batches.append([t.cpu().numpy() for t in st.get_data(50)])
    for u, v in zip(*batches):
        assert np.array_equal(u.view(np.uint32), v.view(np.uint32))
    dev.close()
    back.close()


def test_load_records_refuses_what_does_not_fit_or_parse():
    from alphafive_amd import replay
    S = 5
    rec = [(utils.board_to_state(np.zeros((S, S), np.int8)), np.full((S, S), 0.04, np.float32), None, 1.0, np.float32(1.0))]
    st = replay.DeviceRandomStack(S, 10, device=0, max_episode=3)
    st.load_records(rec * 16, [16], [utils.BLACK_WIN])                  # exactly the ring: 10 + 2*3
    assert st._size() == 16 and st.black_win == 1 and st.white_win == 0
    with pytest.raises(replay.ReplayError):
        st.load_records(rec * 17, [17], [utils.BLACK_WIN])              # one more: refused, nothing truncated
    assert st._size() == 16 and st.data_len == [16]
    with pytest.raises(replay.ReplayError):
        st.load_records(rec * 4, [3], [utils.DRAW])                     # bookkeeping that does not describe the records
    bad = [("f/f/f/f/", rec[0][1], None, 1.0, np.float32(1.0))]         # four rows on a 5x5 board
    with pytest.raises(replay.ReplayError, match="state string"):
        st.load_records(rec + bad, [2], [utils.DRAW])
    assert st._size() == 0 and st.data_len == [] and st.result == []
    st.load_records(rec * 2, [2], [utils.WHITE_WIN])
    assert st._size() == 2 and st.white_win == 1 and st.to_host().data[1][0] == "f/f/f/f/f/"
    st.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 6. pinned to files the unmodified reference wrote
# ---------------------------------------------------------------------------------------------------------------------------
class _PlainUnpickler(pickle.Unpickler):
    """pickle.load in a process that has no alphafive_amd (utils.py:43-49 of the reference): numpy and builtins only."""

    def find_class(self, module, name):
        if module.split(".")[0] not in ("numpy", "builtins", "copyreg", "_codecs"):
            raise pickle.UnpicklingError("%s.%s is not loadable without alphafive_amd" % (module, name))
        return super().find_class(module, name)


def test_reference_pickles_through_the_device_stack(tmp_path, monkeypatch, golden_dir, capsys):
    from alphafive_amd.replay import DeviceRandomStack
    z = np.load(os.path.join(golden_dir, "compat_randomstack.npz"))
    monkeypatch.chdir(tmp_path)
    os.mkdir("data_buffer")
    for stem in ("data", "data_len", "result"):
        with open(os.path.join("data_buffer", "%s120.pkl" % stem), "wb") as f:
            f.write(z["ref_pkl_" + stem].tobytes())
    dev = DeviceRandomStack(11, 300)
    dev.load_pickles(120)
    assert dev._size() == int(z["ref_n_data"]) == 300 and dev.data is None
    assert dev.data_len == z["ref_data_len"].tolist() and dev.result == z["ref_result"].tolist()
    assert (dev.black_win, dev.white_win) == (int(z["ref_black_win"]), int(z["ref_white_win"]))
    np.random.seed(5)
    random.seed(5)
    batch = [t.cpu().numpy() for t in dev.get_data(64)]
    for x, k in zip(batch, ("ref_boards", "ref_weights", "ref_values", "ref_policies")):
        assert x.dtype == z[k].dtype and x.shape == z[k].shape and np.array_equal(x.view(np.uint32), z[k].view(np.uint32)), k
    # and back: what the device stack writes is what the reference wrote
    ref_data = pickle.loads(z["ref_pkl_data"].tobytes())
    assert max(len(d[0]) for d in ref_data) == 80
    os.rename("data_buffer", "from_reference")
    dev.save_pickles(7)                                                  # creates data_buffer/
    loaded = {}
    for stem in ("data", "data_len", "result"):
        with open(os.path.join("data_buffer", "%s7.pkl" % stem), "rb") as f:
            loaded[stem] = _PlainUnpickler(f).load()
    assert loaded["data_len"] == dev.data_len and loaded["result"] == dev.result
    host = utils.RandomStack(11, length=300)
    host.load(7)
    capsys.readouterr()
    assert host.data_len == dev.data_len and host.result == dev.result
    assert (host.black_win, host.white_win) == (dev.black_win, dev.white_win)
    for data in (loaded["data"], host.data):
        assert len(data) == len(ref_data) == 300
        for x, y in zip(ref_data, data):
            assert x[0] == y[0] and x[1].dtype == y[1].dtype and x[1].shape == y[1].shape and (x[1] == y[1]).all()
            assert x[2:] == y[2:] and [type(v) for v in x] == [type(v) for v in y]
    dev.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 7. what af_replay_append_packed stored, looked at directly
# ---------------------------------------------------------------------------------------------------------------------------
def _hand_off_read_out(S, sims, G, length):
    import pseudonet
    from conftest import make_cfg
    from alphafive_amd.engine import SelfPlayEngine
    from alphafive_amd.replay import DeviceRandomStack
    cfg = make_cfg(board_size=S, goal=4, simulation_per_step=sims, upper_simulation_per_step=sims + 8)
    mk = lambda: SelfPlayEngine(cfg, G, lambda x: pseudonet.pseudonet_torch(x, 321, 4096), device=0, seed=13)
    a, b = mk(), mk()
    host, dev = utils.RandomStack(S, length), DeviceRandomStack(S, length, device=0)
    for which, sp, st in (("host", a, host), ("dev", b, dev)):
        random.seed(5)
        np.random.seed(5)
        for rnd in range(14):
            sp.run_ticks(120)
            sp.check()
            if which == "host":
                for rec, res in sp.pop_episodes(64):
                    st.push(rec, res)
            else:
                st.push_packed(sp.post_episodes_device(64), 64, cfg.gamma)
    dev.check()
    assert len(host.data) >= 200 and len(host.data_len) > 10
    _assert_same_stack(host, dev.to_host())
    a.close()
    b.close()
    dev.close()


def test_device_to_device_hand_off_read_out_equals_the_host_records(capsys):
    _hand_off_read_out(S=6, sims=24, G=48, length=400)
    capsys.readouterr()


@pytest.mark.parametrize("S, sims, G, length", [(13, 8, 32, 900), (16, 8, 32, 1200)])
def test_device_to_device_hand_off_read_out_equals_the_host_records_on_four_word_boards(S, sims, G, length, capsys):
    """The same on boards above 128 cells, whose keys carry four 64-bit words per colour: the engine's pack kernels feeding
    af_replay_append_packed's KW = 4 decode, every stored record looked at."""
    _hand_off_read_out(S, sims, G, length)
    capsys.readouterr()


# ---------------------------------------------------------------------------------------------------------------------------
# 8. stop and continue
# ---------------------------------------------------------------------------------------------------------------------------
def test_closed_loop_stops_and_continues(capsys, tmp_path, monkeypatch):
    """MIOpen's backward is not promised to be run-to-run deterministic: the bar is equality of the restored state with what
    the first run held when it saved, not of the continued trajectory."""
    import torch
    from alphafive_amd.engine import SelfPlayEngine
    from alphafive_amd.network import ResNet
    from alphafive_amd.replay import DeviceRandomStack
    from alphafive_amd.train import Trainer, resume, train_loop
    from conftest import make_cfg
    monkeypatch.chdir(tmp_path)
    random.seed(3)
    np.random.seed(3)
    S = 6
    cfg = make_cfg(board_size=S, goal=4, simulation_per_step=16, upper_simulation_per_step=24, batch_size=64)
    cfg.get_lr = lambda step: 1e-3
    cfg.ckpt_path = str(tmp_path / "ckpt")

    class Recording(DeviceRandomStack):
        def save_pickles(self, s=""):
            super().save_pickles(s)
            self.saved = dict(step=s, stack=self.to_host(), trainer=self.trainer.state_dict())

    net = ResNet(S, device="cuda", seed=0)
    sp = SelfPlayEngine(cfg, 64, net.select_backend("hip"), device=0, seed=1)
    stack = Recording(S, 120, device=0)
    tr = stack.trainer = Trainer(net.variables, S, device="cuda")
    assert train_loop(cfg, sp, net, stack, tr, steps=3, log=lambda s: None, resumable=True, ckpt_every=2) >= 3
    saved = stack.saved
    assert saved["step"] == 2 and saved["trainer"]["t"] == 4 and tr.t == 8        # the run went on after it saved
    assert os.path.exists(os.path.join(cfg.ckpt_path, "alphaFive-2.opt.npz")) and os.path.exists("data_buffer/data2.pkl")
    sp.close()
    stack.close()

    net2 = ResNet(S, device="cuda", seed=9)
    sp2 = SelfPlayEngine(cfg, 64, net2.select_backend("hip"), device=0, seed=2)   # a seed the first run did not use
    stack2 = DeviceRandomStack(S, 120, device=0)
    tr2 = Trainer(net2.variables, S, device="cuda")
    logs = []
    step = resume(cfg, net2, stack2, tr2, log=logs.append)
    assert step == 2 and tr2.t == 4
    got = tr2.state_dict()
    for key in ("params", "m", "v"):
        for k, v in saved["trainer"][key].items():
            assert np.array_equal(v.view(np.uint32), got[key][k].view(np.uint32)), (key, k)
    for k, v in saved["trainer"]["params"].items():
        assert np.array_equal(v.view(np.uint32), net2.variables[k].view(np.uint32)), k
    _assert_same_stack(saved["stack"], stack2.to_host())
    assert stack2.is_full()

    assert train_loop(cfg, sp2, net2, stack2, tr2, steps=step + 2, log=logs.append, start_step=step, resumable=True,
                      ckpt_every=2) >= step + 2
    capsys.readouterr()
    assert tr2.t == 12 and sum("xcross_loss" in s for s in logs) == 2
    assert os.path.exists(os.path.join(cfg.ckpt_path, "alphaFive-4.opt.npz")) and os.path.exists("data_buffer/result4.pkl")
    x = torch.zeros((2, 3, S, S), device="cuda")
    p_hip, v_hip = sp2.pv(x) if hasattr(sp2, "pv") else net2.select_backend("hip")(x)
    p_t, v_t = net2.eval_torch(x)
    assert (p_hip - p_t).abs().max().item() < 1e-5                                 # the HIP evaluator has the trainer's weights
    sp2.close()
    stack2.close()
