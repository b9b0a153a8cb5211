"""DeviceRandomStack — utils.RandomStack (reference utils.py:14-146) with the positions resident in HBM
(libaf_replay.so, include/af_replay.h).  Same call surface and the same random draws in the same order as the
reference, so a seeded run produces the same batches as the host class bit for bit (tests/test_gpu_replay.py);
get_data() returns device tensors the trainer consumes without a host round trip.

push() keeps the reference's scalar bookkeeping on the host (one episode at a time, a few Python `random` draws)
and uploads the accepted episode once; push_packed() / iter_push_packed() take the engine's packed DEVICE hand-off buffer
instead: the host reads its header only and the plies are decoded on the device (no 5-tuples, no per-ply Python, no
upload); get_data() draws (which positions, quarter turns, flip) on the host and runs the gather + 8-fold symmetry +
board_to_inputs encoding as one kernel launch.  draw_batches() / get_data_device() take those draws to the device too
(a counter-based generator, specified by draw_reference() below): same distribution, no host work beyond two launches.

Persistence: to_host() reads the ring out as a utils.RandomStack (one af_replay_export: the device writes the records' state
strings), from_host() / load_records() put records back (af_replay_append_states: the device decodes them), and
save_pickles() / load_pickles() exchange the reference's three data_buffer/*.pkl files (utils.py:29-57) on top of those.
"""
import ctypes as C
import os

import numpy as np
import torch

from . import utils

_PKG = os.path.dirname(os.path.abspath(__file__))
_LIBPATH = os.environ.get("AF_REPLAY_LIB") or os.path.join(_PKG, "_lib", "libaf_replay.so")
_lib = None


class ReplayError(RuntimeError):
    pass


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(_LIBPATH):
            raise ImportError(f"{_LIBPATH} not built (python -m alphafive_amd.build)")
        # torch first: its wheel bundles its own HIP runtime; a process in which /opt/rocm's copy was pulled in earlier (by this
        # library's DT_NEEDED) ends up with two runtimes, and the second one finds no device
        import torch  # noqa: F401
        L = C.CDLL(_LIBPATH)
        vp, ip, fp = C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_float)
        L.af_replay_create.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.POINTER(vp)]
        L.af_replay_destroy.argtypes = [vp]
        L.af_replay_destroy.restype = None
        L.af_replay_append.argtypes = [vp, vp, C.c_int32, C.POINTER(C.c_int8), fp, ip, fp, fp]
        L.af_replay_drop_front.argtypes = [vp, C.c_int32]
        L.af_replay_size.argtypes = [vp]
        L.af_replay_sample.argtypes = [vp, vp, C.c_int32, ip, ip, ip, vp, vp, vp, vp]
        L.af_replay_sample_device.argtypes = [vp, vp, C.c_int32, C.c_int32, C.c_uint64, C.c_uint32, vp, vp, vp, vp, vp]
        L.af_replay_append_packed.argtypes = [vp, vp, vp, C.c_int32, C.c_int32, C.c_int32]
        L.af_replay_set_weights.argtypes = [vp, fp, C.c_int32]
        L.af_replay_check.argtypes = [vp, vp]
        L.af_replay_state_stride.argtypes = [vp]
        L.af_replay_export.argtypes = [vp, vp, C.c_int32, C.c_int32, vp, vp, vp, vp, vp, vp]
        L.af_replay_append_states.argtypes = [vp, vp, C.c_int32, vp, C.c_int32, vp, vp, vp, vp]
        L.af_replay_strerror.argtypes = [C.c_int]
        L.af_replay_strerror.restype = C.c_char_p
        _lib = L
    return _lib


def _check(rc, what):
    if rc < 0:
        raise ReplayError(f"{what}: {lib().af_replay_strerror(rc).decode()} (code {rc})")
    return rc


# ---- device-drawn minibatches: the specification af_replay_draw_kernel (csrc/af_replay.hip) is held to, bit for bit ----
DRAW_TAG = 0x52504C59           # "RPLY": fourth Philox counter word of a replay draw (AF_REPLAY_DRAW_TAG)
MAX_DRAW = 4096                 # AF_REPLAY_MAX_DRAW: most samples of one minibatch


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """af_philox4x32 of include/af_noise.h on numpy arrays (or scalars) of 32-bit words -> four uint32 arrays.
    All-zero counter and key -> 6627e8d5 e169c58d bc57ac4c 9b00dbd8."""
    M = np.uint64(0xFFFFFFFF)
    c0, c1, c2, c3 = np.broadcast_arrays(*[np.asarray(c, np.uint64) & M for c in (c0, c1, c2, c3)])
    k0, k1 = int(k0) & 0xFFFFFFFF, int(k1) & 0xFFFFFFFF
    s32 = np.uint64(32)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2         # 32 x 32 -> 64 bits: no overflow
        c0, c1, c2, c3 = (p1 >> s32) ^ c1 ^ np.uint64(k0), p1 & M, (p0 >> s32) ^ c3 ^ np.uint64(k1), p0 & M
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return tuple(c.astype(np.uint32) for c in (c0, c1, c2, c3))


def draw_reference(n, num, batches, seed, draw):
    """Which positions, quarter turns and flips `batches` minibatches of `num` samples take from a buffer of `n` positions
    -> (idx, turns, flip), each int32[batches][k], k = min(num, n).  This is the specification of the device draw
    (af_replay_sample_device); it replaces the reference's global-stream draws (utils.py:120,129,136) by a counter-based
    one with the same distribution.  For minibatch b and logical position i in [0, n), counted from the oldest:

        v        = philox4x32_10(ctr = (i, b, draw mod 2^32, DRAW_TAG), key = (seed mod 2^32, (seed >> 32) mod 2^32))
        key(i)   = v[0] << 32 | i
        turns(i) = v[1] >> 30            0..3, np.rot90's k
        flip(i)  = v[2] >> 31            1 = the vertical flip is applied

    Minibatch b is the k positions with the smallest key, in ascending key order: a uniform k-subset in uniform order, one of
    the 8 symmetries uniformly and independently per sample.  Positions whose 32-bit words are equal are ordered by the lower
    index; that favours lower indices by at most n / 2^32 relative (3e-6 at n = 12000)."""
    n, num, batches = int(n), int(num), int(batches)
    if n < 0 or num < 0 or batches < 0:
        raise ValueError("n, num and batches must not be negative")
    k = min(num, n)
    seed = int(seed)
    i = np.arange(n, dtype=np.uint64)[None, :]
    b = np.arange(batches, dtype=np.uint64)[:, None]
    v = philox4x32_10(i, b, int(draw), DRAW_TAG, seed, seed >> 32)
    key = (v[0].astype(np.uint64) << np.uint64(32)) | i                  # distinct for distinct i
    order = np.argsort(key, axis=1)[:, :k]
    turns = np.take_along_axis(v[1], order, axis=1) >> np.uint32(30)
    flip = np.take_along_axis(v[2], order, axis=1) >> np.uint32(31)
    return order.astype(np.int32), turns.astype(np.int32), flip.astype(np.int32)


class _PackedEpisode(object):
    """Stands for the list of 5-tuples RandomStack.push() receives when the episode lives in a packed DEVICE buffer
    (af_engine_pack_episodes): push() only needs its length; _store() hands (buffer, index) to af_replay_append_packed."""
    __slots__ = ("buf", "max_eps", "index", "T")

    def __init__(self, buf, max_eps, index, T):
        self.buf, self.max_eps, self.index, self.T = buf, max_eps, index, T

    def __len__(self):
        return self.T


class DeviceRandomStack(utils.RandomStack):
    """utils.RandomStack with the positions in HBM (module docstring).  `data` is None; what the host class keeps there is read
    with to_host() and written with load_records() / from_host().  save() / load() are not the way to the reference's pickles
    here: save_pickles() / load_pickles() are."""

    def __init__(self, board_size, length=2000, device=0, max_episode=None, draw_seed=0):
        """`draw_seed`: key of the device-drawn minibatches (draw_batches / get_data_device); `draw_counter`, which starts at 0
        and moves by one per call, is the other half of their address.  Neither touches get_data()."""
        super().__init__(board_size, length)
        self.draw_seed = int(draw_seed)
        self.draw_counter = 0
        self.device = torch.device("cuda", device) if isinstance(device, int) else torch.device(device)
        # a push may append one episode twice before the eviction brings the size back to `length`
        max_episode = max_episode or board_size * board_size
        self._h = C.c_void_p()
        idx = self.device.index if self.device.index is not None else torch.cuda.current_device()
        _check(lib().af_replay_create(board_size, length + 2 * max_episode, idx, C.byref(self._h)), "af_replay_create")
        self.data = None                       # positions live on the device
        self._wtab_gamma = None
        self._max_T = max_episode

    # ---- storage hooks ----
    def _size(self):
        return int(lib().af_replay_size(self._h))

    def _store(self, data):
        if isinstance(data, _PackedEpisode):    # device-to-device: one launch decodes the episode out of the packed buffer
            stream = torch.cuda.current_stream(self.device).cuda_stream
            _check(lib().af_replay_append_packed(self._h, stream, data.buf.data_ptr(), data.max_eps, data.index, data.T),
                   "af_replay_append_packed")
            return
        S, n = self.board_size, len(data)
        boards = np.empty((n, S * S), np.int8)
        pol = np.empty((n, S * S), np.float32)
        last = np.empty(n, np.int32)
        val = np.empty(n, np.float32)
        wts = np.empty(n, np.float32)
        for i, (state, p, la, v, w) in enumerate(data):
            boards[i] = utils.state_to_board(state, S).reshape(-1)
            pol[i] = np.asarray(p, np.float32).reshape(-1)
            last[i] = -1 if la is None else la[0] * S + la[1]
            val[i], wts[i] = v, w
        stream = torch.cuda.current_stream(self.device).cuda_stream
        fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int32)
        _check(lib().af_replay_append(self._h, stream, n, boards.ctypes.data_as(C.POINTER(C.c_int8)), pol.ctypes.data_as(fp),
                                      last.ctypes.data_as(ip), val.ctypes.data_as(fp), wts.ctypes.data_as(fp)),
               "af_replay_append")

    def _drop_front(self, n):
        _check(lib().af_replay_drop_front(self._h, n), "af_replay_drop_front")

    # ---- device-to-device hand-off (main.py:60-61 `stack.push(*q.get())` without the episodes leaving the GPU) ----
    def _ensure_weights(self, gamma):
        if self._wtab_gamma == gamma:
            return
        T = self._max_T
        tab = np.zeros((T + 1, T), np.float32)
        for t in range(1, T + 1):
            tab[t, :t] = utils.construct_weights(t, gamma=gamma)        # utils.py:286-296, numpy float32 arithmetic = the spec
        _check(lib().af_replay_set_weights(self._h, tab.ctypes.data_as(C.POINTER(C.c_float)), T), "af_replay_set_weights")
        self._wtab_gamma = gamma

    def push_packed(self, buf, max_eps, gamma):
        return list(self.iter_push_packed(buf, max_eps, gamma))

    def iter_push_packed(self, buf, max_eps, gamma):
        """Push every episode of a packed DEVICE hand-off buffer (SelfPlayEngine.post_episodes_device(max_eps)) in order.
        The host reads only the buffer's header (episode lengths and final values: 4 + 5*max_eps ints) and runs
        RandomStack.push's accept / duplicate / evict draws on (T, result) — same draws, same order as pushing the 5-tuples;
        the plies themselves are decoded on the device (af_replay_append_packed).  Yields push()'s result episode by episode
        (a generator, so that a training loop can draw batches between two pushes exactly where main.py:60-68 does).
        The buffer must stay untouched until the appends queued on the current stream have run (the engine's next pack
        comes later on the same stream, so the natural order post -> push_packed -> ticks -> post is safe)."""
        assert buf.is_cuda and buf.dtype == torch.int32
        self._ensure_weights(float(gamma))
        head = buf[:4 + 5 * max_eps].cpu().numpy()                       # waits for the pack kernels only
        n = int(head[0])
        finals = head[4 + 4 * max_eps:4 + 5 * max_eps].view(np.float32)
        for e in range(n):
            T = int(head[4 + 4 * e + 2])
            fv = float(finals[e])
            result = utils.DRAW if fv == 0.0 else (utils.BLACK_WIN if T % 2 == 1 else utils.WHITE_WIN)   # main.py:85-93
            yield self.push(_PackedEpisode(buf, max_eps, e, T), result)

    def check(self):
        """Raises if a packed append found its buffer not to hold what the header said (synchronises the stream)."""
        _check(lib().af_replay_check(self._h, torch.cuda.current_stream(self.device).cuda_stream), "af_replay_check")

    # ---- persistence: the ring read out as / filled from the host class's records ----
    def save(self, s=""):
        raise NotImplementedError("DeviceRandomStack keeps positions in HBM; use save_pickles() / load_pickles() for "
                                  "data_buffer/*.pkl, to_host() / from_host() for a utils.RandomStack")

    load = save

    def to_host(self):
        """-> utils.RandomStack holding what this stack holds: `data` as the 5-tuples engine.assemble_episode produces and the
        reference pickles (str, float32[S,S], (i, j) or None, float, np.float32) and the same length / data_len / result /
        black_win / white_win.  One af_replay_export: the ring is gathered and the state strings are written on the device."""
        S, n = self.board_size, self._size()
        host = utils.RandomStack(S, self.length)
        host.data_len, host.result = list(self.data_len), list(self.result)
        host.black_win, host.white_win = self.black_win, self.white_win
        if n == 0:
            return host
        stride = int(lib().af_replay_state_stride(self._h))
        states = np.zeros(n, "S%d" % stride)
        pol = np.empty((n, S, S), np.float32)
        last = np.empty(n, np.int32)
        val = np.empty(n, np.float32)
        wts = np.empty(n, np.float32)
        stream = torch.cuda.current_stream(self.device).cuda_stream
        _check(lib().af_replay_export(self._h, stream, 0, n, states.ctypes.data, None, pol.ctypes.data, last.ctypes.data,
                                      val.ctypes.data, wts.ctypes.data), "af_replay_export")
        la = [None if c < 0 else (c // S, c % S) for c in last.tolist()]
        host.data = list(zip(states.astype("U%d" % stride).tolist(), [p.copy() for p in pol], la, val.tolist(), list(wts)))
        return host

    def load_records(self, data, data_len, result):
        """Replace the content with RandomStack records (`data`: 5-tuples carrying state strings) and their episode bookkeeping;
        black_win / white_win are recounted from `result` as utils.py:50-51 does.  One af_replay_append_states: the strings are
        decoded on the device, and a malformed one is a ReplayError (the stack is left empty then).  More records than the ring
        holds is a ReplayError too, before anything is touched: nothing is truncated."""
        S, n = self.board_size, len(data)
        cap = self.length + 2 * self._max_T
        if n > cap:
            raise ReplayError("%d records do not fit a ring of %d positions (length %d + 2 * max_episode %d)" %
                              (n, cap, self.length, self._max_T))
        if sum(data_len) != n or len(result) != len(data_len):
            raise ReplayError("data_len sums to %d over %d episodes for %d records and %d results" %
                              (sum(data_len), len(data_len), n, len(result)))
        stride = int(lib().af_replay_state_stride(self._h))
        # (a string that does not fit its stride arrives without its NUL, which the device reports)
        states = np.array([d[0].encode("ascii", "replace") for d in data], "S%d" % stride) if n else np.zeros(0, "S%d" % stride)
        pol = np.empty((n, S * S), np.float32)
        for i, d in enumerate(data):
            pol[i] = np.asarray(d[1], np.float32).reshape(-1)
        last = np.array([-1 if d[2] is None else d[2][0] * S + d[2][1] for d in data], np.int32)
        val = np.array([d[3] for d in data], np.float32)
        wts = np.array([d[4] for d in data], np.float32)
        self._drop_front(self._size())
        self.data_len, self.result, self.black_win, self.white_win = [], [], 0, 0
        stream = torch.cuda.current_stream(self.device).cuda_stream
        _check(lib().af_replay_append_states(self._h, stream, n, states.ctypes.data, stride, pol.ctypes.data, last.ctypes.data,
                                             val.ctypes.data, wts.ctypes.data), "af_replay_append_states")
        self.data_len, self.result = [int(v) for v in data_len], list(result)
        self.white_win = self.result.count(utils.WHITE_WIN)
        self.black_win = self.result.count(utils.BLACK_WIN)

    @classmethod
    def from_host(cls, host_stack, device=0, max_episode=None):
        """A device stack with the board size, length and content of a utils.RandomStack."""
        st = cls(host_stack.board_size, host_stack.length, device=device, max_episode=max_episode)
        st.load_records(host_stack.data, host_stack.data_len, host_stack.result)
        return st

    def save_pickles(self, s=""):
        """The reference's three files (utils.py:29-40: data_buffer/data{s}.pkl, data_len{s}.pkl, result{s}.pkl) holding builtins
        and numpy only, so the reference's own RandomStack.load reads them in a process without this package."""
        os.makedirs("data_buffer", exist_ok=True)
        self.to_host().save(s)

    def load_pickles(self, s=""):
        """utils.py:42-57 into the ring: what save_pickles, utils.RandomStack.save or the reference wrote."""
        import pickle
        got = {}
        for attr, stem in self._FILES:
            with open(f"data_buffer/{stem}{s}.pkl", "rb") as f:
                got[attr] = pickle.load(f)
        self.load_records(got["data"], got["data_len"], got["result"])

    def get_data(self, batch_size=1):
        """utils.py:118-146.  Draws: np.random.choice(len, num, replace=False), then per sample
        np.random.choice([0,1,2,3]) (np stream) and random.choice([1,2]) (Python stream) — exactly the reference's."""
        import random as _random
        S = self.board_size
        size = self._size()
        num = min(batch_size, size)
        idx = np.random.choice(size, size=num, replace=False).astype(np.int32)
        turns = np.empty(num, np.int32)
        flip = np.empty(num, np.int32)
        for i in range(num):
            turns[i] = np.random.choice([0, 1, 2, 3])
            flip[i] = 1 if _random.choice([1, 2]) == 1 else 0
        boards = torch.empty((num, 3, S, S), dtype=torch.float32, device=self.device)
        weights = torch.empty((num,), dtype=torch.float32, device=self.device)
        values = torch.empty((num,), dtype=torch.float32, device=self.device)
        policies = torch.empty((num, S * S), dtype=torch.float32, device=self.device)
        stream = torch.cuda.current_stream(self.device).cuda_stream
        ip = C.POINTER(C.c_int32)
        _check(lib().af_replay_sample(self._h, stream, num, idx.ctypes.data_as(ip), turns.ctypes.data_as(ip),
                                      flip.ctypes.data_as(ip), boards.data_ptr(), weights.data_ptr(), values.data_ptr(),
                                      policies.data_ptr()), "af_replay_sample")
        return boards, weights, values, policies

    def draw_batches(self, batch_size, batches, return_draws=False):
        """`batches` independent minibatches of min(batch_size, size) samples, drawn AND gathered on the device (two launches,
        no host draw, no copy, no wait: af_replay_sample_device): boards[B,num,3,S,S], weights[B,num], values[B,num],
        policies[B,num,C] as device tensors, with return_draws=True also the int32[3,B,num] tensor of (logical index, quarter
        turns, flip) per sample.  The draws are draw_reference(size, batch_size, batches, draw_seed, draw_counter) — the
        reference's distribution (utils.py:118-146), not its global streams; get_data() keeps those.  draw_counter moves by one
        per call, whatever `batches` is.  An empty stack gives empty tensors without a launch."""
        S, B = self.board_size, int(batches)
        if B < 1:
            raise ValueError("batches must be at least 1")
        if batch_size > MAX_DRAW:
            raise ValueError("batch_size %d is more than a device draw holds (%d)" % (batch_size, MAX_DRAW))
        num = max(0, min(int(batch_size), self._size()))
        f32 = dict(dtype=torch.float32, device=self.device)
        boards = torch.empty((B, num, 3, S, S), **f32)
        weights = torch.empty((B, num), **f32)
        values = torch.empty((B, num), **f32)
        policies = torch.empty((B, num, S * S), **f32)
        draws = torch.empty((3, B, num), dtype=torch.int32, device=self.device) if return_draws else None
        draw = self.draw_counter & 0xFFFFFFFF
        self.draw_counter += 1
        if num > 0:
            stream = torch.cuda.current_stream(self.device).cuda_stream
            _check(lib().af_replay_sample_device(self._h, stream, num, B, self.draw_seed & 0xFFFFFFFFFFFFFFFF, draw,
                                                 boards.data_ptr(), weights.data_ptr(), values.data_ptr(), policies.data_ptr(),
                                                 draws.data_ptr() if return_draws else None), "af_replay_sample_device")
        out = (boards, weights, values, policies)
        return out + (draws,) if return_draws else out

    def get_data_device(self, batch_size=1):
        """get_data()'s shapes and dtypes from one device-drawn minibatch: draw_batches(batch_size, 1) without the leading
        dimension."""
        return tuple(t[0] for t in self.draw_batches(batch_size, 1))

    def close(self):
        if getattr(self, "_h", None):
            try:
                lib().af_replay_destroy(self._h)
            except Exception:       # interpreter shutdown
                pass
            self._h = None

    __del__ = close
