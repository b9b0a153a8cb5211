"""The eight symmetries of the board in the search: the specification of the kernels of csrc/af_sym.hip (include/af_sym.h), in
numpy, and SymmetricEvaluator, the evaluator that wraps an evaluator with them.

The reference trains with all eight symmetries (utils.py:127-138, RandomStack.get_data); this module brings them to evaluation:

    mode="mean"    a leaf is evaluated under all eight symmetries and the results, mapped back, are averaged: an exactly
                   symmetric evaluator, stronger per simulation, eight forward rows per leaf;
    mode="random"  a leaf is evaluated under one symmetry drawn for it (AlphaGo Zero's evaluator): no extra forward work.

Symmetries are numbered s = 0..7 with turns = s & 3 and flip = s >> 2: np.rot90 by `turns`, then np.flip along the rows if
`flip` — the (quarter turns, flip) pair of af_replay_sample.  s = 0 is the identity.

Everything up to SymmetricEvaluator is numpy only: no GPU and no torch are needed to import this module or to run the
*_reference functions, which are what the kernels are held to bit for bit (tests/test_gpu_symmetry.py).
"""
import numpy as np

AF_SYM_DRAW_TAG = 0x53594d30    # "SYM0": fourth Philox counter word of a symmetry draw (include/af_sym.h)
MODES = ("mean", "random")
MIN_BOARD, MAX_BOARD = 3, 16    # the engine's range of board sizes


def transform(a, s):
    """Symmetry s of the board(s) in the last two axes [S][S] of `a`."""
    s = int(s)
    if not 0 <= s < 8:
        raise ValueError("symmetry %r outside 0..7" % (s,))
    out = np.rot90(a, s & 3, axes=(-2, -1))
    return np.flip(out, axis=-2) if s >> 2 else out


def inverse(a, s):
    """Undoes transform(a, s)."""
    s = int(s)
    if not 0 <= s < 8:
        raise ValueError("symmetry %r outside 0..7" % (s,))
    out = np.flip(a, axis=-2) if s >> 2 else a
    return np.rot90(out, -(s & 3), axes=(-2, -1))


def cell_map(S, s):
    """int32 [S*S]: transform(a, s).reshape(-1)[c] == a.reshape(-1)[cell_map(S, s)[c]]."""
    cells = np.arange(S * S, dtype=np.int32).reshape(S, S)
    return np.ascontiguousarray(transform(cells, s)).reshape(-1)


def expand_reference(planes):
    """[B,3,S,S] -> [8B,3,S,S]: row 8 b + s is transform(planes[b], s); every plane, the last-move plane included, alike."""
    planes = np.asarray(planes)
    B = planes.shape[0]
    out = np.empty((8 * B,) + planes.shape[1:], planes.dtype)
    for s in range(8):
        out[s::8] = transform(planes, s)
    return out


def reduce_reference(policy8, value8, S):
    """(policy8 [8B,C], value8 [8B]) -> (policy [B,C], value [B]) in fp32.  With q_s = inverse(policy8[8 b + s], s):
    policy[b] = ((((((((q_0 + q_1) + q_2) + ...) + q_7)) * 0.125 — seven sequential fp32 additions in the order of s, then one
    multiplication, each rounded once; value[b] the same over value8[8 b + s]."""
    policy8 = np.asarray(policy8, np.float32)
    value8 = np.asarray(value8, np.float32).reshape(-1)
    B = policy8.shape[0] // 8
    p8 = policy8.reshape(B, 8, S, S)
    v8 = value8.reshape(B, 8)
    with np.errstate(all="ignore"):
        pol = np.array(p8[:, 0], np.float32)
        val = np.array(v8[:, 0], np.float32)
        for s in range(1, 8):
            pol = (pol + inverse(p8[:, s], s)).astype(np.float32)
            val = (val + v8[:, s]).astype(np.float32)
        pol = (pol * np.float32(0.125)).astype(np.float32)
        val = (val * np.float32(0.125)).astype(np.float32)
    return pol.reshape(B, S * S), val


def draw_reference(batch, seed, counter):
    """int32 [batch]: the symmetry row b draws at (seed, counter), both 64 bits — s = v[0] >> 29 with
    v = philox4x32_10(b, counter & 0xffffffff, counter >> 32, AF_SYM_DRAW_TAG, seed & 0xffffffff, seed >> 32)."""
    from .replay import philox4x32_10        # af_philox4x32 of include/af_noise.h (replay imports torch: not at import time)
    seed, counter = int(seed) & 0xFFFFFFFFFFFFFFFF, int(counter) & 0xFFFFFFFFFFFFFFFF
    b = np.arange(int(batch), dtype=np.uint64)
    v = philox4x32_10(b, counter & 0xFFFFFFFF, counter >> 32, AF_SYM_DRAW_TAG, seed & 0xFFFFFFFF, seed >> 32)
    return (v[0] >> np.uint32(29)).astype(np.int32)


def apply_reference(planes, syms):
    """[B,3,S,S] -> [B,3,S,S]: row b is transform(planes[b], syms[b]) (the random mode's input side)."""
    planes = np.asarray(planes)
    out = np.empty_like(planes)
    for b, s in enumerate(np.asarray(syms).reshape(-1)[:planes.shape[0]]):
        out[b] = transform(planes[b], s)
    return out


def restore_reference(policy, syms, S):
    """[B,C] -> [B,C]: row b is inverse(policy[b], syms[b]) (the random mode's output side; the value is untouched there)."""
    policy = np.asarray(policy)
    B = policy.shape[0]
    out = np.empty((B, S * S), policy.dtype)
    for b, s in enumerate(np.asarray(syms).reshape(-1)[:B]):
        out[b] = inverse(policy[b].reshape(S, S), s).reshape(-1)
    return out


def check_arguments(mode, board_size, max_batch):
    """What a SymmetricEvaluator can be built with, checked before anything touches the GPU."""
    if mode not in MODES:
        raise ValueError("unknown mode %r: expected one of %s" % (mode, ", ".join(MODES)))
    if not MIN_BOARD <= int(board_size) <= MAX_BOARD:
        raise ValueError("board size %r outside %d..%d" % (board_size, MIN_BOARD, MAX_BOARD))
    if int(max_batch) < 1:
        raise ValueError("max_batch must be at least 1, not %r" % (max_batch,))


class SymmetricEvaluator(object):
    """An evaluator over an evaluator: planes [B,3,S,S] -> (policy [B,C], value [B]) on the device, the inner evaluator seeing
    every leaf under all eight symmetries (mode="mean": af_sym_expand, inner over 8 B rows, af_sym_reduce) or under one drawn
    per leaf (mode="random": af_sym_apply, inner, af_sym_restore).  Launches only, on torch's current stream, so it runs inside
    the captured tick + forward graphs like the evaluators it wraps, and a replayed random-mode capture draws afresh: the draw's
    counter lives on the device.  SelfPlayEngine, DeviceArena and Player take it through the protocol they already have — the
    call, bind_outputs and weights_version.

    make_inner(rows) returns a device evaluator for `rows` positions; it is called once, with 8 * max_batch (mean) or max_batch
    (random).  The weight version is resolved as the engine resolves it (engine.resolve_weights_version) from weights_version=
    or the inner evaluator; the object gets a `weights_version` callable only if one resolves — otherwise the engine's refusals
    for an evaluator that takes bind_outputs but names no version apply (graph replay, the evaluation memo).
    deterministic: whether the evaluator is a pure function of the planes — False in random mode, which the memo refuses."""

    def __init__(self, make_inner, board_size, max_batch, mode="mean", seed=0, device="cuda:0", weights_version=None):
        check_arguments(mode, board_size, max_batch)
        import torch
        from . import sym_hip
        from .engine import resolve_weights_version
        self.mode, self.seed, self.deterministic = mode, int(seed), mode == "mean"
        self.S, self.C, self.max_batch = int(board_size), int(board_size) ** 2, int(max_batch)
        self.device = torch.device(device)
        self._torch = torch
        self._make_inner, self._explicit_version = make_inner, weights_version
        self.sym = sym_hip.HipSym(self.S, self.max_batch, self.device, seed)
        self.rows = (8 if mode == "mean" else 1) * self.max_batch
        self.inner = make_inner(self.rows)
        f32 = dict(dtype=torch.float32, device=self.device)
        self._planes_t = torch.zeros((self.rows, 3, self.S, self.S), **f32)      # what the inner evaluator reads
        self.policy = torch.zeros((self.max_batch, self.C), **f32)
        self.value = torch.zeros((self.max_batch,), **f32)
        ver, _ = resolve_weights_version(self.inner, weights_version)
        if ver is not None:
            self.weights_version = ver

    @property
    def version(self):
        """The resolved weight version, or None: what Player keys its captured graph on."""
        ver = getattr(self, "weights_version", None)
        return ver() if ver is not None else None

    def bind_outputs(self, policy, value):
        """The results go into the caller's tensors (the engine's: no copy per tick), if they hold max_batch rows."""
        if policy.shape[0] >= self.max_batch:
            assert policy.is_contiguous() and value.is_contiguous() and policy.dtype == self._torch.float32
            self.policy, self.value = policy, value

    def _inner_outputs(self, p, v, rows):
        return p.reshape(rows, self.C).contiguous(), v.reshape(rows).contiguous()

    def __call__(self, planes):
        B = planes.shape[0]
        assert 1 <= B <= self.max_batch
        if self.mode == "mean":
            self.sym.expand(planes, self._planes_t, B)
            p8, v8 = self._inner_outputs(*self.inner(self._planes_t[:8 * B]), 8 * B)
            self.sym.reduce(p8, v8, self.policy, self.value, B)
        else:
            self.sym.apply(planes, self._planes_t, B)
            pt, vt = self._inner_outputs(*self.inner(self._planes_t[:B]), B)
            self.sym.restore(pt, vt, self.policy, self.value, B)
        return self.policy[:B], self.value[:B]

    def eval(self, inputs):
        """numpy float32 [B,3,S,S] -> numpy (policy [B,C], value [B]), copied out (the output tensors are overwritten by the
        next call).  Player(cfg, pv_fn=sym.eval) recognises it and plays on a copy(1) of its own."""
        torch = self._torch
        x = torch.from_numpy(np.ascontiguousarray(inputs, np.float32)).to(self.device)
        p, v = self(x)
        return p.cpu().numpy().copy(), v.cpu().numpy().copy()

    def copy(self, max_batch):
        """A new evaluator of the same mode and seed over an inner evaluator of its own."""
        return SymmetricEvaluator(self._make_inner, self.S, max_batch, mode=self.mode, seed=self.seed, device=self.device,
                                  weights_version=self._explicit_version)

    def close(self):
        """Releases the handle, and the inner evaluator if it has a close()."""
        sym, self.sym = getattr(self, "sym", None), None
        if sym is not None:
            sym.close()
        inner, self.inner = getattr(self, "inner", None), None
        if inner is not None and hasattr(inner, "close"):
            inner.close()


def for_net(net, max_batch, mode="mean", seed=0, **evaluator_kw):
    """SymmetricEvaluator over one of the package's nets on its hand-written kernels: a DeepResNet through evaluators of its
    own (evaluator_kw passes through: precision="int8", act_scales=...), a ResNet through select_backend("hip")."""
    from .network_deep import DeepResNet
    if isinstance(net, DeepResNet):
        make_inner = lambda rows: net.evaluator(rows, **evaluator_kw)  # noqa: E731
    else:
        if evaluator_kw:
            raise TypeError("for_net: %s takes no evaluator arguments (%s)" % (type(net).__name__, ", ".join(sorted(evaluator_kw))))
        make_inner = lambda rows: net.select_backend("hip")  # noqa: E731
    return SymmetricEvaluator(make_inner, net.board_size, max_batch, mode=mode, seed=seed, device=net.device)
