"""Symmetry-averaged and random-symmetry evaluation on the device (include/af_sym.h, alphafive_amd/symmetry.py): the four
kernels bit for bit against the numpy specification, the device-resident draw, SymmetricEvaluator over stubs and over the
real evaluators, under stream capture, inside SelfPlayEngine and behind Player."""
import os

import numpy as np
import pytest

from alphafive_amd import symmetry
from conftest import GOLDEN, make_cfg
from test_gpu_graph_loop import _drain, _same_episodes
from test_symmetry_cpu import mixed_rows

pytestmark = pytest.mark.gpu
W = os.path.join(GOLDEN, "alphaFive-6960.weights.npz")
SIZES, BATCHES, MAX_BATCH = (3, 4, 11, 15, 16), (1, 3, 67), 67
SENTINEL = -7.0


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()


def index_planes(B, S):
    """A distinct value per element: flat index + 0.5 (at most 17 significant bits, so k * (x / 2 + 1 / 4) is exact for k <= 8)."""
    return (np.arange(B * 3 * S * S, dtype=np.float32) + np.float32(0.5)).reshape(B, 3, S, S)


def board_planes(B, S, seed):
    """Random positions in the nets' input encoding: mine / theirs / last move, 0 or 1."""
    rng = np.random.RandomState(seed)
    x = np.zeros((B, 3, S * S), np.float32)
    for b in range(B):
        cells = rng.permutation(S * S)[:rng.randint(2, S * S // 2)]
        x[b, 0, cells[0::2]] = 1
        x[b, 1, cells[1::2]] = 1
        x[b, 2, cells[1]] = 1
    return x.reshape(B, 3, S, S)


class Stub5(object):
    """Not equivariant: a fixed random C x C matrix applied with torch to a mix of the three planes."""

    def __init__(self, S, seed=9):
        import torch
        g = torch.Generator().manual_seed(seed)
        self.C = S * S
        self.M = (torch.rand((self.C, self.C), generator=g) * 0.9 + 0.1).cuda()
        self.bias = (torch.rand((self.C,), generator=g) * 0.5 + 0.01).cuda()
        self.w = ((torch.rand((self.C,), generator=g) - 0.5) * 0.3).cuda()

    def __call__(self, planes):
        import torch
        B = planes.shape[0]
        x = (planes[:, 0] + planes[:, 1] * 0.5 + planes[:, 2] * 0.25).reshape(B, self.C)
        return x @ self.M + self.bias, torch.tanh((x * self.w).sum(1))

    def host(self, planes_np):
        p, v = self(_dev(planes_np))
        return p.cpu().numpy(), v.cpu().numpy()


def stub4(planes):
    """Equivariant: the policy is the first plane, cell by cell; the value is constant."""
    import torch
    B = planes.shape[0]
    return planes[:, 0].reshape(B, -1) * 0.5 + 0.25, torch.full((B,), 0.375, dtype=torch.float32, device=planes.device)


# ---- 1. expand and apply ----
@pytest.mark.parametrize("batch", BATCHES)
@pytest.mark.parametrize("S", SIZES)
def test_expand_and_apply_equal_the_spec(S, batch):
    import torch
    from alphafive_amd.sym_hip import HipSym
    seed = 21
    h = HipSym(S, MAX_BATCH, "cuda:0", seed)
    x = index_planes(batch, S)
    xd = _dev(x)
    out8 = torch.full((8 * batch + 1, 3, S, S), SENTINEL, dtype=torch.float32, device="cuda")
    h.expand(xd, out8, batch)
    got = out8.cpu().numpy()
    assert np.array_equal(_bits(got[:8 * batch]), _bits(symmetry.expand_reference(x)))
    assert (got[8 * batch] == SENTINEL).all()
    # the kernel's index arithmetic is cell_map: a plane of cell numbers comes out as the map itself
    cells = np.zeros((1, 3, S, S), np.float32)
    cells[0, :] = np.arange(S * S, dtype=np.float32).reshape(S, S)
    h.expand(_dev(cells), out8, 1)
    got = out8[:8].cpu().numpy()
    for s in range(8):
        assert np.array_equal(got[s, 1].reshape(-1).astype(np.int32), symmetry.cell_map(S, s)), s
    out = torch.full((batch + 1, 3, S, S), SENTINEL, dtype=torch.float32, device="cuda")
    h.apply(xd, out, batch)
    counter, syms = h.state(batch)
    want = symmetry.draw_reference(batch, seed, 0)
    assert counter == 0 and np.array_equal(syms, want)                 # apply does not move the counter
    got = out.cpu().numpy()
    assert np.array_equal(_bits(got[:batch]), _bits(symmetry.apply_reference(x, want)))
    assert (got[batch] == SENTINEL).all()
    if batch < MAX_BATCH:
        assert (h.state()[1][batch:] == 0).all()                       # rows beyond the batch are not drawn for
    h.close()


# ---- 2. reduce ----
def _reduce_inputs(batch, C):
    p8, v8 = mixed_rows(8 * batch, C, seed=5), mixed_rows(8 * batch, 1, seed=6).reshape(-1)
    flat = p8.reshape(-1)
    flat[::7] = np.float32(-0.0)
    flat[3::11] = np.float32(1e-40)                                    # subnormals
    flat[5::13] = np.float32(-3e-41)
    p8[8 * (batch - 1) + 3] = np.inf                                   # one inf row ...
    p8[8 * (batch - 1) + 5, ::2] = -np.inf                             # ... against -inf in half of another: NaN in the spec
    S = int(round(C ** 0.5))
    p8[8 * (batch - 1):8 * batch, [0, S - 1, C - S, C - 1]] = np.float32(-0.0)   # the corners, an orbit: sums of eight -0.0
    v8[::5] = np.float32(-0.0)
    v8[1::9] = np.float32(1e-40)
    return p8, v8


@pytest.mark.parametrize("batch", BATCHES)
@pytest.mark.parametrize("S", SIZES)
def test_reduce_equals_the_spec(S, batch):
    import torch
    from alphafive_amd.sym_hip import HipSym
    C = S * S
    h = HipSym(S, MAX_BATCH, "cuda:0", 0)
    p8, v8 = _reduce_inputs(batch, C)
    pol = torch.full((batch + 1, C), SENTINEL, dtype=torch.float32, device="cuda")
    val = torch.full((batch + 1,), SENTINEL, dtype=torch.float32, device="cuda")
    h.reduce(_dev(p8), _dev(v8), pol, val, batch)
    want_p, want_v = symmetry.reduce_reference(p8, v8, S)
    got_p, got_v = pol.cpu().numpy(), val.cpu().numpy()
    nan = np.isnan(want_p)
    assert nan.any() and np.isinf(want_p).any() and (_bits(want_p) == 0x80000000).any()
    assert np.array_equal(np.isnan(got_p[:batch]), nan)                # NaN where the spec is NaN
    assert np.array_equal(_bits(got_p[:batch])[~nan], _bits(want_p)[~nan])
    assert np.array_equal(_bits(got_v[:batch]), _bits(want_v))
    assert (got_p[batch] == SENTINEL).all() and got_v[batch] == SENTINEL
    h.close()


# ---- 3. draws ----
@pytest.mark.parametrize("seed", (21, 2 ** 63 + 5))
def test_draws_follow_the_device_counter(seed):
    import torch
    from alphafive_amd.sym_hip import HipSym
    S, batch = 11, 67
    C = S * S
    h = HipSym(S, MAX_BATCH, "cuda:0", seed)
    x = index_planes(batch, S)
    xd = _dev(x)
    xt = torch.empty_like(xd)
    pol = torch.empty((batch, C), dtype=torch.float32, device="cuda")
    val_t = torch.arange(batch, dtype=torch.float32, device="cuda")
    val = torch.zeros(batch, dtype=torch.float32, device="cuda")

    def pair(counter):
        h.apply(xd, xt, batch)
        h.restore(xt[:, 0].reshape(batch, C).contiguous(), val_t, pol, val, batch)     # the first plane as the policy
        got_counter, syms = h.state(batch)
        assert got_counter == counter + 1
        assert np.array_equal(syms, symmetry.draw_reference(batch, seed, counter)), counter
        assert np.array_equal(_bits(xt.cpu().numpy()), _bits(symmetry.apply_reference(x, syms)))
        assert np.array_equal(_bits(pol.cpu().numpy()), _bits(x[:, 0].reshape(batch, C)))   # restore(apply(x)) == x
        assert torch.equal(val, val_t)

    assert h.state(batch)[0] == 0
    for k in range(3):
        pair(k)
    h.set_counter(2 ** 32 - 1)
    pair(2 ** 32 - 1)
    pair(2 ** 32)                                                     # the carry reached the high word
    # a second restore without a new apply uses the stored symmetries (and moves the counter once more)
    pol.zero_()
    h.restore(xt[:, 0].reshape(batch, C).contiguous(), val_t, pol, val_t, batch)       # value in place: nothing to move
    assert np.array_equal(_bits(pol.cpu().numpy()), _bits(x[:, 0].reshape(batch, C)))
    assert h.state(batch)[0] == 2 ** 32 + 2
    h.close()


def test_binding_refuses_what_the_library_refuses():
    import torch
    from alphafive_amd.sym_hip import HipSym, SymError
    h = HipSym(4, 2, "cuda:0", 0)
    x = torch.zeros((3, 3, 4, 4), dtype=torch.float32, device="cuda")
    y = torch.zeros((24, 3, 4, 4), dtype=torch.float32, device="cuda")
    for call in (lambda: h.expand(x, y, 3), lambda: h.expand(x, y, 0), lambda: h.apply(x, x, 2)):
        with pytest.raises(SymError) as e:
            call()
        assert e.value.code == -1
    with pytest.raises(SymError):
        h.expand(x.double(), y, 1)
    with pytest.raises(SymError):
        h.expand(x, y[:8], 2)                                         # too few rows for the batch
    h.close()


# ---- 4. / 5. stubs through SymmetricEvaluator ----
@pytest.mark.parametrize("mode", symmetry.MODES)
def test_equivariant_stub_comes_back_unchanged(mode):
    S, B = 11, 3
    x = index_planes(B, S)
    sym = symmetry.SymmetricEvaluator(lambda rows: stub4, S, B, mode=mode, seed=3)
    assert sym.deterministic == (mode == "mean") and not hasattr(sym, "weights_version") and sym.version is None
    p, v = sym(_dev(x))
    want_p, want_v = stub4(_dev(x))
    assert np.array_equal(_bits(p.cpu().numpy()), _bits(want_p.cpu().numpy()))
    assert np.array_equal(_bits(v.cpu().numpy()), _bits(want_v.cpu().numpy()))
    sym.close()
    assert sym.sym is None


@pytest.mark.parametrize("S,B", ((11, 3), (6, 8)))
def test_stub_that_is_not_equivariant_equals_the_spec_on_the_host(S, B):
    import torch
    stub = Stub5(S)
    x = board_planes(B, S, seed=1) + index_planes(B, S) * np.float32(1e-3)
    rows_asked = []

    def make(rows):
        rows_asked.append(rows)
        return stub

    mean = symmetry.SymmetricEvaluator(make, S, B, mode="mean")
    p, v = mean(_dev(x))
    want_p, want_v = symmetry.reduce_reference(*stub.host(symmetry.expand_reference(x)), S)
    assert np.array_equal(_bits(p.cpu().numpy()), _bits(want_p)) and np.array_equal(_bits(v.cpu().numpy()), _bits(want_v))
    assert not np.array_equal(want_p, stub.host(x)[0])                # the stub really is not equivariant
    # into the caller's tensors; eval() is numpy in, copies out
    pol = torch.zeros((B, S * S), dtype=torch.float32, device="cuda")
    val = torch.zeros((B,), dtype=torch.float32, device="cuda")
    mean.bind_outputs(pol, val)
    p, v = mean(_dev(x))
    assert p.data_ptr() == pol.data_ptr() and v.data_ptr() == val.data_ptr()
    assert np.array_equal(_bits(pol.cpu().numpy()), _bits(want_p))
    ep, ev = mean.eval(x[:1])
    assert np.array_equal(_bits(ep), _bits(want_p[:1])) and np.array_equal(_bits(ev), _bits(want_v[:1]))
    mean.bind_outputs(pol[:B - 1], val[:B - 1])                       # too few rows: not taken
    assert mean.policy.data_ptr() == pol.data_ptr() and mean.policy.shape[0] == B

    seed = 2 ** 63 + 5
    rnd = symmetry.SymmetricEvaluator(make, S, B, mode="random", seed=seed, weights_version=4)
    assert rnd.weights_version() == 4 and rnd.version == 4
    for counter in range(2):
        p, v = rnd(_dev(x))
        syms = symmetry.draw_reference(B, seed, counter)
        pt, vt = stub.host(symmetry.apply_reference(x, syms))
        assert np.array_equal(_bits(p.cpu().numpy()), _bits(symmetry.restore_reference(pt, syms, S))), counter
        assert np.array_equal(_bits(v.cpu().numpy()), _bits(vt))
    cp = rnd.copy(2)
    assert (cp.mode, cp.seed, cp.max_batch, cp.version) == ("random", seed, 2, 4) and cp.sym is not rnd.sym
    assert rows_asked == [8 * B, B, 2]
    for e in (mean, rnd, cp):
        e.close()


# ---- 6. the real evaluators ----
def _real_case(name):
    from alphafive_amd.network import ResNet
    from alphafive_amd.network_deep import DeepResNet
    if name == "resnet":
        net = ResNet(11, device="cuda")
        net.load_npz(W)
        return net, 3, {}
    if name == "deep15":
        return DeepResNet(15, blocks=2, device="cuda", seed=3), 2, {}
    net = DeepResNet(11, blocks=2, device="cuda", seed=3)
    if name == "deep_int8":
        return net, 3, dict(precision="int8", act_scales=net.calibrate_int8(board_planes(16, 11, seed=2)))
    return net, 3, {}


@pytest.mark.parametrize("name", ("resnet", "deep_bf16", "deep_int8", "deep15"))
def test_mean_over_the_real_evaluators(name):
    net, B, kw = _real_case(name)
    S = net.board_size
    x = board_planes(B, S, seed=7)
    sym = symmetry.for_net(net, B, mode="mean", **kw)
    assert sym.rows == 8 * B and callable(sym.weights_version)
    p, v = sym(_dev(x))
    got_p, got_v = p.cpu().numpy().copy(), v.cpu().numpy().copy()
    p8, v8 = sym.inner(_dev(symmetry.expand_reference(x)))             # the same inner evaluator, run separately at batch 8B
    want_p, want_v = symmetry.reduce_reference(p8.cpu().numpy(), v8.cpu().numpy(), S)
    assert np.array_equal(_bits(got_p), _bits(want_p)) and np.array_equal(_bits(got_v), _bits(want_v))
    assert np.isfinite(got_p).all() and abs(got_p.sum(1) - 1).max() < 1e-3
    # the average is symmetric although the net is not: the evaluation of a transformed position is the transformed evaluation
    # (to rounding: the eight terms are the same numbers, added in another order)
    p1, _ = sym.inner(_dev(x))
    assert np.abs(p1.cpu().numpy()[:B] - got_p).max() > 1e-6
    for s in (1, 6):
        ps, vs = sym(_dev(symmetry.transform(x, s)))
        back = symmetry.inverse(ps.cpu().numpy().reshape(B, S, S), s).reshape(B, S * S)
        assert np.abs(back - got_p).max() < 1e-6 and np.abs(vs.cpu().numpy() - got_v).max() < 1e-6
    sym.close()
    net.close()


# ---- 7. capture ----
def test_random_mode_draws_afresh_on_every_replay():
    import torch
    S, B, seed = 11, 5, 77
    stub = Stub5(S)
    x = board_planes(B, S, seed=4) + index_planes(B, S) * np.float32(1e-3)
    xd = _dev(x)
    sym = symmetry.SymmetricEvaluator(lambda rows: stub, S, B, mode="random", seed=seed)
    sym(xd)                                                           # warm-up outside the capture: counter 0 -> 1
    torch.cuda.synchronize()
    c = sym.sym.state(B)[0]
    assert c == 1
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, capture_error_mode="thread_local"):
        p, v = sym(xd)
    assert sym.sym.state(B)[0] == c                                   # the capture recorded the launches, it did not run them
    seen = []
    for k in range(3):
        g.replay()
        counter, syms = sym.sym.state(B)
        want = symmetry.draw_reference(B, seed, c + k)
        assert counter == c + k + 1 and np.array_equal(syms, want), k
        pt, vt = stub.host(symmetry.apply_reference(x, want))
        assert np.array_equal(_bits(p.cpu().numpy()), _bits(symmetry.restore_reference(pt, want, S))), k
        assert np.array_equal(_bits(v.cpu().numpy()), _bits(vt))
        seen.append(tuple(syms))
    assert len(set(seen)) == 3
    del g
    sym.close()


# ---- 8. SelfPlayEngine ----
def _composed(stub, S):
    """The spec's operations in the spec's order, on torch ops."""
    import torch

    def t(a, s):
        a = torch.rot90(a, s & 3, dims=(-2, -1))
        return torch.flip(a, dims=(-2,)) if s >> 2 else a

    def inv(a, s):
        a = torch.flip(a, dims=(-2,)) if s >> 2 else a
        return torch.rot90(a, -(s & 3), dims=(-2, -1))

    def pv(planes):
        B = planes.shape[0]
        x8 = torch.stack([t(planes, s) for s in range(8)], 1).reshape(8 * B, 3, S, S).contiguous()
        p8, v8 = stub(x8)
        p8, v8 = p8.reshape(B, 8, S, S), v8.reshape(B, 8)
        pol, val = p8[:, 0], v8[:, 0]
        for s in range(1, 8):
            pol, val = pol + inv(p8[:, s], s), val + v8[:, s]
        return (pol * 0.125).reshape(B, S * S), val * 0.125

    return pv


def test_selfplay_engine_graph_eager_and_composed_agree():
    from alphafive_amd.engine import SelfPlayEngine, EngineError
    S, G = 6, 8
    cfg = make_cfg(board_size=S, goal=4, simulation_per_step=16, upper_simulation_per_step=20)
    stub = Stub5(S)
    mk = lambda mode, **kw: symmetry.SymmetricEvaluator(lambda rows: stub, S, G, mode=mode, seed=5, **kw)   # noqa: E731
    evs = [mk("mean", weights_version=0), mk("mean", weights_version=0)]
    a = SelfPlayEngine(cfg, G, evs[0], device=0, seed=13)
    b = SelfPlayEngine(cfg, G, evs[1], device=0, seed=13)
    c = SelfPlayEngine(cfg, G, _composed(stub, S), device=0, seed=13)
    assert evs[0].policy.data_ptr() == a.policy.data_ptr()           # bound: the engine copies nothing per tick
    for _ in range(40):
        a.run_ticks_graph(16)
    assert a._graph is not None
    b.run_ticks(a.ticks)
    c.run_ticks(a.ticks)
    got = []
    for sp in (a, b, c):
        sp.check()
        got.append(_drain(sp))
    assert len(got[0]) >= G // 2
    assert a.counters() == b.counters() == c.counters()
    _same_episodes(got[0], got[1])
    _same_episodes(got[0], got[2])
    for sp in (a, b, c):
        sp.close()
    # the memo stores an evaluation per position: refused for an evaluator that draws per leaf, taken for the average
    rnd = mk("random", weights_version=0)
    with pytest.raises(EngineError, match="deterministic"):
        SelfPlayEngine(cfg, G, rnd, device=0, seed=13, eval_memo=True)
    m = SelfPlayEngine(cfg, G, evs[0], device=0, seed=13, eval_memo=True)
    m.run_ticks(20)
    m.check()
    m.close()
    # ... and without a version the engine's refusals for one of its own evaluators apply
    plain = mk("mean")
    e = SelfPlayEngine(cfg, G, plain, device=0, seed=13)
    e.tick()
    with pytest.raises(EngineError, match="weights_version"):
        e.run_ticks_graph(4)
    e.close()
    for ev in evs + [rnd, plain]:
        ev.close()


# ---- 9. Player ----
def test_player_plays_on_a_copy_and_equals_the_spec_composed_on_the_host():
    from alphafive_amd import utils
    from alphafive_amd.network import ResNet
    from alphafive_amd.player import Player
    S = 11
    net = ResNet(S, device="cuda")
    net.load_npz(W)
    cfg = make_cfg(simulation_per_step=32, upper_simulation_per_step=40)
    sym = symmetry.for_net(net, 1, mode="mean")

    def host_fn(x):
        return symmetry.reduce_reference(*net.eval(symmetry.expand_reference(x)), S)

    a = Player(cfg, pv_fn=sym.eval, seed=4, game_id=0)
    b = Player(cfg, pv_fn=host_fn, seed=4, game_id=0)
    assert a.backend == "hip" and b.backend == "host"
    copy = a._pv_close
    assert isinstance(copy, symmetry.SymmetricEvaluator) and copy is not sym and copy.max_batch == 1 and copy.mode == "mean"
    assert copy.policy.data_ptr() == a._policy.data_ptr()
    state, last = a.get_init_state(), None
    for _ in range(2):
        pa, aa = a.get_action(state, last_action=last)
        pb, ab = b.get_action(state, last_action=last)
        assert aa == ab and (a.last_visits == b.last_visits).all() and a.last_visits.sum() > 0
        assert np.array_equal(_bits(pa), _bits(pb))
        board = utils.step(utils.state_to_board(state, S), aa)
        state, last = utils.board_to_state(board), aa
    assert a._graph is not None                                       # the copy ran inside the captured tick + forward graph
    a.close()
    b.close()
    assert a._pv_close is None and copy.sym is None and copy.inner is None
    assert sym.sym is not None                                        # the caller's evaluator is the caller's
    sym.close()
    net.close()
