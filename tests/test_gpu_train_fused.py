"""Trainer(fused=True) on the device: the three kernels of libaf_train.so (include/af_train.h) against their specifications
(train_hip.loss_head_reference in fp64, train_hip.adam_reference bit for bit), and the Trainer built on them against the fp64
restatement of the loss, the eager Trainer, its own checkpoints and the evaluator's weight hand-over.
The last section holds every kernel to its specification element by element on the cases of tests/train_cases.py (the rules
are stated there): the loss head inside 2^-40 intervals around fp64 on all five kernels, Adam, its L2 partials and finalize
bit for bit, and four Trainer steps on three nets bit for bit from what the step really fed its kernels."""
import ctypes as C
import os

import numpy as np
import pytest

import train_cases as tc
from conftest import GOLDEN
from test_train_cpu import _batch

pytestmark = pytest.mark.gpu

W = os.path.join(GOLDEN, "alphaFive-6960.weights.npz")
BETA1, BETA2, EPS, L2 = 0.9, 0.999, 1e-8, 4e-5
U = 2.0 ** -24                                                      # unit roundoff of fp32


def _lr_t(t, lr=1e-3):
    return float(lr * np.sqrt(1.0 - BETA2 ** t) / (1.0 - BETA1 ** t))  # Trainer.step


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---------------------------------------------------------------- loss head
def _head_inputs(B, Cn, seed):
    """logits N(0, 3); with three rows or more: row 0 scaled so that its largest |z| is 40 (the max subtraction matters), row 1
    all equal, pi row 0 one-hot; the last row's pi always holds exact zeros.  weights in [0.5, 1.5], winner +-1."""
    rng = np.random.RandomState(seed)
    z = (rng.randn(B, Cn) * 3).astype(np.float32)
    pi = np.exp(rng.randn(B, Cn))
    pi[B - 1, rng.rand(Cn) < 0.5] = 0.0
    pi[B - 1, 0] = 1.0
    if B >= 3:
        z[0] *= np.float32(40.0) / np.abs(z[0]).max()
        z[1] = np.float32(1.25)
        pi[0] = 0.0
        pi[0, Cn // 2] = 1.0
    pi = (pi / pi.sum(axis=1, keepdims=True)).astype(np.float32)
    value = np.tanh(rng.randn(B)).astype(np.float32)
    winner = rng.choice([-1.0, 1.0], size=B).astype(np.float32)
    weight = (0.5 + rng.rand(B)).astype(np.float32)
    return z, value, pi, winner, weight


@pytest.mark.parametrize("B,Cn", [(5, 36), (5, 121), (3, 225), (1, 64), (1, 65), (512, 121)])
def test_loss_head_is_as_close_to_fp64_as_the_torch_ops_it_replaces(B, Cn):
    """Yardstick: the largest absolute error, against fp64, of train.loss_terms's torch-fp32 ops on the same logits and value
    on the device (autograd on two leaf tensors).  The kernel may err at most 4x that (different but legitimate summation
    orders of quantities that are a few ulps each), with a floor of 1e-7; separately for dlogits, dvalue and each scalar."""
    import torch
    from alphafive_amd import train, train_hip
    host = _head_inputs(B, Cn, seed=B * 1000 + Cn)
    ref_dl, ref_dv, ref_rows = train_hip.loss_head_reference(*host)
    ref_terms = train_hip.terms_reference(ref_rows, 0.0)
    z, value, pi, winner, weight = (torch.from_numpy(a).cuda() for a in host)
    # the parent's arithmetic
    zl, vl = z.clone().requires_grad_(True), value.clone().requires_grad_(True)
    t = train.loss_terms({}, None, pi, winner, weight, forward=lambda params, x: (zl, vl))
    gl, gv = torch.autograd.grad(t["total"], [zl, vl])
    # the kernels
    dl, dv, rows = train_hip.loss_head(z, value, pi, winner, weight)
    terms = train_hip.finalize(rows, None, 0, L2).cpu().numpy().astype(np.float64)
    err = lambda got, ref: float(np.abs(got.detach().cpu().numpy().astype(np.float64) - ref).max())  # noqa: E731
    pairs = [("dlogits", err(dl, ref_dl), err(gl, ref_dl)), ("dvalue", err(dv, ref_dv), err(gv, ref_dv))]
    for i, k in enumerate(("total", "cross_entropy", "value_loss", "entropy")):
        pairs.append((k, abs(terms[i] - ref_terms[k]), abs(float(t[k]) - ref_terms[k])))
    for name, mine, torchs in pairs:
        print("loss head (%d, %d) %-13s kernel %.3e   torch fp32 %.3e" % (B, Cn, name, mine, torchs))
    for name, mine, torchs in pairs:
        assert mine <= max(4.0 * torchs, 1e-7), (name, mine, torchs)
    assert np.isfinite(rows.cpu().numpy()).all()
    # a rerun gives the same bits
    dl2, dv2, rows2 = train_hip.loss_head(z, value, pi, winner, weight)
    terms2 = train_hip.finalize(rows2, None, 0, L2)
    assert torch.equal(dl, dl2) and torch.equal(dv, dv2) and torch.equal(rows, rows2)
    assert np.array_equal(_bits(terms2.cpu().numpy()), _bits(terms.astype(np.float32)))


def test_loss_head_refuses_bad_arguments():
    import torch
    from alphafive_amd import train_hip
    L = train_hip.lib()
    x = torch.zeros(8, device="cuda")
    p = x.data_ptr()
    assert L.af_train_loss_head(None, 1, 1025, p, p, p, p, p, p, p, p) == train_hip.ERR_RANGE
    assert L.af_train_loss_head(None, 0, 4, p, p, p, p, p, p, p, p) == train_hip.ERR_ARG
    assert L.af_train_loss_head(None, 1, 4, p, p, None, p, p, p, p, p) == train_hip.ERR_ARG
    assert L.af_train_finalize(None, 1, None, 0, None, 0.0, p) == train_hip.ERR_ARG
    with pytest.raises(train_hip.TrainError):
        train_hip.loss_head(torch.zeros((2, 4), device="cuda"), x[:2], torch.zeros((2, 5), device="cuda"), x[:2], x[:2])


# ---------------------------------------------------------------- Adam
SIZES = [1, 3, 63, 64, 65, 257, 1025, 128 * 128 * 9]


def _adam_state(sizes, seed):
    rng = np.random.RandomState(seed)
    p = [(rng.randn(n) * 0.1).astype(np.float32) for n in sizes]
    return p, [np.zeros(n, np.float32) for n in sizes], [np.zeros(n, np.float32) for n in sizes]


def _grads(sizes, rng):
    out = []
    for n in sizes:
        g = (rng.randn(n) * 1e-2).astype(np.float32)
        g[rng.rand(n) < 0.25] = 0.0                                 # with v = 0: m / eps, and 0 / eps
        out.append(g)
    return out


def test_adam_equals_its_numpy_specification_bit_for_bit():
    """Three consecutive steps (lr_t of t = 1, 2, 3) and one with t = 1000 over variables of every size around the wave, the
    workgroup and the chunk, mixed decay flags; p, m and v after each step are adam_reference's bits."""
    import torch
    from alphafive_amd import train_hip
    decay = [True, False, True, False, True, False, True, True]    # mixed; the 72-chunk variable is under it, for the L2 sum
    p, m, v = _adam_state(SIZES, 0)
    dev = lambda arrs: [torch.from_numpy(a.copy()).cuda() for a in arrs]  # noqa: E731
    dp, dm, dv = dev(p), dev(m), dev(v)
    table = train_hip.VarTable(dp, dm, dv, decay)
    assert table.n_partials == sum(-(-n // train_hip.ADAM_CHUNK) for n in SIZES) == 7 + 72
    partials = torch.full((table.n_partials,), -1.0, device="cuda")
    rng = np.random.RandomState(1)
    for t in (1, 2, 3, 1000):
        g = _grads(SIZES, rng)
        lr_t = _lr_t(t)
        table.set_grads(dev(g))
        p_before = [a.copy() for a in p]
        assert train_hip.adam(table, lr_t, BETA1, BETA2, EPS, L2, partials) == table.n_partials
        for i in range(len(SIZES)):
            p[i], m[i], v[i] = train_hip.adam_reference(p[i], g[i], m[i], v[i], decay[i], lr_t, BETA1, BETA2, EPS, L2)
            for name, got, ref in (("p", dp[i], p[i]), ("m", dm[i], m[i]), ("v", dv[i], v[i])):
                bad = _bits(got.cpu().numpy()) != _bits(ref)
                assert not bad.any(), "t=%d variable %d (%d elements) %s: %d elements differ" % (t, i, SIZES[i], name, bad.sum())
        _check_l2(train_hip, partials, p_before, decay)
    assert all(np.isfinite(a).all() for a in p)


def _check_l2(train_hip, partials, p_before, decay):
    """The L2 share of terms[0] = l2_coef * sum(p^2) / 2 over the decay variables, p before the update.  It is a reduction of
    positive terms, so it is held to the fp64 sum with the bound of its blocking: a workgroup sums a chunk of ADAM_CHUNK = 2048
    elements into one partial and af_train_finalize sums the P partials.  However the adds inside a block and over the blocks
    are arranged (here: 8 per thread in sequence + a 6-level butterfly + 3 adds over the waves; then ceil(P / 256) per thread
    + the same tree), no term passes through more than 2048 adds in its block and P adds over the blocks, plus the rounding of
    its own square: d = P + 2048 + 1 roundings, relative error <= d u / (1 - d u).  Three more roundings follow: l2_coef to
    fp32, the halving (exact) and the product."""
    import torch
    P = partials.numel()
    exact = sum(float((a.astype(np.float64) ** 2).sum()) for a, d in zip(p_before, decay) if d)
    d = P + train_hip.ADAM_CHUNK + 1
    bound = d * U / (1 - d * U)
    got = partials.cpu().numpy().astype(np.float64)
    assert (got >= 0).all()
    # per variable: its own partials against its own sum
    off = 0
    for a, dec in zip(p_before, decay):
        k = -(-a.size // train_hip.ADAM_CHUNK)
        s = float((a.astype(np.float64) ** 2).sum()) if dec else 0.0
        dk = k + train_hip.ADAM_CHUNK + 1
        assert abs(got[off:off + k].sum() - s) <= dk * U / (1 - dk * U) * s, (a.size, dec)
        off += k
    terms = train_hip.finalize(torch.zeros((1, train_hip.ROW_TERMS), dtype=torch.float64, device="cuda"), partials, P, L2).cpu().numpy()
    assert terms[1] == 0 and terms[2] == 0 and terms[3] == 0
    ref = L2 * exact / 2
    assert abs(float(terms[0]) - ref) <= (bound + 3 * U) * 1.001 * ref, (float(terms[0]), ref)


def test_adam_over_more_variables_than_one_table_holds():
    """70 variables of 5 elements: 64 in the first launch, 6 in the second, partials 0..63 and 64..69."""
    import torch
    from alphafive_amd import train_hip
    sizes = [5] * 70
    decay = [i % 3 != 0 for i in range(70)]
    p, m, v = _adam_state(sizes, 2)
    g = _grads(sizes, np.random.RandomState(3))
    dev = lambda arrs: [torch.from_numpy(a.copy()).cuda() for a in arrs]  # noqa: E731
    dp, dg, dm, dv = dev(p), dev(g), dev(m), dev(v)
    partials = torch.full((70,), -1.0, device="cuda")
    assert train_hip.adam(list(zip(dp, dg, dm, dv, decay)), _lr_t(1), BETA1, BETA2, EPS, L2, partials) == 70
    for i in range(70):
        rp, rm, rv = train_hip.adam_reference(p[i], g[i], m[i], v[i], decay[i], _lr_t(1), BETA1, BETA2, EPS, L2)
        for got, ref in ((dp[i], rp), (dm[i], rm), (dv[i], rv)):
            assert np.array_equal(_bits(got.cpu().numpy()), _bits(ref)), i
    _check_l2(train_hip, partials, p, decay)


def test_adam_refuses_bad_arguments_and_launches_nothing():
    import torch
    from alphafive_amd import train_hip
    L = train_hip.lib()
    t = [torch.full((8,), 0.5, device="cuda") for _ in range(4)]
    partials = torch.full((4,), -1.0, device="cuda")
    arr = (train_hip.Var * 65)()
    for e in arr:
        e.p, e.g, e.m, e.v, e.n, e.decay = t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), t[3].data_ptr(), 8, 1
    args = (0.1, BETA1, BETA2, EPS, L2, partials.data_ptr())
    assert L.af_train_adam(None, 65, arr, *args) == train_hip.ERR_ARG          # one more than the table holds
    assert L.af_train_adam(None, 0, arr, *args) == train_hip.ERR_ARG
    assert L.af_train_adam(None, 1, None, *args) == train_hip.ERR_ARG
    assert L.af_train_adam(None, 1, arr, 0.1, BETA1, BETA2, EPS, L2, None) == train_hip.ERR_ARG
    arr[1].g = None
    assert L.af_train_adam(None, 2, arr, *args) == train_hip.ERR_ARG           # a null pointer in the second entry
    arr[1].g, arr[1].n = t[1].data_ptr(), -1
    assert L.af_train_adam(None, 2, arr, *args) == train_hip.ERR_ARG           # n < 0
    assert L.af_train_adam_partials(1, (C.c_int64 * 1)(-1)) == train_hip.ERR_ARG
    torch.cuda.synchronize()
    assert all(bool((x == 0.5).all()) for x in t) and bool((partials == -1.0).all())
    assert train_hip.lib().af_train_strerror(train_hip.ERR_ARG) == b"bad argument"
    with pytest.raises(train_hip.TrainError):
        train_hip.adam([(t[0], t[1][:4], t[2], t[3], True)], 0.1, BETA1, BETA2, EPS, L2, partials)


# ---------------------------------------------------------------- Trainer
S, NB = 6, 32


def _trainer(variables, S=S, **kw):
    from alphafive_amd import train
    return train.Trainer(variables, S, device="cuda", **kw)


@pytest.fixture(scope="module")
def net6():
    from alphafive_amd.network import ResNet
    return ResNet(S, device="cpu", seed=4)


def test_first_fused_step_logs_the_fp64_loss_and_training_lowers_it(net6):
    from oracle import net_fp64
    boards, weights, winner, pol = _batch(S, NB, seed=1)
    tr = _trainer(net6.variables, fused=True)
    assert tr.step(boards, weights, winner, pol, lr=1e-3, metrics=False) is None
    tr = _trainer(net6.variables, fused=True)
    m0 = tr.step(boards, weights, winner, pol, lr=1e-3)
    ref = net_fp64.loss_terms(net6.variables, boards, pol, winner, weights)
    for k in ("total", "cross_entropy", "value_loss", "entropy"):
        print("fused step 1 %-13s %.8f   fp64 %.8f" % (k, m0[k], ref[k]))
        assert abs(m0[k] - ref[k]) < 2e-5 * max(1.0, abs(ref[k])), k
    last = m0
    for _ in range(15):
        last = tr.step(boards, weights, winner, pol, lr=1e-3)
    assert last["total"] < m0["total"] - 0.05


def test_one_fused_step_lands_on_the_eager_one(net6):
    """The first step moves every element by about lr * sign(g) whatever |g| is, so where g is rounding noise the step is
    arbitrary: compare the elements whose eager |g| exceeds 1e-4 of their variable's largest; at most 5 % may be left out."""
    import torch
    from alphafive_amd import train
    lr = 1e-3
    boards, weights, winner, pol = _batch(S, NB, seed=1)
    eager, fused = _trainer(net6.variables), _trainer(net6.variables, fused=True)
    dev = lambda a: torch.from_numpy(a).cuda()  # noqa: E731
    terms = train.loss_terms(eager.params, dev(boards), dev(pol), dev(winner), dev(weights))
    g = dict(zip(eager.params, torch.autograd.grad(terms["total"], list(eager.params.values()))))
    eager.step(boards, weights, winner, pol, lr=lr)
    fused.step(boards, weights, winner, pol, lr=lr)
    a, b = eager.variables(), fused.variables()
    left_out = total = 0
    for k in a:
        ga = g[k].abs().cpu().numpy()
        keep = ga > 1e-4 * ga.max()
        left_out += int((~keep).sum())
        total += keep.size
        assert np.abs(a[k] - b[k])[keep].max() <= 1e-3 * lr, k
    print("fused vs eager: %d of %d elements left out (%.3f %%)" % (left_out, total, 100.0 * left_out / total))
    assert left_out < 0.05 * total


def _same_state(a, b):
    sa, sb = a.state_dict(), b.state_dict()
    assert sa["t"] == sb["t"]
    for key in ("params", "m", "v"):
        for k in sa[key]:
            assert np.array_equal(_bits(sa[key][k]), _bits(sb[key][k])), (key, k)


@pytest.fixture
def deterministic_autograd():
    """Bit-identical continuation needs bit-identical gradients, and the convolutions' backward passes (MIOpen, through PyTorch
    autograd: not this path's code) may pick solvers that accumulate with atomics unless asked not to."""
    import torch
    was = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    yield
    torch.backends.cudnn.deterministic = was


def test_fused_state_round_trips_in_memory_and_through_files(net6, tmp_path, deterministic_autograd):
    from alphafive_amd.network import ResNet
    boards, weights, winner, pol = _batch(S, NB, seed=1)
    other = ResNet(S, device="cpu", seed=9).variables
    a = _trainer(net6.variables, fused=True)
    for _ in range(2):
        a.step(boards, weights, winner, pol, lr=1e-3, metrics=False)
    b = _trainer(other, fused=True)
    ptrs = {k: p.data_ptr() for k, p in b.params.items()}
    b.load_state_dict(a.state_dict())
    assert ptrs == {k: p.data_ptr() for k, p in b.params.items()}              # in place: the views keep their storage
    a.save(str(tmp_path), 60)
    a.save_state(str(tmp_path), 60)
    c = _trainer(other, fused=True)
    c.load_state(str(tmp_path), 60)
    _same_state(a, b)
    _same_state(a, c)
    for tr in (a, b, c):
        tr.step(boards, weights, winner, pol, lr=1e-3, metrics=False)
    _same_state(a, b)
    _same_state(a, c)
    assert a.t == 3 and all(p.is_leaf and p.requires_grad for p in a.params.values())
    flat = a._flat["params"]
    assert all(flat.data_ptr() <= p.data_ptr() < flat.data_ptr() + 4 * flat.numel() for p in a.params.values())


def test_weights_reach_the_evaluator_on_the_device_as_through_the_host():
    import torch
    from alphafive_amd.network import ResNet
    S11, nb = 11, 32
    net = ResNet(S11, device="cuda")
    net.load_npz(W)
    tr = _trainer(net.variables, S=S11, fused=True)
    boards, weights, winner, pol = _batch(S11, nb, seed=3)
    tr.step(boards, weights, winner, pol, lr=1e-3, metrics=False)
    host = ResNet(S11, device="cuda")
    try:
        x = torch.from_numpy(boards).cuda()
        pv = net.select_backend("hip")
        p0, _ = pv(x)
        p0 = p0.clone()
        net.set_variables_device(tr.device_variables())
        p, v = pv(x)
        p, v = p.clone(), v.clone()
        host.set_variables(tr.variables())
        ph, vh = host.select_backend("hip")(x)
        assert torch.equal(p, ph) and torch.equal(v, vh)
        assert not torch.equal(p, p0)                                           # the step moved the weights
    finally:
        net.close()
        host.close()


def test_one_fused_step_of_the_deep_net_logs_what_the_eager_one_logs():
    """No fp64 restatement of the deep net's loss exists: the eager deep Trainer's metrics stand in, under the same 2e-5 bar."""
    import torch
    from alphafive_amd import network_deep, train
    S7, nb = 7, 8
    net = network_deep.DeepResNet(S7, blocks=2, width=128, device="cpu", dtype=torch.float32, seed=4)
    boards, weights, winner, pol = _batch(S7, nb, seed=5)
    kw = dict(forward=train.forward_train_deep, shapes=net.variable_shapes())
    eager, fused = _trainer(net.variables, S=S7, **kw), _trainer(net.variables, S=S7, fused=True, **kw)
    assert list(fused.params) == list(net.variable_shapes())
    me, mf = eager.step(boards, weights, winner, pol, lr=1e-3), fused.step(boards, weights, winner, pol, lr=1e-3)
    for k in ("total", "cross_entropy", "value_loss", "entropy"):
        print("deep step 1 %-13s fused %.8f   eager %.8f" % (k, mf[k], me[k]))
        assert abs(mf[k] - me[k]) < 2e-5 * max(1.0, abs(me[k])), k
    m2 = fused.step(boards, weights, winner, pol, lr=1e-3)
    assert np.isfinite(list(m2.values())).all() and m2["total"] != mf["total"]


# ---------------------------------------------------------------- element by element, on the cases of tests/train_cases.py
SENTINEL = -777.25


def _dev(a, pad=0):
    """A device copy of a host array, `pad` sentinel elements (rows) longer."""
    import torch
    t = torch.tensor(np.asarray(a))
    if pad:
        t = torch.cat([t, torch.full((pad,) + tuple(t.shape[1:]), SENTINEL, dtype=t.dtype)])
    return t.cuda()


def _loss_head_abi(inputs):
    """af_train_loss_head through the C ABI, outputs two rows longer than B and pre-filled -> host (dlogits, dvalue, rows), B + 2 rows."""
    import torch
    from alphafive_amd import train_hip
    B, Cn = inputs[0].shape
    dev = [_dev(a) for a in inputs]
    dl = torch.full((B + 2, Cn), SENTINEL, dtype=torch.float32, device="cuda")
    dv = torch.full((B + 2,), SENTINEL, dtype=torch.float32, device="cuda")
    rows = torch.full((B + 2, train_hip.ROW_TERMS), SENTINEL, dtype=torch.float64, device="cuda")
    rc = train_hip.lib().af_train_loss_head(torch.cuda.current_stream().cuda_stream, B, Cn, *(t.data_ptr() for t in dev),
                                            dl.data_ptr(), dv.data_ptr(), rows.data_ptr())
    assert rc == 0, rc
    torch.cuda.synchronize()
    return dl.cpu().numpy(), dv.cpu().numpy(), rows.cpu().numpy()


@pytest.mark.parametrize("K", [1, 2, 4, 8, 16])
def test_loss_head_kernel_meets_the_interval_rule_on_every_case(K):
    """af_train_loss_head_kernel<K> on every case of tc.HEAD_CASES it runs: tc.check_loss_head (dlogits inside its 2^-40
    interval around fp64, dvalue / vsq / w * vsq bit for bit, the three sums inside their bounds), nothing written at or
    past row B, the same bits on a rerun.  Measured on an MI355X: profiles/train_fused.md."""
    cases = [(B, Cn) for B, Cn in tc.HEAD_CASES if tc.per_lane(Cn) == K]
    assert cases
    total = dict(n=0, near=0, flips=0)
    worst = worst_rows = relative_only = 0.0
    for B, Cn in cases:
        inputs = tc.head_case(B, Cn)
        dl, dv, rows = _loss_head_abi(inputs)
        for name, a in (("dlogits", dl), ("dvalue", dv), ("row_terms", rows)):
            assert (a[B:] == SENTINEL).all(), "(%d, %d): %s written at or past row B" % (B, Cn, name)
        r = tc.check_loss_head(inputs, dl[:B], dv[:B], rows[:B], what="kernel<%d> (%d, %d)" % (K, B, Cn), parts=tc.head_reference(B, Cn))
        print("kernel<%d> (%d, %d): worst |got - ref| / e %.3g, worst row-term ratio %.3g, %d of %d near, %d of them not float32(ref)"
              % (K, B, Cn, r["worst"], r["worst_rows"], r["near"], r["n"], r["flips"]))
        worst, worst_rows, relative_only = max(worst, r["worst"]), max(worst_rows, r["worst_rows"]), max(relative_only, r["relative_only"])
        for k in total:
            total[k] += r[k]
        again = _loss_head_abi(inputs)
        assert all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip((dl, dv, rows), again)), (B, Cn)
    print("af_train_loss_head_kernel<%d>: %d cases, %d elements, worst |got - ref| / e %.3g, worst row-term ratio %.3g, near share %.4f %% "
          "(%d elements, %d not float32(ref)); xent / ent against 2^-40 * sum |term| alone: %.3g"
          % (K, len(cases), total["n"], worst, worst_rows, 100.0 * total["near"] / max(1, total["n"]), total["near"], total["flips"], relative_only))
    assert worst <= 1 and worst_rows <= 1


def _adam_on_device(p, g, m, v, decay, lr_t, n_partials):
    """One train_hip.adam over host arrays -> (p, m, v, partials) as the device left them; the partials buffer is two longer
    than needed and must keep its sentinel there."""
    import torch
    from alphafive_amd import train_hip
    dp, dg, dm, dv = ([_dev(a) for a in arrs] for arrs in (p, g, m, v))
    partials = torch.full((n_partials + 2,), SENTINEL, device="cuda")
    assert train_hip.adam(list(zip(dp, dg, dm, dv, decay)), lr_t, BETA1, BETA2, EPS, L2, partials) == n_partials
    host = lambda ts: [t.cpu().numpy() for t in ts]  # noqa: E731
    out = partials.cpu().numpy()
    assert (out[n_partials:] == SENTINEL).all()
    return host(dp), host(dm), host(dv), out[:n_partials]


def test_adam_and_its_partials_on_planted_values_bit_for_bit():
    """tc.adam_case(): four steps over every size around the wave, the workgroup and the chunk, one variable carrying subnormal
    g * g, v, m and l2_coef * p, overflow to inf, +-inf and NaN gradients, signed zeros and p = 3e38: p, m, v and every L2
    partial are the references' bits (NaN where the reference is NaN)."""
    import torch
    from alphafive_amd import train_hip
    c = tc.adam_case()
    dp, dm, dv = ([_dev(a) for a in c[k]] for k in "pmv")
    table = train_hip.VarTable(dp, dm, dv, c["decay"])
    partials = torch.full((table.n_partials + 2,), SENTINEL, device="cuda")
    p, m, v = c["p"], c["m"], c["v"]
    n = 0
    for t in range(tc.ADAM_STEPS):
        table.set_grads([_dev(a) for a in c["g"][t]])
        assert train_hip.adam(table, c["lr_t"][t], BETA1, BETA2, EPS, L2, partials) == table.n_partials
        ref = tc.adam_step_reference(p, c["g"][t], m, v, c["decay"], c["lr_t"][t])
        got = tuple([x.cpu().numpy() for x in ts] for ts in (dp, dm, dv)) + (partials.cpu().numpy()[:table.n_partials],)
        n += tc.check_adam(got, ref, "step %d" % (t + 1))
        assert (partials.cpu().numpy()[table.n_partials:] == SENTINEL).all()
        p, m, v = ref[:3]
    print("Adam on planted values: %d elements over %d steps bit for bit" % (n, tc.ADAM_STEPS))


@pytest.mark.parametrize("nvars", [64, 65, 129])
def test_adam_tables_exactly_full_one_over_and_three_launches(nvars):
    p, g, m, v, decay = tc.table_case(nvars)
    got = _adam_on_device(p, g, m, v, decay, tc.lr_t(3), nvars)
    tc.check_adam(got, tc.adam_step_reference(p, g, m, v, decay, tc.lr_t(3)), "%d variables" % nvars)


def test_adam_skips_empty_variables_first_in_the_middle_and_last():
    """n = 0 entries with valid pointers (the C ABI) and with the null pointers of empty tensors (VarTable): their buffers keep
    their sentinel, they own no partial, and their neighbours' chunks are right."""
    import torch
    from alphafive_amd import train_hip
    rng = np.random.RandomState(21)
    sizes = [0, 5, 2049, 0, 0, 64, 0]
    decay = [True, True, True, False, True, False, True]
    p = [(rng.randn(n) * 0.1).astype(np.float32) for n in sizes]
    g, m = ([(rng.randn(n) * 1e-2).astype(np.float32) for n in sizes] for _ in range(2))
    v = [(rng.rand(n) * 1e-4).astype(np.float32) for n in sizes]
    ref = tc.adam_step_reference(p, g, m, v, decay, tc.lr_t(2))
    assert ref[3].size == 1 + 2 + 1
    # the null pointers of empty tensors, through VarTable
    assert torch.empty(0, device="cuda").data_ptr() == 0
    tc.check_adam(_adam_on_device(p, g, m, v, decay, tc.lr_t(2), 4), ref, "empty tensors")
    # valid pointers: every empty entry points at four sentinel elements of its own
    bufs = [[_dev(a, pad=4 if a.size == 0 else 0) for a in arrs] for arrs in (p, g, m, v)]
    arr = (train_hip.Var * len(sizes))()
    for k, e in enumerate(arr):
        e.p, e.g, e.m, e.v = (bufs[j][k].data_ptr() for j in range(4))
        e.n, e.decay = sizes[k], int(decay[k])
    partials = torch.full((6,), SENTINEL, device="cuda")
    rc = train_hip.lib().af_train_adam(torch.cuda.current_stream().cuda_stream, len(sizes), arr, tc.lr_t(2), BETA1, BETA2, EPS, L2,
                                       partials.data_ptr())
    assert rc == 4
    torch.cuda.synchronize()
    host = [[t.cpu().numpy() for t in ts] for ts in bufs]
    for k, n in enumerate(sizes):
        if n == 0:
            assert all((host[j][k] == SENTINEL).all() and host[j][k].size == 4 for j in range(4)), k
    cut = lambda ts: [a[:n] for a, n in zip(ts, sizes)]  # noqa: E731
    out = partials.cpu().numpy()
    tc.check_adam((cut(host[0]), cut(host[2]), cut(host[3]), out[:4]), ref, "valid pointers")
    assert (out[4:] == SENTINEL).all()
    # a table of empty variables only launches nothing
    assert train_hip.lib().af_train_adam(None, 1, arr, tc.lr_t(2), BETA1, BETA2, EPS, L2, partials.data_ptr()) == 0


def test_finalize_equals_its_reference_bit_for_bit_on_every_case():
    """B in {1, 255, 256, 257, 1000} x n_partials in {0, 1, 255, 256, 257, 1500}: the strided loop over more than 256 entries on
    both inputs, cancelling row terms so that the order of the fp64 adds shows in the fp32 results."""
    from alphafive_amd import train_hip
    for B, P in tc.FIN_CASES:
        rows, partials = tc.finalize_case(B, P)
        got = train_hip.finalize(_dev(rows), _dev(partials, pad=2) if P else None, P, L2).cpu().numpy()
        tc.check_finalize(got, rows, partials, L2, "finalize B = %d, %d partials" % (B, P))


def _decay_by_name(name):
    return "bias" not in name and "bn" not in name                     # train.Trainer._init_fused


@pytest.mark.parametrize("kind,nvars,launches", [("net42", 42, 1), ("deep2", 24, 1), ("deep9", 66, 2)])
def test_four_fused_steps_are_the_specifications_bit_for_bit(kind, nvars, launches, monkeypatch):
    """Four steps, a different batch each, with what the step feeds its kernels recorded (the gradients VarTable.set_grads
    receives, the loss head's inputs and outputs): params, m and v of every variable after each step are adam_reference of the
    state before it with the recorded gradient in the variable's logical layout, the name rule for decay and float32(lr_t) of
    that t; the recorded dlogits / dvalue / row terms meet tc.check_loss_head on the recorded logits; the four logged scalars
    are finalize_reference of the recorded rows and l2_partials_reference of the parameters before the step.  Recording the
    gradients makes this independent of autograd's reproducibility."""
    import torch
    from alphafive_amd import network_deep, train, train_hip
    if kind == "net42":
        from alphafive_amd.network import ResNet
        Sx, nb, kw = 6, 33, {}
        net = ResNet(Sx, device="cpu", seed=4)
    else:
        Sx, nb = 7, 9
        net = network_deep.DeepResNet(Sx, blocks=2 if kind == "deep2" else 9, width=32, device="cpu", dtype=torch.float32, seed=4)
        kw = dict(forward=train.forward_train_deep, shapes=net.variable_shapes())
    tr = _trainer(net.variables, S=Sx, fused=True, **kw)
    names = list(tr.params)
    assert len(names) == nvars and len(tr._table.groups) == launches
    rec = {}
    set_grads, loss_head = tr._table.set_grads, train_hip.loss_head

    def record_grads(grads):
        grads = list(grads)
        rec["g"] = [g.detach().clone() for g in grads]
        return set_grads(grads)

    def record_head(*inputs):
        out = loss_head(*inputs)
        rec["head"] = [t.detach().clone() for t in inputs + tuple(out)]
        return out

    monkeypatch.setattr(tr._table, "set_grads", record_grads)
    monkeypatch.setattr(train_hip, "loss_head", record_head)
    compared = 0
    for t in range(1, 5):
        boards, weights, winner, pol = _batch(Sx, nb, seed=40 + t)
        before = tr.state_dict()
        rec.clear()
        metrics = tr.step(boards, weights, winner, pol, lr=1e-3)
        after = tr.state_dict()
        assert after["t"] == t and len(rec["g"]) == nvars
        lr_t = np.float32(_lr_t(t))
        partials = []
        for k, g in zip(names, rec["g"]):
            p0 = before["params"][k]
            assert tuple(g.shape) == p0.shape, k
            ref = train_hip.adam_reference(p0, g.cpu().numpy(), before["m"][k], before["v"][k], _decay_by_name(k), lr_t,
                                           BETA1, BETA2, EPS, train_hip.L2_COEF)
            for key, r in zip(("params", "m", "v"), ref):
                compared += tc.check_bits(after[key][k], r, "%s step %d %s %s" % (kind, t, key, k))
            partials.append(train_hip.l2_partials_reference(p0, _decay_by_name(k)))
        head = [x.cpu().numpy() for x in rec["head"]]
        assert np.array_equal(head[2], pol) and np.array_equal(head[3], winner) and np.array_equal(head[4], weights)
        r = tc.check_loss_head(tuple(head[:5]), *head[5:], what="%s step %d" % (kind, t))
        terms = train_hip.finalize_reference(head[7], np.concatenate(partials), train_hip.L2_COEF)
        got = np.array([metrics[k] for k in ("total", "cross_entropy", "value_loss", "entropy")], np.float32)
        assert [float(x) for x in got] == [metrics[k] for k in ("total", "cross_entropy", "value_loss", "entropy")]
        tc.check_bits(got, terms, "%s step %d logged scalars" % (kind, t))
        compared += r["n"] + 4
    print("%s: %d elements compared over four steps (%d variables, %d partials, %d Adam launches per step)"
          % (kind, compared, nvars, tr._table.n_partials, launches))
