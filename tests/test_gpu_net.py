"""HIP forward pass (libaf_net.so through the C ABI) vs the fp64 restatement (1e-5, the tolerance
BASELINE.json states for the value) and vs the plain PyTorch fp32 reference of the same graph."""
import os

import numpy as np
import pytest

from conftest import GOLDEN
from oracle import net_fp64

pytestmark = pytest.mark.gpu
W = os.path.join(GOLDEN, "alphaFive-6960.weights.npz")


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


def test_hip_net_matches_fp64_restatement_and_torch_reference():
    import torch
    from alphafive_amd.network import ResNet
    net = ResNet(11, device="cuda")
    net.load_npz(W)
    pv = net.select_backend("hip")
    x = _positions(11, 512)
    xt = torch.from_numpy(x).cuda()
    p, v = pv(xt)
    p, v = p.cpu().numpy().copy(), v.cpu().numpy().copy()
    assert p.shape == (512, 121) and v.shape == (512,)
    p64, v64 = net_fp64.forward(net.variables, x)      # all 512 positions (the fp64 restatement is one dgemm per tap)
    dv, dp = np.abs(v - v64), np.abs(p - p64)
    print("|dv| max %.3g  |dp| max %.3g (first 96: %.3g)" % (dv.max(), dp.max(), dp[:96].max()))
    assert dv.max() < 1e-5                             # BASELINE.json: value within 1e-5 (fp32) — on every position
    # north_star binds the value only; the probabilities meet the same bar on all 512 positions (r6: 4.1e-6 measured)
    assert dp.max() < 1e-5
    pt, vt = net.eval_torch(xt)                        # plain PyTorch fp32 reference (MIOpen picks Winograd)
    # ... next to a measurement of what 24-bit arithmetic does on the same inputs: PyTorch's own fp32 evaluation against the same fp64
    # restatement on the same 512 positions (the reference's class; r6: |dv| 6.8e-6, |dp| 3.5e-6 vs the kernel's 4.5e-6 / 4.1e-6) — the
    # split-operand kernel is held to 2x of PyTorch-fp32's own worst error, per output
    dpt, dvt = np.abs(pt.cpu().numpy() - p64), np.abs(vt.cpu().numpy() - v64)
    print("PyTorch fp32 ops: |dv| max %.3g  |dp| max %.3g" % (dvt.max(), dpt.max()))
    assert dp.max() <= 2.0 * dpt.max() and dv.max() <= 2.0 * dvt.max()
    assert (torch.from_numpy(v).cuda() - vt).abs().max().item() < 5e-5
    assert (torch.from_numpy(p).cuda() - pt).abs().max().item() < 5e-5
    assert np.allclose(p.sum(1), 1.0, atol=1e-5)
    # deterministic: same input, same bits
    p2, v2 = pv(xt)
    assert (p2.cpu().numpy() == p).all() and (v2.cpu().numpy() == v).all()
    # SURVEY §8c sanity values of the shipped checkpoint
    p0, v0 = pv(torch.zeros((1, 3, 11, 11), device="cuda"))
    assert abs(float(v0[0]) - 0.10429) < 1e-5 and int(p0.argmax()) == 5 * 11 + 8


@pytest.mark.parametrize("S,B", [(11, 1), (11, 7), (11, 33), (15, 40), (15, 1), (15, 300), (7, 100), (6, 65)])
def test_hip_net_ragged_batches_and_board_sizes(S, B):
    import torch
    from alphafive_amd.network import ResNet
    net = ResNet(S, device="cuda", seed=S)
    if S == 11:
        net.load_npz(W)
    pv = net.select_backend("hip")
    x = _positions(S, B, seed=B)
    p, v = pv(torch.from_numpy(x).cuda())
    p, v = p.cpu().numpy().copy(), v.cpu().numpy().copy()
    idx = np.unique(np.concatenate([np.arange(min(B, 20)), np.arange(max(0, B - 4), B)]))      # the first positions and the ragged tail
    p64, v64 = net_fp64.forward(net.variables, x[idx])
    assert np.abs(v[idx] - v64).max() < 1e-5
    assert np.abs(p[idx] - p64).max() < 1e-5
    # batch independence: position b evaluated alone gives the same bits as inside the batch
    p1, v1 = pv(torch.from_numpy(x[B - 1:B]).cuda())
    p1, v1 = p1.clone(), v1.clone()                    # pv returns views of its output buffers
    pb, vb = pv(torch.from_numpy(x).cuda())
    assert (p1[0] == pb[B - 1]).all() and v1[0] == vb[B - 1]


def test_flop_count_matches_survey():
    from alphafive_amd import net_hip
    from alphafive_amd.network import ResNet
    net = ResNet(11, device="cuda")
    h = net_hip.HipNet(net.variables, 11, 4, net.device)
    assert h.flops_per_position == 118_727_264         # 59,363,632 MAC
    h.close()


def test_alternate_conv_paths_agree_with_fp64():
    """The fp32-MFMA Winograd path (af_net_tune(0, 1): 24-bit operands, the path of the other board sizes and of bench.py's
    config2_fp32mfma leg) and the default fp16 split-operand path (5) both stay within the bar; removed paths are refused."""
    import torch
    from alphafive_amd import net_hip
    from alphafive_amd.network import ResNet
    net = ResNet(11, device="cuda")
    net.load_npz(W)
    pv = net.select_backend("hip")
    x = _positions(11, 70, seed=4)
    xt = torch.from_numpy(x).cuda()
    p64, v64 = net_fp64.forward(net.variables, x[:32])
    try:
        for mode in (1, 5):
            net_hip.tune(0, mode)
            p, v = pv(xt)
            assert np.abs(v[:32].cpu().numpy() - v64).max() < 1e-5, mode
            assert np.abs(p[:32].cpu().numpy() - p64).max() < 1e-5, mode
        for gone in (0, 2, 3, 4):
            with pytest.raises(net_hip.NetError):
                net_hip.tune(0, gone)
        # ... and the split-operand path with the r1 head kernels on fp32 planes instead of its own fused heads (af_net_tune(9, 0)),
        # plus slot independence of the default path: a position's outputs do not depend on where in the batch it sits
        net_hip.tune(9, 0)
        p, v = pv(xt)
        assert np.abs(v[:32].cpu().numpy() - v64).max() < 1e-5 and np.abs(p[:32].cpu().numpy() - p64).max() < 1e-5
        net_hip.tune(9, 1)
        p, v = (t.clone() for t in pv(xt))
        perm = torch.randperm(70, generator=torch.Generator().manual_seed(1)).cuda()
        pp, vp = pv(xt[perm].contiguous())
        assert torch.equal(pp, p[perm]) and torch.equal(vp, v[perm])
    finally:
        net_hip.tune(0, 5)
        net_hip.tune(9, 1)


def test_hip_evaluator_follows_weight_updates():
    """A weight update (set_variables / restore / load_npz — what train_loop and a checkpoint reload do) must reach the
    hand-written kernels: the evaluator handed out by select_backend("hip") repacks and re-uploads on its next call."""
    import torch
    from alphafive_amd.network import ResNet, random_variables
    net = ResNet(11, device="cuda", seed=1)
    pv = net.select_backend("hip")
    x = _positions(11, 40, seed=9)
    xt = torch.from_numpy(x).cuda()
    p1, v1 = (t.clone() for t in pv(xt))
    net.set_variables(random_variables(11, seed=2))
    p2, v2 = (t.clone() for t in pv(xt))
    p64, v64 = net_fp64.forward(net.variables, x)
    assert np.abs(p2.cpu().numpy() - p64).max() < 1e-5 and np.abs(v2.cpu().numpy() - v64).max() < 1e-5
    assert (p2 - p1).abs().max().item() > 1e-4            # it really was a different weight set
    net.load_npz(W)
    p3, v3 = pv(xt)
    p64, v64 = net_fp64.forward(net.variables, x)
    assert np.abs(p3.cpu().numpy() - p64).max() < 1e-5 and np.abs(v3.cpu().numpy() - v64).max() < 1e-5


@pytest.mark.parametrize("S,B,bits", [(11, 600, 256), (11, 5, 128 | 256), (15, 300, 64), (15, 3, 128)])
def test_round5_launch_variants_are_bit_identical(S, B, bits):
    """r5 added three launch structures that claim the SAME bits as the ones they replace: blocks 3 and 5 as one kernel each
    (af_block_f16s; af_net_tune(7, 256) = two launches per block), the 15x15 half classes + corner kernel (af_conv_f16s_h15 /
    af_corner_f16s; bit 64 = the two-halves launch) and the small-batch pixel-tile split (af_conv_f16s_sb; bit 128 = one workgroup
    per position).  Same input through both structures: policy and value equal bit for bit."""
    import torch
    from alphafive_amd import net_hip
    from alphafive_amd.network import ResNet
    net = ResNet(S, device="cuda", seed=S + 1)
    if S == 11:
        net.load_npz(W)
    xt = torch.from_numpy(_positions(S, B, seed=B)).cuda()
    try:
        pv = net.select_backend("hip")
        p_new, v_new = (t.clone() for t in pv(xt))
        net_hip.tune(7, bits)
        p_old, v_old = (t.clone() for t in pv(xt))
    finally:
        net_hip.tune(7, 0)
    assert torch.equal(p_new, p_old) and torch.equal(v_new, v_old)
    p64, v64 = net_fp64.forward(net.variables, _positions(S, B, seed=B)[:8])
    assert np.abs(v_new[:8].cpu().numpy() - v64).max() < 1e-5


@pytest.mark.parametrize("B", [1, 2, 5, 8])
def test_single_launch_small_batch_forward_is_bit_identical_to_the_launch_sequence(B):
    """r6: <= 8 positions on 11x11 run as ONE launch of dataflow roles (af_small_forward_f16s: every workgroup of the
    nine dependent launches becomes a role that waits for its producers' counters) + the policy dense layer.  Same role bodies, same
    operands: policy and value equal the launch sequence's (af_net_tune(7, 2048)) bit for bit, run after run (the counters are
    re-armed by the last role out), no wait ever gives up, and a batch evaluated alone equals its slots inside a large batch."""
    import torch
    from alphafive_amd import net_hip
    from alphafive_amd.network import ResNet
    net = ResNet(11, device="cuda")
    net.load_npz(W)
    h = net_hip.HipNet(net.variables, 11, 64, net.device)
    x = _positions(11, 64, seed=77 + B)
    xt = torch.from_numpy(x).cuda()
    pb, vb = (t.clone() for t in h(xt))                       # the batched kernels (64 positions)
    try:
        net_hip.tune(7, 2048)
        p_old, v_old = (t.clone() for t in h(xt[:B].contiguous()))
    finally:
        net_hip.tune(7, 0)
    for rep in range(20):                                     # back to back: the counters re-arm
        p_new, v_new = (t.clone() for t in h(xt[rep % 3:rep % 3 + B].contiguous()))
        if rep % 3 == 0:
            assert torch.equal(p_new, p_old) and torch.equal(v_new, v_old), rep
        assert torch.equal(p_new, pb[rep % 3:rep % 3 + B]) and torch.equal(v_new, vb[rep % 3:rep % 3 + B]), rep
    assert h.small_forward_error() == 0
    p64, v64 = net_fp64.forward(net.variables, x[:B])
    assert np.abs(v_old.cpu().numpy() - v64).max() < 1e-5
    h.close()


def test_single_launch_small_batch_forward_inside_a_hip_graph():
    """The Player replays 16 x (tick + forward) as a HIP graph: the single launch must capture and replay (its counters live in
    device memory and are re-armed on the device)."""
    import torch
    from alphafive_amd import net_hip
    from alphafive_amd.network import ResNet
    net = ResNet(11, device="cuda")
    net.load_npz(W)
    h = net_hip.HipNet(net.variables, 11, 8, net.device)
    xt = torch.from_numpy(_positions(11, 3, seed=5)).cuda()
    p0, v0 = (t.clone() for t in h(xt))
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(16):
            h(xt)
    for _ in range(5):
        h.policy.zero_(), h.value.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(h.policy[:3], p0) and torch.equal(h.value[:3], v0)
    assert h.small_forward_error() == 0
    h.close()


def test_forward_output_digests_are_pinned():
    """A change of ANY bit of the forward's arithmetic must be a decision, not an accident: CRC32 of policy and value on fixed inputs
    (tools/forward_digest.py; 11x11 alphaFive-6960 at batch 600 / 5 — the batched kernels / the single-launch roles — and 15x15
    random init at 300 / 3).  The digests were recorded on the r6 tree BEFORE its source clean-ups (folded build switches, pruned
    variants) and are unchanged by them; the engine-vs-oracle tests use the same kernels on both sides and could not see such a change."""
    import sys
    from conftest import REPO
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import forward_digest
    assert forward_digest.digests() == {"S11_B600": "4f50b3f7d08132dc", "S11_B5": "441e8ce5d7f1f336",
                                        "S15_B300": "75d9f0dcac1b2d1d", "S15_B3": "57cc8bcb0af5cd8e"}


def _forward_variants():
    import sys
    if GOLDEN not in sys.path:
        sys.path.insert(0, GOLDEN)
    import make_forward_variant_digests as m
    return m


@pytest.mark.parametrize("S,B", [(11, 1), (11, 8), (11, 9), (11, 300), (15, 3), (15, 127), (15, 128), (15, 300), (7, 5)])
def test_forward_variants_match_the_recorded_digests(S, B):
    """The host side of af_conv_f16s.hip chooses between launch forms (f16s_plan: single launch of roles / paired branches / branch
    launches, tile split, half classes, fused blocks, ...) by batch size and the af_net_tune bits.  Policy and value of every setting
    of tests/golden/make_forward_variant_digests.py — default, each key-7 A/B bit, the forced side stream, the fp32 heads, the fp32
    path — at the smallest batches either side of every branch of that choice are the bytes recorded with the library of the commit
    the record names (SHA-256, tests/golden/forward_variant_digests.json), and the key-7 values include/af_net.h documents as "same
    results bit for bit" give the default's digest at the same shape."""
    import json
    m = _forward_variants()
    assert (S, B) in m.SHAPES
    with open(m.OUT) as f:
        recorded = json.load(f)["digests"][m.shape_key(S, B)]
    got = m.digests_of(S, B)
    assert set(got) == set(recorded) == {m.setting_key(s) for s in m.SETTINGS}
    for k in sorted(got):
        print("%s %-12s %s" % (m.shape_key(S, B), k, "same" if got[k] == recorded[k] else "DIFFERENT: %s, recorded %s" % (got[k], recorded[k])))
    assert got == recorded
    for s in m.SAME_BITS_AS_DEFAULT:
        assert got[m.setting_key(s)] == got["default"], (m.shape_key(S, B), m.setting_key(s))


@pytest.mark.parametrize("S,B", [(7, 5), (11, 17)])
def test_fp32_path_without_side_stream_and_with_valu_policy_head(S, B):
    """The two settings of the fp32 Winograd path (af_net_tune(0, 1)) that no recorded digest takes: the value branch on the caller's
    stream (af_net_tune(4, 0): the same kernels in one queue, so the bits of the side-stream default) and the VALU policy head
    (af_net_tune(5, 0): another summation order for the policy, held to the fp64 restatement; the value does not pass through it).
    7x7, 5 positions: a board size without a split-operand handle, one head workgroup; 11x11, 17 positions: two workgroups of the
    MFMA head with a ragged tail, three of the VALU head."""
    import hashlib
    import torch
    from alphafive_amd import net_hip
    from alphafive_amd.network import ResNet
    net = ResNet(S, device="cuda", seed=S)
    if S == 11:
        net.load_npz(W)
    pv = net.select_backend("hip")
    x = _positions(S, B, seed=B)
    xt = torch.from_numpy(x).cuda()
    p64, v64 = net_fp64.forward(net.variables, x)

    def run(key, value):
        net_hip.tune(key, value)
        p, v = (t.cpu().numpy().copy() for t in pv(xt))
        net_hip.tune(key, 1)
        print("S%d_B%d tune(%d, %d): policy %s value %s  |dp| %.3g |dv| %.3g" % (
            S, B, key, value, hashlib.sha256(p.tobytes()).hexdigest()[:16], hashlib.sha256(v.tobytes()).hexdigest()[:16],
            np.abs(p - p64).max(), np.abs(v - v64).max()))
        return p, v

    try:
        net_hip.tune(0, 1)
        p_side, v_side = run(4, 1)
        p_one, v_one = run(4, 0)
        p_mfma, v_mfma = run(5, 1)
        p_valu, v_valu = run(5, 0)
    finally:
        net_hip.tune(0, 5)
        net_hip.tune(4, 1)
        net_hip.tune(5, 1)
    assert p_side.shape == (B, S * S) and v_side.shape == (B,)
    assert (p_one.view(np.uint32) == p_side.view(np.uint32)).all() and (v_one.view(np.uint32) == v_side.view(np.uint32)).all()
    assert (v_valu.view(np.uint32) == v_mfma.view(np.uint32)).all()
    assert np.abs(p_valu - p64).max() < 1e-5
