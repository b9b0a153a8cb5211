"""The int8 tower (csrc/af_tower_i8.hip) on the GPU against its numpy specification (alphafive_amd/tower_i8.py): packers byte for
byte, the entry quantiser element for element, every convolution form one layer at a time under the comparison rule of
tests/tower_i8_cases.py, the whole forward against the device's own per-layer sequence, the Python plumbing and the refusals."""
import ctypes as C

import numpy as np
import pytest

import tower_i8_cases as gen
from alphafive_amd import tower_i8 as t8
from tower_gpu import _Tune, planes, same_bits

pytestmark = pytest.mark.gpu
W, S, NPIX = 128, 11, 121
MAXB = gen.NPOS + 8
SENT8, SENT16 = 0x55, 0x4B4B


def _tt(wb):
    import torch
    return (torch.from_numpy(np.asarray(wb[0], np.float32)), torch.from_numpy(np.asarray(wb[1], np.float32)))


def _tower(blocks, scales, max_batch=MAXB, **kw):
    from alphafive_amd import tower_hip
    return tower_hip.HipTower([{k: _tt(b[k]) for k in ("c1", "c2", "res")} for b in blocks], S, W, max_batch, "cuda:0",
                              precision="int8", act_scales=scales, **kw)


def _expected_buffers(blocks, scales):
    """af_tower_i8_debug_weights' buffers from the specification: 4 per block, then the scales and their reciprocals."""
    a = np.asarray(scales, np.float32)
    out = []
    for i, b in enumerate(blocks):
        qw = t8.quantize_weights(b["c1"], b["c2"], b["res"], a[2 * i], a[2 * i + 1])
        out += [t8.pack_fragments(qw["q1"]), t8.pack_fragments(qw["q2"], qw["qp"]),
                np.concatenate([qw["m1"], qw["b1"]]), np.concatenate([qw["m2"], qw["b2"]])]
    out.append(np.concatenate([a, t8.reciprocal(a)]))
    return [np.ascontiguousarray(x).view(np.uint8).reshape(-1) for x in out]


def _assert_buffers(got, want, what):
    names = ["w1q", "w2q", "mb1", "mb2"]
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        name = "scales" if i == len(got) - 1 else "block %d %s" % (i // 4, names[i % 4])
        assert g.shape == w.shape, (what, name, g.shape, w.shape)
        bad = np.flatnonzero(g != w)
        assert bad.size == 0, "%s: %s differs in %d of %d bytes, first at byte %d: got %d, expected %d" % (
            what, name, bad.size, g.size, bad[0], g[bad[0]], w[bad[0]])


# ------------------------------------------------------------------ 1. packers ------------------------------------------------------------------
def test_packers_write_the_specifications_bytes_through_the_host_setters():
    blocks, scales = gen.case_blocks("both"), gen.layer_case("both")["scales"]
    tw = _tower(blocks, scales, max_batch=2)
    try:
        _assert_buffers(tw.debug_weights_i8(), _expected_buffers(blocks, scales), "host setters")
        # new scales: the multipliers, and through the ratio folded into the projection the second stream, follow
        new = (scales * np.array([1.5, 0.75, 1.25, 2.0], np.float32)).astype(np.float32)
        before = tw.debug_weights_i8()
        tw.enable_i8(new)
        after = tw.debug_weights_i8()
        _assert_buffers(after, _expected_buffers(blocks, new), "enable with new scales")
        assert (before[1] != after[1]).any() and (before[2] != after[2]).any() and (before[3] != after[3]).any()
        assert np.array_equal(before[0], after[0])                    # the first convolution's int8 weights do not depend on a scale
        # and the setters again, under the new scales, from other weights
        other = gen.case_blocks("conv1")
        for b, blk in enumerate(other):
            tw.set_block(b, {k: _tt(blk[k]) for k in ("c1", "c2", "res")})
        _assert_buffers(tw.debug_weights_i8(), _expected_buffers(other, new), "set_block after enable")
    finally:
        tw.close()


def _net_blocks(variables, blocks):
    return [dict(c1=(variables["tower/block%d_conv1/kernel" % b], variables["tower/block%d_conv1/bias" % b]),
                 c2=(variables["tower/block%d_conv2/kernel" % b], variables["tower/block%d_conv2/bias" % b]),
                 res=(variables["tower/block%d_res/kernel" % b], variables["tower/block%d_res/bias" % b])) for b in range(blocks)]


def test_packers_write_the_specifications_bytes_through_load_device():
    import torch
    from alphafive_amd.network_deep import DeepResNet
    net = DeepResNet(11, blocks=2, seed=3)
    scales = np.array([0.02, 0.011, 0.017, 0.013], np.float32)
    try:
        ev = net.select_backend("hip", 4, precision="int8", act_scales=scales)
        _assert_buffers(ev.tower.debug_weights_i8(), _expected_buffers(_net_blocks(net.variables, 2), scales), "constructor")
        v0 = net.version
        # fp32 tensors that are NOT bf16 values: the int8 packers quantise the caller's fp32 kernels as given (biases arrive rounded)
        rng = np.random.default_rng(5)
        new = {k: torch.from_numpy((v + rng.standard_normal(v.shape) * 0.01 * (np.abs(v).max() + 0.1)).astype(np.float32)).cuda()
               for k, v in net.variables.items()}
        net.set_variables_device(new)
        assert net.version == v0 + 1
        want = {k: (net.variables[k] if k.endswith("bias") else new[k].cpu().numpy()) for k in new}
        _assert_buffers(ev.tower.debug_weights_i8(), _expected_buffers(_net_blocks(want, 2), scales), "load_device")
        # the bf16 buffers next to them are the ones a bf16 tower packs from the same tensors
        other = net.evaluator(4)
        other.tower.load_device({k: (t if not k.endswith("bias") else net._tensor(net._named()[k]).float()) for k, t in new.items()})
        for a, b in zip(ev.tower.debug_weights(), other.tower.debug_weights()):
            assert np.array_equal(a, b)
    finally:
        net.close()


# ------------------------------------------------------------------ 2. quantiser ------------------------------------------------------------------
def test_quantiser_equals_the_reference_on_every_element():
    import torch
    from oracle import tower_fp64 as ref64
    B = 5
    rng = np.random.default_rng(9)
    x = ref64.bf16_round(rng.standard_normal((B, W, S, S)) * 0.5)
    n = np.arange(W * NPIX).reshape(W, S, S)
    x[1] = (n % 255 - 127 + 0.5) / 32.0                               # exact ties at r = 32: (k + 1/2) / 32, |2k + 1| < 256 is a bf16 value
    x[2] = np.where(n % 2 == 0, 4.0 + n % 7, -4.0 - n % 5)            # saturates both ways (|x| * 32 >= 128)
    x[3, :, 0, :] = 127.5 / 32                                        # the tie at the clamp
    assert np.array_equal(ref64.bf16_round(x), x)
    scales = np.array([1 / 32.0, 1.0, 1.0, 1.0], np.float32)
    want = t8.quantize_activation(x, t8.reciprocal(scales)[0])
    assert (want == 127).any() and (want == -127).any() and (np.abs(x[1] * 32 % 1) == 0.5).all()
    tw = _tower([gen.null_block(), gen.null_block()], scales, max_batch=B + 2)
    try:
        tw.load_nchw(torch.from_numpy(x.astype(np.float32)).cuda().to(torch.bfloat16))
        tw.xq.fill_(SENT8)
        tw.xq[:B, :, :S] = 0
        tw.xq[:B, :, S + NPIX:] = 0
        tw.quantize_i8(tw.x, tw.xq, B)
        torch.cuda.synchronize()
        got = tw.xq.cpu().numpy()
        assert np.array_equal(t8.from_c16(got[:B]), want)
        assert (got[B:] == SENT8).all() and not got[:B, :, :S].any() and not got[:B, :, S + NPIX:].any()
    finally:
        tw.close()


# ------------------------------------------------------------------ 3. one layer at a time ------------------------------------------------------------------
@pytest.fixture(scope="module")
def towers():
    made = {}

    def get(name):
        if name not in made:
            made[name] = _tower(gen.case_blocks(name), gen.layer_case(name)["scales"])
        return made[name]
    yield get
    for tw in made.values():
        tw.close()


def _run_layer(tw, name, bf16_out, B):
    """The case's layer on its first B positions -> the output as numpy NCHW (int8, or bf16 values as fp32), with the checks that
    nothing at or past B and no zero row was written."""
    import torch
    c = gen.layer_case(name)
    tw.xq.fill_(SENT8)
    tw.gq.fill_(SENT8)
    tw.x.view(torch.int16).fill_(SENT16)
    for buf in (tw.xq, tw.gq, tw.x):
        buf[:B, :, :S] = 0
        buf[:B, :, S + NPIX:] = 0
    tw.xq[:B].copy_(torch.from_numpy(t8.to_c16(c["hq"][:B])))
    if c["second"]:
        tw.gq[:B].copy_(torch.from_numpy(t8.to_c16(c["gq"][:B])))
        out = tw.x if bf16_out else tw.xq                             # in place on the block input, as af_tower_forward_i8 runs it
        tw.conv_i8(0, True, tw.gq, tw.xq, out, B)
    else:
        out = tw.x if bf16_out else tw.gq
        tw.conv_i8(0, False, tw.xq, None, out, B)
    torch.cuda.synchronize()
    for nm, buf in (("xq", tw.xq), ("gq", tw.gq)):
        assert bool((buf[B:] == SENT8).all()), f"{nm}: a position at or past batch {B} was written"
        assert not bool(buf[:B, :, :S].any()) and not bool(buf[:B, :, S + NPIX:].any()), f"{nm}: a zero row was written"
    xb = tw.x.view(torch.int16)
    assert bool((xb[B:] == SENT16).all()), f"x: a position at or past batch {B} was written"
    assert not bool(xb[:B, :, :S].any()) and not bool(xb[:B, :, S + NPIX:].any()), "x: a zero row was written"
    if not bf16_out:
        assert bool((xb[:B, :, S:S + NPIX] == SENT16).all()), "the int8 form wrote the bf16 buffer"
        return t8.from_c16(out[:B].cpu().numpy())
    return tw.store_nchw(B).float().cpu().numpy()


@pytest.mark.parametrize("bf16_out", [False, True], ids=["int8 out", "bf16 out"])
@pytest.mark.parametrize("name", gen.CASES)
def test_one_layer_against_the_reference(towers, name, bf16_out):
    tw = towers(name)
    ref, t64, pre, r_out = gen.layer_reference(name, bf16_out)
    for B, grid in ((1, 0), (2, 0), (7, 0), (33, 0), (7, 3), (33, 3)):    # tune(1, 3): batch 7 is three ragged passes
        with _Tune(k1=grid):
            out = _run_layer(tw, name, bf16_out, B)
        gen.compare(out, ref[:B], t64[:B], pre[:B], r_out, "%s, %s, batch %d, grid %s" % (name, "bf16 out" if bf16_out else "int8 out", B, grid or "default"))


# ------------------------------------------------------------------ 4. whole forward ------------------------------------------------------------------
@pytest.mark.parametrize("blocks", [1, 3])
def test_forward_is_the_devices_own_layer_sequence(blocks):
    """af_tower_forward_i8 = quantise + the per-layer launches, bit for bit; and each of those layers, on the input the device
    itself gave it, is the reference's layer under the comparison rule (so one-step differences do not compound)."""
    import torch
    tc = gen.tower_case(blocks)
    B = tc["x"].shape[0]
    a = tc["scales"]
    r = t8.reciprocal(a)
    tw = _tower(tc["blocks"], a, max_batch=B + 1)
    try:
        x = torch.from_numpy(tc["x"].astype(np.float32)).cuda().to(torch.bfloat16)
        tw.load_nchw(x)
        tw.forward_i8(B)
        torch.cuda.synchronize()
        whole = tw.x.clone()
        assert not bool(tw.xq[B:].any()) and not bool(tw.gq[B:].any()) and not bool(tw.x[B:].view(torch.int16).any())
        tw.xq.zero_()
        tw.gq.zero_()
        tw.load_nchw(x)
        tw.quantize_i8(tw.x, tw.xq, B)
        hq = t8.from_c16(tw.xq[:B].cpu().numpy())
        assert np.array_equal(hq, t8.quantize_activation(tc["x"], r[0]))
        for b in range(blocks):
            last = b == blocks - 1
            qw = t8.quantize_weights(tc["blocks"][b]["c1"], tc["blocks"][b]["c2"], tc["blocks"][b]["res"], a[2 * b], a[2 * b + 1])
            tw.conv_i8(b, False, tw.xq, None, tw.gq, B)
            gq = t8.from_c16(tw.gq[:B].cpu().numpy())
            ref, t64, pre = t8.conv_reference(hq, qw["q1"], qw["m1"], qw["b1"], r[2 * b + 1])
            gen.compare(gq, ref, t64, pre, r[2 * b + 1], "block %d first convolution" % b)
            tw.conv_i8(b, True, tw.gq, tw.xq, tw.x if last else tw.xq, B)
            r_out = None if last else r[2 * b + 2]
            ref, t64, pre = t8.conv_reference(gq, qw["q2"], qw["m2"], qw["b2"], r_out, hq, qw["qp"])
            if last:
                gen.compare(tw.store_nchw(B).float().cpu().numpy(), ref, t64, pre, None, "block %d second convolution (bf16)" % b)
            else:
                hq = t8.from_c16(tw.xq[:B].cpu().numpy())
                gen.compare(hq, ref, t64, pre, r_out, "block %d second convolution" % b)
        torch.cuda.synchronize()
        assert torch.equal(tw.x.view(torch.int16), whole.view(torch.int16))
    finally:
        tw.close()


# ------------------------------------------------------------------ 5. plumbing ------------------------------------------------------------------
@pytest.fixture(scope="module")
def net2():
    from alphafive_amd.network_deep import DeepResNet
    net = DeepResNet(11, blocks=2, seed=0)
    scales = net.calibrate_int8(planes(16, seed=2, S=11))
    yield net, scales
    net.close()


def test_int8_evaluator_evaluates_and_does_not_depend_on_the_batch(net2):
    import torch
    net, scales = net2
    x = planes(8, S=11)
    bf = net.evaluator(8)
    p0, v0 = [t.clone() for t in bf(x)]
    ev = net.select_backend("hip", 8, precision="int8", act_scales=scales)
    try:
        p, v = [t.clone() for t in ev(x)]
        assert p.shape == (8, 121) and v.shape == (8,)
        assert float((p.sum(1) - 1).abs().max()) < 1e-5 and float(p.min()) >= 0 and float(v.abs().max()) <= 1
        assert not same_bits((p,), (p0,))                             # it is not the bf16 path
        assert float((p - p0).abs().max()) < 0.05 and float((v - v0).abs().max()) < 0.2     # ... and it is the same net
        p1, v1 = [t.clone() for t in ev(x[:1])]
        assert same_bits((p1, v1), (p[:1], v[:1]))
        # a bf16 evaluator of the same net is bit-identical before and after the int8 one exists
        assert same_bits(bf(x), (p0, v0))
        fresh = net.evaluator(8)
        assert same_bits(fresh(x), (p0, v0))
        fresh.close()
    finally:
        ev.close()
        bf.close()


def test_device_update_and_captured_graph_follow_the_new_weights(net2):
    import torch
    from alphafive_amd.network_deep import DeepResNet
    net, scales = net2
    x = planes(8, S=11)
    old = {k: torch.from_numpy(v).cuda() for k, v in net.variables.items()}
    ev = net.evaluator(8, precision="int8", act_scales=scales)
    try:
        tw = ev.tower
        before = [t.clone() for t in ev(x)]
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, capture_error_mode="thread_local"):
            tw.stem(x)
            tw.forward_i8(8)
            tw.heads(8)
            tw.dense(8)
        g.replay()
        torch.cuda.synchronize()
        assert same_bits((tw.policy[:8], tw.value[:8]), before)
        other = DeepResNet(11, blocks=2, seed=1)
        new = {k: torch.from_numpy(v).cuda() for k, v in other.variables.items()}
        version = ev.weights_version()
        net.set_variables_device(new)
        assert ev.weights_version() == version + 1
        after = [t.clone() for t in ev(x)]
        assert not same_bits(after, before)
        fresh = net.evaluator(8, precision="int8", act_scales=scales)
        assert same_bits(fresh(x), after)
        fresh.close()
        g.replay()
        torch.cuda.synchronize()
        assert same_bits((tw.policy[:8], tw.value[:8]), after)
        del g
        other.close()
    finally:
        net.set_variables_device(old)
        ev.close()


# ------------------------------------------------------------------ 6. refusals ------------------------------------------------------------------
def test_int8_calls_are_refused_before_enable_and_on_15x15():
    import torch
    from alphafive_amd import tower_hip
    L = tower_hip.lib()
    blk = {k: _tt(v) for k, v in gen.null_block().items()}
    tw = tower_hip.HipTower([blk], 11, W, 2, "cuda:0")
    xq = torch.zeros((2, 8, 144, 16), dtype=torch.int8, device="cuda")
    gq = torch.zeros_like(xq)
    try:
        assert L.af_tower_forward_i8(tw._h, None, tw.x.data_ptr(), xq.data_ptr(), gq.data_ptr(), 1) == -3
        assert L.af_tower_quantize_i8(tw._h, None, tw.x.data_ptr(), xq.data_ptr(), 1) == -3
        assert L.af_tower_conv_i8(tw._h, None, 0, 0, xq.data_ptr(), None, gq.data_ptr(), 0, 1) == -3
        with pytest.raises(tower_hip.TowerError) as e:
            tw.forward_i8(1)
        assert e.value.code == -3
        one = (C.c_float * 2)(1.0, 1.0)
        assert L.af_tower_i8_enable(tw._h, one, 3) == -1              # wrong n
        assert L.af_tower_i8_enable(tw._h, (C.c_float * 2)(1.0, 0.0), 2) == -1
        assert L.af_tower_i8_enable(tw._h, (C.c_float * 2)(1.0, float("inf")), 2) == -1
        assert L.af_tower_i8_enable(tw._h, (C.c_float * 2)(float("nan"), 1.0), 2) == -1
        # enabled, but this block's weights were set before: no int8 weights until its setter runs again
        assert L.af_tower_i8_enable(tw._h, one, 2) == 0
        assert L.af_tower_forward_i8(tw._h, None, tw.x.data_ptr(), xq.data_ptr(), gq.data_ptr(), 1) == -3
        tw.set_block(0, blk)
        assert L.af_tower_forward_i8(tw._h, None, tw.x.data_ptr(), xq.data_ptr(), gq.data_ptr(), 1) == 0
        assert L.af_tower_conv_i8(tw._h, None, 0, 1, gq.data_ptr(), xq.data_ptr(), xq.data_ptr(), 0, 1) == -1   # the last block's output has no int8 scale
        torch.cuda.synchronize()
    finally:
        tw.close()
    t15 = tower_hip.HipTower([blk], 15, W, 2, "cuda:0")
    try:
        assert L.af_tower_i8_enable(t15._h, (C.c_float * 2)(1.0, 1.0), 2) == -1
        assert L.af_tower_forward_i8(t15._h, None, t15.x.data_ptr(), xq.data_ptr(), gq.data_ptr(), 1) == -1
        assert L.af_tower_i8_plane_bytes(t15._h) == 0
    finally:
        t15.close()
    with pytest.raises(ValueError, match="11x11"):
        tower_hip.HipTower([blk], 15, W, 2, "cuda:0", precision="int8", act_scales=[1.0, 1.0])
