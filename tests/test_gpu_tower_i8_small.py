"""The int8 tower's tile-parallel form (af_tower_conv_i8_small, af_tower_forward_i8_small) on the GPU: every layer form bit-equal
to the persistent kernel AND under the comparison rule of tests/tower_i8_cases.py against the numpy specification, the whole
forward against the persistent forward and the device's own per-layer sequence, captured graphs across weight and scale updates,
the evaluator's independence of batch and form, Player over an int8 evaluator against the C oracle, and the refusals."""
import ctypes as C

import numpy as np
import pytest

import oracle
import tower_i8_cases as gen
import tower_i8_gpu as hlp
from alphafive_amd import tower_i8 as t8
from conftest import make_cfg
from tower_gpu import planes, same_bits

pytestmark = pytest.mark.gpu
W, S, NPIX = hlp.W, hlp.S, hlp.NPIX
BATCHES = (1, 2, 7, 33)          # 4, 8, 28 and 132 workgroups: one position, two, an odd count, every position of the cases


@pytest.fixture(scope="module")
def towers():
    yield from hlp.case_towers()


# ------------------------------------------------------------------ 1. one layer, every form ------------------------------------------------------------------
@pytest.mark.parametrize("bf16_out", [False, True], ids=["int8 out", "bf16 out"])
@pytest.mark.parametrize("name", gen.CASES)
def test_one_layer_equals_the_persistent_kernel_and_meets_the_reference(towers, name, bf16_out):
    import torch
    tw = towers(name)
    ref, t64, pre, r_out = gen.layer_reference(name, bf16_out)
    for B in BATCHES:
        what = "%s, %s, batch %d" % (name, "bf16 out" if bf16_out else "int8 out", B)
        want, left_p = hlp.run_layer(tw, name, bf16_out, B, small=False)
        out, left_s = hlp.run_layer(tw, name, bf16_out, B, small=True)
        for nm, a, b in zip(("xq", "gq", "x"), left_s, left_p):
            assert torch.equal(a, b), "%s: buffer %s differs from the persistent kernel's in %d elements" % (what, nm, int((a != b).sum()))
        assert np.array_equal(out.view(np.uint32) if out.dtype == np.float32 else out, want.view(np.uint32) if want.dtype == np.float32 else want), what
        gen.compare(out, ref[:B], t64[:B], pre[:B], r_out, what + ", tile-parallel")


# ------------------------------------------------------------------ 2. whole forward ------------------------------------------------------------------
@pytest.mark.parametrize("blocks", [1, 3])
def test_forward_small_equals_forward_and_is_the_devices_own_layer_sequence(blocks):
    """af_tower_forward_i8_small leaves x, xq and gq as af_tower_forward_i8 does, bit for bit, at every batch; and it is
    quantise + the per-layer small launches, each of which, on the input the device itself gave it, is the reference's layer
    under the comparison rule (so one-step differences do not compound)."""
    import torch
    tc = gen.tower_case(blocks, n=gen.NPOS)
    a = tc["scales"]
    r = t8.reciprocal(a)
    tw = hlp.tower(tc["blocks"], a, max_batch=gen.NPOS + 1)
    qws = [t8.quantize_weights(b["c1"], b["c2"], b["res"], a[2 * i], a[2 * i + 1]) for i, b in enumerate(tc["blocks"])]
    try:
        x = torch.from_numpy(tc["x"].astype(np.float32)).cuda().to(torch.bfloat16)
        for B in BATCHES:
            want = hlp.run_forward(tw, x, B, small=False)
            got = hlp.run_forward(tw, x, B, small=True)
            for nm, g, w in zip(("x", "xq", "gq"), got, want):
                assert torch.equal(g, w), "blocks %d, batch %d: %s differs from af_tower_forward_i8's in %d elements" % (blocks, B, nm, int((g != w).sum()))
            # layer by layer, on the device's own trace
            tw.load_nchw(x[:B])
            tw.quantize_i8(tw.x, tw.xq, B)
            hq = t8.from_c16(tw.xq[:B].cpu().numpy())
            assert np.array_equal(hq, t8.quantize_activation(tc["x"][:B], r[0]))
            for b in range(blocks):
                last, qw = b == blocks - 1, qws[b]
                tw.conv_i8_small(b, False, tw.xq, None, tw.gq, B)
                gq = t8.from_c16(tw.gq[:B].cpu().numpy())
                ref, t64, pre = t8.conv_reference(hq, qw["q1"], qw["m1"], qw["b1"], r[2 * b + 1])
                gen.compare(gq, ref, t64, pre, r[2 * b + 1], "batch %d block %d first convolution" % (B, b))
                tw.conv_i8_small(b, True, tw.gq, tw.xq, tw.x if last else tw.xq, B)
                r_out = None if last else r[2 * b + 2]
                ref, t64, pre = t8.conv_reference(gq, qw["q2"], qw["m2"], qw["b2"], r_out, hq, qw["qp"])
                if last:
                    gen.compare(tw.store_nchw(B).float().cpu().numpy(), ref, t64, pre, None, "batch %d block %d second convolution (bf16)" % (B, b))
                else:
                    hq = t8.from_c16(tw.xq[:B].cpu().numpy())
                    gen.compare(hq, ref, t64, pre, r_out, "batch %d block %d second convolution" % (B, b))
            torch.cuda.synchronize()
            assert torch.equal(tw.x.view(torch.int16), got[0]) and torch.equal(tw.gq, got[2])
    finally:
        tw.close()


# ------------------------------------------------------------------ 3. capture and updates ------------------------------------------------------------------
@pytest.fixture(scope="module")
def net2():
    net = hlp.deep_net(2, seed=0)
    scales = net.calibrate_int8(planes(16, seed=2, S=11))
    yield net, scales
    net.close()


@pytest.mark.parametrize("B", [1, 8])
def test_captured_small_forward_follows_weight_and_scale_updates(net2, B):
    import torch
    net, scales = net2
    x = planes(B, seed=4, S=11)
    old = {k: torch.from_numpy(v).cuda() for k, v in net.variables.items()}
    ev = net.evaluator(B, precision="int8", act_scales=scales)

    def small(e):
        tw = e.tower
        tw.stem(x)
        tw.forward_i8_small(B)
        tw.heads(B)
        return [t.clone() for t in tw.dense(B)]
    try:
        tw = ev.tower
        before = small(ev)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, capture_error_mode="thread_local"):
            tw.stem(x)
            tw.forward_i8_small(B)
            tw.heads(B)
            tw.dense(B)
        g.replay()
        torch.cuda.synchronize()
        assert same_bits((tw.policy[:B], tw.value[:B]), before)
        # new weights, on the device
        other = hlp.deep_net(2, seed=1)
        net.set_variables_device({k: torch.from_numpy(v).cuda() for k, v in other.variables.items()})
        other.close()
        fresh = net.evaluator(B, precision="int8", act_scales=scales)
        after = small(fresh)
        fresh.close()
        assert not same_bits(after, before)
        g.replay()
        torch.cuda.synchronize()
        assert same_bits((tw.policy[:B], tw.value[:B]), after)
        # new scales
        new = (scales * np.linspace(1.5, 0.75, scales.size)).astype(np.float32)
        tw.enable_i8(new)
        assert np.array_equal(tw.act_scales, new) and tw.act_scales.dtype == np.float32
        fresh = net.evaluator(B, precision="int8", act_scales=new)
        rescaled = small(fresh)
        fresh.close()
        assert not same_bits(rescaled, after)
        g.replay()
        torch.cuda.synchronize()
        assert same_bits((tw.policy[:B], tw.value[:B]), rescaled)
        del g
    finally:
        net.set_variables_device(old)
        ev.close()


# ------------------------------------------------------------------ 4. evaluator ------------------------------------------------------------------
def test_evaluator_bits_do_not_depend_on_batch_or_form(net2):
    import torch
    net, scales = net2
    x = planes(8, S=11)
    bf = net.evaluator(8)
    p0, v0 = [t.clone() for t in bf(x)]
    ev = net.evaluator(64, precision="int8", act_scales=scales)

    def run(tw, xs, small):
        n = xs.shape[0]
        tw.stem(xs.contiguous())
        (tw.forward_i8_small if small else tw.forward_i8)(n)
        tw.heads(n)
        return [t.clone() for t in tw.dense(n)]
    try:
        tw = ev.tower
        assert isinstance(tw.small_batch_i8, int) and tw.small_batch_i8 >= 0
        whole = run(tw, x, False)
        assert same_bits(run(tw, x, True), whole)
        assert not same_bits((whole[0],), (p0,))                      # it is not the bf16 path
        for i in (0, 5):
            for small in (False, True):
                one = run(tw, x[i:i + 1], small)
                assert same_bits(one, (whole[0][i:i + 1], whole[1][i:i + 1])), (i, small)
        assert same_bits([t.clone() for t in ev(x)], whole)
        assert same_bits([t.clone() for t in ev(x[:1].contiguous())], (whole[0][:1], whole[1][:1]))
        n = tw.small_batch_i8
        if n > 0:                                                     # eval_hip's choice on both sides of the constant
            calls = []
            big = planes(n + 1, seed=6, S=11)
            ev3 = net.evaluator(n + 1, precision="int8", act_scales=scales)
            t3 = ev3.tower
            s3, b3 = t3.forward_i8_small, t3.forward_i8
            t3.forward_i8_small = lambda b: (calls.append(("small", b)), s3(b))[1]
            t3.forward_i8 = lambda b: (calls.append(("persistent", b)), b3(b))[1]
            at = [t.clone() for t in ev3(big[:n].contiguous())]
            above = [t.clone() for t in ev3(big)]
            assert calls == [("small", n), ("persistent", n + 1)], calls
            assert same_bits(at, (above[0][:n], above[1][:n]))
            ev3.close()
        # a bf16 evaluator of the same net has its old bits before and after
        assert same_bits(bf(x), (p0, v0))
        fresh = net.evaluator(8)
        assert same_bits(fresh(x), (p0, v0))
        fresh.close()
        # the evaluator's numpy face
        pn, vn = ev.eval(x.cpu().numpy())
        assert isinstance(pn, np.ndarray) and pn.dtype == np.float32 and pn.shape == (8, NPIX) and vn.shape == (8,)
        assert np.array_equal(pn.view(np.uint32), whole[0].cpu().numpy().view(np.uint32))
        assert np.array_equal(vn.view(np.uint32), whole[1].cpu().numpy().view(np.uint32))
    finally:
        ev.close()
        bf.close()


# ------------------------------------------------------------------ 5. Player ------------------------------------------------------------------
def _np_eval(ev):
    import torch

    def f(x):
        p, v = ev(torch.from_numpy(np.ascontiguousarray(x, np.float32)).cuda())
        return p.cpu().numpy().copy(), v.cpu().numpy().copy()
    return f


@pytest.mark.parametrize("training", [True, False], ids=["training", "play"])
def test_player_over_an_int8_evaluator_matches_the_oracle(training):
    """Player(pv_fn=ev.eval), ev an int8 evaluator: the leaves stay on the device and go through an int8 evaluator of the Player's
    own, 16 x (tick + forward) replayed as a HIP graph.  Moves, visit vectors, policy bits and the whole tree equal the oracle's,
    which is fed leaf by leaf through a second int8 evaluator of the same net and scales."""
    from alphafive_amd.player import Player
    from test_gpu_parity import _compare_tree
    from test_gpu_realnet import _drive
    deep = hlp.deep_net(2, seed=3)
    try:
        scales = deep.calibrate_int8(planes(16, seed=2, S=11))
        ev = deep.evaluator(4, precision="int8", act_scales=scales)
        cfg = make_cfg(board_size=11, simulation_per_step=60, upper_simulation_per_step=80)
        pl = Player(cfg, training=training, pv_fn=ev.eval, seed=11, game_id=2)
        assert pl.backend == "hip" and pl._pv_owner is deep
        own = pl._pv_device
        assert own is not ev and own.tower is not ev.tower and own.tower.precision == "int8" and own.tower.max_batch == 1
        assert np.array_equal(own.tower.act_scales, ev.tower.act_scales) and own.tower.policy is pl._policy
        feed = deep.evaluator(1, precision="int8", act_scales=scales)
        orc = oracle.OraclePlayer(cfg, training=training, rng_mode=oracle.RNG_PHILOX, seed=11, game_id=2, pv_fn=_np_eval(feed))
        _drive(pl, orc, training, 3, S=11)
        assert pl._graph is not None and pl._graph[1] is not None           # the HIP-graph path ran
        _compare_tree(pl._engine.tree_dump(0), orc, 11)
        assert len(pl.tree) == orc.tree_size()
        pl.close()
        assert own.tower._h is None and ev.tower._h                          # the Player closed its own evaluator, not the caller's
        # Player(pv_fn=deep.eval) on the same net: a bf16 tower, as before
        pb = Player(cfg, training=training, pv_fn=deep.eval, seed=11, game_id=2)
        assert pb.backend == "hip" and pb._pv_device.tower.precision == "bf16"
        pb.close()
    finally:
        deep.close()


# ------------------------------------------------------------------ 6. refusals ------------------------------------------------------------------
def test_small_int8_calls_are_refused_as_the_persistent_ones_are():
    import torch
    from alphafive_amd import tower_hip
    L = tower_hip.lib()
    blk = {k: hlp.tt(v) for k, v in gen.null_block().items()}
    tw = tower_hip.HipTower([blk, blk], 11, W, 2, "cuda:0")
    xq = torch.zeros((2, 8, 144, 16), dtype=torch.int8, device="cuda")
    gq = torch.zeros_like(xq)
    x, q, g = tw.x.data_ptr(), xq.data_ptr(), gq.data_ptr()
    try:
        assert L.af_tower_i8_small_batch(tw._h) >= 0 and L.af_tower_i8_small_batch(None) == 0
        assert tw.small_batch_i8 == L.af_tower_i8_small_batch(tw._h)
        # before enable
        assert L.af_tower_forward_i8_small(tw._h, None, x, q, g, 1) == -3
        assert L.af_tower_conv_i8_small(tw._h, None, 0, 0, q, None, g, 0, 1) == -3
        with pytest.raises(tower_hip.TowerError) as e:
            tw.forward_i8_small(1)
        assert e.value.code == -3
        # enabled, but the blocks' weights were set before: no int8 weights until a setter runs again, block by block
        assert L.af_tower_i8_enable(tw._h, (C.c_float * 4)(1.0, 1.0, 1.0, 1.0), 4) == 0
        assert L.af_tower_forward_i8_small(tw._h, None, x, q, g, 1) == -3
        tw.set_block(0, blk)
        assert L.af_tower_conv_i8_small(tw._h, None, 0, 0, q, None, g, 0, 1) == 0
        assert L.af_tower_conv_i8_small(tw._h, None, 1, 0, q, None, g, 0, 1) == -3
        assert L.af_tower_forward_i8_small(tw._h, None, x, q, g, 1) == -3
        tw.set_block(1, blk)
        assert L.af_tower_forward_i8_small(tw._h, None, x, q, g, 2) == 0
        # arguments
        assert L.af_tower_forward_i8_small(None, None, x, q, g, 1) == -1
        assert L.af_tower_forward_i8_small(tw._h, None, None, q, g, 1) == -1
        assert L.af_tower_forward_i8_small(tw._h, None, x, None, g, 1) == -1
        assert L.af_tower_forward_i8_small(tw._h, None, x, q, None, 1) == -1
        assert L.af_tower_forward_i8_small(tw._h, None, x, q, g, 0) == -1
        assert L.af_tower_forward_i8_small(tw._h, None, x, q, g, -4) == -1
        assert L.af_tower_conv_i8_small(None, None, 0, 0, q, None, g, 0, 1) == -1
        assert L.af_tower_conv_i8_small(tw._h, None, 0, 0, None, None, g, 0, 1) == -1
        assert L.af_tower_conv_i8_small(tw._h, None, 0, 0, q, None, None, 0, 1) == -1
        assert L.af_tower_conv_i8_small(tw._h, None, 0, 1, g, None, q, 0, 1) == -1     # the second convolution needs the block input
        assert L.af_tower_conv_i8_small(tw._h, None, 0, 0, q, None, g, 0, 0) == -1
        assert L.af_tower_conv_i8_small(tw._h, None, 2, 0, q, None, g, 0, 1) == -1
        assert L.af_tower_conv_i8_small(tw._h, None, -1, 0, q, None, g, 0, 1) == -1
        assert L.af_tower_conv_i8_small(tw._h, None, 1, 1, g, q, q, 0, 1) == -1        # the last block's output has no int8 scale
        assert L.af_tower_conv_i8_small(tw._h, None, 1, 1, g, q, x, 1, 1) == 0
        torch.cuda.synchronize()
    finally:
        tw.close()
    t15 = tower_hip.HipTower([blk], 15, W, 2, "cuda:0")
    try:
        assert L.af_tower_forward_i8_small(t15._h, None, t15.x.data_ptr(), q, g, 1) == -1
        assert L.af_tower_conv_i8_small(t15._h, None, 0, 0, q, None, g, 0, 1) == -1
        assert L.af_tower_i8_small_batch(t15._h) == 0 and t15.small_batch_i8 == 0
    finally:
        t15.close()
