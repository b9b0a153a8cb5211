"""The device calibration of the int8 tower (af_tower_i8_calibrate; csrc/af_tower_i8.hip) on the GPU: the absmax kernel alone
against numpy over the board pixels, the scales against tower_i8.scales_from_absmax of maxima taken through the public bf16 API,
the re-packed buffers against a fresh evaluator built through the host path, capture and weight hand-over, the refusal path, and
the distance from the host calibrator (DeepResNet.calibrate_int8) under the project's torch-bf16 rule."""
import numpy as np
import pytest

from alphafive_amd import tower_i8 as t8
from tower_gpu import planes, same_bits

pytestmark = pytest.mark.gpu
W, S, NPIX, PIX = 128, 11, 121, 144
BATCHES = (1, 7, 33)
MAXB = 40


# ------------------------------------------------------------------ 1. the absmax kernel alone ------------------------------------------------------------------
@pytest.fixture(scope="module")
def plain_tower():
    """A bf16 handle: af_tower_i8_absmax needs no enable."""
    import torch
    from alphafive_amd import tower_hip
    z3, z1, zb = torch.zeros(W, W, 3, 3), torch.zeros(W, W, 1, 1), torch.zeros(W)
    tw = tower_hip.HipTower([dict(c1=(z3, zb), c2=(z3, zb), res=(z1, zb))], S, W, 2, "cuda:0")
    yield tw
    tw.close()


def _bf16_bits(value):
    return int(np.asarray(value, np.float32).view(np.uint32) >> 16)


def _random_bits(B, seed):
    """uint16 [B + 1][16][144][8]: bf16 values of N(0, 1) everywhere — the zero rows and the pad unit included, and one position
    more than the batch — so that a kernel that reads outside the board pixels of the batch reads something."""
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((B + 1, 16, PIX, 8)).astype(np.float32).view(np.uint32) >> 16).astype(np.uint16)


def _board_absmax(bits, B):
    return int((bits[:B, :, S:S + NPIX, :] & 0x7fff).max())


def _device_absmax(tw, bits, B):
    import torch
    x = torch.from_numpy(bits.view(np.int16)).cuda().view(torch.bfloat16)
    return tw.absmax(x, B)


@pytest.mark.parametrize("B", (1, 2, 7, 33))
def test_absmax_kernel_equals_numpy_over_the_board_pixels(plain_tower, B):
    tw = plain_tower
    big, huge = _bf16_bits(37.5), _bf16_bits(1.0e30)
    base = _random_bits(B, 10 + B)
    assert _board_absmax(base, B) < big
    cases = {}
    cases["random"] = base
    c = base.copy(); c[0, 0, S, 0] = big; cases["first board unit of position 0, octet 0"] = c
    c = base.copy(); c[B - 1, 15, S + NPIX - 1, 7] = big; cases["last board unit of the last position, octet 15, element 7"] = c
    c = base.copy(); c[B // 2, 7, S + 60, 3] = big | 0x8000; cases["a negative value of the largest magnitude"] = c
    c = np.zeros_like(base); c[B - 1, 9, S + 5, 2] = 0x8000; cases["-0.0 only"] = c
    cases["all zero"] = np.zeros_like(base)
    c = base.copy()                                                   # everything that is not a board pixel of the batch, loud
    c[:, :, :S, :] = huge; c[:, :, S + NPIX:, :] = huge | 0x8000; c[B] = huge
    cases["borders and the position behind the batch"] = c
    c = base.copy(); c[B - 1, 3, S + 17, 5] = 0x7f80; cases["+inf"] = c
    c = base.copy(); c[0, 12, S + 120, 1] = 0xff80; c[0, 1, S, 0] = big; cases["-inf"] = c
    c = base.copy(); c[B - 1, 8, S + 64, 6] = 0x7fc1; c[0, 0, S + 1, 0] = 0x7f80; cases["a NaN next to an infinity"] = c
    c = base.copy(); c[0, 15, S + 3, 4] = 0xffa0; cases["a negative NaN"] = c
    for name, bits in cases.items():
        want, got = _board_absmax(bits, B), _device_absmax(tw, bits, B)
        assert got == want, "batch %d, %s: device 0x%04x, numpy 0x%04x" % (B, name, got, want)
    assert _board_absmax(cases["-0.0 only"], B) == 0 and _board_absmax(cases["borders and the position behind the batch"], B) < big
    assert _board_absmax(cases["+inf"], B) == 0x7f80 and _board_absmax(cases["-inf"], B) == 0x7f80
    assert _board_absmax(cases["a NaN next to an infinity"], B) == 0x7fc1 and _board_absmax(cases["a negative NaN"], B) == 0x7fa0
    # the word is max-ed into, not overwritten: what the caller left there stays if it is larger
    import torch
    word = torch.full((1,), 0x7000, dtype=torch.int32, device="cuda")
    x = torch.from_numpy(base.view(np.int16)).cuda().view(torch.bfloat16)
    from alphafive_amd import tower_hip
    assert tower_hip.lib().af_tower_i8_absmax(tw._h, None, x.data_ptr(), B, word.data_ptr()) == 0
    assert int(word.item()) == 0x7000


def test_absmax_kernel_behind_the_grid_cap():
    """The grid is a thread per four units up to 1024 workgroups = 541 positions; behind that a thread takes further rounds of
    four: 545 positions, the maximum in the last board unit of the last one, everything behind the batch loud."""
    import torch
    from alphafive_amd import tower_hip
    B = 545
    z3, z1, zb = torch.zeros(W, W, 3, 3), torch.zeros(W, W, 1, 1), torch.zeros(W)
    tw = tower_hip.HipTower([dict(c1=(z3, zb), c2=(z3, zb), res=(z1, zb))], S, W, 1, "cuda:0")
    try:
        bits = _random_bits(B, 3)
        bits[B] = _bf16_bits(1.0e30)
        want = _board_absmax(bits, B)
        x = torch.from_numpy(bits.view(np.int16)).cuda().view(torch.bfloat16)
        assert tw.absmax(x, B) == want
        x[B - 1, 15, S + NPIX - 1, 7] = 37.5
        assert tw.absmax(x, B) == _bf16_bits(37.5) > want
        x[0, 0, S, 0] = -64.0
        assert tw.absmax(x, B) == _bf16_bits(64.0)
    finally:
        tw.close()


def test_absmax_and_calibrate_refuse_bad_arguments(plain_tower):
    import torch
    from alphafive_amd import tower_hip
    L, tw = tower_hip.lib(), plain_tower
    word = torch.zeros(1, dtype=torch.int32, device="cuda")
    assert L.af_tower_i8_absmax(tw._h, None, tw.x.data_ptr(), 0, word.data_ptr()) == -1
    assert L.af_tower_i8_absmax(tw._h, None, None, 1, word.data_ptr()) == -1
    assert L.af_tower_i8_absmax(tw._h, None, tw.x.data_ptr(), 1, None) == -1
    assert L.af_tower_i8_absmax(None, None, tw.x.data_ptr(), 1, word.data_ptr()) == -1
    # a handle that is not enabled: calibrate and its status are ERR_STATE, bad arguments come first
    assert L.af_tower_i8_calibrate(tw._h, None, tw.x.data_ptr(), tw.g.data_ptr(), 1, 1.0) == -3
    for margin in (0.0, -1.0, float("inf"), float("nan")):
        assert L.af_tower_i8_calibrate(tw._h, None, tw.x.data_ptr(), tw.g.data_ptr(), 1, margin) == -1
    assert L.af_tower_i8_calibrate(tw._h, None, tw.x.data_ptr(), tw.g.data_ptr(), 0, 1.0) == -1
    assert L.af_tower_i8_calibrate(tw._h, None, None, tw.g.data_ptr(), 1, 1.0) == -1
    assert L.af_tower_i8_calibrate(tw._h, None, tw.x.data_ptr(), None, 1, 1.0) == -1
    import ctypes as C
    st, n = C.c_int32(), C.c_int32()
    assert L.af_tower_i8_calibration_status(tw._h, C.byref(st), C.byref(n)) == -3
    assert L.af_tower_i8_calibration_status(tw._h, None, C.byref(n)) == -1
    with pytest.raises(ValueError):
        tw.calibrate_i8(planes(1, S=11))                              # a bf16 tower, refused in Python
    # enabled, but the block's weights were set before: no int8 weights yet (af_tower_forward_i8's condition)
    one = (C.c_float * 2)(1.0, 1.0)
    z3, z1, zb = torch.zeros(W, W, 3, 3), torch.zeros(W, W, 1, 1), torch.zeros(W)
    late = tower_hip.HipTower([dict(c1=(z3, zb), c2=(z3, zb), res=(z1, zb))], S, W, 2, "cuda:0")
    try:
        assert L.af_tower_i8_enable(late._h, one, 2) == 0
        assert L.af_tower_i8_calibrate(late._h, None, late.x.data_ptr(), late.g.data_ptr(), 1, 1.0) == -3
        assert L.af_tower_i8_calibration_status(late._h, C.byref(st), C.byref(n)) == 0 and (st.value, n.value) == (0, 0)
    finally:
        late.close()
    t15 = tower_hip.HipTower([dict(c1=(z3, zb), c2=(z3, zb), res=(z1, zb))], 15, W, 1, "cuda:0")
    try:
        assert L.af_tower_i8_calibrate(t15._h, None, t15.x.data_ptr(), t15.g.data_ptr(), 1, 1.0) == -1
        assert L.af_tower_i8_absmax(t15._h, None, t15.x.data_ptr(), 1, word.data_ptr()) == -1
        assert L.af_tower_i8_calibration_status(t15._h, C.byref(st), C.byref(n)) == -1
    finally:
        t15.close()
    torch.cuda.synchronize()


# ------------------------------------------------------------------ 2. the whole calibration ------------------------------------------------------------------
@pytest.fixture(scope="module")
def net3():
    """The 3-block net, host-calibrated scales to build evaluators with, and the absmax the device must find for the first B of
    the 33 random-stone planes, B in BATCHES — taken through the public bf16 API: towers over the block prefixes [:1], [:2], [:3]
    run forward (the kernels the calibration launches, so the same bits), store_nchw is h_k and scratch_nchw g_{k-1}."""
    import torch
    from alphafive_amd import tower_hip
    from alphafive_amd.network_deep import DeepResNet
    net = DeepResNet(11, blocks=3, seed=0)
    x = planes(33, S=11)
    scales0 = net.calibrate_int8(planes(16, seed=2, S=11))
    expected = {B: [None] * 6 for B in BATCHES}
    for k in (1, 2, 3):
        tw = tower_hip.HipTower(net.tower[:k], S, W, 33, "cuda:0", stem=net.stem)
        try:
            for B in BATCHES:
                tw.stem(x[:B].contiguous())
                if k == 1:
                    expected[B][0] = float(tw.store_nchw(B).float().abs().max())
                tw.forward(B)
                expected[B][2 * k - 1] = float(tw.scratch_nchw(B).float().abs().max())
                if k < 3:
                    expected[B][2 * k] = float(tw.store_nchw(B).float().abs().max())
        finally:
            tw.close()
    expected = {B: np.array(v, np.float32) for B, v in expected.items()}
    for v in expected.values():
        assert np.isfinite(v).all() and (v > 0).all()
    yield net, x, scales0, expected
    net.close()


def _bits32(a):
    return np.asarray(a, np.float32).view(np.uint32)


def _run(tw, x, small):
    """The whole evaluation on one form of the int8 blocks -> clones of (policy, value)."""
    B = x.shape[0]
    tw.stem(x.contiguous())
    (tw.forward_i8_small if small else tw.forward_i8)(B)
    tw.heads(B)
    p, v = tw.dense(B)
    return p.clone(), v.clone()


def _assert_same_buffers(a, b, what):
    assert len(a) == len(b)
    for i, (u, v) in enumerate(zip(a, b)):
        assert u.shape == v.shape and np.array_equal(u, v), "%s: int8 buffer %d of %d differs in %d bytes" % (what, i, len(a), int((u != v).sum()))


def test_device_scales_are_the_specification_of_the_bf16_towers_absmax(net3):
    net, x, scales0, expected = net3
    ev = net.evaluator(MAXB, precision="int8", act_scales=scales0)
    little = net.evaluator(4, precision="int8", act_scales=scales0)   # B > max_batch: the scratch route
    try:
        assert ev.tower.calibration_status() == (0, 0)
        assert np.array_equal(_bits32(ev.tower.read_act_scales()), _bits32(scales0))
        count = 0
        for B in BATCHES:
            for margin in (1.0, 1.25):
                want, want_r = t8.scales_from_absmax(expected[B], margin)
                assert t8.calibration_ok(expected[B], margin)
                version = net.version
                net.calibrate_int8_device(x[:B].contiguous(), margin, evaluators=[ev, little])
                assert net.version == version + 1
                count += 1
                for name, tw in (("own buffers", ev.tower), ("scratch buffers", little.tower)):
                    got = tw.read_act_scales()
                    assert np.array_equal(_bits32(got), _bits32(want)), "batch %d margin %s, %s: device %s, specification %s" % (
                        B, margin, name, got, want)
                    assert tw.calibration_status() == (0, count)
                    both = tw.debug_weights_i8()[-1].view(np.float32)
                    assert np.array_equal(_bits32(both[6:]), _bits32(want_r))
        assert np.array_equal(_bits32(ev.tower.act_scales), _bits32(scales0))     # the host's copy is the last HOST-given one
    finally:
        ev.close()
        little.close()


@pytest.mark.parametrize("B", BATCHES)
def test_repacked_buffers_and_outputs_equal_a_fresh_evaluators(net3, B):
    net, x, scales0, _ = net3
    xb = x[:B].contiguous()
    ev = net.evaluator(MAXB, precision="int8", act_scales=scales0)
    try:
        before = ev.tower.debug_weights_i8()
        net.calibrate_int8_device(xb, 1.25, evaluators=[ev])
        scales = ev.tower.read_act_scales()
        assert not np.array_equal(scales, scales0)
        fresh = net.evaluator(MAXB, precision="int8", act_scales=scales)
        try:
            after = ev.tower.debug_weights_i8()
            _assert_same_buffers(after, fresh.tower.debug_weights_i8(), "batch %d" % B)
            assert any((u != v).any() for u, v in zip(before, after))
            for small in (True, False):
                assert same_bits(_run(ev.tower, xb, small), _run(fresh.tower, xb, small)), "batch %d, %s form" % (B, "tile-parallel" if small else "persistent")
            assert same_bits(ev(xb), fresh(xb))
        finally:
            fresh.close()
    finally:
        ev.close()


def test_capture_and_weight_hand_over_follow_the_device_calibration(net3):
    import torch
    from alphafive_amd.network_deep import DeepResNet
    net, x33, scales0, _ = net3
    x = x33[:8].contiguous()
    old = {k: torch.from_numpy(v).cuda() for k, v in net.variables.items()}
    other, third = DeepResNet(11, blocks=3, seed=1), DeepResNet(11, blocks=3, seed=2)
    ev = net.evaluator(8, precision="int8", act_scales=scales0)
    try:
        tw = ev.tower
        net.calibrate_int8_device(x, evaluators=[ev])
        first = tw.read_act_scales()
        before = _run(tw, x, False)
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
        # (a) a graph captured BEFORE the hand-over replays with the new weights under scales measured on them
        new = {k: torch.from_numpy(v).cuda() for k, v in other.variables.items()}
        version = ev.weights_version()
        net.set_variables_device(new, calibrate_on=x)
        assert ev.weights_version() == version + 1
        second = tw.read_act_scales()
        assert tw.calibration_status() == (0, 2) and not np.array_equal(first, second)
        fresh = net.evaluator(8, precision="int8", act_scales=second)
        want = [t.clone() for t in fresh(x)]
        _assert_same_buffers(tw.debug_weights_i8(), fresh.tower.debug_weights_i8(), "set_variables_device(calibrate_on)")
        fresh.close()
        assert not same_bits(want, before)
        g.replay()
        torch.cuda.synchronize()
        assert same_bits((tw.policy[:8], tw.value[:8]), want)
        # (b) [load_device; calibrate_i8] captured, replayed over changed source tensors (a bf16 net's values: biases as packed)
        hold = {k: t.clone() for k, t in new.items()}
        g2 = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g2, capture_error_mode="thread_local"):
            tw.load_device(hold)
            tw.calibrate_i8(x)
        for k, v in third.variables.items():
            hold[k].copy_(torch.from_numpy(v))
        g2.replay()
        torch.cuda.synchronize()
        assert tw.calibration_status() == (0, 3)
        fresh3 = third.evaluator(8, precision="int8", act_scales=tw.read_act_scales())
        want3 = [t.clone() for t in fresh3(x)]
        _assert_same_buffers(tw.debug_weights_i8(), fresh3.tower.debug_weights_i8(), "captured [load_device; calibrate_i8]")
        fresh3.close()
        assert not same_bits(want3, want)
        g.replay()
        torch.cuda.synchronize()
        assert same_bits((tw.policy[:8], tw.value[:8]), want3)
        # (c) the old weights handed back and calibrated again: the first scales, and the first outputs, bit for bit
        net.set_variables_device(old, calibrate_on=x)
        assert np.array_equal(_bits32(tw.read_act_scales()), _bits32(first)) and tw.calibration_status() == (0, 4)
        g.replay()
        torch.cuda.synchronize()
        assert same_bits((tw.policy[:8], tw.value[:8]), before)
        del g, g2
    finally:
        net.set_variables_device(old)
        ev.close()
        other.close()
        third.close()


def test_a_calibration_that_meets_an_infinity_is_refused_whole():
    import torch
    from alphafive_amd.network_deep import DeepResNet
    net = DeepResNet(11, blocks=3, seed=4)
    x = planes(7, seed=3, S=11)
    try:
        ev = net.evaluator(8, precision="int8", act_scales=net.calibrate_int8(x))
        tw = ev.tower
        net.calibrate_int8_device(x)
        assert tw.calibration_status() == (0, 1)
        good = net.variables
        bad = {k: v.copy() for k, v in good.items()}
        bad["tower/block0_conv1/bias"][:] = np.inf                    # finite planes, an infinite g_0, NaN behind it
        net.set_variables(bad)
        scales, buffers = tw.read_act_scales(), tw.debug_weights_i8()
        net.calibrate_int8_device(x, 1.25)
        torch.cuda.synchronize()
        assert tw.calibration_status() == (1, 1)
        assert np.array_equal(_bits32(tw.read_act_scales()), _bits32(scales))
        _assert_same_buffers(tw.debug_weights_i8(), buffers, "refused calibration")
        # and the next good one is taken
        net.set_variables(good)
        net.calibrate_int8_device(x, 1.25)
        assert tw.calibration_status() == (0, 2)
        assert not np.array_equal(tw.read_act_scales(), scales)
    finally:
        net.close()


def test_device_scales_are_as_close_to_the_host_calibrators_as_torch_bf16(net3):
    """The standing rule of tests/test_gpu_realnet.py (_assert_no_worse_than_torch_bf16) on the scales: the device calibration
    measures the bf16 kernels where calibrate_int8 measures the fp32 torch path; its relative distance from calibrate_int8 may be
    at most twice that of the all-PyTorch bf16 path measured layer by layer the same way, plus one bf16 ulp (2^-9, relative)."""
    import torch
    import torch.nn.functional as F
    net, x, scales0, expected = net3
    host = net.calibrate_int8(x).astype(np.float64)
    dev = t8.scales_from_absmax(expected[33], 1.0)[0].astype(np.float64)
    ev = net.evaluator(MAXB, precision="int8", act_scales=scales0)
    try:
        net.calibrate_int8_device(x, evaluators=[ev])
        assert np.array_equal(ev.tower.read_act_scales().astype(np.float64), dev)
    finally:
        ev.close()
    with torch.no_grad():
        h = F.elu(F.conv2d(x.to(net.dtype), *net.stem, padding=2))
        amax = []
        for blk in net.tower:
            g = F.elu(F.conv2d(h, *blk["c1"], padding=1))
            amax += [h.abs().max(), g.abs().max()]
            h = F.elu(F.conv2d(h, *blk["res"]) + F.conv2d(g, *blk["c2"], padding=1))
        tor = (torch.stack(amax).double().cpu().numpy() / 127.0).astype(np.float32).astype(np.float64)
    e_dev, e_tor = np.abs(dev - host) / host, np.abs(tor - host) / host
    print("scales against calibrate_int8 (fp32 torch), relative: device max %.3g mean %.3g; torch bf16 max %.3g mean %.3g"
          % (e_dev.max(), e_dev.mean(), e_tor.max(), e_tor.mean()))
    assert e_dev.max() <= 2.0 * e_tor.max() + 2.0 ** -9
