"""af_tower_forward_small (csrc/af_tower_bf16.hip: af_tower_conv_small, one workgroup per pixel tile, weights streamed) at both board
sizes: against fp64 in the exact regime of tests/tower_cases.py, against the persistent kernels bit for bit on random data, through
the whole net on either side of HipTower.small_batch, under a captured graph across a weight update, and its ABI errors."""
import ctypes

import numpy as np
import pytest

import tower_cases as gen
import tower_gpu
from tower_cases import ISOLATIONS
from tower_gpu import _assert_untouched, _mismatch, _poison, _t, _Tune, planes, same_bits

pytestmark = pytest.mark.gpu
SIZES = (11, 15)
W = gen.W
NWIDE = 96                                           # positions of the whole-net reference: more than small_batch + 1 at either size


@pytest.fixture(scope="module", params=SIZES)
def sized_towers(request):
    gen_ = tower_gpu.block_towers(request.param)
    yield request.param, next(gen_)
    for _ in gen_:                                   # (runs the generator's clean-up)
        pass


def _run_block_small(tw, h_dev, B):
    """tower_gpu._run_block with the new entry point: one forward_small of a single-block tower -> (block output, mid activation)."""
    _poison(tw, B)
    tw.load_nchw(h_dev[:B])
    tw.forward_small(B)
    _assert_untouched(tw, B)
    return tw.store_nchw(B), tw.scratch_nchw(B)


@pytest.mark.parametrize("iso", ISOLATIONS)
def test_small_block_convolutions_are_exact(sized_towers, iso):
    """Every (cout, cin, tap, pixel) of one convolution on the tile-parallel kernel: mid activation and block output bit-equal to
    fp64 at batch 1, 2, 3 and the case's own count; nothing at or past the batch and no zero row written."""
    import torch
    S, towers = sized_towers
    tw, h_dev, (ref_out, ref_g) = towers("exact", iso)
    for B in (1, 2, 3, h_dev.shape[0]):
        out, g = _run_block_small(tw, h_dev, B)
        assert torch.equal(g, ref_g[:B]), f"{S}x{S} mid activation, batch {B}: " + _mismatch(g, ref_g[:B])
        assert torch.equal(out, ref_out[:B]), f"{S}x{S} block output, batch {B}: " + _mismatch(out, ref_out[:B])


def _two_block_tower(S, max_batch):
    """Two blocks of random (bf16-valued) weights, every convolution and projection non-zero, from the rounded-regime generators."""
    import torch
    from alphafive_amd import tower_hip
    c1, c2, pj = (gen.rounded_block_case(S, iso) for iso in ISOLATIONS)
    tt = lambda wb: (torch.from_numpy(np.asarray(wb[0], np.float32)), torch.from_numpy(np.asarray(wb[1], np.float32)))  # noqa: E731
    res0 = tt(pj["res"])
    res1 = (res0[0].flip(0).contiguous(), tt(c2["res"])[1])          # (the only random projection of the generators, couts reversed)
    blocks = [dict(c1=tt(c1["c1"]), c2=tt(c2["c2"]), res=res0), dict(c1=tt(pj["c1"]), c2=tt(c1["c1"]), res=res1)]
    return tower_hip.HipTower(blocks, S, W, max_batch, "cuda:0"), _t(c1["h"][:max_batch], torch.bfloat16)


@pytest.mark.parametrize("S", SIZES)
def test_small_forward_has_the_bits_of_the_persistent_kernels(S):
    """forward_small(B) against forward(B) from the same input, under engine 3 (af_tower_conv3 + af_tower_conv at 11x11) and engine
    0 (af_tower_conv for both): x and g equal bit for bit.  33 positions cross the 32 an XCD group of the persistent grid walks."""
    import torch
    tw, h = _two_block_tower(S, 33 + 3)
    try:
        for B in (1, 2, 5, 33):
            _poison(tw, B)
            tw.load_nchw(h[:B])
            tw.forward_small(B)
            _assert_untouched(tw, B)
            small = (tw.x[:B].clone(), tw.g[:B].clone())
            assert bool(small[0].float().abs().sum() > 0) and bool(torch.isfinite(small[0].float()).all())
            for engine in (3, 0):
                tw.load_nchw(h[:B])
                with _Tune(k3=engine):
                    tw.forward(B)
                torch.cuda.synchronize()
                assert torch.equal(tw.x[:B], small[0]), f"x, batch {B}, engine {engine}"
                assert torch.equal(tw.g[:B], small[1]), f"g, batch {B}, engine {engine}"
    finally:
        tw.close()


@pytest.fixture(scope="module", params=SIZES)
def deep_net(request):
    from alphafive_amd.network_deep import DeepResNet
    S = request.param
    net = DeepResNet(S, blocks=2, width=W, device="cuda", seed=5)
    pv = net.select_backend("hip", NWIDE)
    tw = net._tower
    assert tw.small_batch + 1 <= NWIDE
    x = planes(NWIDE, seed=3, S=S)

    def persistent(B):                               # eval_hip's sequence on the persistent kernels, whatever small_batch is
        tw.stem(x[:B].contiguous())
        tw.forward(B)
        tw.heads(B)
        return tuple(t.clone() for t in tw.dense(B))
    ref, wide = persistent(64), persistent(NWIDE)    # computed once; `wide` serves the batches past 64 and repeats ref on its rows
    assert same_bits((wide[0][:64], wide[1][:64]), ref)
    yield S, net, pv, x, wide
    net.close()


def test_positions_do_not_depend_on_the_batch(deep_net):
    """Row i of the evaluation at B = 64 on the persistent kernels = eval_hip of position i alone = rows of eval_hip at B = 1 and 2:
    the same bits for policy and value, on whichever tower kernel eval_hip picks."""
    S, net, pv, x, ref = deep_net
    for i in (0, 7, 63):
        got = tuple(t.clone() for t in pv(x[i:i + 1].contiguous()))
        assert same_bits(got, (ref[0][i:i + 1], ref[1][i:i + 1])), f"{S}x{S}: position {i} alone"
    for k in (1, 2):
        got = tuple(t.clone() for t in pv(x[:k].contiguous()))
        assert same_bits(got, (ref[0][:k], ref[1][:k])), f"{S}x{S}: batch {k}"


def test_positions_do_not_depend_on_the_form_across_small_batch(deep_net):
    """... and at B = small_batch and small_batch + 1: the last batch on the tile-parallel kernel, the first on the persistent ones."""
    S, net, pv, x, ref = deep_net
    tw = net._tower
    if tw.small_batch == 0:
        pytest.skip("af_tower_small_batch is 0 at %dx%d: eval_hip never takes the small form, no threshold to cross" % (S, S))
    for k in (tw.small_batch, tw.small_batch + 1):
        got = tuple(t.clone() for t in pv(x[:k].contiguous()))
        assert same_bits(got, (ref[0][:k], ref[1][:k])), f"{S}x{S}: batch {k} (small_batch {tw.small_batch})"


def test_small_forward_replays_in_a_graph_across_a_weight_update(deep_net):
    """[stem; forward_small; heads; dense] at B = 1 captured and replayed; after load_device with other weights the same graph
    gives the bits of an eager evaluation with the new weights (launches only, every buffer keeps its address)."""
    import torch
    from alphafive_amd.network_deep import DeepResNet
    S, net, pv, x, ref = deep_net
    tw = net._tower
    x1 = x[5:6].contiguous()

    def run():
        tw.stem(x1)
        tw.forward_small(1)
        tw.heads(1)
        return tw.dense(1)
    run()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        run()
    tw.policy.zero_()
    tw.value.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert same_bits((tw.policy[:1], tw.value[:1]), (ref[0][5:6], ref[1][5:6]))
    other = DeepResNet(S, blocks=2, width=W, device="cuda", seed=6)
    old = {k: torch.from_numpy(v).cuda() for k, v in net.variables.items()}
    try:
        tw.load_device({k: torch.from_numpy(v).cuda() for k, v in other.variables.items()})
        tw.policy.zero_()
        tw.value.zero_()
        g.replay()
        torch.cuda.synchronize()
        got = (tw.policy[:1].clone(), tw.value[:1].clone())
        want = tuple(t.clone() for t in other.select_backend("hip", 1)(x1))
        assert same_bits(got, want)
        assert not torch.equal(got[0], ref[0][5:6])
    finally:
        tw.load_device(old)                          # the module's net goes on with its own weights
        other.close()
    assert same_bits(tuple(t.clone() for t in pv(x1)), (ref[0][5:6], ref[1][5:6]))


def test_small_forward_abi_errors():
    """af_tower_forward_small: batch 0 or a null pointer is AF_TOWER_ERR_ARG (-1); before every block is set AF_TOWER_ERR_STATE (-3)."""
    import torch
    from alphafive_amd import tower_hip
    L = tower_hip.lib()
    tw = tower_gpu._tower(11, {}, 2)                 # a null block, set
    try:
        x, g = tw.x.data_ptr(), tw.g.data_ptr()
        assert L.af_tower_forward_small(tw._h, None, x, g, 0) == -1
        assert L.af_tower_forward_small(tw._h, None, x, g, -3) == -1
        assert L.af_tower_forward_small(tw._h, None, None, g, 1) == -1
        assert L.af_tower_forward_small(tw._h, None, x, None, 1) == -1
        assert L.af_tower_forward_small(None, None, x, g, 1) == -1
        assert L.af_tower_forward_small(tw._h, None, x, g, 1) == 0
        assert L.af_tower_small_batch(None) == 0 and L.af_tower_small_batch(tw._h) == tw.small_batch >= 0
        h = ctypes.c_void_p()
        assert L.af_tower_create(11, 128, 2, 0, ctypes.byref(h)) == 0
        try:
            assert L.af_tower_forward_small(h, None, x, g, 1) == -3
        finally:
            L.af_tower_destroy(h)
        torch.cuda.synchronize()
    finally:
        tw.close()
