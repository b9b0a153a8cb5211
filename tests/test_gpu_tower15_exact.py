"""The bf16 tower kernels on 15x15 boards (csrc/af_tower_bf16.hip, Geo<15>) against oracle/tower_fp64.py, one layer at a time.
The cases, the two regimes and the error bound are those of tests/tower_cases.py; tests/test_tower15_reference_cpu.py proves —
without a GPU — that the exact-regime cases meet the conditions under which the kernels must reproduce fp64 bit for bit.

What is particular to 15x15: the convolution runs every board as two half-board pseudo-positions (rows 0..7 and 8..14) that stage
one row of their sibling; the block's second convolution runs in place, so a half may stage a row its sibling has already
overwritten.  It must never multiply it: the "conv2" and "proj" isolations, whose outputs on rows 7 and 8 depend on stones on both
sides of the seam, are wrong integers if it does.  Stem, heads and dense layers run whole positions in 8 tiles."""
import pytest

import tower_cases as gen
import tower_gpu
from oracle import tower_fp64 as ref64
from tower_cases import ISOLATIONS, NDIST, W
from tower_gpu import _assert_untouched, _mismatch, _null_block, _poison, _run_block, _t, _tower, _Tune, _worst_ratio

pytestmark = pytest.mark.gpu
S = 15
NPIX, NROUND = gen.SIZES[S].NPIX, gen.SIZES[S].NROUND
DEPTHS = (0, 8, 12, 16)          # tune key 0: the default ring depths (12 / 6), then each depth the key accepts
# (batch, persistent workgroups = tune key 1; 0 = one per CU, at most one per half board)
#   1, 2, 3: a single position, two, an odd count (6 half boards)
#   9 / 17 / 25 on 8 workgroups: 18 / 34 / 50 half boards = 3 / 5 / 7 iterations for the first workgroups, one fewer for the rest:
#       both LDS buffer parities, the first, steady and last iterations of the persistent loop; with an even grid a workgroup
#       keeps one half, so both halves meet both parities
#   130: 260 half boards, more than one pass of 256 workgroups;  232: every (cin, pixel) site non-zero once
CONFIGS = ((1, 0), (2, 0), (3, 0), (9, 8), (17, 8), (25, 8), (130, 0), (232, 0))


def test_the_library_takes_11_and_15_and_nothing_else():
    from alphafive_amd import tower_hip
    for size in (9, 13, 19):
        with pytest.raises(tower_hip.TowerError) as e:
            tower_hip.HipTower([_null_block()], size, W, 1, "cuda:0")
        assert e.value.code == -1
    tw = _tower(S, {}, 2)
    try:
        assert tw.pix == 256 and tw.x.shape == (2, 16, 256, 8) and tw.policy.shape == (2, 225)
        assert tw.flops_per_position == 2 * (128 * 128 * 19) * 225
    finally:
        tw.close()


@pytest.fixture(scope="module")
def block_towers():
    yield from tower_gpu.block_towers(S)


@pytest.mark.parametrize("depth", DEPTHS)
@pytest.mark.parametrize("iso", ISOLATIONS)
def test_block_convolutions_are_exact(block_towers, iso, depth):
    """Every (cout, cin, tap, pixel, position) of one convolution, at every ring depth, batch and grid: bit equality with fp64."""
    tower_gpu.check_block_convolutions_are_exact(block_towers, iso, depth, CONFIGS)


@pytest.mark.parametrize("engine", [0, 2])
def test_tune_key_3_changes_nothing_on_a_15x15_handle(block_towers, engine):
    """af_tower_conv3 walks whole positions: a 15x15 handle runs af_tower_conv for both convolutions whatever key 3 says."""
    import torch
    tw, h_dev, (ref_out, ref_g) = block_towers("exact", "proj")
    out, g = _run_block(tw, h_dev, 25, 0, 8, engine=engine)
    assert torch.equal(g, ref_g[:25]) and torch.equal(out, ref_out[:25])


@pytest.fixture(scope="module")
def ends_tower():
    yield from tower_gpu.ends_tower(S, NDIST + 5 + 3)


@pytest.mark.parametrize("B", [1, 3, NDIST + 5])
def test_stem_is_exact(ends_tower, B):
    """All 75 taps at corners, edges, the interior and both sides of the seam; a full, an empty and randomly filled boards."""
    import torch
    tw, case = ends_tower, gen.exact_stem_case(S)
    y, _ = ref64.stem(case["planes"], case["w"], case["b"])
    ref = _t(ref64.bf16_round(y), torch.bfloat16)
    # batches 1 and 3 would see only the full and the empty board and one single stone: rotate so that each batch starts elsewhere
    idx = (torch.arange(B, device="cuda") + (0 if B > 3 else 2 * B)) % NDIST
    planes = _t(case["planes"])[idx].contiguous()
    _poison(tw, B)
    tw.stem(planes)
    _assert_untouched(tw, B)
    out = tw.store_nchw(B)
    assert torch.equal(out, ref[idx]), _mismatch(out, ref[idx])


def test_stem_single_stones_and_boards_one_position_at_a_time(ends_tower):
    """Batch 1 on each of the 64 distinct positions: the full board, the empty one, every single stone, the random fills."""
    import torch
    tw, case = ends_tower, gen.exact_stem_case(S)
    y, _ = ref64.stem(case["planes"], case["w"], case["b"])
    ref = _t(ref64.bf16_round(y), torch.bfloat16)
    planes = _t(case["planes"])
    _poison(tw, 1)
    for i in range(NDIST):
        tw.stem(planes[i:i + 1].contiguous())
        out = tw.store_nchw(1)
        assert torch.equal(out, ref[i:i + 1]), f"position {i}: " + _mismatch(out, ref[i:i + 1])
    _assert_untouched(tw, 1)


@pytest.mark.parametrize("B", [1, 3, NDIST + 5])
def test_heads_are_exact(ends_tower, B):
    """The heads' 1x1 convolutions on an integer tower output: the MFMA kernel (the only one at 15x15, whatever key 4 says) = fp64."""
    import torch
    tw, case = ends_tower, gen.exact_heads_case(S)
    vin, _, pin, _ = ref64.heads(case["h"], case["vconv"], case["pconv"])
    ref_v, ref_p = _t(ref64.bf16_round(vin), torch.bfloat16), _t(ref64.bf16_round(pin), torch.bfloat16)
    idx = torch.arange(B, device="cuda") % NDIST
    h = _t(case["h"], torch.bfloat16)[idx].contiguous()
    for kernel in (1, 0):
        _poison(tw, B)
        tw.load_nchw(h)
        with _Tune(k4=kernel):
            v, p = tw.heads(B)
        _assert_untouched(tw, B)
        assert v.shape == (B, 4 * NPIX) and p.shape == (B, 16 * NPIX)
        assert torch.equal(v, ref_v[idx]), f"key 4 = {kernel}, value: " + _mismatch(v, ref_v[idx])
        assert torch.equal(p, ref_p[idx]), f"key 4 = {kernel}, policy: " + _mismatch(p, ref_p[idx])


@pytest.fixture(scope="module")
def dense_tower():
    yield from tower_gpu.dense_tower(S, 65 + 3)


@pytest.mark.parametrize("B", [1, 31, 32, 33, 65])
def test_dense_matches_fp64_to_1e5(dense_tower, B):
    """Logits and z are exact in fp32 whatever the summation order, so what is left is __expf, tanhf and one division:
    policy and value within 1e-5 of fp64, every row 225 entries summing to 1 within 1e-5, nothing written past the batch."""
    tower_gpu.check_dense_matches_fp64_to_1e5(dense_tower, B)


# ------------------------------------------------------------------ rounded regime ------------------------------------------------------------------
@pytest.mark.parametrize("B", [33, NROUND])
@pytest.mark.parametrize("iso", ISOLATIONS)
def test_block_convolutions_meet_the_rounding_bound(block_towers, iso, B):
    """Per element, one convolution at a time: the stored mid activation against ELU(conv1) and the block output against the
    second convolution of the mid activation that was stored, so each comparison crosses exactly one rounding to bf16."""
    import torch
    tw, h_dev, _ = block_towers("rounded", iso)
    case = gen.rounded_block_case(S, iso)
    got = {}
    for depth in DEPTHS:
        out, g = _run_block(tw, h_dev, B, depth, 0)
        got[depth] = (out.clone(), g.clone())
    for depth in DEPTHS[1:]:                         # the same MFMAs in the same order: the ring depth changes no bit
        assert torch.equal(got[depth][0], got[0][0]) and torch.equal(got[depth][1], got[0][1]), depth
    out, g = got[0]
    assert torch.isfinite(out.float()).all()
    g_ref, A1, out_ref, A2 = ref64.block(case["h"][:B], case["c1"], case["c2"], case["res"], mid=g.double().cpu().numpy())
    assert (g_ref < 0).any() and (out_ref < 0).any()                 # the ELU's negative side is exercised
    assert _worst_ratio(S, g, g_ref, A1, 1152, f"{iso} B={B} first convolution") <= 1.0
    assert _worst_ratio(S, out, out_ref, A2, 1280, f"{iso} B={B} second convolution + projection") <= 1.0


@pytest.mark.parametrize("B", [33, NROUND])
def test_stem_and_heads_meet_the_rounding_bound(B):
    import torch
    c = gen.rounded_ends_case(S)
    tw = _tower(S, {}, B + 3, stem=c["stem"], vconv=c["vconv"], pconv=c["pconv"])
    try:
        y, A = ref64.stem(c["planes"][:B], *c["stem"])
        _poison(tw, B)
        tw.stem(_t(c["planes"][:B]))
        _assert_untouched(tw, B)
        assert (y < 0).any()
        assert _worst_ratio(S, tw.store_nchw(B), y, A, 75, f"stem B={B}") <= 1.0
        vin, Av, pin, Ap = ref64.heads(c["h"][:B], c["vconv"], c["pconv"])
        _poison(tw, B)
        tw.load_nchw(_t(c["h"][:B], torch.bfloat16))
        v, p = tw.heads(B)
        _assert_untouched(tw, B)
        assert _worst_ratio(S, v, vin, Av, 128, f"heads value B={B}") <= 1.0
        assert _worst_ratio(S, p, pin, Ap, 128, f"heads policy B={B}") <= 1.0
    finally:
        tw.close()
