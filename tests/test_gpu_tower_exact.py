"""The bf16 tower kernels (csrc/af_tower_bf16.hip) on 11x11 boards against oracle/tower_fp64.py, one layer at a time.  The cases,
the exact and the rounded regime, the three isolations of a residual block and the error bound are those of tests/tower_cases.py;
tests/test_tower_reference_cpu.py checks, from the reference alone, that the exact-regime cases meet their conditions."""
import pytest

import tower_cases as gen
import tower_gpu
from oracle import tower_fp64 as ref64
from tower_cases import ISOLATIONS, NDIST
from tower_gpu import SENT16, _assert_untouched, _bits16, _mismatch, _poison, _run_block, _t, _tower, _Tune, _worst_ratio

pytestmark = pytest.mark.gpu
S = 11
NPIX, NROUND = gen.SIZES[S].NPIX, gen.SIZES[S].NROUND
# (engine = tune key 3, ring depth = tune key 0): af_tower_conv3 + af_tower_conv, af_tower_conv3 for both, af_tower_conv<*, depth>;
# engines 3 and 2 run at depth 8 whatever key 0 says: (3, 16) and (2, 12) pin that a depth is neither refused nor honoured there
ENGINES = ((3, 0), (2, 0), (0, 0), (0, 8), (0, 12), (0, 16), (3, 16), (2, 12))
# (batch, persistent workgroups = tune key 1).  Default grid min(batch, CUs): a multiple of 8 (XCD swizzle on) at 8 and 128 only.
# 121 positions on 3 / 8 / 16 workgroups: 41 / 16 / 8 iterations each, both LDS buffer parities, ragged last passes.
# 9 / 17 / 25 positions on 8 workgroups: workgroup 0 runs 2 / 3 / 4 positions, the others one fewer — af_tower_conv3's
# first-position form, its drain after the last position, and one steady-state position more.
CONFIGS = tuple((b, 0) for b in (1, 2, 8, 9, 121, 128)) + tuple((121, g) for g in (3, 8, 16)) + tuple((b, 8) for b in (9, 17, 25))


@pytest.fixture(scope="module")
def block_towers():
    yield from tower_gpu.block_towers(S)


@pytest.mark.parametrize("engine, depth", ENGINES)
@pytest.mark.parametrize("iso", ISOLATIONS)
def test_block_convolutions_are_exact(block_towers, iso, engine, depth):
    """Every (cout, cin, tap, pixel, position) of one convolution, on every kernel, batch and grid: bit equality with fp64."""
    tower_gpu.check_block_convolutions_are_exact(block_towers, iso, depth, CONFIGS, engine)


def test_tune_rejects_undocumented_values_and_keeps_the_setting(block_towers):
    """af_tower_tune: a rejected value leaves the previous setting in force — shown on key 2's "no stores" bit, whose
    effect is visible: af_tower_conv keeps storing nothing after the rejected call."""
    import torch
    from alphafive_amd import tower_hip
    tw, h_dev, (ref_out, _) = block_towers("exact", "conv1")
    B = 9
    try:
        tower_hip.tune(3, 0)
        tower_hip.tune(2, 2)
        for key, bad in ((0, 5), (0, 7), (0, 24), (0, -8), (1, -1), (2, 8), (2, -1), (3, 1), (4, 2), (4, -1), (5, 0), (-1, 0)):
            with pytest.raises(tower_hip.TowerError):
                tower_hip.tune(key, bad)
        tw.load_nchw(h_dev[:B])
        _bits16(tw.g[:B, :, S:S + NPIX]).fill_(SENT16)
        tw.forward(B)                                # the rejected tune(2, 8) did not clear the "no stores" bit ...
        torch.cuda.synchronize()
        assert bool((_bits16(tw.g[:B, :, S:S + NPIX]) == SENT16).all()) and torch.equal(tw.store_nchw(B), h_dev[:B])
    finally:
        for k, v in ((0, 0), (1, 0), (2, 0), (3, 3), (4, 1)):
            tower_hip.tune(k, v)
    tw.load_nchw(h_dev[:B])
    tw.forward(B)                                    # ... nor did any of them leave something else behind
    assert torch.equal(tw.store_nchw(B), ref_out[:B])


@pytest.fixture(scope="module")
def ends_tower():
    yield from tower_gpu.ends_tower(S, 2048 + 5 + 3)         # 2048 + 5 positions + room for the sentinels


@pytest.mark.parametrize("B", [1, 121, 1024 + 5])
def test_stem_is_exact(ends_tower, B):
    """All 75 taps at corners, edges and interior; 1024 + 5 wraps the stem's grid cap of 1024 (64 distinct positions, tiled)."""
    import torch
    tw, case = ends_tower, gen.exact_stem_case(S)
    y, _ = ref64.stem(case["planes"], case["w"], case["b"])
    ref = _t(ref64.bf16_round(y), torch.bfloat16)
    idx = torch.arange(B, device="cuda") % NDIST
    planes = _t(case["planes"])[idx].contiguous()
    _poison(tw, B)
    tw.stem(planes)
    _assert_untouched(tw, B)
    out = tw.store_nchw(B)
    n = min(B, NDIST)
    assert torch.equal(out[:n], ref[:n]), _mismatch(out[:n], ref[:n])
    assert torch.equal(out, out[idx]), "a repeat of a position differs from its first occurrence"


@pytest.mark.parametrize("B", [1, 121, 2048 + 5])
def test_heads_are_exact_on_both_kernels(ends_tower, B):
    """The heads' 1x1 convolutions on an integer tower output: MFMA kernel = VALU kernel = fp64; 2048 + 5 wraps the grid cap."""
    import torch
    tw, case = ends_tower, gen.exact_heads_case(S)
    vin, _, pin, _ = ref64.heads(case["h"], case["vconv"], case["pconv"])
    ref_v, ref_p = _t(ref64.bf16_round(vin), torch.bfloat16), _t(ref64.bf16_round(pin), torch.bfloat16)
    idx = torch.arange(B, device="cuda") % NDIST
    h = _t(case["h"], torch.bfloat16)[idx].contiguous()
    n = min(B, NDIST)
    for kernel in (1, 0):
        _poison(tw, B)
        tw.load_nchw(h)
        with _Tune(k4=kernel):
            v, p = tw.heads(B)
        _assert_untouched(tw, B)
        assert torch.equal(v[:n], ref_v[:n]), f"heads kernel {kernel}, value: " + _mismatch(v[:n], ref_v[:n])
        assert torch.equal(p[:n], ref_p[:n]), f"heads kernel {kernel}, policy: " + _mismatch(p[:n], ref_p[:n])
        assert torch.equal(v, v[idx]) and torch.equal(p, p[idx]), "a repeat of a position differs from its first occurrence"


@pytest.fixture(scope="module")
def dense_tower():
    yield from tower_gpu.dense_tower(S, 32768 + 5 + 3)       # 32768 + 5 positions reach the second trip of the kernel's loop over 32-position groups


@pytest.mark.parametrize("B", [1, 31, 32, 33, 65, 32768 + 5])
def test_dense_matches_fp64_to_1e5(dense_tower, B):
    """Logits and z are exact in fp32 whatever the summation order, so what is left is __expf, tanhf and one division:
    policy and value within 1e-5 of fp64 (the project's fp32 bar), rows summing to 1; vfc2's bias is not zero."""
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
    h = case["h"][:B]
    got = {}
    for engine, depth in ENGINES:
        out, g = _run_block(tw, h_dev, B, depth, 0, engine)
        got[(engine, depth)] = (out.clone(), g.clone())
    for depth in (8, 12, 16):                        # the same MFMAs in the same order: the ring depth changes no bit
        assert torch.equal(got[(0, depth)][0], got[(0, 0)][0]) and torch.equal(got[(0, depth)][1], got[(0, 0)][1]), depth
    assert torch.equal(got[(3, 0)][0], got[(0, 0)][0]) and torch.equal(got[(3, 0)][1], got[(0, 0)][1])    # engine 3 = engine 0
    assert torch.isfinite(got[(2, 0)][0].float()).all() and torch.isfinite(got[(3, 0)][0].float()).all()
    refs = {}
    for engine in (3, 2):                            # engine 0 equals engine 3 by bits
        out, g = got[(engine, 0)]
        key = g.cpu().view(torch.int16).numpy().tobytes()
        if key not in refs:
            refs[key] = ref64.block(h, case["c1"], case["c2"], case["res"], mid=g.double().cpu().numpy())
        g_ref, A1, out_ref, A2 = refs[key]
        assert (g_ref < 0).any() and (out_ref < 0).any()             # the ELU's negative side is exercised
        assert _worst_ratio(S, g, g_ref, A1, 1152, f"{iso} B={B} engine {engine} first convolution") <= 1.0
        assert _worst_ratio(S, out, out_ref, A2, 1280, f"{iso} B={B} engine {engine} second convolution + projection") <= 1.0


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
        for kernel in (1, 0):
            _poison(tw, B)
            tw.load_nchw(_t(c["h"][:B], torch.bfloat16))
            with _Tune(k4=kernel):
                v, p = tw.heads(B)
            _assert_untouched(tw, B)
            assert _worst_ratio(S, v, vin, Av, 128, f"heads kernel {kernel} value B={B}") <= 1.0
            assert _worst_ratio(S, p, pin, Ap, 128, f"heads kernel {kernel} policy B={B}") <= 1.0
    finally:
        tw.close()
