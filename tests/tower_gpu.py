"""What the GPU tests of the bf16 tower share at both board sizes: towers over the cases of tests/tower_cases.py, sentinels behind
the batch, tune keys that are put back, and the comparisons.  torch is imported inside the functions, so importing this module
costs nothing on a machine without a GPU."""
import numpy as np

import tower_cases as gen
from oracle import tower_fp64 as ref64

W, NDIST = gen.W, gen.NDIST
SENT16 = 0x4B4B                  # bf16 bit pattern (a finite 1.3e7) no kernel here can produce
SENT32 = -777.25


def _t(a, dtype=None):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to("cuda", dtype or torch.float32)


def _null_block():
    import torch
    z3, z1, zb = torch.zeros(W, W, 3, 3), torch.zeros(W, W, 1, 1), torch.zeros(W)
    return dict(c1=(z3, zb), c2=(z3, zb), res=(z1, zb))


def _tower(S, case, max_batch, **kw):
    import torch
    from alphafive_amd import tower_hip
    tt = lambda wb: (torch.from_numpy(np.asarray(wb[0], np.float32)), torch.from_numpy(np.asarray(wb[1], np.float32)))  # noqa: E731
    blocks = [dict(c1=tt(case["c1"]), c2=tt(case["c2"]), res=tt(case["res"]))] if "c1" in case else [_null_block()]
    for k in ("stem", "vconv", "pconv"):
        if k in kw:
            kw[k] = tt(kw[k])
    if "dense" in kw:
        kw["dense"] = tuple(torch.from_numpy(np.asarray(a, np.float32)) for a in kw["dense"])
    return tower_hip.HipTower(blocks, S, W, max_batch, "cuda:0", **kw)


def _bits16(t):
    import torch
    return t.view(torch.int16)                       # same element size: a view of the very memory, whatever the strides


def _poison(tw, B):
    """Positions at or past B of every buffer a kernel writes hold a sentinel; the zero rows of the positions below B are zero."""
    S, NPIX = tw.S, tw.S * tw.S
    for buf in (tw.x, tw.g, tw.vin, tw.pin):
        _bits16(buf[B:]).fill_(SENT16)
    for buf in (tw.x, tw.g):                         # (the zero rows of a position an earlier, smaller batch had poisoned)
        buf[:B, :, :S] = 0
        buf[:B, :, S + NPIX:] = 0
    tw.policy[B:].fill_(SENT32)
    tw.value[B:].fill_(SENT32)


def _assert_untouched(tw, B):
    """... and still do, bit for bit; the two zero rows (and the pad unit behind them) of the positions below B are still zero."""
    import torch
    S, NPIX = tw.S, tw.S * tw.S
    torch.cuda.synchronize()
    for name in ("x", "g", "vin", "pin"):
        assert bool((_bits16(getattr(tw, name)[B:]) == SENT16).all()), f"{name}: a position at or past batch {B} was written"
    for name in ("policy", "value"):
        assert bool((getattr(tw, name)[B:] == SENT32).all()), f"{name}: a position at or past batch {B} was written"
    for name in ("x", "g"):
        buf = getattr(tw, name)[:B]
        assert not bool(_bits16(buf[:, :, :S]).any()) and not bool(_bits16(buf[:, :, S + NPIX:]).any()), f"{name}: a zero row was written"


class _Tune(object):
    """Tune keys set for one run; every key is put back to its default whatever happens."""

    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        from alphafive_amd import tower_hip
        try:
            for k, v in self.kv.items():
                tower_hip.tune(int(k[1:]), v)
        except Exception:
            self.__exit__()
            raise

    def __exit__(self, *exc):
        from alphafive_amd import tower_hip
        for k, v in ((0, 0), (1, 0), (2, 0), (3, 3), (4, 1)):
            tower_hip.tune(k, v)


def _run_block(tw, h_dev, B, depth, grid, engine=3):
    """One forward of a single-block tower under (ring depth = tune key 0, workgroups = key 1, engine = key 3) -> (block output,
    mid activation), both NCHW."""
    _poison(tw, B)
    tw.load_nchw(h_dev[:B])
    with _Tune(k3=engine, k0=depth, k1=grid):
        tw.forward(B)
    _assert_untouched(tw, B)
    return tw.store_nchw(B), tw.scratch_nchw(B)


def _mismatch(out, ref):
    """Where two NCHW activations (or two [position, feature] head outputs, which have no board rows to name) differ."""
    bad = (out != ref).nonzero()
    return "%d of %d elements differ; first at (position, channel, y, x) = %s: got %s, expected %s; rows hit: %s" % (
        bad.shape[0], out.numel(), bad[0].tolist(), out[tuple(bad[0])].item(), ref[tuple(bad[0])].item(),
        sorted(set(bad[:, 2].tolist())) if out.dim() == 4 else "-") if bad.shape[0] else "equal"


def _worst_ratio(S, out, ref, A, n, what):
    """max over elements of |out - ref| / bound, printed (the headroom of the derived bound) and returned."""
    err = np.abs(out.double().cpu().numpy() - ref)
    ratio = float((err / gen.error_bound(ref, A, n)).max())
    print("rounded regime %dx%d, %s: worst |error| / bound = %.3f (max |error| %.3g)" % (S, S, what, ratio, err.max()))
    return ratio


# ------------------------------------------------------------------ bodies of the module fixtures ------------------------------------------------------------------
def block_towers(S):
    """One single-block tower per isolation and regime, with its input on the device and — exact regime — the reference."""
    import torch
    made = {}

    def get(regime, iso):
        if (regime, iso) not in made:
            case = gen.exact_block_case(S, iso) if regime == "exact" else gen.rounded_block_case(S, iso)
            n = case["h"].shape[0]
            tw = _tower(S, case, n + 8)
            ref = None
            if regime == "exact":
                g, _, out, _ = gen.exact_block_reference(S, iso)
                ref = (_t(ref64.bf16_round(out), torch.bfloat16), _t(ref64.bf16_round(g), torch.bfloat16))
            made[(regime, iso)] = (tw, _t(case["h"], torch.bfloat16), ref)
        return made[(regime, iso)]
    yield get
    for tw, _, _ in made.values():
        tw.close()


def ends_tower(S, max_batch):
    """Stem + heads of the exact regime on one tower (null block)."""
    st, hd = gen.exact_stem_case(S), gen.exact_heads_case(S)
    tw = _tower(S, {}, max_batch, stem=(st["w"], st["b"]), vconv=hd["vconv"], pconv=hd["pconv"])
    yield tw
    tw.close()


def dense_tower(S, max_batch):
    """The one tower of the dense tests."""
    c = gen.exact_dense_case(S)
    tw = _tower(S, {}, max_batch, dense=(c["vfc1"][0], c["vfc1"][1], c["vfc2"][0], c["vfc2"][1], c["pfc"][0], c["pfc"][1]))
    yield tw
    tw.close()


# ------------------------------------------------------------------ test bodies that are the same at both sizes ------------------------------------------------------------------
def check_block_convolutions_are_exact(towers, iso, depth, configs, engine=3):
    """The single-block tower of `iso` at every (batch, grid) of `configs`: mid activation and block output bit-equal to fp64."""
    import torch
    tw, h_dev, (ref_out, ref_g) = towers("exact", iso)
    for B, grid in configs:
        out, g = _run_block(tw, h_dev, B, depth, grid, engine)
        assert torch.equal(g, ref_g[:B]), f"mid activation, batch {B}, grid {grid}: " + _mismatch(g, ref_g[:B])
        assert torch.equal(out, ref_out[:B]), f"block output, batch {B}, grid {grid}: " + _mismatch(out, ref_out[:B])


def check_dense_matches_fp64_to_1e5(tw, B):
    """The dense layers on the first B positions of the exact case, tiled: policy and value within 1e-5 of fp64, every row NPIX
    entries summing to 1 within 1e-5, nothing written past the batch, a repeat equal to its first occurrence."""
    import torch
    S = tw.S
    c = gen.exact_dense_case(S)
    policy, value, _, _ = ref64.dense(c["vin"], c["pin"], c["vfc1"], c["vfc2"], c["pfc"])
    idx = torch.arange(B, device="cuda") % NDIST
    _poison(tw, B)
    tw.vin[:B] = _t(c["vin"], torch.bfloat16)[idx]
    tw.pin[:B] = _t(c["pin"], torch.bfloat16)[idx]
    p, v = tw.dense(B)
    _assert_untouched(tw, B)
    assert p.shape == (B, S * S)
    n = min(B, NDIST)
    ep = np.abs(p[:n].double().cpu().numpy() - policy[:n]).max()
    ev = np.abs(v[:n].double().cpu().numpy() - value[:n]).max()
    es = float((p.double().sum(1) - 1).abs().max())
    print("dense %dx%d B=%d: max |policy - fp64| %.3g, |value - fp64| %.3g, |row sum - 1| %.3g" % (S, S, B, ep, ev, es))
    assert ep <= 1e-5 and ev <= 1e-5 and es <= 1e-5
    assert torch.equal(p, p[idx]) and torch.equal(v, v[idx]), "a repeat of a position differs from its first occurrence"


# ------------------------------------------------------------------ whole-net tests ------------------------------------------------------------------
def planes(n, seed=1, *, S):
    """Random-stone positions: [n, 3, S, S] of 0 / 1 (own stones, opponent's stones, side to move)."""
    import torch
    rng = np.random.default_rng(seed)
    x = np.zeros((n, 3, S, S), np.float32)
    stones = rng.integers(0, 3, size=(n, S, S))
    x[:, 0], x[:, 1] = stones == 1, stones == 2
    x[:, 2] = rng.integers(0, 2, size=(n, 1, 1))
    return torch.from_numpy(x).cuda()


def same_bits(a, b):
    import torch
    return all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))
