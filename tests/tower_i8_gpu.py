"""What the GPU tests of the int8 tower's two forms share: towers over the cases of tests/tower_i8_cases.py (used unchanged),
sentinels behind the batch, and one layer / one forward run on either form.  torch is imported inside the functions, so
importing this module costs nothing on a machine without a GPU."""
import numpy as np

import tower_i8_cases as gen
from alphafive_amd import tower_i8 as t8

W, S, NPIX = 128, 11, 121
MAXB = gen.NPOS + 8
SENT8, SENT16 = 0x55, 0x4B4B     # an int8 filler and a bf16 bit pattern (a finite 1.3e7) the kernels are told apart from


def tt(wb):
    import torch
    return (torch.from_numpy(np.asarray(wb[0], np.float32)), torch.from_numpy(np.asarray(wb[1], np.float32)))


def tower(blocks, scales, max_batch=MAXB, **kw):
    from alphafive_amd import tower_hip
    return tower_hip.HipTower([{k: tt(b[k]) for k in ("c1", "c2", "res")} for b in blocks], S, W, max_batch, "cuda:0",
                              precision="int8", act_scales=scales, **kw)


def case_towers():
    """Body of a module fixture: one two-block tower per layer case, made on first use."""
    made = {}

    def get(name):
        if name not in made:
            made[name] = tower(gen.case_blocks(name), gen.layer_case(name)["scales"])
        return made[name]
    yield get
    for tw in made.values():
        tw.close()


def run_layer(tw, name, bf16_out, B, small):
    """The case's layer on its first B positions, on the tile-parallel kernel (small) or the persistent one, the second
    convolution in place on the block input as the forwards run it -> (the output as numpy NCHW: int8, or bf16 values as fp32;
    clones of xq, gq and x as they were left), with the checks that nothing at or past B and no zero row was written and that the
    int8 form left the bf16 buffer alone."""
    import torch
    c = gen.layer_case(name)
    conv = tw.conv_i8_small if small else tw.conv_i8
    tw.xq.fill_(SENT8)
    tw.gq.fill_(SENT8)
    tw.x.view(torch.int16).fill_(SENT16)
    for buf in (tw.xq, tw.gq, tw.x):
        buf[:B, :, :S] = 0
        buf[:B, :, S + NPIX:] = 0
    tw.xq[:B].copy_(torch.from_numpy(t8.to_c16(c["hq"][:B])))
    if c["second"]:
        tw.gq[:B].copy_(torch.from_numpy(t8.to_c16(c["gq"][:B])))
        out = tw.x if bf16_out else tw.xq
        conv(0, True, tw.gq, tw.xq, out, B)
    else:
        out = tw.x if bf16_out else tw.gq
        conv(0, False, tw.xq, None, out, B)
    torch.cuda.synchronize()
    for nm, buf in (("xq", tw.xq), ("gq", tw.gq)):
        assert bool((buf[B:] == SENT8).all()), f"{nm}: a position at or past batch {B} was written"
        assert not bool(buf[:B, :, :S].any()) and not bool(buf[:B, :, S + NPIX:].any()), f"{nm}: a zero row was written"
    xb = tw.x.view(torch.int16)
    assert bool((xb[B:] == SENT16).all()), f"x: a position at or past batch {B} was written"
    assert not bool(xb[:B, :, :S].any()) and not bool(xb[:B, :, S + NPIX:].any()), "x: a zero row was written"
    left = (tw.xq.clone(), tw.gq.clone(), xb.clone())
    if not bf16_out:
        assert bool((xb[:B, :, S:S + NPIX] == SENT16).all()), "the int8 form wrote the bf16 buffer"
        return t8.from_c16(out[:B].cpu().numpy()), left
    return tw.store_nchw(B).float().cpu().numpy(), left


def run_forward(tw, x, B, small):
    """Stem output x (bf16 NCHW on the device) -> clones of x, xq and gq after the blocks, on either form, from buffers that hold
    sentinels at and past B."""
    import torch
    tw.xq.fill_(SENT8)
    tw.gq.fill_(SENT8)
    tw.x.view(torch.int16).fill_(SENT16)
    for buf in (tw.xq, tw.gq, tw.x):
        buf[:B, :, :S] = 0
        buf[:B, :, S + NPIX:] = 0
    tw.load_nchw(x[:B])
    (tw.forward_i8_small if small else tw.forward_i8)(B)
    torch.cuda.synchronize()
    xb = tw.x.view(torch.int16)
    assert bool((tw.xq[B:] == SENT8).all()) and bool((tw.gq[B:] == SENT8).all()) and bool((xb[B:] == SENT16).all()), \
        f"a position at or past batch {B} was written"
    for buf in (tw.xq, tw.gq, xb):
        assert not bool(buf[:B, :, :S].any()) and not bool(buf[:B, :, S + NPIX:].any()), "a zero row was written"
    return xb.clone(), tw.xq.clone(), tw.gq.clone()


def deep_net(blocks=2, seed=0):
    from alphafive_amd.network_deep import DeepResNet
    return DeepResNet(11, blocks=blocks, seed=seed)
