"""The int8 small-batch surface where no GPU is needed: _HipEvaluator.eval exists, the branch Player takes for the eval of an
evaluator over a cpu net, and the three new prototypes of include/af_tower_bf16.h against the binding."""
import os
import re

import numpy as np

from conftest import make_cfg

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S = 11


def _net(seed=2):
    import torch
    from alphafive_amd.network_deep import DeepResNet
    return DeepResNet(S, blocks=2, width=128, device="cpu", dtype=torch.float32, seed=seed)


class _Tower(object):
    """Stands in for a HipTower: what Player's recognition and _HipEvaluator.eval look at."""
    precision, act_scales, max_batch, _h = "int8", np.ones(4, np.float32), 4, None

    def close(self):
        pass


def test_hip_evaluator_has_eval_with_deep_evals_contract():
    """numpy float32 [B,3,S,S] in, (prob, value) numpy out, copied: what the evaluator's __call__ returned, which here is stood in
    for (the kernels need a GPU; tests/test_gpu_tower_i8_small.py runs them)."""
    import torch
    from alphafive_amd.network_deep import _HipEvaluator
    net = _net()
    ev = _HipEvaluator(net, _Tower())
    assert callable(getattr(ev, "eval", None)) and ev.eval.__name__ == "eval" and ev.eval.__self__ is ev
    seen = []
    p0, v0 = torch.full((3, S * S), 1.0 / (S * S)), torch.tensor([0.25, -0.5, 0.0])

    def eval_hip(x, tower):
        seen.append((x.clone(), tower))
        return p0, v0
    net.eval_hip = eval_hip
    x = (np.random.default_rng(1).random((3, 3, S, S)) < 0.3).astype(np.float64)      # converted to float32 on the way in
    p, v = ev.eval(x)
    assert isinstance(p, np.ndarray) and isinstance(v, np.ndarray) and p.dtype == np.float32 and v.dtype == np.float32
    assert p.shape == (3, S * S) and v.shape == (3,)
    assert len(seen) == 1 and seen[0][1] is ev.tower and seen[0][0].dtype == torch.float32
    assert np.array_equal(seen[0][0].numpy(), x.astype(np.float32))
    assert np.array_equal(p, p0.numpy()) and np.array_equal(v, v0.numpy())
    p[:] = 0
    assert float(p0.min()) > 0                                                          # copied out


def test_player_over_an_evaluator_of_a_cpu_net_keeps_the_host_path(monkeypatch):
    """Player(pv_fn=ev.eval) with ev over a net that is not on a cuda device: evaluations cross the host boundary through pv_fn, no
    evaluator is taken from the net.  (Engine and device tensors stood in for, as in tests/test_deep_eval_cpu.py.)"""
    import torch
    from alphafive_amd import player
    from alphafive_amd.network_deep import _HipEvaluator

    class _Engine(object):
        def __init__(self, *a, **kw):
            pass

        def close(self):
            pass
    real_zeros = torch.zeros
    monkeypatch.setattr(player._eng, "Engine", _Engine)
    monkeypatch.setattr(torch, "zeros", lambda *a, **kw: real_zeros(*a, **{k: v for k, v in kw.items() if k != "device"}))
    net = _net()
    made = []
    monkeypatch.setattr(net, "evaluator", lambda *a, **kw: made.append((a, kw)) or None, raising=False)
    ev = _HipEvaluator(net, _Tower())
    pl = player.Player(make_cfg(), training=True, pv_fn=ev.eval, seed=1, game_id=0)
    assert pl.backend == "host" and pl._pv_device is None and pl._pv_owner is None and pl._pv_close is None and not made
    assert pl.pv_fn == ev.eval
    pl.close()


def _params(header, name):
    m = re.search(r"\b" + name + r"\s*\(([^)]*)\)\s*;", header)
    assert m, name
    return [a for a in m.group(1).split(",") if a.strip() and a.strip() != "void"]


def test_int8_small_prototypes_agree_with_the_binding():
    from alphafive_amd import tower_hip
    hdr = open(os.path.join(REPO, "include", "af_tower_bf16.h")).read()
    L = tower_hip.lib()
    assert len(_params(hdr, "af_tower_forward_i8_small")) == len(_params(hdr, "af_tower_forward_i8")) == 6
    assert len(L.af_tower_forward_i8_small.argtypes) == len(L.af_tower_forward_i8.argtypes) == 6
    assert len(_params(hdr, "af_tower_conv_i8_small")) == len(_params(hdr, "af_tower_conv_i8")) == 9
    assert len(L.af_tower_conv_i8_small.argtypes) == len(L.af_tower_conv_i8.argtypes) == 9
    assert len(_params(hdr, "af_tower_i8_small_batch")) == len(L.af_tower_i8_small_batch.argtypes) == 1
    assert re.search(r"\bint\s+af_tower_forward_i8_small\s*\(", hdr) and re.search(r"\bint32_t\s+af_tower_i8_small_batch\s*\(", hdr)
