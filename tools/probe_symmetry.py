"""Measurements behind profiles/symmetric_eval.md, one process per call, the forms alternating inside it:

    python tools/probe_symmetry.py legs        Player moves/s plain against mean (ResNet, DeepResNet bf16 and int8; 11x11, 500 / 642
                                               simulations), SelfPlayEngine ms per tick plain / random / mean at 4096 games (HIP
                                               events around 16-tick graph replays), the four kernels alone at 4096 rows
    python tools/probe_symmetry.py breakdown   one leaf, captured graphs of 200 dependent evaluations, us each: the forward at 1 row,
                                               at 8 rows, and expand + forward at 8 rows + reduce

Prints one JSON document at the end."""
import json
import os
import sys
import time
import types

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from alphafive_amd import symmetry, utils                      # noqa: E402
from alphafive_amd.engine import SelfPlayEngine                # noqa: E402
from alphafive_amd.network import ResNet                       # noqa: E402
from alphafive_amd.network_deep import DeepResNet              # noqa: E402
from alphafive_amd.player import Player                        # noqa: E402
from alphafive_amd.sym_hip import HipSym                       # noqa: E402

W = os.path.join(REPO, "tests", "golden", "alphaFive-6960.weights.npz")
S, N = 11, 200
cfg = types.SimpleNamespace(board_size=S, goal=5, simulation_per_step=500, upper_simulation_per_step=642, init_temp=1.2, gamma=0.94,
                            tau_decay_rate=0.94, tau_decay_rate_r=0.9, dirichlet_alpha=0.3, c_puct=5.0)


def legs():
    res = {}

    def play(pl, moves):
        pl.reset()
        state, last = pl.get_init_state(), None
        t0 = time.perf_counter()
        for _ in range(moves):
            _, a = pl.get_action(state, last_action=last)          # ends in a device synchronisation (move_result)
            state, last = utils.board_to_state(utils.step(utils.state_to_board(state, S), a)), a
        return time.perf_counter() - t0

    def player_leg(name, plain_fn, sym):
        forms = {"plain": Player(cfg, pv_fn=plain_fn, seed=11, game_id=0), "mean": Player(cfg, pv_fn=sym.eval, seed=11, game_id=0)}
        assert all(p.backend == "hip" for p in forms.values())
        moves, rounds = 5, 5
        for p in forms.values():
            play(p, 2)                                              # warm-up: weight pack, capture
        rates = {k: [] for k in forms}
        for _ in range(rounds):
            for k, p in forms.items():
                rates[k].append(moves / play(p, moves))
        for p in forms.values():
            p.close()
        res["player_" + name] = {k: dict(moves_per_s=[round(x, 2) for x in v], median=round(float(np.median(v)), 2)) for k, v in rates.items()}
        res["player_" + name]["mean_over_plain"] = round(float(np.median(rates["mean"]) / np.median(rates["plain"])), 3)
        print(name, res["player_" + name], flush=True)

    net = ResNet(S, device="cuda")
    net.load_npz(W)
    sym = symmetry.for_net(net, 1, mode="mean")
    player_leg("resnet", net.eval, sym)
    sym.close()

    deep = DeepResNet(S, blocks=8, width=128, device="cuda")
    sym = symmetry.for_net(deep, 1, mode="mean")
    player_leg("deep_bf16", deep.eval, sym)
    sym.close()
    rng = np.random.RandomState(0)
    cal = (rng.rand(64, 3, S, S) < 0.15).astype(np.float32)
    kw = dict(precision="int8", act_scales=deep.calibrate_int8(cal))
    ev = deep.evaluator(1, **kw)
    sym = symmetry.for_net(deep, 1, mode="mean", **kw)
    player_leg("deep_int8", ev.eval, sym)
    sym.close()
    ev.close()
    deep.close()

    # ---- SelfPlayEngine, 4096 games: ms per tick inside the 16-tick graph, HIP events around each replay ----
    G, n = 4096, 16
    engines = {"plain": SelfPlayEngine(cfg, G, net.select_backend("hip"), device=0, seed=3),
               "random": SelfPlayEngine(cfg, G, symmetry.for_net(net, G, mode="random", seed=1), device=0, seed=3),
               "mean": SelfPlayEngine(cfg, G, symmetry.for_net(net, G, mode="mean"), device=0, seed=3)}
    for sp in engines.values():
        for _ in range(3):
            sp.run_ticks_graph(n)
    torch.cuda.synchronize()
    for _ in range(4):
        for sp in engines.values():
            for _ in range(4):
                sp.run_ticks_graph(n, timed=True)
    torch.cuda.synchronize()
    res["engine_4096"] = {}
    for k, sp in engines.items():
        ms = [e0.elapsed_time(e1) / t for t, e0, e1 in sp.replay_events]
        res["engine_4096"][k] = dict(ms_per_tick_median=round(float(np.median(ms)), 4), min=round(min(ms), 4), max=round(max(ms), 4), replays=len(ms))
        sp.check()
        sp.close()
    print(res["engine_4096"], flush=True)

    # ---- the four kernels alone at 4096 rows (HIP events around 200 launches each) ----
    h = HipSym(S, G, "cuda:0", 5)
    f32 = dict(dtype=torch.float32, device="cuda")
    x, x8, xt = torch.rand((G, 3, S, S), **f32), torch.empty((8 * G, 3, S, S), **f32), torch.empty((G, 3, S, S), **f32)
    p8, v8 = torch.rand((8 * G, S * S), **f32), torch.rand((8 * G,), **f32)
    p, v = torch.empty((G, S * S), **f32), torch.empty((G,), **f32)
    calls = {"expand": lambda: h.expand(x, x8, G), "reduce": lambda: h.reduce(p8, v8, p, v, G), "apply": lambda: h.apply(x, xt, G),
             "restore": lambda: h.restore(p8, v8, p, v, G)}
    res["kernels_4096_us"] = {}
    for k, fn in calls.items():
        for _ in range(20):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(200):
            fn()
        e1.record()
        torch.cuda.synchronize()
        res["kernels_4096_us"][k] = round(e0.elapsed_time(e1) * 1000 / 200, 2)
    print(res["kernels_4096_us"], flush=True)
    return res


def breakdown():
    res = {}

    def graph_of(fn):
        fn()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, capture_error_mode="thread_local"):
            for _ in range(N):
                fn()
        return g

    def leg(name, ev1, ev8, sym):
        x1 = (torch.rand((1, 3, S, S), device="cuda") < 0.2).float()
        x8 = (torch.rand((8, 3, S, S), device="cuda") < 0.2).float()
        graphs = {"forward_1_row": graph_of(lambda: ev1(x1)), "forward_8_rows": graph_of(lambda: ev8(x8)),
                  "expand_forward8_reduce": graph_of(lambda: sym(x1))}
        out = {k: [] for k in graphs}
        for g in graphs.values():
            g.replay()
        torch.cuda.synchronize()
        for _ in range(7):
            for k, g in graphs.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                g.replay()
                e1.record()
                torch.cuda.synchronize()
                out[k].append(e0.elapsed_time(e1) * 1000 / N)
        res[name] = {k: round(float(np.median(v)), 2) for k, v in out.items()}
        print(name, res[name], flush=True)

    net = ResNet(S, device="cuda")
    net.load_npz(W)
    sym = symmetry.for_net(net, 1, mode="mean")
    leg("resnet", net.select_backend("hip"), net.select_backend("hip"), sym)
    deep = DeepResNet(S, blocks=8, width=128, device="cuda")
    sym = symmetry.for_net(deep, 1, mode="mean")
    leg("deep_bf16", deep.evaluator(1), deep.evaluator(8), sym)
    cal = (np.random.RandomState(0).rand(64, 3, S, S) < 0.15).astype(np.float32)
    kw = dict(precision="int8", act_scales=deep.calibrate_int8(cal))
    sym = symmetry.for_net(deep, 1, mode="mean", **kw)
    leg("deep_int8", deep.evaluator(1, **kw), deep.evaluator(8, **kw), sym)
    return res


if __name__ == "__main__":
    what = {"legs": legs, "breakdown": breakdown}.get(sys.argv[1] if len(sys.argv) > 1 else "")
    if what is None:
        sys.exit(__doc__)
    print(json.dumps(what(), indent=1))
