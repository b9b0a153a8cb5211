"""The int8 tower against the bf16 one (profiles/tower_int8.md).

    python tools/probe_tower_int8.py speed      # af_tower_forward_i8 against af_tower_forward, alternating in one process, + the quantiser alone
    python tools/probe_tower_int8.py quality    # bf16 hip path and int8 path against eval_device(dtype=float32) on 512 positions
    python tools/probe_tower_int8.py small      # profiles/tower_int8_small.md: af_tower_forward_i8_small against af_tower_forward_i8 inside the
                                                # whole evaluation (one graph per form, alternating replays), + the bf16 small form
    python tools/probe_tower_int8.py player     # Player moves/s: int8 and bf16 through Player's own evaluator, numpy wrappers, eval_device

Env: REPS (200 timed forwards per form and batch), BS ("8192,256"), BLOCKS (8), OUT (a file that gets the JSON as well); small:
REPLAYS (300), SMALL_BS ("1,2,4,8,16,32,64,128,256"); player: MOVES (16 timed moves per path and round), ROUNDS (2), SIMS ("500,642")."""
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
from alphafive_amd.network_deep import DeepResNet                      # noqa: E402

REPS = int(os.environ.get("REPS", 200))
BS = [int(b) for b in os.environ.get("BS", "8192,256").split(",")]
BLOCKS = int(os.environ.get("BLOCKS", 8))
S = 11


def _planes(n, seed):
    rng = np.random.default_rng(seed)
    x = np.zeros((n, 3, S, S), np.float32)
    stones = rng.integers(0, 3, size=(n, S, S))
    x[:, 0], x[:, 1] = stones == 1, stones == 2
    x[:, 2] = rng.integers(0, 2, size=(n, 1, 1))
    return torch.from_numpy(x).cuda()


def _stats(pairs):
    us = sorted(1e3 * a.elapsed_time(b) for a, b in pairs)
    return {"median_us": round(statistics.median(us), 1), "min_us": round(us[0], 1), "max_us": round(us[-1], 1),
            "p05_us": round(us[int(0.05 * len(us))], 1), "p95_us": round(us[int(0.95 * len(us))], 1), "n": len(us)}


def speed():
    net = DeepResNet(S, blocks=BLOCKS, width=128, device="cuda", seed=0)
    scales = net.calibrate_int8(_planes(256, 1))
    bf, i8 = net.evaluator(max(BS)), net.evaluator(max(BS), precision="int8", act_scales=scales)
    out = {"blocks": BLOCKS, "reps": REPS}
    for B in BS:
        x = _planes(B, 2)
        forms = {"bf16_forward": (bf.tower, lambda tw: tw.forward(B)), "int8_forward": (i8.tower, lambda tw: tw.forward_i8(B)),
                 "int8_quantise_only": (i8.tower, lambda tw: tw.quantize_i8(tw.x, tw.xq, B))}
        for tw, run in forms.values():                                 # warm-up: every shape the timed window uses
            for _ in range(5):
                tw.stem(x)
                run(tw)
        torch.cuda.synchronize()
        ev = {n: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(REPS)] for n in forms}
        for r in range(REPS):                                          # alternating; the stem refills the input outside the timed pair
            for name, (tw, run) in forms.items():
                tw.stem(x)
                e0, e1 = ev[name][r]
                e0.record()
                run(tw)
                e1.record()
        torch.cuda.synchronize()
        row = {name: _stats(ev[name]) for name in forms}
        row["int8_over_bf16_median"] = round(row["int8_forward"]["median_us"] / row["bf16_forward"]["median_us"], 4)
        out["B%d" % B] = row
    net.close()
    return out


def quality():
    net = DeepResNet(S, blocks=BLOCKS, width=128, device="cuda", seed=0)
    calib, x = _planes(512, 11), _planes(512, 12)
    scales = net.calibrate_int8(calib)
    p32, v32 = net.eval_device(x, dtype=torch.float32)
    out = {"blocks": BLOCKS, "positions": 512, "act_scales": [float(a) for a in scales]}
    for name, ev in (("bf16_hip", net.evaluator(512)), ("int8_hip", net.evaluator(512, precision="int8", act_scales=scales))):
        p, v = ev(x)
        dp, dv = (p - p32).abs(), (v - v32.float()).abs()
        out[name] = {"max_dp": float(dp.max()), "mean_dp": float(dp.mean()), "max_dv": float(dv.max()), "mean_dv": float(dv.mean()),
                     "top1_agreement": float((p.argmax(1) == p32.argmax(1)).float().mean())}
        ev.close()
    net.close()
    return out


def _graph_of(tw, x, form):
    """One whole evaluation — stem, (quantiser,) 2 * BLOCKS convolutions, heads, dense — as a captured graph."""
    B = x.shape[0]

    def run():
        tw.stem(x)
        getattr(tw, form)(B)
        tw.heads(B)
        tw.dense(B)
    for _ in range(3):
        run()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        run()
    return g


def small():
    """profiles/tower_small_batch.md's protocol for int8: per batch the forms alternate replay by replay in one process, each
    replay between its own pair of events, after 20 warm-up replays."""
    replays = int(os.environ.get("REPLAYS", 300))
    bs = [int(b) for b in os.environ.get("SMALL_BS", "1,2,4,8,16,32,64,128,256").split(",")]
    net = DeepResNet(S, blocks=BLOCKS, width=128, device="cuda", seed=1)
    scales = net.calibrate_int8(_planes(256, 1))
    bf, i8 = net.evaluator(max(bs)), net.evaluator(max(bs), precision="int8", act_scales=scales)
    out = {"blocks": BLOCKS, "replays": replays, "small_batch_i8_in_library": i8.tower.small_batch_i8}
    for B in bs:
        x = _planes(B, B)
        graphs = {"int8_persistent": (i8.tower, _graph_of(i8.tower, x, "forward_i8")), "int8_small": (i8.tower, _graph_of(i8.tower, x, "forward_i8_small")),
                  "bf16_small": (bf.tower, _graph_of(bf.tower, x, "forward_small"))}
        bits = {}
        for name, (tw, g) in graphs.items():
            for _ in range(20):
                g.replay()
            torch.cuda.synchronize()
            bits[name] = (tw.policy[:B].clone(), tw.value[:B].clone())
        same = all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(bits["int8_persistent"], bits["int8_small"]))
        ev = {n: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(replays)] for n in graphs}
        for r in range(replays):
            for name, (_, g) in graphs.items():
                e0, e1 = ev[name][r]
                e0.record()
                g.replay()
                e1.record()
        torch.cuda.synchronize()
        row = {"int8_forms_same_bits": same}
        for name in graphs:
            row[name] = _stats(ev[name])
        out["B%d" % B] = row
        del graphs
    net.close()
    return out


class _TorchOwner(object):
    """An owner Player sends to eval_device (backend "device")."""

    def __init__(self, net):
        self.device, self.eval_device = net.device, net.eval_device

    def eval(self, x):
        p, v = self.eval_device(torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(self.device))
        return p.float().cpu().numpy(), v.float().cpu().numpy()


def player():
    """profiles/tower_small_batch.md's Player protocol with the int8 paths added."""
    sys.path.insert(0, os.path.join(R, "tests"))
    from conftest import make_cfg
    from alphafive_amd import utils
    from alphafive_amd.player import Player
    sims, cap = (int(v) for v in os.environ.get("SIMS", "500,642").split(","))
    moves, rounds = int(os.environ.get("MOVES", 16)), int(os.environ.get("ROUNDS", 2))
    net = DeepResNet(S, blocks=BLOCKS, width=128, device="cuda", seed=1)
    scales = net.calibrate_int8(_planes(256, 1))
    i8 = net.evaluator(1, precision="int8", act_scales=scales)
    tw = i8.tower

    def wrapper(form):
        def f(x):
            tw.stem(torch.from_numpy(np.ascontiguousarray(x, np.float32)).cuda())
            getattr(tw, form)(1)
            tw.heads(1)
            p, v = tw.dense(1)
            return p.cpu().numpy().copy(), v.cpu().numpy().copy()
        return f
    paths = {"int8_evaluator_eval_hip_graph": i8.eval, "deep_eval_bf16_hip_graph": net.eval,
             "numpy_wrapper_int8_persistent_kernels": wrapper("forward_i8"), "numpy_wrapper_int8_small_kernels": wrapper("forward_i8_small"),
             "eval_device_torch": _TorchOwner(net).eval}
    cfg = make_cfg(board_size=S, simulation_per_step=sims, upper_simulation_per_step=cap)
    out = {"sims": [sims, cap], "blocks": BLOCKS, "small_batch_i8_in_library": tw.small_batch_i8}
    for rnd in range(rounds):
        for name, fn in paths.items():
            pl = Player(cfg, training=True, pv_fn=fn, seed=7, game_id=3)
            state, last, over, n = pl.get_init_state(), None, False, 0
            t0 = None
            while not over and n < moves + 1:
                if n == 1:                           # the first move (graph capture, lazy allocations) is warm-up
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                _, act = pl.get_action(state, last_action=last)
                board = utils.step(utils.state_to_board(state, S), act)
                state, last, n = utils.board_to_state(board), act, n + 1
                over, _ = utils.is_game_over(board, cfg.goal)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            precision = getattr(getattr(pl._pv_device, "tower", None), "precision", None)
            out.setdefault(name, {"backend": pl.backend, "own_tower_precision": precision, "rounds": []})["rounds"].append(
                {"moves": n - 1, "seconds": round(dt, 3), "moves_per_s": round((n - 1) / dt, 2)})
            pl.close()
    net.close()
    return out


if __name__ == "__main__":
    what = sys.argv[1] if len(sys.argv) > 1 else "speed"
    res = {"speed": speed, "quality": quality, "small": small, "player": player}[what]()
    text = json.dumps(res, indent=1)
    print(text)
    if os.environ.get("OUT"):
        with open(os.environ["OUT"], "w") as f:
            f.write(text + "\n")
