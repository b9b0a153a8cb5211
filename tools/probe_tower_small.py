"""The bf16 tower at small batches (profiles/tower_small_batch.md): af_tower_forward_small against af_tower_forward inside the whole
evaluation, and Player moves/s on the three paths a deep net can be played through.

    python tools/probe_tower_small.py forward     # per board size and batch: median, min..max of REPLAYS graph replays per form
    python tools/probe_tower_small.py player      # Player(pv_fn=deep.eval) | numpy wrappers over select_backend("hip", 1) | eval_device
    python tools/probe_tower_small.py trace       # a few replays of both forms at B = 1, to run under rocprofv3 --kernel-trace --stats

Env: REPLAYS (300), BS ("1,2,4,8,16,32,64,128,256"), SIZES ("11,15"), BLOCKS (8), MOVES (16 timed moves per path and round; 0 = a
whole game), ROUNDS (2), SIMS ("500,642"), OUT (a file that gets the JSON as well)."""
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

REPLAYS = int(os.environ.get("REPLAYS", 300))
BS = [int(b) for b in os.environ.get("BS", "1,2,4,8,16,32,64,128,256").split(",")]
SIZES = [int(s) for s in os.environ.get("SIZES", "11,15").split(",")]
BLOCKS = int(os.environ.get("BLOCKS", 8))


def _planes(B, S, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand((B, 3, S, S), generator=g) < 0.2).float().cuda()


def _graph_of(tw, x, small):
    """One whole evaluation — stem, 2 * BLOCKS convolutions, heads, dense — as a captured graph."""
    B = x.shape[0]

    def run():
        tw.stem(x)
        (tw.forward_small if small else tw.forward)(B)
        tw.heads(B)
        tw.dense(B)
    for _ in range(3):
        run()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        run()
    return g


def forward():
    out = {}
    for S in SIZES:
        net = DeepResNet(S, blocks=BLOCKS, width=128, device="cuda", seed=1)
        ev = net.evaluator(max(BS))
        tw = ev.tower
        out["S%d_small_batch_in_library" % S] = tw.small_batch
        for B in BS:
            x = _planes(B, S, B)
            graphs = {"persistent": _graph_of(tw, x, False), "small": _graph_of(tw, x, True)}
            bits = {}
            for name, g in graphs.items():
                for _ in range(20):
                    g.replay()
                torch.cuda.synchronize()
                bits[name] = (tw.policy[:B].clone(), tw.value[:B].clone())
            same = all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(bits["persistent"], bits["small"]))
            ev_ = {n: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(REPLAYS)] for n in graphs}
            for r in range(REPLAYS):                 # alternating, each replay between its own pair of events
                for name, g in graphs.items():
                    e0, e1 = ev_[name][r]
                    e0.record()
                    g.replay()
                    e1.record()
            torch.cuda.synchronize()
            row = {"same_bits": same}
            for name in graphs:
                us = sorted(1e3 * a.elapsed_time(b) for a, b in ev_[name])
                row[name] = {"median_us": round(statistics.median(us), 2), "min_us": round(us[0], 2), "max_us": round(us[-1], 2),
                             "p95_us": round(us[int(0.95 * len(us))], 2)}
            out["S%d_B%d" % (S, B)] = row
            del graphs
        ev.close()
    return out


class _TorchOwner(object):
    """An owner Player sends to eval_device (backend "device"): the all-PyTorch bf16 path it picked for a deep net before."""

    def __init__(self, net):
        self.device, self.eval_device = net.device, net.eval_device

    def eval(self, x):
        p, v = self.eval_device(torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(self.device))
        return p.float().cpu().numpy(), v.float().cpu().numpy()


def player():
    sys.path.insert(0, os.path.join(R, "tests"))
    from conftest import make_cfg
    from alphafive_amd import utils
    from alphafive_amd.player import Player
    sims, cap = (int(v) for v in os.environ.get("SIMS", "500,642").split(","))
    moves, rounds = int(os.environ.get("MOVES", 16)), int(os.environ.get("ROUNDS", 2))
    S = 11
    net = DeepResNet(S, blocks=BLOCKS, width=128, device="cuda", seed=1)
    host_ev = net.select_backend("hip", 1)
    tw = net._tower

    def host_fn(x):                                  # the host-boundary path as it is now (eval_hip picks the tower's form) ...
        p, v = host_ev(torch.from_numpy(np.ascontiguousarray(x, np.float32)).cuda())
        return p.cpu().numpy().copy(), v.cpu().numpy().copy()

    def host_persistent_fn(x):                       # ... and on the persistent kernels: what there was for this job before
        tw.stem(torch.from_numpy(np.ascontiguousarray(x, np.float32)).cuda())
        tw.forward(1)
        tw.heads(1)
        p, v = tw.dense(1)
        return p.cpu().numpy().copy(), v.cpu().numpy().copy()
    paths = {"deep_eval_hip_graph": net.eval, "numpy_wrapper_persistent_kernels": host_persistent_fn,
             "numpy_wrapper_over_select_backend": host_fn, "eval_device_torch": _TorchOwner(net).eval}
    cfg = make_cfg(board_size=S, simulation_per_step=sims, upper_simulation_per_step=cap)
    out = {"sims": [sims, cap], "blocks": BLOCKS, "small_batch_in_library": net._tower.small_batch}
    for rnd in range(rounds):
        for name, fn in paths.items():
            pl = Player(cfg, training=True, pv_fn=fn, seed=7, game_id=3)
            state, last, over, n = pl.get_init_state(), None, False, 0
            t0 = None
            while not over and (moves == 0 or n < moves + 1):
                if n == 1:                           # the first move (graph capture, lazy allocations) is warm-up
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                _, act = pl.get_action(state, last_action=last)
                board = utils.step(utils.state_to_board(state, S), act)
                state, last, n = utils.board_to_state(board), act, n + 1
                over, _ = utils.is_game_over(board, cfg.goal)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            out.setdefault(name, {"backend": pl.backend, "rounds": []})["rounds"].append(
                {"moves": n - 1, "seconds": round(dt, 3), "moves_per_s": round((n - 1) / dt, 2)})
            pl.close()
    net.close()
    return out


def trace():
    for S in SIZES:
        net = DeepResNet(S, blocks=BLOCKS, width=128, device="cuda", seed=1)
        ev = net.evaluator(1)
        x = _planes(1, S, 1)
        for small in (False, True):
            g = _graph_of(ev.tower, x, small)
            for _ in range(50):
                g.replay()
            torch.cuda.synchronize()
        ev.close()
    return {"trace": "done"}


if __name__ == "__main__":
    what = sys.argv[1] if len(sys.argv) > 1 else "forward"
    res = {"forward": forward, "player": player, "trace": trace}[what]()
    text = json.dumps(res, indent=1)
    print(text)
    if os.environ.get("OUT"):
        with open(os.environ["OUT"], "w") as f:
            f.write(text + "\n")
