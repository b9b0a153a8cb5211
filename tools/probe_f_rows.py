"""Timings of the callers of the hot path next to their host forms, one JSON line each:
  replay   utils.RandomStack.get_data(512) (host numpy, the reference's algorithm) vs DeviceRandomStack.get_data(512) (device ring)
  hand-off engine -> replay, device to device (af_replay_append_packed), episodes/s
  arena    alphafive_amd.arena.play_matches: N batched games of two weight sets, games/s and moves/s
  arena_device   the same match through play_matches (the yardstick), play_matches_device(graph=True) and (graph=False): the paths
           alternate, --reps times each after one warm-up match each; wall time around a final synchronise; the results of the
           three paths must be equal.  Prints one JSON line per match and a markdown table (profiles/arena_device_vs_host.md).
  replay_draws   minibatch sampling with host draws and with device draws at 2,000 and 12,000 positions: DeviceRandomStack.get_data(512)
           (the yardstick), get_data_device(512) and draw_batches(512, 4) per minibatch alternate in one process, max(--reps, 30)
           times each after warm-up; per call the wall time around a synchronise and the time until the call returns (host).  Then
           4 x (sample + Trainer.step(metrics=False)) at batch 512 with get_data and with one draw_batches(512, 4), alternating.
           Prints one JSON line per figure and the markdown tables of profiles/replay_device_draws.md.
Usage: probe_f_rows.py [rows ...] [--games N] [--reps R]      rows: replay hand-off arena arena_device replay_draws (default: all but replay_draws)"""
import contextlib
import io
import json
import os
import random
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
from alphafive_amd import utils                                       # noqa: E402
from alphafive_amd.replay import DeviceRandomStack                     # noqa: E402
from alphafive_amd.network import ResNet, random_variables             # noqa: E402
from alphafive_amd.engine import SelfPlayEngine                        # noqa: E402
from alphafive_amd import arena                                        # noqa: E402
from bench import make_cfg                                             # noqa: E402
from test_gpu_replay import _episodes                                  # noqa: E402

W = os.path.join(REPO, "tests", "golden", "alphaFive-6960.weights.npz")
ARGS = sys.argv[1:]
ROWS = [a for a in ARGS if not a.startswith("--") and not a.isdigit()] or ["replay", "hand-off", "arena", "arena_device"]
ARENA = any(r in ROWS for r in ("arena", "arena_device"))
GAMES = int(ARGS[ARGS.index("--games") + 1]) if "--games" in ARGS else 1024
REPS = int(ARGS[ARGS.index("--reps") + 1]) if "--reps" in ARGS else 3
net = ResNet(11, device="cuda")
net.load_npz(W)

if "replay" in ROWS:
    random.seed(1)
    np.random.seed(1)
    eps = _episodes(11, 120, seed=3)
    host, devs = utils.RandomStack(11, 2000), DeviceRandomStack(11, 2000, device=0)
    for rec, res in eps:
        host.push(rec, res)
        devs.push(rec, res)
    for name, st in (("host RandomStack (numpy)", host), ("DeviceRandomStack (HBM ring)", devs)):
        for _ in range(3):
            st.get_data(512)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(30):
            b = st.get_data(512)
        torch.cuda.synchronize()
        print(json.dumps({"row": "f1 get_data(512)", "impl": name, "ms": (time.perf_counter() - t0) / 30 * 1e3,
                          "positions_in_buffer": int(st._size()) if hasattr(st, "_size") else None}), flush=True)

if "replay_draws" in ROWS:
    from alphafive_amd.train import Trainer
    reps = max(REPS, 30)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        t1 = time.perf_counter()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, (t1 - t0) * 1e3, out

    def spread(t):
        return "%.3f | %.3f .. %.3f" % (float(np.median(t)), min(t), max(t))

    tables = []
    for length in (2000, 12000):
        random.seed(1)
        np.random.seed(1)
        st = DeviceRandomStack(11, length, device=0, draw_seed=1)
        with contextlib.redirect_stdout(io.StringIO()):      # push() reports its running averages
            while not st.is_full():
                for rec, res in _episodes(11, 40, seed=st._size() + 3):
                    st.push(rec, res)
        paths = (("get_data(512) (host draws)", lambda: st.get_data(512), 1),
                 ("get_data_device(512)", lambda: st.get_data_device(512), 1),
                 ("draw_batches(512, 4), per minibatch", lambda: st.draw_batches(512, 4), 4))
        wall, host = {n: [] for n, _, _ in paths}, {n: [] for n, _, _ in paths}
        for rep in range(reps + 3):                          # 3 warm-up rounds (allocator, selection buffer), not reported
            for name, fn, per in paths:
                w, h, _ = timed(fn)
                if rep >= 3:
                    wall[name].append(w / per)
                    host[name].append(h / per)
        base = float(np.median(wall[paths[0][0]]))
        for name, _, _ in paths:
            print(json.dumps({"row": "f1 minibatch sampling, host vs device draws", "impl": name, "positions_in_buffer": st._size(),
                              "reps": reps, "wall_ms_median": float(np.median(wall[name])), "wall_ms_min": min(wall[name]),
                              "wall_ms_max": max(wall[name]), "host_ms_median": float(np.median(host[name]))}), flush=True)
            tables.append("| %d | %s | %s | %s | %.2fx |" % (st._size(), name, spread(wall[name]), spread(host[name]),
                                                             base / float(np.median(wall[name]))))
        if length == 12000:
            tr = Trainer(net.variables, 11, device="cuda")

            def host_step():
                for _ in range(4):
                    tr.step(*st.get_data(512), 1e-3, metrics=False)

            def device_step():
                drawn = st.draw_batches(512, 4)
                for i in range(4):
                    tr.step(*(t[i] for t in drawn), 1e-3, metrics=False)
            steps = {"4 x (get_data + step)": [], "draw_batches(512, 4) + 4 x step": []}
            for rep in range(reps + 3):
                for name, fn in zip(steps, (host_step, device_step)):
                    w, _, _ = timed(fn)
                    if rep >= 3:
                        steps[name].append(w)
            for name, t in steps.items():
                print(json.dumps({"row": "f1 four minibatches + four Trainer.step(metrics=False), batch 512", "impl": name,
                                  "positions_in_buffer": st._size(), "reps": reps, "wall_ms_median": float(np.median(t)),
                                  "wall_ms_min": min(t), "wall_ms_max": max(t)}), flush=True)
            step_table = ["| %s | %s |" % (name, spread(t)) for name, t in steps.items()]
        st.close()
    print("| positions | path | wall ms (median) | wall ms (min .. max) | host ms (median) | host ms (min .. max) | vs get_data |")
    print("|---|---|---|---|---|---|---|")
    print("\n".join(tables))
    print("| 4 minibatches + 4 steps, 12000 positions | wall ms (median) | wall ms (min .. max) |")
    print("|---|---|---|")
    print("\n".join(step_table), flush=True)

if "hand-off" in ROWS:
    cfg = make_cfg(60, 80, 11)
    sp = SelfPlayEngine(cfg, 1024, net.select_backend("hip"), device=0, seed=0)
    st = DeviceRandomStack(11, 200000, device=0)
    pushed, t_push = 0, 0.0
    t0 = time.perf_counter()
    while pushed < 2000:
        sp.run_ticks(256)
        sp.check()
        t1 = time.perf_counter()
        for r in st.iter_push_packed(sp.post_episodes_device(256), 256, cfg.gamma):
            pushed += 1
        st.check()
        torch.cuda.synchronize()
        t_push += time.perf_counter() - t1
    print(json.dumps({"row": "f1 hand-off engine -> replay, device to device", "episodes": pushed, "hand_off_s": t_push,
                      "episodes_per_s_of_hand_off_time": pushed / t_push, "whole_loop_s": time.perf_counter() - t0}), flush=True)
    sp.close()

if ARENA:
    cfg = make_cfg(200, 260, 11)
    n2 = ResNet(11, device="cuda")
    n2.set_variables(random_variables(11, seed=2))
if "arena" in ROWS:
    for G in (64, 512):
        t0 = time.perf_counter()
        r = arena.play_matches(cfg, net.select_backend("hip"), n2.select_backend("hip"), G, device=0)
        dt = time.perf_counter() - t0
        print(json.dumps({"row": "f4 arena (choose_best_player.py:38-60), 200 sims/move", "games": G, "s": dt, "games_per_s": G / dt,
                          "moves_per_s": float(sum(r["lengths"])) / dt, "wins": r["wins"], "draws": r["draws"]}), flush=True)

if "arena_device" in ROWS:
    pv0, pv1 = net.select_backend("hip"), n2.select_backend("hip")
    paths = (("play_matches (host loop)", lambda: arena.play_matches(cfg, pv0, pv1, GAMES, device=0)),
             ("play_matches_device graph=True", lambda: arena.play_matches_device(cfg, pv0, pv1, GAMES, device=0, graph=True)),
             ("play_matches_device graph=False", lambda: arena.play_matches_device(cfg, pv0, pv1, GAMES, device=0, graph=False)))
    times, ref = {name: [] for name, _ in paths}, None
    for rep in range(REPS + 1):                              # rep 0 = warm-up (weight pack, allocator), not reported
        for name, fn in paths:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = fn()
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            if ref is None:
                ref = r
            assert r == ref, "the paths disagree: %s" % name
            if rep:
                times[name].append(dt)
            print(json.dumps({"row": "f4 arena, device loop vs host loop, 200 sims/move", "impl": name, "rep": rep, "games": GAMES, "s": dt,
                              "games_per_s": GAMES / dt, "moves_per_s": float(sum(r["lengths"])) / dt, "wins": r["wins"],
                              "draws": r["draws"]}), flush=True)
    moves = float(sum(ref["lengths"]))
    base = float(np.median(times[paths[0][0]]))
    print("| path | s (median) | s (min .. max) | games/s | moves/s | speed vs play_matches |")
    print("|---|---|---|---|---|---|")
    for name, _ in paths:
        t = times[name]
        med = float(np.median(t))
        print("| %s | %.2f | %.2f .. %.2f | %.1f | %.0f | %.2fx |" % (name, med, min(t), max(t), GAMES / med, moves / med, base / med), flush=True)
