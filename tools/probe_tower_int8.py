"""The int8 tower against the bf16 one (profiles/tower_int8.md).

    python tools/probe_tower_int8.py speed      # af_tower_forward_i8 against af_tower_forward, alternating in one process, + the quantiser alone
    python tools/probe_tower_int8.py quality    # bf16 hip path and int8 path against eval_device(dtype=float32) on 512 positions

Env: REPS (200 timed forwards per form and batch), BS ("8192,256"), BLOCKS (8), OUT (a file that gets the JSON as well)."""
import json
import os
import statistics
import sys

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


if __name__ == "__main__":
    what = sys.argv[1] if len(sys.argv) > 1 else "speed"
    res = {"speed": speed, "quality": quality}[what]()
    text = json.dumps(res, indent=1)
    print(text)
    if os.environ.get("OUT"):
        with open(os.environ["OUT"], "w") as f:
            f.write(text + "\n")
