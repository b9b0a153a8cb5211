"""How long does one optimiser step of alphafive_amd.train.Trainer take on the device, next to the rate at which the self-play
engine finishes episodes?  (main.py:62-70: four minibatches of config.batch_size = 512 per ACCEPTED episode.)
Measurement for SURVEY 8f rank 2 (a caller of the hot path); prints one JSON line.  Env: B (512), STEPS (60), SYNC (1: read the scalars every step).

MODE (env) selects what runs:
  (unset)  the eager Trainer, STEPS steps timed as one block: the original measurement.
  ab       an eager and a fused Trainer (Trainer(fused=True): libaf_train.so) built from the same weights in this process,
           alternating, metrics=False: STEPS timed steps each (wall time around one step and a device synchronise) after WARMUP (5)
           rounds; then the body of train_loop for one accepted episode without its draw — four steps back to back, one synchronise
           — again alternating, STEPS rounds each.  One JSON line per mode and measurement: median, min, max.
  eager | fused   that Trainer alone, for a profiler: WARMUP steps, a marker kernel (a cumsum, which no step launches), STEPS
           steps with metrics=False, the marker again.  Kernels between the markers / STEPS = kernels per step."""
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from alphafive_amd.train import Trainer                                # noqa: E402

B, STEPS = int(os.environ.get("B", 512)), int(os.environ.get("STEPS", 60))
MODE, WARMUP = os.environ.get("MODE", ""), int(os.environ.get("WARMUP", 5))
dev = torch.device("cuda", 0)
with np.load(os.path.join(REPO, "tests", "golden", "alphaFive-6960.weights.npz")) as z:
    var = {k: z[k] for k in z.files}
g = torch.Generator(device="cpu").manual_seed(0)
boards = (torch.rand((B, 3, 11, 11), generator=g) < 0.1).float().to(dev)
pol = torch.softmax(torch.randn((B, 121), generator=g), dim=1).to(dev)
val = (torch.randint(0, 2, (B,), generator=g).float() * 2 - 1).to(dev)
wts = torch.ones(B).to(dev)


def spread(name, what, ts):
    ts = np.asarray(ts) * 1e3
    return {"batch": B, "mode": name, "what": what, "n": len(ts), "ms_median": float(np.median(ts)), "ms_min": float(ts.min()),
            "ms_max": float(ts.max())}


def timed(tr, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        tr.step(boards, wts, val, pol, 1e-3, metrics=False)
    torch.cuda.synchronize()
    return time.perf_counter() - t0


if MODE == "ab":
    trainers = {"eager": Trainer(var, 11, device=dev), "fused": Trainer(var, 11, device=dev, fused=True)}
    for _ in range(WARMUP):
        for tr in trainers.values():
            tr.step(boards, wts, val, pol, 1e-3)
    for what, steps in (("one step, metrics=False", 1), ("four steps back to back, metrics=False", 4)):
        ts = {name: [] for name in trainers}
        for _ in range(STEPS):
            for name, tr in trainers.items():
                ts[name].append(timed(tr, steps))
        for name in trainers:
            print(json.dumps(spread(name, what, ts[name])), flush=True)
    for name, tr in trainers.items():
        print(json.dumps({"mode": name, "t": tr.t, **tr.step(boards, wts, val, pol, 1e-3)}), flush=True)
    sys.exit(0)

if MODE in ("eager", "fused"):
    tr = Trainer(var, 11, device=dev, fused=MODE == "fused")
    marker = torch.arange(7, device=dev, dtype=torch.float32)
    for _ in range(WARMUP):
        tr.step(boards, wts, val, pol, 1e-3)
    marker.cumsum(0)
    dt = timed(tr, STEPS)
    marker.cumsum(0)
    torch.cuda.synchronize()
    print(json.dumps({"batch": B, "mode": MODE, "steps": STEPS, "ms_per_step": dt / STEPS * 1e3}))
    sys.exit(0)

tr = Trainer(var, 11, device=dev)
for _ in range(5):
    tr.step(boards, wts, val, pol, 1e-3)
torch.cuda.synchronize()
t0 = time.perf_counter()
for _ in range(STEPS):
    m = tr.step(boards, wts, val, pol, 1e-3, metrics=os.environ.get("SYNC", "1") == "1")
torch.cuda.synchronize()
m = m or tr.step(boards, wts, val, pol, 1e-3)
dt = (time.perf_counter() - t0) / STEPS
flop = 3 * 118727264 * B                                               # forward + two backward passes of the same contraction
print(json.dumps({"batch": B, "sync_every_step": os.environ.get("SYNC", "1") == "1", "ms_per_step": dt * 1e3, "steps_per_s": 1 / dt, "positions_per_s": B / dt,
                  "algorithmic_tflops": flop / dt / 1e12, "loss_total": m["total"],
                  "note": "PyTorch-ROCm autograd (MIOpen fp32 convolutions) + TF-style Adam; one host sync per step for the logged scalars"}))
