"""What does handing the trainer's weights to the self-play evaluator cost?  11x11, an evaluator sized for 4096 positions, the
alphaFive-6960 weights in a live Trainer.  One hand-off = the update + the first forward of 4096 positions with the new weights,
ended by a device synchronise (host clock around it).  Two paths, alternated in one process after both have been warmed:
  (a) host    net.set_variables(trainer.variables())                       — 42 copies to the host, host re-pack, af_net_finalize
  (b) device  net.set_variables_device(trainer.device_variables())         — device snapshot, af_net_update_device in place
Between hand-offs the trainer takes one optimiser step (outside the timed window), so every hand-off carries new weights.
Prints one JSON line with medians and interquartile ranges in ms.  Env: REPEATS (20, at least 20 of each), B (4096).

`probe_weight_handoff.py host_load`: HipNet.load(variables) alone on one handle of that size — one warm-up load, then five, each between
two device synchronisations (host clock) — as one JSON line.  AF_NET_LIB selects the library, so a parent build and a change run
back to back in separate processes."""
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from alphafive_amd.network import ResNet                               # noqa: E402
from alphafive_amd.train import Trainer                                # noqa: E402

S = 11
B, REPEATS = int(os.environ.get("B", 4096)), max(20, int(os.environ.get("REPEATS", 20)))
dev = torch.device("cuda", 0)


def host_load():
    from alphafive_amd import net_hip
    with np.load(os.path.join(REPO, "tests", "golden", "alphaFive-6960.weights.npz")) as z:
        sets = [{k: np.ascontiguousarray(z[k], np.float32) for k in z.files}]
    sets.append({k: (a * np.float32(0.5)) for k, a in sets[0].items()})        # every load carries other weights than the one before
    h = net_hip.HipNet(sets[0], S, B, dev)
    ms = []
    for i in range(6):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        h.load(sets[(i + 1) % 2])
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    h.close()
    print(json.dumps({"probe": "host_load", "library": os.path.basename(os.path.dirname(net_hip._LIBPATH)) + "/" + os.path.basename(net_hip._LIBPATH),
                      "board": S, "max_batch": B, "warmup_ms": ms[0], "samples_ms": ms[1:], "median_ms": float(np.median(ms[1:]))}))


if sys.argv[1:] == ["host_load"]:
    host_load()
    sys.exit(0)

net = ResNet(S, device=dev)
net.load_npz(os.path.join(REPO, "tests", "golden", "alphaFive-6960.weights.npz"))
trainer = Trainer(net.variables, S, device=dev)
pv = net.select_backend("hip")
g = torch.Generator(device="cpu").manual_seed(0)
planes = (torch.rand((B, 3, S, S), generator=g) < 0.1).float().to(dev)
TB = 512
boards = (torch.rand((TB, 3, S, S), generator=g) < 0.1).float().to(dev)
pol = torch.softmax(torch.randn((TB, S * S), generator=g), dim=1).to(dev)
val = (torch.randint(0, 2, (TB,), generator=g).float() * 2 - 1).to(dev)
wts = torch.ones(TB).to(dev)


def hand_off(on_device):
    trainer.step(boards, wts, val, pol, 1e-4, metrics=False)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    if on_device:
        net.set_variables_device(trainer.device_variables())
    else:
        net.set_variables(trainer.variables())
    _, v = pv(planes)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    return dt * 1e3, float(v[0])


pv(planes)                      # builds the evaluator at its full size
for _ in range(3):              # warm both paths
    hand_off(False)
    hand_off(True)
times = {False: [], True: []}
for _ in range(REPEATS):
    for on_device in (False, True):
        ms, _ = hand_off(on_device)
        times[on_device].append(ms)
torch.cuda.synchronize()
t0 = time.perf_counter()
for _ in range(10):
    pv(planes)
torch.cuda.synchronize()
fwd_ms = (time.perf_counter() - t0) / 10 * 1e3


def stats(a):
    q1, med, q3 = np.percentile(np.asarray(a), [25, 50, 75])
    return {"median_ms": float(med), "iqr_ms": float(q3 - q1), "min_ms": float(min(a)), "max_ms": float(max(a)), "n": len(a)}


a, b = stats(times[False]), stats(times[True])
print(json.dumps({"board": S, "max_batch": B, "repeats_each": REPEATS, "host_path": a, "device_path": b,
                  "forward_alone_ms": fwd_ms, "host_over_device": a["median_ms"] / b["median_ms"],
                  "device_below_host_by_more_than_host_iqr": bool(a["median_ms"] - b["median_ms"] > a["iqr_ms"]),
                  "note": "one hand-off = weight update + first forward of max_batch positions, ended by a device synchronise; "
                          "one optimiser step between hand-offs, outside the timed window"}))
net.close()
