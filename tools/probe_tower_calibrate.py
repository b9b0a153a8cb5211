"""What does giving the int8 tower new ACTIVATION scales cost?  8 blocks x 128, 256 calibration positions, one process:
  (a) device  HipTower.calibrate_i8(planes)                      — stem + af_tower_i8_calibrate: the bf16 layers with an absmax launch
              in front of each, the finalize kernel and the int8 re-pack from the handle's fp32 keep; launches only
  (b) host    DeepResNet.calibrate_int8(planes) + enable_i8(...) — the route before it: an fp32 PyTorch forward layer by layer
              ending in .cpu(), then af_tower_i8_enable (two device synchronisations, a host copy, one pack launch per block)
  (c) scale   the stem + af_tower_forward (bf16, persistent kernels) at the same batch
(a) and (c) between device events, (b) by the host clock between two device synchronisations; alternated over ROUNDS rounds
after warm-up, median and min..max of each.  Also the host-side enqueue time of (a).  Prints one JSON line.  Run it under a time
limit:
    timeout -k 10 300 python tools/probe_tower_calibrate.py      (env B: calibration positions, 256; ROUNDS: 9)"""
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from alphafive_amd.network_deep import DeepResNet                      # noqa: E402


def planes(n, seed=1):
    rng = np.random.default_rng(seed)
    x = np.zeros((n, 3, 11, 11), np.float32)
    stones = rng.integers(0, 3, size=(n, 11, 11))
    x[:, 0], x[:, 1] = stones == 1, stones == 2
    x[:, 2] = rng.integers(0, 2, size=(n, 1, 1))
    return torch.from_numpy(x).cuda()


def events(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3


def main():
    B, rounds = int(os.environ.get("B", 256)), int(os.environ.get("ROUNDS", 9))
    deep = DeepResNet(11, blocks=8, width=128, device="cuda", seed=1)
    x = planes(B)
    ev = deep.evaluator(B, precision="int8", act_scales=deep.calibrate_int8(x))
    tw = ev.tower

    def device():
        tw.calibrate_i8(x)

    def host():
        tw.enable_i8(deep.calibrate_int8(x))

    def forward():
        tw.stem(x)
        tw.forward(B)

    for _ in range(3):
        device(), host(), forward()
    torch.cuda.synchronize()
    dev_us, host_us, fwd_us = [], [], []
    for _ in range(rounds):
        dev_us.append(events(device))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        host()
        torch.cuda.synchronize()
        host_us.append((time.perf_counter() - t0) * 1e6)
        fwd_us.append(events(forward))
    device()
    status = tw.calibration_status()
    dev_scales, host_scales = tw.read_act_scales().astype(np.float64), deep.calibrate_int8(x).astype(np.float64)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(20):
        device()
    enq = (time.perf_counter() - t0) / 20 * 1e6
    torch.cuda.synchronize()
    spread = lambda v: dict(median=statistics.median(v), min=min(v), max=max(v))  # noqa: E731
    print(json.dumps(dict(B=B, blocks=8, rounds=rounds, status_and_count=status,
                          device_calibrate_us=spread(dev_us), host_calibrate_and_enable_us=spread(host_us), bf16_stem_forward_us=spread(fwd_us),
                          device_calibrate_host_enqueue_us=enq,
                          max_relative_difference_of_scales=float((np.abs(dev_scales - host_scales) / host_scales).max()))))
    deep.close()


if __name__ == "__main__":
    main()
