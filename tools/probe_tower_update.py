"""What does giving the bf16 tower (BASELINE configs[4]: 8 blocks x 128, an evaluator sized for 8192 positions) a new weight set cost?
  (a) device  HipTower.load_device(tensors)       — af_tower_update_device: the pack kernels over fp32 device tensors, in place
  (b) host    DeepResNet.select_backend("hip", G) — the only way before load_device: a new handle (one allocation) through the host
              setters (tensors to the host, a synchronous copy into the handle's staging area and the same pack kernels, eleven
              times) and new activation buffers
Both in one process, alternated over five rounds after warm-up.  (a): device events around 20 back-to-back calls (per-call mean of the
window) and around 20 single calls; (b): host clock between two device synchronisations.  Also DeepResNet.set_variables_device (the
copies into the net's own tensors + load_device) and the host-side enqueue time of one load_device.  Prints one JSON line; the ratio
in it is median (b) over the median of (a)'s five window means.  Run it under a time limit:
    timeout -k 10 300 python tools/probe_tower_update.py        (env G: positions the evaluator is sized for, 8192)"""
import json
import os
import statistics
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from alphafive_amd.network_deep import DeepResNet                      # noqa: E402


def main():
    G = int(os.environ.get("G", 8192))
    deep = DeepResNet(11, blocks=8, width=128, device="cuda", seed=1)
    pv = deep.select_backend("hip", G)
    tw = deep._tower
    src = {k: torch.from_numpy(v).cuda() for k, v in deep.variables.items()}
    x = torch.zeros((G, 3, 11, 11), device="cuda")
    x[:, 2] = 1
    ref = tuple(t.clone() for t in pv(x))
    for _ in range(5):
        tw.load_device(src)
    torch.cuda.synchronize()
    got = tuple(t.clone() for t in pv(x))
    same = all(torch.equal(a, b) for a, b in zip(ref, got))
    win, single, host, setdev = [], [], [], []
    for r in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(20):
            tw.load_device(src)
        e1.record()
        e1.synchronize()
        win.append(e0.elapsed_time(e1) / 20 * 1e3)
        for _ in range(20):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            tw.load_device(src)
            b.record()
            b.synchronize()
            single.append(a.elapsed_time(b) * 1e3)
        # DeepResNet.set_variables_device: the copies into the net's own tensors + load_device
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        a.record()
        deep.set_variables_device(src)
        b.record()
        b.synchronize()
        setdev.append(((time.perf_counter() - t0) * 1e3, a.elapsed_time(b)))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        deep.select_backend("hip", G)
        torch.cuda.synchronize()
        host.append((time.perf_counter() - t0) * 1e3)
        tw.close()
        tw = deep._tower
        for _ in range(3):
            tw.load_device(src)
        torch.cuda.synchronize()
    # host enqueue cost of one call (no wait)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(20):
        tw.load_device(src)
    enq = (time.perf_counter() - t0) / 20 * 1e6
    torch.cuda.synchronize()
    res = dict(G=G, blocks=8, outputs_unchanged_by_update=same,
               load_device_us_per_call_windows_of_20=win, load_device_us_median_window=statistics.median(win),
               load_device_us_single_call_median=statistics.median(single), load_device_us_single_min_max=[min(single), max(single)],
               load_device_host_enqueue_us=enq,
               set_variables_device_ms_host_and_device=setdev,
               select_backend_ms=host, select_backend_ms_median=statistics.median(host))
    res["ratio_select_backend_over_load_device"] = res["select_backend_ms_median"] * 1e3 / res["load_device_us_median_window"]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
