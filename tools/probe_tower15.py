"""The 8-block bf16 net on 15x15 boards: hand-written tower (select_backend("hip")) against the all-PyTorch path
(select_backend("torch")) on the same weights and positions, with the 11x11 net beside it (profiles/tower_15x15.md).

    python tools/probe_tower15.py [--batch 4096] [--rounds 12] [--reps 10] [--out FILE]
    python tools/probe_tower15.py --kernels     # a few forwards of each net and nothing else: the run to put under a kernel trace

The two paths are timed alternately in one process after a warm-up of both: `rounds` rounds of [hip x reps | torch x reps], each
bracketed by device events; the median round and the spread (min .. max) are reported.  The pieces of the hip path (stem, tower,
heads, dense) are timed the same way.  The share of the bf16 peak is af_tower_flops_per_position x batch / tower time over
2.5 PFLOP/s (dense bf16 MFMA): the tower's share, not the whole net's."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from alphafive_amd import tower_hip  # noqa: E402
from alphafive_amd.network_deep import DeepResNet  # noqa: E402

PEAK_BF16 = 2.5e15


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def stats(ms):
    return dict(median_ms=float(np.median(ms)), min_ms=float(np.min(ms)), max_ms=float(np.max(ms)))


def make(S, B, seed):
    net = DeepResNet(S, blocks=8, width=128, device="cuda", seed=seed)
    g = torch.Generator().manual_seed(5)
    for blk in net.tower:
        for k in ("res", "c1", "c2"):
            blk[k] = (blk[k][0], (torch.randn(128, generator=g) * 0.1).to("cuda", torch.bfloat16))
    x = (torch.rand((B, 3, S, S), device="cuda") < 0.2).float()
    return net, x, net.select_backend("hip", B), net.select_backend("torch", B)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--kernels", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    B, out = a.batch, {"batch": a.batch, "device": torch.cuda.get_device_name(0)}
    for S in (15, 11):
        net, x, hip, tor = make(S, B, seed=S)
        tw = net._tower
        if a.kernels:
            for _ in range(3):
                hip(x)
            torch.cuda.synchronize()
            tw.close()
            continue
        for _ in range(3):                                   # warm-up of every shape the timed windows use
            hip(x), tor(x)
        torch.cuda.synchronize()
        p_h, v_h = (t.clone() for t in hip(x))
        p_t, v_t = tor(x)
        r = {"max_abs_policy_diff": float((p_h - p_t.float()).abs().max()), "max_abs_value_diff": float((v_h - v_t.float()).abs().max())}
        ms_h, ms_t = [], []
        for _ in range(a.rounds):                            # alternating, so that both see the same machine
            ms_h.append(timed(lambda: hip(x), a.reps))
            ms_t.append(timed(lambda: tor(x), a.reps))
        r["hip"], r["torch"] = stats(ms_h), stats(ms_t)
        r["torch_over_hip"] = r["torch"]["median_ms"] / r["hip"]["median_ms"]
        pieces = (("stem", lambda: tw.stem(x)), ("tower", lambda: tw.forward(B)), ("heads", lambda: tw.heads(B)), ("dense", lambda: tw.dense(B)))
        for name, fn in pieces:
            fn()
        for name, fn in pieces:
            r[name] = stats([timed(fn, a.reps) for _ in range(a.rounds)])
        flops = tw.flops_per_position * B
        r["tower_flops"] = flops
        r["tower_share_of_bf16_peak"] = flops / (r["tower"]["median_ms"] * 1e-3) / PEAK_BF16
        r["conv_launch_us_mean"] = r["tower"]["median_ms"] * 1e3 / 16
        if S == 15:                                          # ring depths of tune key 0 (the default is 12 / 6)
            for depth in (8, 12, 16):
                tower_hip.tune(0, depth)
                tw.forward(B)
                r["tower_depth_%d" % depth] = stats([timed(lambda: tw.forward(B), a.reps) for _ in range(4)])
            tower_hip.tune(0, 0)
        out["S%d" % S] = r
        tw.close()
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
