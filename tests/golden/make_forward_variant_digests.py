#!/usr/bin/env python
"""tests/golden/forward_variant_digests.json: the SHA-256 of the policy bytes and of the value bytes af_net_forward writes, for
every launch form the dispatch of the split-operand path can take — SHAPES x SETTINGS below.

The file was recorded on an MI355X with libaf_net built from commit 29a2629 ("libaf_net: pack weights in one place, the device
packers"), the last one whose launch code chose its form by bare integers in several places (launch_layer_g's switch, the two
_ok predicates, four ways to fill F16sArgs).  The single launch plan that replaced them is held to these bytes by
tests/test_gpu_net.py::test_forward_variants_match_the_recorded_digests.  Re-running the script on a later commit only shows
whether that commit still reproduces the file: a difference is a change of the arithmetic or of the dispatch, to be made on
purpose and explained, never a reason to overwrite the file quietly.

Shapes: the smallest batches on each side of every branch of the dispatch.  Weights as tools/forward_digest.py chooses them
(alphaFive-6960 on 11x11, random init seed S + 1 elsewhere), inputs from test_gpu_net._positions(S, B, seed=B), one handle of
max_batch B per shape.

Needs a GPU.
usage: python tests/golden/make_forward_variant_digests.py [--check]    (--check: compare with the file instead of writing it)"""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
for p in (os.path.dirname(TESTS), TESTS):
    if p not in sys.path:
        sys.path.insert(0, p)

OUT = os.path.join(HERE, "forward_variant_digests.json")
RECORDED_ON = "29a2629"
SHAPES = (
    (11, 1), (11, 8),        # single launch of roles
    (11, 9),                 # first batch past the small-batch threshold: paired branches, two workgroup classes
    (11, 300),               # more positions than CUs: a persistent workgroup takes several
    (15, 3),                 # pixel-tile split
    (15, 127), (15, 128),    # either side of the half-class launch
    (15, 300),
    (7, 5),                  # a board without the split-operand path
)
# (af_net_tune key, value) pairs applied on top of the defaults; every key is put back after the forward
DEFAULTS = {0: 5, 4: 1, 7: 0, 9: 1}
SETTINGS = ((),) + tuple(((7, b),) for b in (16, 32, 64, 128, 256, 512, 1024, 2048, 128 | 256)) + (((4, 2),), ((9, 0),), ((0, 1),))
# include/af_net.h documents these key-7 values as "same results bit for bit" as the default
SAME_BITS_AS_DEFAULT = tuple(((7, b),) for b in (64, 128, 256, 512, 1024, 2048, 128 | 256))


def shape_key(S, B):
    return "S%d_B%d" % (S, B)


def setting_key(setting):
    return "+".join("key%d=%d" % kv for kv in setting) or "default"


def digests_of(S, B):
    """{setting key: [sha256 of the policy bytes, sha256 of the value bytes]} of one shape, every setting"""
    import torch
    from alphafive_amd import net_hip
    from alphafive_amd.network import ResNet
    from test_gpu_net import _positions
    net = ResNet(S, device="cuda", seed=S + 1)
    if S == 11:
        net.load_npz(os.path.join(HERE, "alphaFive-6960.weights.npz"))
    h = net_hip.HipNet(net.variables, S, B, net.device)
    xt = torch.from_numpy(_positions(S, B, seed=B)).cuda()
    out = {}
    try:
        for setting in SETTINGS:
            try:
                for k, v in setting:
                    net_hip.tune(k, v)
                p, v = h(xt)
                out[setting_key(setting)] = [hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest() for t in (p, v)]
            finally:
                for k, _ in setting:
                    net_hip.tune(k, DEFAULTS[k])
    finally:
        h.close()
    return out


def main():
    rec = {"recorded_on_commit": RECORDED_ON, "digests": {}}
    for S, B in SHAPES:
        rec["digests"][shape_key(S, B)] = d = digests_of(S, B)
        differ = [setting_key(s) for s in SAME_BITS_AS_DEFAULT if d[setting_key(s)] != d["default"]]
        print("%-9s %d settings; documented as the default's bits but different: %s" % (shape_key(S, B), len(d), differ or "none"), flush=True)
    if "--check" in sys.argv:
        with open(OUT) as f:
            old = json.load(f)["digests"]
        bad = [(k, s) for k in rec["digests"] for s in rec["digests"][k] if rec["digests"][k][s] != old.get(k, {}).get(s)]
        print("check: %d forwards differ from %s %s" % (len(bad), OUT, bad))
        sys.exit(1 if bad or set(old) != set(rec["digests"]) else 0)
    out = OUT
    if "--out" in sys.argv:
        out = sys.argv[sys.argv.index("--out") + 1]
    with open(out, "w") as f:
        json.dump(rec, f, indent=0, sort_keys=True)
        f.write("\n")
    print("%s: %d shapes x %d settings, %d bytes" % (out, len(SHAPES), len(SETTINGS), os.path.getsize(out)))


if __name__ == "__main__":
    main()
