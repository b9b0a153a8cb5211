#!/usr/bin/env python
"""tests/golden/packed_weight_digests.json: what af_net_set_variable + af_net_finalize make of the weight sets of
tests/test_gpu_net_update.py — the SHA-256 of every buffer of HipNet.debug_weights(), in af_net_debug_weights' order, and
HipNet.debug_scales() as uint32 bit patterns — for its 4 CASES x (plain, scaled, zero) at max_batch 8.

The file was recorded with libaf_net built from commit c9da17f ("Hand trained weights to the evaluator on the device, in place"),
the last one whose af_net_finalize packed on the host (pack_layer, pack_proj, pack_frags, the stem loop, pack_wino, pad_bias).
Those packers are gone; this record of their bytes is the specification the device packers are held to.  Re-running the script
on a later commit only shows whether that commit still reproduces the file: a difference is a layout change, to be made on
purpose and explained, never a reason to overwrite the file quietly.

Needs a GPU.  The inputs are the checkpoint fixture and np.random.RandomState streams, imported from the test module so that
they cannot drift from the test's.

usage: python tests/golden/make_packed_weight_digests.py [--check]      (--check: compare with the file instead of writing it)"""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
for p in (os.path.dirname(TESTS), TESTS):
    if p not in sys.path:
        sys.path.insert(0, p)

OUT = os.path.join(HERE, "packed_weight_digests.json")
VARIANTS = ("plain", "scaled", "zero")
MAX_BATCH = 8


def key(case, variant):
    return "%dx%d-%s-%s" % (case[0], case[0], case[1], variant)


def state_of(handle):
    """the record of one handle: {"buffers": [sha256 hex, ...], "scales": [uint32, ...]}"""
    import numpy as np
    return {"buffers": [hashlib.sha256(b.tobytes()).hexdigest() for b in handle.debug_weights()],
            "scales": [int(u) for u in handle.debug_scales().view(np.uint32)]}


def main():
    from alphafive_amd import net_hip
    from test_gpu_net_update import CASES, _variant, _weights
    rec = {}
    for case in CASES:
        for variant in VARIANTS:
            H = net_hip.HipNet(_variant(_weights(case), variant), case[0], MAX_BATCH, "cuda")
            try:
                rec[key(case, variant)] = state_of(H)
            finally:
                H.close()
            print("%-22s %d buffers, %d scales" % (key(case, variant), len(rec[key(case, variant)]["buffers"]),
                                                   len(rec[key(case, variant)]["scales"])), flush=True)
    if "--check" in sys.argv:
        with open(OUT) as f:
            old = json.load(f)
        bad = [k for k in rec if rec[k] != old.get(k)]
        print("check: %d of %d combinations differ from %s %s" % (len(bad), len(rec), OUT, bad))
        sys.exit(1 if bad or set(old) != set(rec) else 0)
    with open(OUT, "w") as f:
        json.dump(rec, f, indent=0, sort_keys=True)
        f.write("\n")
    print("%s: %d combinations, %d bytes" % (OUT, len(rec), os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
