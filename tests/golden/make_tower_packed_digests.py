#!/usr/bin/env python
"""tests/golden/tower_packed_digests.json: what af_tower_set_block / _set_stem / _set_heads / _set_dense make of three weight
sets of tests/test_gpu_tower_update.py — the SHA-256 of every buffer of HipTower.debug_weights(), in af_tower_debug_weights'
order — for weight_set(10, False) at 2 blocks, weight_set(38, False, 8) and weight_set(39, False, 9): ties, signed zeros,
denormals, values that overflow to inf and NaNs in every tensor that has room for them.

The file was recorded on an MI355X with libaf_tower.so built from commit 198d37c ("Replay: draw minibatches on the device"),
the last one whose setters packed on the host (bf16_rne, pack_tower and the loops inside the four setters), with the weight
generator of this commit.  That library was built into a scratch directory and selected with AF_TOWER_LIB.  Those packers are
gone; this record of their bytes is what oracle/tower_pack.py — the specification the device packers are held to — is checked
against (tests/test_tower_pack_cpu.py).  Re-running the script on a later commit only shows whether that commit still
reproduces the file: a difference is a layout change, to be made on purpose and explained, never a reason to overwrite the
file quietly.

Needs a GPU.  The inputs come from the test module's own generator, imported so that they cannot drift from the test's.

usage: python tests/golden/make_tower_packed_digests.py [--check]      (--check: compare with the file instead of writing it)"""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
for p in (os.path.dirname(TESTS), TESTS):
    if p not in sys.path:
        sys.path.insert(0, p)

OUT = os.path.join(HERE, "tower_packed_digests.json")
SETS = ((10, 2), (38, 8), (39, 9))          # (seed, blocks) of weight_set(seed, False, blocks)


def key(seed, blocks):
    return "seed%d-%dblocks" % (seed, blocks)


def digests(buffers):
    return [hashlib.sha256(b.tobytes()).hexdigest() for b in buffers]


def main():
    from test_gpu_tower_update import host_tower, weight_set
    rec = {}
    for seed, blocks in SETS:
        H = host_tower(weight_set(seed, False, blocks), max_batch=1, blocks=blocks)
        try:
            rec[key(seed, blocks)] = digests(H.debug_weights())
        finally:
            H.close()
        print("%-16s %d buffers" % (key(seed, blocks), len(rec[key(seed, blocks)])), flush=True)
    if "--check" in sys.argv:
        with open(OUT) as f:
            old = json.load(f)
        bad = [k for k in rec if rec[k] != old.get(k)]
        print("check: %d of %d sets differ from %s %s" % (len(bad), len(rec), OUT, bad))
        sys.exit(1 if bad or set(old) != set(rec) else 0)
    with open(OUT, "w") as f:
        json.dump(rec, f, indent=0, sort_keys=True)
        f.write("\n")
    print("%s: %d sets, %d bytes" % (OUT, len(rec), os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
