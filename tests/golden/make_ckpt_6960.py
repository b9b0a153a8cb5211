#!/usr/bin/env python
"""tests/golden/ckpt_6960.npz: the TensorFlow checkpoint the reference ships (/root/reference/ckpt: checkpoint,
alphaFive-6960.index, alphaFive-6960.data-00000-of-00001), in a form that does not repeat the 3 MB of weights already in
tests/golden/alphaFive-6960.weights.npz (build container only; the reference never travels).

The .data file holds nothing but the raw float32 bytes of the model variables, one after another.  Recorded (data only):
  checkpoint      bytes of the `checkpoint` state file
  index           bytes of alphaFive-6960.index
  data_names      variable names in .data order; data_offsets: their byte offsets (found by matching each variable's bytes from
                  alphaFive-6960.weights.npz, not by reading the index)
  data_size, data_sha256   size and SHA-256 of the .data file, so that a rebuild from the npz can be checked byte for byte

usage: python tests/golden/make_ckpt_6960.py [/root/reference]"""
import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
    ck = os.path.join(ref, "ckpt")
    with open(os.path.join(ck, "alphaFive-6960.data-00000-of-00001"), "rb") as f:
        data = f.read()
    with open(os.path.join(ck, "alphaFive-6960.index"), "rb") as f:
        index = f.read()
    with open(os.path.join(ck, "checkpoint"), "rb") as f:
        state = f.read()
    with np.load(os.path.join(HERE, "alphaFive-6960.weights.npz")) as z:
        found = []
        for k in z.files:
            b = np.ascontiguousarray(z[k], np.float32).tobytes()
            off = data.find(b)
            assert off >= 0 and data.find(b, off + 1) < 0, k
            found.append((off, k, len(b)))
    found.sort()
    pos = 0
    for off, k, n in found:                       # the variables tile the file exactly
        assert off == pos, k
        pos += n
    assert pos == len(data)
    out = os.path.join(HERE, "ckpt_6960.npz")
    np.savez_compressed(out, checkpoint=np.frombuffer(state, np.uint8), index=np.frombuffer(index, np.uint8),
                        data_names=np.array([k for _, k, _ in found]), data_offsets=np.array([o for o, _, _ in found], np.int64),
                        data_size=np.int64(len(data)), data_sha256=np.array(hashlib.sha256(data).hexdigest()))
    print("%s: %d variables, .data %d bytes, .index %d bytes" % (out, len(found), len(data), len(index)))


if __name__ == "__main__":
    main()
