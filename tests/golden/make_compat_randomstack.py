#!/usr/bin/env python
"""tests/golden/compat_randomstack.npz: what the UNMODIFIED reference utils.RandomStack (utils.py:29-57, 121-146) makes of the
replay pickles alphafive_amd.utils.RandomStack.save writes (build container only; the reference never travels).

The stack is the one tests/test_compat.py builds (14 seeded 11x11 episodes pushed into RandomStack(11, length=300) under
random.seed(1)).  Recorded (data only):
  ref_data_len, ref_result, ref_black_win, ref_white_win, ref_n_data   the reference's bookkeeping after load(60)
  ref_boards, ref_weights, ref_values, ref_policies                    its get_data(batch_size=64) under np.random.seed(5),
                                                                       random.seed(5)
  ref_pkl_data, ref_pkl_data_len, ref_pkl_result                       the bytes of the three pickles its save(120) writes

usage: python tests/golden/make_compat_randomstack.py [/root/reference]"""
import importlib.util
import os
import random
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))


def main():
    ref_dir = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
    spec = importlib.util.spec_from_file_location("af_reference_utils", os.path.join(ref_dir, "utils.py"))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    from test_compat import build_stack
    out = {}
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        os.chdir(tmp)
        try:
            os.mkdir("data_buffer")
            a = build_stack()
            a.save(60)
            b = ref.RandomStack(11, length=300)
            b.load(60)
            out.update(ref_data_len=np.asarray(b.data_len, np.int32), ref_result=np.asarray(b.result, np.int32),
                       ref_black_win=np.int32(b.black_win), ref_white_win=np.int32(b.white_win), ref_n_data=np.int32(len(b.data)))
            np.random.seed(5)
            random.seed(5)
            boards, weights, values, policies = b.get_data(batch_size=64)
            out.update(ref_boards=boards, ref_weights=weights, ref_values=values, ref_policies=policies)
            b.save(120)
            for stem in ("data", "data_len", "result"):
                with open(os.path.join("data_buffer", "%s120.pkl" % stem), "rb") as f:
                    out["ref_pkl_" + stem] = np.frombuffer(f.read(), np.uint8)
        finally:
            os.chdir(cwd)
    path = os.path.join(HERE, "compat_randomstack.npz")
    np.savez_compressed(path, **out)
    print("%s: %d positions in %d episodes, batch of %d" % (path, out["ref_n_data"], len(out["ref_data_len"]), len(out["ref_values"])))


if __name__ == "__main__":
    main()
