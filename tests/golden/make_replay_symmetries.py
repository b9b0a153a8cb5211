#!/usr/bin/env python
"""tests/golden/replay_symmetries.npz: what the UNMODIFIED reference utils.RandomStack.get_data (utils.py:118-146) returns for one
position per board size under each of its 8 symmetries (build container only; the reference never travels).

Per S = 3..16 the position is replay_cases.fixture_position(S): a board whose 8 images are pairwise distinct, policy = arange(C),
last move at cell 1, and once more with no last move.  The reference's three draws (np.random.choice for the positions and the
quarter turns, random.choice for the flip) are dictated by replay_cases.scripted_draws, which replaces the two functions in this
process for the duration of the call; the reference's file is loaded as it is.  Recorded (data only), per S:
  board_S     int8[S,S]        the position's board (+1 mine / -1 theirs)
  boards_S    float32[8,3,S,S] get_data's boards, symmetry i = (k, flip) = replay_cases.SYMMETRIES[i]
  policies_S  float32[8,C]     its policies
  none_boards_S, none_policies_S   float32[3,S,S], float32[C]: the same position without a last move, at NONE_SYMMETRY
Before it writes, the script runs the full check the fixture stands for: every S, every last cell and none, all 8 symmetries
(12,040 cases) of replay_cases.augment_reference against the reference.

usage: python tests/golden/make_replay_symmetries.py [/root/reference]"""
import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

NONE_SYMMETRY = (1, 1)


def main():
    import replay_cases as rc
    ref_dir = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
    spec = importlib.util.spec_from_file_location("af_reference_utils", os.path.join(ref_dir, "utils.py"))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    out, cases = {}, 0
    for S in rc.SIZES:
        C = S * S
        board, policy, last = rc.fixture_position(S)
        st = ref.RandomStack(S, length=10)
        st.data = rc.host_records(ref.board_to_state, np.stack([board.reshape(C)] * 2), np.stack([policy] * 2),
                                  np.array([last, -1]), np.array([1.0, -1.0]), np.array([1.0, 1.0]))
        turns, flips = [k for k, f in rc.SYMMETRIES], [f for k, f in rc.SYMMETRIES]
        boards, _, _, policies = rc.scripted_get_data(st, [0] * 8, turns, flips)
        nb, _, _, npol = rc.scripted_get_data(st, [1], NONE_SYMMETRY[:1], NONE_SYMMETRY[1:])
        assert boards.dtype == policies.dtype == np.float32 and boards.shape == (8, 3, S, S) and policies.shape == (8, C)
        assert len(set(b.tobytes() for b in boards)) == 8
        out["board_%d" % S], out["boards_%d" % S], out["policies_%d" % S] = board, boards, policies
        out["none_boards_%d" % S], out["none_policies_%d" % S] = nb[0], npol[0]
        # the whole agreement, not recorded: every last cell and none, all 8 symmetries
        cb, cp, cl, cv, cw, _ = rc.sample_cases(S)
        idx, tt, ff = rc.sample_triples(S)
        st = ref.RandomStack(S, length=10)
        st.data = rc.host_records(ref.board_to_state, cb, cp, cl, cv, cw)
        got = rc.scripted_get_data(st, idx, tt, ff)
        assert not rc.differing(got, rc.sample_expected(S), rc.SAMPLE_OUTPUTS), S
        cases += len(idx)
    out["none_symmetry"] = np.array(NONE_SYMMETRY, np.int32)
    path = os.path.join(HERE, "replay_symmetries.npz")
    np.savez_compressed(path, **out)
    print("%s: %d sizes, %d bytes; augment_reference equals the reference on %d cases" % (path, len(rc.SIZES), os.path.getsize(path), cases))


if __name__ == "__main__":
    main()
