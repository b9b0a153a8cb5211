#!/usr/bin/env python
"""Record the UNMODIFIED reference's utils.is_game_over (utils.py:199-235) on the crafted boards of tests/terminal_cases.py — every
pair (board_size, goal) of terminal_cases.PAIRS, the children handed to the descent test and the roots handed to the root test —
as tests/golden/rules_envelope.npz.  Like make_golden.py this runs in the build container only: the reference never travels.

    python tests/golden/make_rules_envelope.py

Data only: per board S, goal, the board padded to 16x16, `last` (-1 for a root), the class index (terminal_cases.CLASSES for a
child, len(CLASSES) + index into ROOT_KINDS for a root) and the reference's (over, value).
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, "/root/reference")

import utils as refutils           # noqa: E402  (reference)

import terminal_cases as tc        # noqa: E402  (build's own)


def boards_of(S, goal):
    """(board, last, class index) of everything the tests of a pair look at, in the generator's order."""
    out = [(c.child, c.last, tc.CLASSES.index(c.cls)) for c in tc.cases(S, goal)]
    out += [(r.board, -1, len(tc.CLASSES) + tc.ROOT_KINDS.index(r.kind)) for r in tc.roots(S, goal)]
    return out


def main():
    rec = dict(S=[], goal=[], board=[], last=[], cls=[], over=[], value=[])
    for S, goal in tc.PAIRS:
        for b, last, cls in boards_of(S, goal):
            over, value = refutils.is_game_over(b.copy(), goal)
            pad = np.zeros((16, 16), np.int8)
            pad[:S, :S] = b
            for k, v in zip(("S", "goal", "board", "last", "cls", "over", "value"), (S, goal, pad, last, cls, over, value)):
                rec[k].append(v)
        print((S, goal), len(rec["S"]), "boards so far")
    path = os.path.join(HERE, "rules_envelope.npz")
    np.savez_compressed(path, S=np.array(rec["S"], np.int8), goal=np.array(rec["goal"], np.int8),
                        board=np.array(rec["board"], np.int8), last=np.array(rec["last"], np.int16),
                        cls=np.array(rec["cls"], np.int8), over=np.array(rec["over"], np.bool_),
                        value=np.array(rec["value"], np.float32))
    print("rules_envelope:", len(rec["S"]), "boards,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
