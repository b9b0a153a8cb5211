"""oracle/tower_pack.py — the numpy specification of the bf16 tower's weight layout — reproduces, without a GPU, the bytes the
library's former host packers wrote: tests/golden/tower_packed_digests.json holds the SHA-256 of every buffer those packers made
of three weight sets of tests/test_gpu_tower_update.py (tests/golden/make_tower_packed_digests.py says how it was recorded).
The sets carry ties, signed zeros, denormals, values that overflow to inf and NaNs, at 2, 8 and 9 blocks."""
import hashlib
import json
import os

import numpy as np
import pytest

from oracle import tower_pack
from test_gpu_tower_update import weight_set

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tower_packed_digests.json")) as _f:
    RECORD = json.load(_f)


def test_the_record_covers_the_three_sets():
    assert sorted(RECORD) == ["seed10-2blocks", "seed38-8blocks", "seed39-9blocks"]
    assert [len(RECORD[k]) for k in sorted(RECORD)] == [4 * 2 + 12, 4 * 8 + 12, 4 * 9 + 12]


@pytest.mark.parametrize("seed,blocks", [(10, 2), (38, 8), (39, 9)])
def test_pack_reference_reproduces_the_recorded_bytes(seed, blocks):
    buffers = tower_pack.pack_reference(weight_set(seed, False, blocks), blocks)
    assert all(b.dtype == np.uint8 and b.ndim == 1 for b in buffers)
    got = [hashlib.sha256(b.tobytes()).hexdigest() for b in buffers]
    want = RECORD["seed%d-%dblocks" % (seed, blocks)]
    assert len(got) == len(want) == 4 * blocks + 12
    assert [i for i, (g, w) in enumerate(zip(got, want)) if g != w] == []


def test_bf16_bits_on_every_class_of_input():
    """Round to nearest even on the bit pattern, worked by hand: ties to the even neighbour in both directions, the carry into the
    exponent and into inf, zeros and denormals untouched, NaNs kept NaN with their sign."""
    f32 = lambda bits: np.array(bits, np.uint32).view(np.float32)  # noqa: E731
    cases = [(0x3F808000, 0x3F80), (0x3F818000, 0x3F82), (0xBF808000, 0xBF80), (0xBF818000, 0xBF82), (0x3F808001, 0x3F81),
             (0x3DFF8000, 0x3E00), (0x7F7F8000, 0x7F80), (0xFF7FFFFF, 0xFF80), (0x7F7F7FFF, 0x7F7F), (0x00000000, 0x0000),
             (0x80000000, 0x8000), (0x00011C0F, 0x0001), (0x7F800000, 0x7F80), (0xFF800000, 0xFF80),
             (0x7FC00001, 0x7FC0), (0xFFC00000, 0xFFC0), (0x7F800001, 0x7FC0), (0xFF80FFFF, 0xFFC0), (0x7FA51234, 0x7FE5)]
    got = tower_pack.bf16_bits(f32([c[0] for c in cases]))
    assert got.dtype == np.uint16 and [int(g) for g in got] == [c[1] for c in cases]
    assert sorted(tower_pack.PERM.tolist()) == list(range(32))
