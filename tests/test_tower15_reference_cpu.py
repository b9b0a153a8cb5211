"""The 15x15 cases of the bf16 tower kernels (csrc/af_tower_bf16.hip, Geo<15>), without a GPU: from oracle/tower_fp64.py alone, the
conditions under which a bf16 MFMA kernel must reproduce fp64 bit for bit on them.  The generators and the conditions are stated in
tests/tower_cases.py; tests/test_gpu_tower15_exact.py runs the kernels on these cases."""
import pytest

import tower_cases as gen

S = 15


@pytest.mark.parametrize("iso", gen.ISOLATIONS)
def test_exact_block_generators_meet_the_exactness_conditions(iso):
    gen.check_exact_block_generator(S, iso)


def test_exact_stem_generator_meets_the_exactness_conditions():
    gen.check_exact_stem_generator(S)


def test_exact_heads_generator_meets_the_exactness_conditions():
    gen.check_exact_heads_generator(S)


def test_exact_dense_generator_meets_the_exactness_conditions():
    gen.check_exact_dense_generator(S)
