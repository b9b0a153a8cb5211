"""alphafive_amd/symmetry.py, the parts that need no GPU: the group laws of the eight symmetries, the (quarter turns, flip)
convention, the summation order of the symmetry average, the balance of the per-leaf draw, the C ABI of libaf_sym.so as far as
it answers without a device, and the constructor's refusals."""
import ctypes
import itertools
import os
import re

import numpy as np
import pytest

from alphafive_amd import symmetry
from alphafive_amd.replay import philox4x32_10
from conftest import REPO

SIZES = range(3, 17)


def _board(S, lead=()):
    return (np.arange(int(np.prod(lead, dtype=np.int64)) * S * S, dtype=np.float32) + 0.5).reshape(tuple(lead) + (S, S))


def mixed_rows(n, C, seed=3):
    """[n, C] float32 of mixed magnitude, 1 down to 1e-8, both signs: sums whose fp32 result depends on the order."""
    rng = np.random.RandomState(seed)
    mag = np.float32(10.0) ** (-rng.randint(0, 9, size=(n, C))).astype(np.float32)
    sign = np.where(rng.rand(n, C) < 0.5, -1.0, 1.0).astype(np.float32)
    return (sign * mag * rng.uniform(0.5, 1.0, size=(n, C)).astype(np.float32)).astype(np.float32)


@pytest.mark.parametrize("S", SIZES)
def test_group_laws(S):
    a = _board(S, (2, 3))
    images = []
    for s in range(8):
        t = symmetry.transform(a, s)
        assert t.shape == a.shape
        assert np.array_equal(symmetry.inverse(t, s), a)
        assert np.array_equal(symmetry.transform(symmetry.inverse(a, s), s), a)
        m = symmetry.cell_map(S, s)
        assert m.dtype == np.int32 and m.shape == (S * S,) and sorted(m.tolist()) == list(range(S * S))
        assert np.array_equal(np.ascontiguousarray(t).reshape(2, 3, -1), a.reshape(2, 3, -1)[..., m])
        images.append(np.ascontiguousarray(t[0, 0]))
    assert np.array_equal(images[0], a[0, 0])                      # s = 0 is the identity
    assert np.array_equal(symmetry.cell_map(S, 0), np.arange(S * S))
    for x, y in itertools.combinations(range(8), 2):
        assert not np.array_equal(images[x], images[y]), (x, y)     # all-distinct cells: eight different images


@pytest.mark.parametrize("S", (3, 4, 11, 16))
def test_convention_is_rot90_then_flip(S):
    a = _board(S)
    for s in range(8):
        turns = s & 3
        want = np.rot90(a, turns)
        if s >= 4:
            want = np.flip(want, 0)
        assert np.array_equal(symmetry.transform(a, s), want), s
    with pytest.raises(ValueError):
        symmetry.transform(a, 8)


def test_expand_apply_restore_follow_transform():
    S, B = 5, 3
    planes = _board(S, (B, 3))
    p8 = symmetry.expand_reference(planes)
    assert p8.shape == (8 * B, 3, S, S)
    for b in range(B):
        for s in range(8):
            assert np.array_equal(p8[8 * b + s], symmetry.transform(planes[b], s))
    syms = np.array([5, 0, 2], np.int32)
    t = symmetry.apply_reference(planes, syms)
    for b in range(B):
        assert np.array_equal(t[b], symmetry.transform(planes[b], syms[b]))
    back = symmetry.restore_reference(t[:, 0].reshape(B, S * S), syms, S)
    assert np.array_equal(back, planes[:, 0].reshape(B, S * S))


def test_summation_order_is_sequential_fp32():
    S, B = 4, 6
    C = S * S
    policy8, value8 = mixed_rows(8 * B, C), mixed_rows(8 * B, 1, seed=4).reshape(-1)
    pol, val = symmetry.reduce_reference(policy8, value8, S)
    assert pol.dtype == np.float32 and val.dtype == np.float32 and pol.shape == (B, C) and val.shape == (B,)
    want_p, want_v = np.zeros((B, C), np.float32), np.zeros(B, np.float32)
    q = np.zeros((B, 8, C), np.float32)
    for b in range(B):
        for s in range(8):
            q[b, s] = symmetry.inverse(policy8[8 * b + s].reshape(S, S), s).reshape(C)
        for c in range(C):
            acc = np.float32(q[b, 0, c])
            for s in range(1, 8):
                acc = np.float32(acc + np.float32(q[b, s, c]))
            want_p[b, c] = np.float32(acc * np.float32(0.125))
        acc = np.float32(value8[8 * b])
        for s in range(1, 8):
            acc = np.float32(acc + np.float32(value8[8 * b + s]))
        want_v[b] = np.float32(acc * np.float32(0.125))
    assert np.array_equal(pol.view(np.uint32), want_p.view(np.uint32))
    assert np.array_equal(val.view(np.uint32), want_v.view(np.uint32))
    # the order is observable: numpy's own mean over the eight terms (contiguous, so summed as a tree) rounds differently somewhere
    tree = np.ascontiguousarray(q.transpose(0, 2, 1)).mean(axis=-1, dtype=np.float32)
    assert np.allclose(pol, tree, rtol=1e-5, atol=1e-9) and (pol != tree).any()


@pytest.mark.parametrize("seed,counter,lo,hi", [(21, 0, 987, 1046), (21, 1, 984, 1052), (2 ** 63 + 5, 0, 948, 1059),
                                                (21, 2 ** 32 - 1, 951, 1112), (21, 2 ** 32, 985, 1079)])
def test_draw_counts(seed, counter, lo, hi):
    n = 8192
    syms = symmetry.draw_reference(n, seed, counter)
    assert syms.dtype == np.int32 and syms.shape == (n,)
    # ... which is the stated Philox block, written out here
    v = philox4x32_10(np.arange(n, dtype=np.uint64), counter & 0xFFFFFFFF, counter >> 32, 0x53594d30, seed & 0xFFFFFFFF, seed >> 32)
    assert np.array_equal(syms, (v[0] >> np.uint32(29)).astype(np.int32))
    counts = np.bincount(syms, minlength=8)
    assert counts.shape == (8,) and counts.sum() == n
    assert 896 <= counts.min() and counts.max() <= 1152, counts       # +-12.5 % around 1024, about 4.3 sigma
    assert (counts.min(), counts.max()) == (lo, hi), counts           # the recorded figures of these (seed, counter) pairs


def test_draws_differ_between_counters_and_seeds():
    a, b, c = symmetry.draw_reference(256, 21, 0), symmetry.draw_reference(256, 21, 1), symmetry.draw_reference(256, 22, 0)
    assert (a != b).any() and (a != c).any()
    assert (symmetry.draw_reference(256, 21, 2 ** 32) != a).any()     # the high word of the counter is part of the address


# ---- the C ABI, as far as it answers without a device ----
def _lib():
    L = ctypes.CDLL(os.path.join(REPO, "alphafive_amd", "_lib", "libaf_sym.so"))
    vp, i32 = ctypes.c_void_p, ctypes.c_int32
    L.af_sym_create.argtypes = [i32, i32, i32, ctypes.c_uint64, ctypes.POINTER(vp)]
    L.af_sym_expand.argtypes = [vp, vp, vp, vp, i32]
    L.af_sym_reduce.argtypes = [vp, vp, vp, vp, vp, vp, i32]
    L.af_sym_apply.argtypes = [vp, vp, vp, vp, i32]
    L.af_sym_restore.argtypes = [vp, vp, vp, vp, vp, vp, i32]
    L.af_sym_set_counter.argtypes = [vp, vp, ctypes.c_uint64]
    L.af_sym_state.argtypes = [vp, vp, vp, vp, i32]
    L.af_sym_strerror.argtypes = [ctypes.c_int]
    L.af_sym_strerror.restype = ctypes.c_char_p
    return L


def test_header_prototypes_are_exported():
    hdr = open(os.path.join(REPO, "include", "af_sym.h")).read()
    names = sorted(set(re.findall(r"\b(af_sym_\w+)\s*\(", hdr)))
    assert set(names) >= {"af_sym_abi_version", "af_sym_create", "af_sym_destroy", "af_sym_expand", "af_sym_reduce", "af_sym_apply",
                          "af_sym_restore", "af_sym_set_counter", "af_sym_state", "af_sym_strerror"}
    L = _lib()
    for name in names:
        assert hasattr(L, name), name
    assert L.af_sym_abi_version() == 1
    assert int(re.search(r"#define\s+AF_SYM_DRAW_TAG\s+0x([0-9a-fA-F]+)u", hdr).group(1), 16) == symmetry.AF_SYM_DRAW_TAG == 0x53594d30
    assert L.af_sym_strerror(-1) == b"bad argument" and L.af_sym_strerror(-2) == b"HIP runtime error"


def test_bad_arguments_are_refused_without_a_gpu():
    L = _lib()
    ERR_ARG = -1
    a, b, c, d = (ctypes.c_void_p(x) for x in (0x1000, 0x2000, 0x3000, 0x4000))    # never dereferenced: refused before any launch
    fake = ctypes.c_void_p(1)                                                      # ... and neither is this handle
    out = ctypes.c_void_p()
    for S, mb in ((2, 1), (17, 1), (11, 0), (11, -3), (16, 2 ** 31 - 1)):
        assert L.af_sym_create(S, mb, 0, 0, ctypes.byref(out)) == ERR_ARG, (S, mb)
    assert L.af_sym_create(11, 1, 0, 0, None) == ERR_ARG
    # null handle
    assert L.af_sym_expand(None, None, a, b, 1) == ERR_ARG
    assert L.af_sym_reduce(None, None, a, b, c, d, 1) == ERR_ARG
    assert L.af_sym_apply(None, None, a, b, 1) == ERR_ARG
    assert L.af_sym_restore(None, None, a, b, c, d, 1) == ERR_ARG
    assert L.af_sym_set_counter(None, None, 0) == ERR_ARG
    assert L.af_sym_state(None, None, None, None, 0) == ERR_ARG
    # null pointers
    assert L.af_sym_expand(fake, None, None, b, 1) == ERR_ARG and L.af_sym_expand(fake, None, a, None, 1) == ERR_ARG
    assert L.af_sym_apply(fake, None, None, b, 1) == ERR_ARG and L.af_sym_apply(fake, None, a, None, 1) == ERR_ARG
    for i in range(4):
        args = [a, b, c, d]
        args[i] = None
        assert L.af_sym_reduce(fake, None, *args, 1) == ERR_ARG, i
        assert L.af_sym_restore(fake, None, *args, 1) == ERR_ARG, i
    # batch < 1
    for batch in (0, -1):
        assert L.af_sym_expand(fake, None, a, b, batch) == ERR_ARG
        assert L.af_sym_reduce(fake, None, a, b, c, d, batch) == ERR_ARG
        assert L.af_sym_apply(fake, None, a, b, batch) == ERR_ARG
        assert L.af_sym_restore(fake, None, a, b, c, d, batch) == ERR_ARG
    # an input that aliases the output it is permuted into
    assert L.af_sym_expand(fake, None, a, a, 1) == ERR_ARG
    assert L.af_sym_apply(fake, None, a, a, 1) == ERR_ARG
    assert L.af_sym_restore(fake, None, a, b, a, d, 1) == ERR_ARG
    assert L.af_sym_reduce(fake, None, a, b, a, d, 1) == ERR_ARG
    assert L.af_sym_state(fake, None, None, None, -1) == ERR_ARG


# ---- the Python surface ----
def _never(rows):
    raise AssertionError("make_inner called although the arguments are refused")


@pytest.mark.parametrize("kw", [dict(mode="median"), dict(mode=None), dict(board_size=2), dict(board_size=17), dict(max_batch=0),
                                dict(max_batch=-4)])
def test_constructor_refuses_before_touching_the_gpu(kw):
    args = dict(board_size=11, max_batch=4, mode="mean")
    args.update(kw)
    with pytest.raises(ValueError):
        symmetry.SymmetricEvaluator(_never, args["board_size"], args["max_batch"], mode=args["mode"])


def test_module_imports_without_torch():
    import subprocess
    import sys
    code = ("import sys; sys.modules['torch'] = None; import importlib.util as u; "
            "spec = u.spec_from_file_location('symmetry_alone', %r); m = u.module_from_spec(spec); spec.loader.exec_module(m); "
            "import numpy as np; a = np.arange(9.).reshape(3, 3); assert (m.inverse(m.transform(a, 6), 6) == a).all(); "
            "assert m.reduce_reference(np.ones((8, 9), np.float32), np.ones(8, np.float32), 3)[1][0] == 1") % (
                os.path.join(REPO, "alphafive_amd", "symmetry.py"),)
    assert subprocess.run([sys.executable, "-c", code]).returncode == 0
