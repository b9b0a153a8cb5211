"""The C-ABI library loads on a GPU-less host and exports every symbol include/af_engine.h declares;
the host-only entry points (state codec, error strings) behave like utils.py."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import GOLDEN, REPO

LIB = os.path.join(REPO, "alphafive_amd", "_lib", "libaf_hip.so")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        from alphafive_amd import build
        build.build_all()
    return ctypes.CDLL(LIB)


def test_every_declared_symbol_is_exported(lib):
    hdr = open(os.path.join(REPO, "include", "af_engine.h")).read()
    names = set(re.findall(r"\b(af_[a-z_0-9]+)\s*\(", hdr))
    assert len(names) >= 18
    for n in names:
        assert hasattr(lib, n), f"{n} declared in af_engine.h but not exported"
    lib.af_abi_version.restype = ctypes.c_int
    assert lib.af_abi_version() == 6


def test_state_key_codec_roundtrip(lib):
    from alphafive_amd import engine as eng
    z = np.load(os.path.join(GOLDEN, "rules.npz"))
    for k in range(len(z["S"])):
        S = int(z["S"][k])
        s = str(z["state"][k])
        key = eng.state_to_key(s, S)
        b = z["board"][k][:S, :S]
        kw = len(key) // 2
        for c in range(S * S):
            mine = (int(key[c >> 6]) >> (c & 63)) & 1
            theirs = (int(key[kw + (c >> 6)]) >> (c & 63)) & 1
            assert mine == (b[c // S, c % S] == 1) and theirs == (b[c // S, c % S] == -1)
        assert eng.key_to_state(key, S) == s
    with pytest.raises(eng.EngineError):
        eng.state_to_key("l/l/x9/", 11)


def test_error_strings_and_bad_args(lib):
    lib.af_strerror.restype = ctypes.c_char_p
    assert b"store full" in lib.af_strerror(-3)
    from alphafive_amd import engine as eng
    from conftest import make_cfg
    with pytest.raises(eng.EngineError):
        eng.Engine(make_cfg(board_size=17), 1)          # 289 cells > 256: rejected before touching HIP
    with pytest.raises(eng.EngineError):
        eng.Engine(make_cfg(goal=12), 1)


def test_product_fails_loudly_without_a_gpu(lib):
    """No CPU fallback: on a host without a HIP device creating an engine raises (AF_ERR_HIP)."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    from alphafive_amd import engine as eng
    from conftest import make_cfg
    with pytest.raises(eng.EngineError):
        eng.Engine(make_cfg(), 4)
    from alphafive_amd.player import Player
    with pytest.raises(Exception):
        Player(make_cfg(), training=True, pv_fn=lambda x: None)


@pytest.mark.parametrize("header, libname, prefix, least", [("af_net.h", "libaf_net.so", "af_net_", 8),
                                                             ("af_tower_bf16.h", "libaf_tower.so", "af_tower_", 13),
                                                             ("af_replay.h", "libaf_replay.so", "af_replay_", 7)])
def test_net_libraries_export_every_declared_symbol(lib, header, libname, prefix, least):
    """include/af_net.h (fp32 net), af_tower_bf16.h (bf16 net of BASELINE configs[4]), af_replay.h (device replay buffer)."""
    hdr = open(os.path.join(REPO, "include", header)).read()
    names = set(re.findall(r"\b(" + prefix + r"[a-z_0-9]+)\s*\(", hdr))
    assert len(names) >= least
    nl = ctypes.CDLL(os.path.join(REPO, "alphafive_amd", "_lib", libname))
    for n in names:
        assert hasattr(nl, n), f"{n} declared in {header} but not exported"
    fn = getattr(nl, prefix + "strerror")
    fn.restype = ctypes.c_char_p
    assert fn(-1) == b"bad argument"


def test_tower_tune_accepts_only_documented_values(lib):
    """af_tower_tune (include/af_tower_bf16.h): key 0 ring depth 0 / 8 / 12 / 16, key 1 workgroups >= 0, key 2 ablation bits 0..7,
    key 3 engine 0 / 2 / 3, key 4 heads kernel 0 / 1; everything else is AF_TOWER_ERR_ARG (a depth of 5 used to mean 8 silently).
    tests/test_gpu_tower_exact.py shows on the GPU that a rejected call leaves the previous setting in force."""
    nl = ctypes.CDLL(os.path.join(REPO, "alphafive_amd", "_lib", "libaf_tower.so"))
    tune = nl.af_tower_tune
    tune.argtypes = [ctypes.c_int32, ctypes.c_int32]
    good = {0: (8, 12, 16, 0), 1: (1, 3, 1 << 20, 0), 2: (1, 7, 0), 3: (0, 2, 3), 4: (0, 1)}      # the default last
    bad = {0: (-1, 1, 5, 7, 9, 24, 32), 1: (-1, -256), 2: (-1, 8, 255), 3: (-1, 1, 4), 4: (-1, 2), 5: (0,), -1: (0,)}
    try:
        for key, values in good.items():
            for v in values:
                assert tune(key, v) == 0, (key, v)
        for key, values in bad.items():
            for v in values:
                assert tune(key, v) == -1, (key, v)
    finally:
        for key, values in good.items():
            tune(key, values[-1])
