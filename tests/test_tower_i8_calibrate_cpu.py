"""The device calibration of the int8 tower, the part that needs no GPU: the specification of its arithmetic
(tower_i8.scales_from_absmax / calibration_ok) against hand-computed fp32 cases, the refusals of tower_hip.check_calibration, and
the host path of DeepResNet.set_variables_device(..., calibrate_on=...)."""
import numpy as np
import pytest

from alphafive_amd import tower_i8 as t8

f32 = np.float32


def _bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def test_scales_from_absmax_is_the_stated_fp32_sequence():
    # absmax 127 -> a = 1, r = 1; 63.5 -> 0.5, 2; 1.0 -> fp32(1 / 127) = 0x3c010204, r = fp32(1 / that) = 127 exactly
    a, r = t8.scales_from_absmax([127.0, 63.5, 1.0], 1.0)
    assert a.dtype == np.float32 and r.dtype == np.float32
    assert _bits(a).tolist() == [0x3f800000, 0x3f000000, 0x3c010204]
    assert _bits(r).tolist() == [0x3f800000, 0x40000000, 0x42fe0000]
    # margin 1.5: the product is rounded to fp32 first, then divided: 127 * 1.5 = 190.5 -> a = 1.5; 2 * 1.5 / 127 = fp32(3 / 127)
    a, r = t8.scales_from_absmax([127.0, 2.0], 1.5)
    assert _bits(a).tolist() == [0x3fc00000, _bits(f32(3.0) / f32(127.0)).tolist()]
    assert _bits(r).tolist() == [_bits(f32(1.0) / f32(1.5)).tolist(), _bits(f32(1.0) / (f32(3.0) / f32(127.0))).tolist()]
    # two roundings, not one: an absmax and a margin whose exact product is no fp32 number
    x, m = f32(1.0 + 2.0 ** -23), f32(1.0 + 2.0 ** -22)
    a, _ = t8.scales_from_absmax([x], m)
    assert _bits(a)[0] == _bits((x * m).astype(np.float32) / f32(127.0))
    # bf16 values as the device measures them
    a, r = t8.scales_from_absmax(np.array([3.140625, 0.00390625], np.float32), 1.25)
    for i, v in enumerate((3.140625, 0.00390625)):
        want = f32(f32(f32(v) * f32(1.25)) / f32(127.0))
        assert _bits(a)[i] == _bits(want) and _bits(r)[i] == _bits(f32(1.0) / want)


def test_an_absmax_of_zero_gives_scale_one_whatever_the_margin():
    for margin in (1.0, 1.5, 1e-30, 3e38):
        a, r = t8.scales_from_absmax([0.0, -0.0], margin)
        assert _bits(a).tolist() == [0x3f800000] * 2 and _bits(r).tolist() == [0x3f800000] * 2
        assert t8.calibration_ok([0.0, -0.0], margin)


def test_calibration_ok_refuses_what_cannot_be_a_scale():
    assert t8.calibration_ok([1.0, 0.5, 0.0, 3.0e38], 1.0)
    big = f32(3.0e38)                                     # finite, but 3e38 * 1.5 overflows fp32: a = inf
    a, _ = t8.scales_from_absmax([big], 1.5)
    assert np.isinf(a[0])
    assert not t8.calibration_ok([1.0, big], 1.5)
    assert not t8.calibration_ok([1.0, np.nan], 1.0)
    assert not t8.calibration_ok([np.inf, 1.0], 1.0)
    tiny = f32(2.0 ** -133)                               # the smallest bf16 subnormal: a margin can push a down to 0
    assert t8.calibration_ok([tiny], 1.0)
    assert not t8.calibration_ok([tiny], 1e-20)
    # what passes is what check_scales accepts
    a, _ = t8.scales_from_absmax([1.0, 0.5, 0.0, 2.0], 1.25)
    assert np.array_equal(t8.check_scales(a, 2), a)


def test_check_calibration_refuses_before_the_gpu():
    from alphafive_amd import tower_hip
    tower_hip.check_calibration("int8", 11, 1.0)
    tower_hip.check_calibration("int8", 11, 1.25)
    with pytest.raises(ValueError):
        tower_hip.check_calibration("bf16", 11, 1.0)
    with pytest.raises(ValueError):
        tower_hip.check_calibration("int8", 15, 1.0)
    for margin in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError):
            tower_hip.check_calibration("int8", 11, margin)


def test_set_variables_device_with_calibrate_on_is_the_host_path_on_a_cpu_net():
    import torch
    from alphafive_amd.network_deep import DeepResNet
    net = DeepResNet(11, blocks=1, device="cpu", seed=0)
    other = DeepResNet(11, blocks=1, device="cpu", seed=1)
    new = {k: torch.from_numpy(v) for k, v in other.variables.items()}
    planes = torch.zeros(2, 3, 11, 11)
    v0 = net.version
    net.set_variables_device(new, calibrate_on=planes, margin=1.25)
    assert net.version == v0 + 1
    for k, v in net.variables.items():
        assert np.array_equal(v, other.variables[k]), k
    with pytest.raises(ValueError):                       # nothing on a cpu net is int8: there is no evaluator to calibrate
        net.calibrate_int8_device(planes)
