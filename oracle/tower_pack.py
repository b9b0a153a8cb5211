"""The weight layout of the bf16 residual tower (csrc/af_tower_bf16.hip), restated in numpy: what every weight-derived device
buffer of an af_tower handle holds, byte for byte, for a given set of fp32 variables.  TEST INFRASTRUCTURE ONLY.

This file is the specification of the layout.  tests/golden/tower_packed_digests.json ties it to the bytes the library's
former host packers wrote (tests/test_tower_pack_cpu.py); the device packers are held to it buffer by buffer
(tests/test_gpu_tower_update.py).

An A fragment row is 8 bf16 = 16 bytes: element e of lane `lane`.  Lane half lane >> 5 picks the upper 8 of a k-step's 16
reduction indices; lane & 31 is an MFMA row, which `perm` maps to the output it computes so that a lane's 16 accumulator rows are
16 consecutive outputs.  Variables are DeepResNet's (network_deep.variable_shapes): convolutions OIHW, dense layers [in][out].
"""
import numpy as np

_M = np.arange(32)
PERM = 16 * ((_M >> 2) & 1) + 8 * (_M >> 4) + 4 * ((_M >> 3) & 1) + (_M & 3)      # MFMA row -> output within a 32-wide tile


def bf16_bits(a):
    """float32 -> bfloat16 bit patterns (uint16), round to nearest even on the bit pattern: ties both ways, the carry runs into
    the exponent and up to inf, denormals and -0 stay as they are.  A NaN keeps its sign and upper payload and gets bit 0x40
    (so a NaN whose payload sits in the low half does not become an infinity)."""
    u = np.ascontiguousarray(a, np.float32).view(np.uint32).astype(np.uint64)
    rounded = (u + 0x7FFF + ((u >> 16) & 1)) >> 16
    nan = (u & 0x7FFFFFFF) > 0x7F800000
    return np.where(nan, (u >> 16) | 0x40, rounded).astype(np.uint16)


def bf16_f32(a):
    """float32 -> the bf16-rounded value, held in float32."""
    return (bf16_bits(a).astype(np.uint32) << 16).view(np.float32)


def _fragments(bits, tiles, ksteps, tile_major):
    """bits uint16 [32 * tiles outputs][16 * ksteps reduction indices] (already padded with zeros) -> the fragment stream
    [tile][k-step][lane][e] (tile_major) or [k-step][tile][lane][e], as bytes."""
    lane, e = np.arange(64)[:, None], np.arange(8)[None, :]
    o = 32 * np.arange(tiles)[:, None, None, None] + PERM[lane & 31]
    k = 16 * np.arange(ksteps)[None, :, None, None] + 8 * (lane >> 5) + e
    out = bits[o, k]                                                            # [tile][k-step][lane][e]
    return np.ascontiguousarray(out if tile_major else out.transpose(1, 0, 2, 3)).view(np.uint8).reshape(-1)


def _bytes(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint8).reshape(-1).copy()


def _block(c1_w, c1_b, c2_w, c2_b, res_w, res_b):
    """w1, w2: [wave = 32 outputs][s][lane][e] with reduction index s = 8 * tap + cc for the 3x3 taps (16 input channels per
    k-step: channel 16 cc + 8 (lane >> 5) + e) and, in w2 only, s = 72 + cc for the 1x1 projection.  b1 = c1_b;
    b2 = c2_b + res_b, one fp32 add."""
    k3 = lambda w: bf16_bits(w).reshape(128, 128, 9).transpose(0, 2, 1).reshape(128, 9 * 128)  # noqa: E731  [cout][tap][cin]
    w1 = _fragments(k3(c1_w), 4, 72, True)
    w2 = _fragments(np.concatenate([k3(c2_w), bf16_bits(res_w).reshape(128, 128)], axis=1), 4, 80, True)
    with np.errstate(over="ignore"):                                            # a sum past the largest float is inf, as on the device
        b2 = np.asarray(c2_b, np.float32) + np.asarray(res_b, np.float32)
    return [w1, w2, _bytes(c1_b), _bytes(b2)]


def pack_reference(variables, blocks):
    """{name: float32 array} -> the 4 * blocks + 12 buffers as uint8 arrays, in af_tower_debug_weights' order
    (include/af_tower_bf16.h): w1, w2, b1, b2 of every block, then stem_w, stem_b, heads_w, heads_b, heads_a, heads_b32,
    dense_wp, dense_wv, dense_pb, dense_vb1, dense_vw2, dense_vb2."""
    V = variables
    out = []
    for b in range(blocks):
        out += _block(*[V["tower/block%d_%s/%s" % (b, layer, part)] for layer in ("conv1", "conv2", "res")
                        for part in ("kernel", "bias")])
    # stem: a k-step holds two groups g = (cin, ky) of one kernel row each: 5 taps + 3 zeros; group 15 does not exist
    stem = np.zeros((128, 16, 8), np.uint16)
    stem[:, :15, :5] = bf16_bits(V["stem/kernel"]).reshape(128, 15, 5)
    out += [_fragments(stem.reshape(128, 128), 4, 8, True), _bytes(V["stem/bias"])]
    # the heads' 1x1 convolutions, 20 outputs: 4 value rows, then 16 policy rows
    hw = np.concatenate([np.asarray(V["value/conv/kernel"], np.float32).reshape(4, 128),
                         np.asarray(V["policy/conv/kernel"], np.float32).reshape(16, 128)])
    hb = np.concatenate([np.asarray(V["value/conv/bias"], np.float32), np.asarray(V["policy/conv/bias"], np.float32)])
    ha = np.zeros((32, 128), np.uint16)                                         # MFMA form: outputs 20..31 are zero rows
    ha[:20] = bf16_bits(hw)
    hb32 = np.zeros(32, np.float32)
    hb32.view(np.uint32)[:20] = hb.view(np.uint32)
    out += [_bytes(bf16_f32(hw)), _bytes(hb), _fragments(ha, 1, 8, True), _bytes(hb32)]
    # dense layers, [k-step][output tile][lane][e]: policy fc [1936][121] padded to 128 outputs, value fc1 [484][64] padded to
    # K = 496, both with zeros
    wp = np.zeros((128, 1936), np.uint16)
    wp[:121] = bf16_bits(V["policy/fc/kernel"]).reshape(1936, 121).T
    wv = np.zeros((64, 496), np.uint16)
    wv[:, :484] = bf16_bits(V["value/fc1/kernel"]).reshape(484, 64).T
    pb = np.full(128, -1.0e30, np.float32)                                      # outputs 121..127: out of the softmax
    pb.view(np.uint32)[:121] = bf16_f32(V["policy/fc/bias"]).view(np.uint32)
    out += [_fragments(wp, 4, 121, False), _fragments(wv, 2, 31, False), _bytes(pb), _bytes(bf16_f32(V["value/fc1/bias"])),
            _bytes(bf16_f32(np.asarray(V["value/fc2/kernel"], np.float32).reshape(64))), _bytes(bf16_f32(V["value/fc2/bias"]))]
    return out
