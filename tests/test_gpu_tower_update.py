"""The bf16 tower's weights, packed by the device packers through either way in — the host setters (af_tower_set_block / _set_stem /
_set_heads / _set_dense: staged copies, one block or one range of the ends kernel each) and af_tower_update_device (device
tensors, in place) — must be the bytes oracle/tower_pack.py specifies (numpy, tied to the former host packers' bytes by
tests/test_tower_pack_cpu.py) in every buffer of HipTower.debug_weights(); a setter must write its own group's buffers and no
other; and the update must be what the header says it is: stream-ordered launches only, so a forward queued before it sees the
old weights, one queued behind it the new ones, a graph captured before it — or before a host setter — replays with the new
weights and [update; forward] can itself be captured.  Two blocks throughout: a packer that mixes up blocks is caught.

Weight sets are Glorot-like random with non-zero biases, all tensors distinct, and carry in every tensor (as far as it has
room) the fp32 values on which a bf16 conversion can go wrong: exact ties that round down to an even and up from an odd
mantissa, both signs; +0 and -0; a denormal (1e-40); and — except in the sets a forward runs on — +-3.39e38 (the largest finite
bf16 after rounding), +-3.4e38 (inf after rounding) and, in the kernels, four NaNs."""
import ctypes
import functools

import numpy as np
import pytest

import tower_gpu
from tower_gpu import same_bits

pytestmark = pytest.mark.gpu

S, W, BLOCKS, MAXB = 11, 128, 2, 32
NBUF = 4 * BLOCKS + 12
planes = functools.partial(tower_gpu.planes, S=S)    # random-stone positions [n, 3, 11, 11]


def _f32(bits):
    return np.array(bits, np.uint32).view(np.float32)


# ties: low half exactly 0x8000; upper half even (stays) / odd (rounds up to the next even), and their negatives
# (0x3DFF8000: the round-up carries into the exponent)
_FINITE_SPECIALS = np.concatenate([_f32([0x3F808000, 0x3F818000, 0x80000000]), np.array([1e-40], np.float32),
                                   _f32([0x00000000, 0xBF808000, 0xBF818000, 0x3DFF8000, 0x3F7E8000]), np.array([-1e-40], np.float32)])
# +-3.39e38 lies between the largest finite bf16 (3.3895e38) and the midpoint to 2^128 (3.3961e38): it rounds to that largest
# finite value, not to inf; +-3.4e38 lies above the midpoint and does overflow to inf.  Both pairs are planted.
_HUGE_SPECIALS = np.array([3.39e38, -3.39e38, 3.4e38, -3.4e38], np.float32)
# NaNs, both signs: two quiet ones, and two whose payload lies in the low half only — rounding those like numbers would carry
# into +-inf.  Planted in tensors of two or more dimensions only: a bias is added (b2 = c2_b + res_b), and which payload an add
# of NaNs returns is the adder's business, not the packer's.
_NAN_SPECIALS = _f32([0x7FC00001, 0xFFC00000, 0x7F800001, 0xFF80FFFF])


def weight_set(seed, finite, blocks=BLOCKS):
    """{name: float32 array} for a tower of `blocks` blocks (2 unless said).  The specials sit at the same flat positions of every tensor (so b2 = c2_b + res_b
    never adds infinities of opposite sign); a tensor shorter than the list takes its head.  Without `finite`, kernels carry
    the NaNs behind the rest."""
    from alphafive_amd import network_deep
    rng = np.random.default_rng(seed)
    specials = _FINITE_SPECIALS if finite else np.concatenate([_FINITE_SPECIALS[:4], _HUGE_SPECIALS, _FINITE_SPECIALS[4:]])
    out = {}
    for name, shape in network_deep.variable_shapes(S, blocks, W).items():
        if len(shape) == 1:
            a = rng.standard_normal(shape) * 0.1
        else:
            rf = int(np.prod(shape[2:])) if len(shape) == 4 else 1
            fan_in, fan_out = (shape[1] * rf, shape[0] * rf) if len(shape) == 4 else (shape[0], shape[1])
            a = (rng.random(shape) * 2 - 1) * np.sqrt(6.0 / (fan_in + fan_out))
        a = np.ascontiguousarray(a, np.float32)
        flat = a.reshape(-1)
        mine = specials if finite or len(shape) == 1 else np.concatenate([specials, _NAN_SPECIALS])
        n = min(flat.size, mine.size)
        flat[:n] = mine[:n]
        out[name] = a
    return out


def host_tower(V, dense=True, max_batch=MAXB, blocks=BLOCKS):
    """A fresh handle that got V through the host setters."""
    import torch
    from alphafive_amd import tower_hip
    t = lambda n: torch.from_numpy(V[n])  # noqa: E731
    pair = lambda n: (t(n + "/kernel"), t(n + "/bias"))  # noqa: E731
    blocks = [dict(c1=pair("tower/block%d_conv1" % b), c2=pair("tower/block%d_conv2" % b), res=pair("tower/block%d_res" % b))
              for b in range(blocks)]
    return tower_hip.HipTower(blocks, S, W, max_batch, "cuda:0", stem=pair("stem"), vconv=pair("value/conv"), pconv=pair("policy/conv"),
                              dense=_dense(V) if dense else None)


def _dense(V):
    import torch
    return tuple(torch.from_numpy(V[n]) for n in ("value/fc1/kernel", "value/fc1/bias", "value/fc2/kernel", "value/fc2/bias",
                                                   "policy/fc/kernel", "policy/fc/bias"))


def host_set(tw, V, stem=False, heads=False, dense=False, blocks=()):
    """The named host setters of the handle, with V's tensors."""
    import torch
    pair = lambda n: (torch.from_numpy(V[n + "/kernel"]), torch.from_numpy(V[n + "/bias"]))  # noqa: E731
    for b in blocks:
        tw.set_block(b, dict(c1=pair("tower/block%d_conv1" % b), c2=pair("tower/block%d_conv2" % b), res=pair("tower/block%d_res" % b)))
    if stem:
        tw.set_stem(pair("stem"))
    if heads:
        tw.set_heads(pair("value/conv"), pair("policy/conv"))
    if dense:
        tw.set_dense(_dense(V))


def assert_buffers(got, want, what):
    assert len(got) == len(want)
    for i, (x, y) in enumerate(zip(got, want)):
        assert x.size == y.size and x.size > 0, "%s: buffer %d has %d bytes, expected %d" % (what, i, x.size, y.size)
        bad = np.flatnonzero(x != y)
        assert bad.size == 0, "%s: buffer %d (%d bytes): %d bytes differ, first at %d" % (what, i, x.size, bad.size, bad[0])


def on_device(V):
    import torch
    return {k: torch.from_numpy(v).cuda() for k, v in V.items()}


def forward(tw, x):
    """DeepResNet.eval_hip over the handle: stem -> tower -> heads -> dense; clones of (policy, value)."""
    from alphafive_amd.network_deep import DeepResNet
    net = DeepResNet.__new__(DeepResNet)
    net._tower = tw
    p, v = net.eval_hip(x)
    return p.clone(), v.clone()


@pytest.fixture(scope="module")
def sets():
    """The weight sets of this module, made once: V (with infinities) and the finite V0, V1, V2."""
    return dict(V=weight_set(10, False), U=weight_set(11, True), V0=weight_set(20, True), V1=weight_set(21, True), V2=weight_set(22, True))


@pytest.fixture(scope="module")
def packed(sets):
    """oracle.tower_pack.pack_reference of the sets the byte comparisons use, made once."""
    from oracle.tower_pack import pack_reference
    return {k: pack_reference(sets[k], BLOCKS) for k in ("V", "V0", "V1")}


@pytest.fixture(scope="module")
def refs(sets):
    """Outputs of fresh host-set handles on the 32 positions, per finite weight set."""
    import torch
    x = planes(MAXB)
    out = {}
    for k in ("V0", "V1", "V2"):
        tw = host_tower(sets[k])
        out[k] = forward(tw, x)
        torch.cuda.synchronize()
        tw.close()
    return x, out


def test_specials_are_what_they_claim():
    """The generator's planted values: ties in both directions, signed zeros, denormals, values that overflow to inf."""
    bits = _FINITE_SPECIALS.view(np.uint32)
    assert sum(1 for b in bits if b & 0xFFFF == 0x8000 and (b >> 16) & 1 == 0) >= 2 and sum(1 for b in bits if b & 0xFFFF == 0x8000 and (b >> 16) & 1) >= 2
    assert 0x80000000 in bits and 0 in bits and any(0 < (b & 0x7FFFFFFF) < 0x00800000 for b in bits)
    huge = _HUGE_SPECIALS.view(np.uint32) & 0x7FFFFFFF
    assert np.isfinite(_FINITE_SPECIALS).all() and np.isfinite(_HUGE_SPECIALS).all() and (huge >> 16 == 0x7F7F).all()
    assert (huge[:2] & 0xFFFF < 0x8000).all() and (huge[2:] & 0xFFFF > 0x8000).all()        # 3.39e38 stays finite, 3.4e38 overflows
    nans = _NAN_SPECIALS.view(np.uint32)
    assert np.isnan(_NAN_SPECIALS).all() and sorted(int(b) >> 31 for b in nans) == [0, 0, 1, 1]
    assert sum(1 for b in nans if b & 0x7FFF0000 == 0x7F800000) == 2       # the payload in the low half only: rounded like a number, +-inf
    V = weight_set(10, False)
    for name, v in V.items():                                              # NaNs in every kernel, in no bias, and in no finite set
        assert np.isnan(v).sum() == (4 if v.ndim > 1 else 0), name
        assert set(v.reshape(-1)[np.isnan(v.reshape(-1))].view(np.uint32).tolist()) == (set(nans.tolist()) if v.ndim > 1 else set()), name
    assert not any(np.isnan(v).any() for v in weight_set(20, True).values())
    assert len(V) == 12 + 6 * BLOCKS and all(v.reshape(-1)[0].view(np.uint32) == 0x3F808000 for v in V.values())
    assert not np.array_equal(V["tower/block0_conv1/kernel"], V["tower/block1_conv1/kernel"])
    assert not np.array_equal(V["tower/block0_conv2/bias"], V["tower/block1_conv2/bias"])


def test_device_packers_write_the_host_setters_bytes(sets, packed):
    """Handle A through the host setters, handle B through load_device: both hold the specification's bytes."""
    import torch
    A, B = host_tower(sets["V"]), host_tower(sets["U"])
    try:
        before = B.debug_weights()
        B.load_device(on_device(sets["V"]))
        a, b = A.debug_weights(), B.debug_weights()
        assert len(a) == len(b) == len(packed["V"]) == NBUF
        changed = sum(1 for x, y in zip(before, b) if not np.array_equal(x, y))
        assert changed > 4 * BLOCKS + 6, changed                       # not two untouched copies
        assert_buffers(a, packed["V"], "host setters")
        assert_buffers(b, packed["V"], "load_device")
        w1 = a[0].view(np.uint16)
        assert (w1 == 0x7F80).any() and (w1 == 0xFF80).any() and (w1 == 0x8000).any()     # inf both ways and -0 made it into the fragments
        assert (w1 == 0x7F7F).any() and (w1 == 0xFF7F).any() and (w1 == 0x3E00).any()     # 3.39e38 did not overflow; the carry into the exponent
        assert (w1 == 0x7FC0).any() and (w1 == 0xFFC0).any()                              # NaNs stayed NaNs, signs kept ...
        assert np.count_nonzero(w1 == 0x7F80) == 1 and np.count_nonzero(w1 == 0xFF80) == 1    # ... none turned into a second +-inf
        assert a[4 * BLOCKS + 11].size == 4                            # dense_vb2 is a device word
        torch.cuda.synchronize()
    finally:
        A.close()
        B.close()


@pytest.mark.parametrize("blocks", [8, 9])
def test_device_packers_write_the_host_setters_bytes_at_full_depth(blocks):
    """The depth the feature exists for — 8 blocks (BASELINE configs[4]): every block slot of one pack launch filled — and 9, which
    takes a second launch for the block past the eighth.  Same byte-for-byte comparison as above."""
    import torch
    from oracle.tower_pack import pack_reference
    V = weight_set(30 + blocks, False, blocks)
    want = pack_reference(V, blocks)
    A, B = host_tower(V, max_batch=1, blocks=blocks), host_tower(weight_set(40 + blocks, True, blocks), max_batch=1, blocks=blocks)
    try:
        before = B.debug_weights()
        B.load_device(on_device(V))
        a, b = A.debug_weights(), B.debug_weights()
        assert len(a) == len(b) == len(want) == 4 * blocks + 12
        assert all(not np.array_equal(x, y) for x, y in zip(before[:4 * blocks], b[:4 * blocks]))      # every block's four buffers were written
        assert_buffers(a, want, "host setters")
        assert_buffers(b, want, "load_device")
        for i in range(4):                               # ... each with its own block's weights
            assert len({a[4 * blk + i].tobytes() for blk in range(blocks)}) == blocks
        torch.cuda.synchronize()
    finally:
        A.close()
        B.close()


def test_a_host_setter_writes_its_own_buffers_only(sets, packed):
    """Each setter launches one block or one range of the ends kernel, with the other groups' source pointers null: on a fully
    set handle holding V0, a setter given V1's tensors must leave its own buffers as V1 packs and every other buffer as V0 does
    — a range one thread too long or too short shows in the neighbour's first or its own last word."""
    E = 4 * BLOCKS                                                  # stem_w, stem_b | heads_w, heads_b, heads_a, heads_b32 | dense_*
    steps = [("set_heads", dict(heads=True), range(E + 2, E + 6)), ("set_stem", dict(stem=True), range(E, E + 2)),
             ("set_dense", dict(dense=True), range(E + 6, E + 12)), ("set_block(1)", dict(blocks=(1,)), range(4, 8))]
    tw = host_tower(sets["V0"])
    try:
        want = list(packed["V0"])
        assert_buffers(tw.debug_weights(), want, "V0")
        for what, groups, own in steps:
            host_set(tw, sets["V1"], **groups)
            for i in own:
                # the step has something to show (dense_vb2 is one word, the special every tensor starts with, in both sets)
                assert want[i].size == 4 or not np.array_equal(want[i], packed["V1"][i]), i
                want[i] = packed["V1"][i]
            assert_buffers(tw.debug_weights(), want, what)
    finally:
        tw.close()


def test_captured_forward_sees_later_host_setters(sets, refs):
    """The host setters write into the buffers the handle has owned since it was created: a graph captured over it replays with
    the weights they gave."""
    import torch
    x, out = refs
    tw = host_tower(sets["V0"])
    try:
        forward(tw, x)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, capture_error_mode="thread_local"):
            tw.stem(x)
            tw.forward(MAXB)
            tw.heads(MAXB)
            tw.dense(MAXB)
        g.replay()
        torch.cuda.synchronize()
        assert same_bits((tw.policy, tw.value), out["V0"])
        host_set(tw, sets["V1"], stem=True, heads=True, dense=True, blocks=range(BLOCKS))
        g.replay()
        torch.cuda.synchronize()
        assert same_bits((tw.policy, tw.value), out["V1"])
        del g
    finally:
        tw.close()


@pytest.mark.parametrize("engine", [3, 0], ids=["default", "tune(3, 0)"])
def test_forward_after_device_update_is_the_host_set_forward(sets, refs, engine):
    from alphafive_amd import tower_hip
    x, out = refs
    B = host_tower(sets["V0"])
    try:
        B.load_device(on_device(sets["V1"]))
        A = host_tower(sets["V1"])
        try:
            tower_hip.tune(3, engine)
            for n in (32, 9, 1):
                pa, pb = forward(A, x[:n].contiguous()), forward(B, x[:n].contiguous())
                assert same_bits(pa, pb), n
                if engine == 3:
                    assert same_bits(pb, (out["V1"][0][:n], out["V1"][1][:n])), n
        finally:
            tower_hip.tune(3, 3)
            A.close()
    finally:
        B.close()


def test_update_is_ordered_on_its_stream(sets, refs):
    import torch
    x, out = refs
    tw = host_tower(sets["V0"])
    v1 = on_device(sets["V1"])
    st = torch.cuda.Stream()
    try:
        st.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(st):                    # back to back, no wait between
            r0 = forward(tw, x)
            tw.load_device(v1)
            r1 = forward(tw, x)
        st.synchronize()
        assert same_bits(r0, out["V0"]) and same_bits(r1, out["V1"])
        assert not torch.equal(r0[0], r1[0]) and not torch.equal(r0[1], r1[1])
    finally:
        tw.close()


def test_captured_forward_sees_a_later_update(sets, refs):
    """stem -> tower -> heads -> dense captured once; replayed after load_device it must give the new weights' outputs: every
    weight-derived value is read from a buffer that keeps its address, none is a by-value kernel argument."""
    import torch
    x, out = refs
    tw = host_tower(sets["V0"])
    try:
        forward(tw, x)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, capture_error_mode="thread_local"):
            tw.stem(x)
            tw.forward(MAXB)
            tw.heads(MAXB)
            tw.dense(MAXB)
        g.replay()
        torch.cuda.synchronize()
        assert same_bits((tw.policy, tw.value), out["V0"])
        tw.load_device(on_device(sets["V1"]))
        g.replay()
        torch.cuda.synchronize()
        assert same_bits((tw.policy, tw.value), out["V1"])
        del g
    finally:
        tw.close()


def test_update_and_forward_captured_together(sets, refs):
    """[load_device(src); forward] as one graph, replayed over source tensors overwritten in place."""
    import torch
    x, out = refs
    tw = host_tower(sets["V0"])
    try:
        src = on_device(sets["V1"])
        tw.load_device(src)
        forward(tw, x)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, capture_error_mode="thread_local"):
            tw.load_device(src)
            tw.stem(x)
            tw.forward(MAXB)
            tw.heads(MAXB)
            tw.dense(MAXB)
        g.replay()
        torch.cuda.synchronize()
        assert same_bits((tw.policy, tw.value), out["V1"])
        for k, t in src.items():
            t.copy_(torch.from_numpy(sets["V2"][k]))
        g.replay()
        torch.cuda.synchronize()
        assert same_bits((tw.policy, tw.value), out["V2"])
        del g
    finally:
        tw.close()


def test_refusals_change_nothing(sets, refs):
    import torch
    from alphafive_amd import tower_hip
    x, out = refs
    ERR_ARG, ERR_STATE = -1, -3
    tw = host_tower(sets["V0"])
    nodense = host_tower(sets["V0"], dense=False)
    try:
        v1 = on_device(sets["V1"])
        names = tower_hip.update_names(BLOCKS)
        before = tw.debug_weights()

        def unchanged():
            now = tw.debug_weights()
            return all(np.array_equal(a, b) for a, b in zip(before, now)) and same_bits(forward(tw, x), out["V0"])

        # a missing tensor: by name, as a short list, and — at the C ABI — a short table and a null entry
        short = {k: v for k, v in v1.items() if k != "tower/block1_conv2/kernel"}
        with pytest.raises(tower_hip.TowerError):
            tw.load_device(short)
        with pytest.raises(tower_hip.TowerError):
            tw.load_device([v1[k] for k in names[:-1]])
        n = len(names)
        ptrs = (ctypes.c_void_p * n)(*[v1[k].data_ptr() for k in names])
        counts = (ctypes.c_int64 * n)(*[v1[k].numel() for k in names])
        L = tower_hip.lib()
        assert L.af_tower_update_device(tw._h, None, ptrs, counts, n - 1) == ERR_ARG
        assert L.af_tower_update_device(tw._h, None, None, counts, n) == ERR_ARG
        assert L.af_tower_update_device(None, None, ptrs, counts, n) == ERR_ARG
        holed = (ctypes.c_void_p * n)(*[v1[k].data_ptr() for k in names])
        holed[9] = None
        assert L.af_tower_update_device(tw._h, None, holed, counts, n) == ERR_ARG
        assert unchanged()
        # a wrong-sized tensor: the last of the table (a checker that launches as it goes would have packed the rest by then), the first, one in between
        for name in ("policy/fc/bias", "stem/kernel", "tower/block1_res/kernel"):
            wrong = dict(v1)
            wrong[name] = torch.zeros(v1[name].numel() + 1, device="cuda")
            with pytest.raises(tower_hip.TowerError) as e:
                tw.load_device(wrong)
            assert e.value.code == ERR_ARG
        for bad in (v1["stem/bias"].double(), v1["stem/kernel"].permute(0, 1, 3, 2), v1["stem/bias"].cpu()):
            wrong = dict(v1)
            wrong["stem/bias" if bad.dim() == 1 else "stem/kernel"] = bad
            with pytest.raises(tower_hip.TowerError):
                tw.load_device(wrong)
        assert unchanged()
        # a handle whose dense layers were never set has no buffers to write into
        nd_before = nodense.debug_weights()
        assert [i for i, b in enumerate(nd_before) if b is None] == list(range(4 * BLOCKS + 6, NBUF))
        with pytest.raises(tower_hip.TowerError) as e:
            nodense.load_device(v1)
        assert e.value.code == ERR_STATE
        assert all((a is None and b is None) or np.array_equal(a, b) for a, b in zip(nd_before, nodense.debug_weights()))
        assert L.af_tower_debug_weights(tw._h, NBUF, None, 0) == ERR_ARG and L.af_tower_debug_weights(tw._h, -1, None, 0) == ERR_ARG
        assert L.af_tower_debug_weights(tw._h, 0, None, 0) == 4 * 72 * 64 * 16
        # a good update then goes through ...
        tw.load_device(v1)
        assert same_bits(forward(tw, x), out["V1"])
        # ... and the host setters on the same handle afterwards restore the first forward
        V0 = sets["V0"]
        t = lambda k: torch.from_numpy(V0[k])  # noqa: E731
        pair = lambda k: (t(k + "/kernel"), t(k + "/bias"))  # noqa: E731
        torch.cuda.synchronize()
        for b in range(BLOCKS):
            tw.set_block(b, dict(c1=pair("tower/block%d_conv1" % b), c2=pair("tower/block%d_conv2" % b), res=pair("tower/block%d_res" % b)))
        tw.set_stem(pair("stem"))
        tw.set_heads(pair("value/conv"), pair("policy/conv"))
        tw.set_dense(_dense(V0))
        assert unchanged()
    finally:
        tw.close()
        nodense.close()


def test_set_variables_repacks_the_tower_in_place(sets, monkeypatch):
    """DeepResNet.set_variables, the host path, on a net with a hip backend: the host setters on the tower it has — no new handle,
    the engine's bound outputs stay bound — and the bits of a fresh net that got the same weights before select_backend."""
    import torch
    from alphafive_amd import tower_hip
    from alphafive_amd.network_deep import DeepResNet
    made = []
    real_init = tower_hip.HipTower.__init__

    def counting_init(self, *a, **kw):
        made.append(self)
        real_init(self, *a, **kw)
    monkeypatch.setattr(tower_hip.HipTower, "__init__", counting_init)

    deep = DeepResNet(S, blocks=BLOCKS, width=W, device="cuda", seed=7)
    pv = deep.select_backend("hip", MAXB)
    first = deep._tower
    policy, value = torch.zeros((MAXB, S * S), device="cuda"), torch.zeros(MAXB, device="cuda")
    pv.bind_outputs(policy, value)
    x = planes(MAXB)
    before = tuple(t.clone() for t in pv(x))
    version = pv.weights_version()
    try:
        deep.set_variables(sets["V1"])
        assert deep._tower is first and len(made) == 1                      # re-packed in place: no new handle
        assert pv.weights_version() == version + 1
        assert first.policy is policy and first.value is value
        policy.zero_()
        value.zero_()
        p, v = pv(x)
        assert p.data_ptr() == policy.data_ptr() and v.data_ptr() == value.data_ptr()
        got = (policy.clone(), value.clone())
        assert not torch.equal(got[0], before[0]) and not torch.equal(got[1], before[1])       # the outputs move
        fresh = DeepResNet(S, blocks=BLOCKS, width=W, device="cuda", seed=99)
        fresh.set_variables(sets["V1"])
        assert len(made) == 1                                               # (no backend yet: nothing to re-pack)
        try:
            ref = tuple(t.clone() for t in fresh.select_backend("hip", MAXB)(x))
        finally:
            if getattr(fresh, "_tower", None) is not None:
                fresh._tower.close()
        assert same_bits(got, ref)
    finally:
        first.close()


def test_live_trainer_drives_the_evaluator(monkeypatch):
    """A deep Trainer on the device, three steps; after each the evaluator takes the parameters without the host and must give the
    bits of a fresh DeepResNet that got trainer.variables() through the host path."""
    import torch
    from alphafive_amd import tower_hip, train
    from alphafive_amd.network_deep import DeepResNet
    from test_gpu_realnet import _assert_no_worse_than_torch_bf16
    made = []
    real_init = tower_hip.HipTower.__init__

    def counting_init(self, *a, **kw):
        made.append(self)
        real_init(self, *a, **kw)
    monkeypatch.setattr(tower_hip.HipTower, "__init__", counting_init)

    deep = DeepResNet(S, blocks=BLOCKS, width=W, device="cuda", seed=7)
    pv = deep.select_backend("hip", MAXB)
    first = deep._tower
    assert len(made) == 1
    trainer = train.Trainer(deep.variables, S, device="cuda", forward=train.forward_train_deep, shapes=deep.variable_shapes())
    rng = np.random.default_rng(3)
    n = 64
    boards = planes(n, seed=5)
    pi = torch.from_numpy(rng.dirichlet(np.ones(S * S) * 0.3, size=n).astype(np.float32)).cuda()
    z = torch.from_numpy(rng.choice([-1.0, 1.0], size=n).astype(np.float32)).cuda()
    w = torch.ones(n, device="cuda")
    x = planes(MAXB, seed=6)
    wide = planes(10 * MAXB, seed=8)
    last = tuple(t.clone() for t in pv(x))
    for step in range(3):
        trainer.step(boards, w, z, pi, 1e-3, metrics=False)
        version = pv.weights_version()
        count = len(made)
        deep.set_variables_device(trainer.device_variables())
        assert len(made) == count == 1 and deep._tower is first            # re-packed in place: no new handle
        assert pv.weights_version() == version + 1
        got = tuple(t.clone() for t in pv(x))
        fresh = DeepResNet(S, blocks=BLOCKS, width=W, device="cuda", seed=99)
        fresh.set_variables(trainer.variables())
        ref = tuple(t.clone() for t in fresh.select_backend("hip", MAXB)(x))
        assert same_bits(got, ref), step
        assert not torch.equal(got[0], last[0]) and not torch.equal(got[1], last[1]), step      # the outputs move
        for k, v in fresh.variables.items():                                # the net's own tensors follow ...
            assert np.array_equal(v.view(np.uint32), deep.variables[k].view(np.uint32)), k
        # ... so eval_device does, under the pair's usual bars.  Those include argmax agreement within 0.02, a fraction that at 32
        # positions would allow no single flip between two near-equal cells of a barely trained policy (1 / 32 > 0.02): the bars are
        # applied as tests/test_gpu_realnet.py applies them, on ~300 positions — here ten batches of 32 through the same evaluator
        pw, vw = zip(*[tuple(t.clone() for t in pv(wide[i:i + MAXB].contiguous())) for i in range(0, wide.shape[0], MAXB)])
        _assert_no_worse_than_torch_bf16(deep, wide, torch.cat(pw), torch.cat(vw))
        fresh._tower.close()
        made.pop()
        last = got
    first.close()
