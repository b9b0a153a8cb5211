"""BASELINE configs[4]: a deeper policy/value net — N residual blocks of the reference's block type
(network.py:52-56: 1x1 projection || 3x3+ELU -> 3x3, add, ELU) at constant width, the reference's two heads,
evaluated in bf16.  The whole forward runs on the hand-written MFMA kernels of csrc/af_tower_bf16.hip
(`select_backend("hip")`, the bench default): 5x5 stem, residual tower (99 % of the FLOPs), the heads' 1x1
convolutions and the three dense layers + softmax.  `eval_device` is the
all-PyTorch reference path.  Performance-only configuration (no checkpoint exists for
it, random init, no bit parity); it plugs into SelfPlayEngine through the same
planes[G,3,S,S] -> (prob[G,C], value[G]) evaluator seam as the fp32 net.
"""
import collections
import threading
import weakref

import numpy as np
import torch
import torch.nn.functional as F


def variable_shapes(board_size, blocks=8, width=128):
    """{name: shape}, ordered as af_tower_update_device takes the tensors (include/af_tower_bf16.h; tower_hip.update_names):
    kernels OIHW, dense layers [in][out].  Every bias name contains "bias" (train.loss_terms leaves those out of its L2 term)."""
    C, w = board_size * board_size, width
    shapes = collections.OrderedDict()
    shapes["stem/kernel"], shapes["stem/bias"] = (w, 3, 5, 5), (w,)
    for b in range(blocks):
        for layer, k in (("conv1", 3), ("conv2", 3), ("res", 1)):
            shapes["tower/block%d_%s/kernel" % (b, layer)] = (w, w, k, k)
            shapes["tower/block%d_%s/bias" % (b, layer)] = (w,)
    for layer, kshape in (("value/conv", (4, w, 1, 1)), ("policy/conv", (16, w, 1, 1)), ("value/fc1", (4 * C, 64)),
                          ("value/fc2", (64, 1)), ("policy/fc", (16 * C, C))):
        shapes[layer + "/kernel"], shapes[layer + "/bias"] = kshape, (kshape[0],) if len(kshape) == 4 else (kshape[1],)
    return shapes


class _HipEvaluator(object):
    """planes -> (prob, value) on the hand-written kernels (the tower's precision, bf16 or int8, picks the blocks' kernels in
    eval_hip, the batch picks their form: tile-parallel or persistent, the same bits); bind_outputs lets the engine own the result tensors.  An evaluator
    owns its tower — handle, packed weights, activation buffers, bound outputs — so every consumer of a net (a Player, a self-play
    engine, an arena) has one of its own; the net re-packs all of them when its weights change (DeepResNet._towers)."""

    def __init__(self, net, tower):
        self.net, self.tower = net, tower

    def __call__(self, x):
        return self.net.eval_hip(x, self.tower)

    def eval(self, inputs):
        """DeepResNet.eval's contract on this evaluator's tower (its precision, its scales): numpy float32 [B,3,S,S] -> numpy
        (prob [B,S*S], value [B]), copied out.  B <= the evaluator's max_batch.  Player(pv_fn=ev.eval) recognises it like
        DeepResNet.eval and plays on an evaluator of its own with this one's precision and scales."""
        x = torch.from_numpy(np.ascontiguousarray(inputs, np.float32))
        p, v = self(x.to(self.net.device))
        return p.cpu().numpy().copy(), v.cpu().numpy().copy()     # (the tower's output tensors are overwritten by the next call)

    def bind_outputs(self, policy, value):
        if policy.shape[0] >= self.tower.max_batch:
            self.tower.bind_outputs(policy, value)

    def weights_version(self):
        """What a captured graph of this evaluator is keyed on (SelfPlayEngine.run_ticks_graph): the net's pack counter, which
        select_backend() and every re-pack of the towers' weights, from the host or on the device, bump."""
        return self.net._pack_version

    def close(self):
        """Releases the tower and leaves the net's registry.  The net's primary evaluator (select_backend) takes net._tower along."""
        self.net._evaluators.discard(self)
        if getattr(self.net, "_tower", None) is self.tower:
            self.net._tower = None
        if self.tower is not None:
            self.tower.close()


class DeepResNet(object):
    def __init__(self, board_size, blocks=8, width=128, device="cuda", dtype=torch.bfloat16, seed=0):
        self.board_size, self.blocks, self.width = board_size, blocks, width
        self.device, self.dtype = torch.device(device), dtype
        g = torch.Generator().manual_seed(seed)
        C = board_size * board_size

        def glorot(*shape):                      # OIHW / [in,out], tf.layers default initialiser
            rf = int(np.prod(shape[2:])) if len(shape) == 4 else 1
            fan_in, fan_out = (shape[1] * rf, shape[0] * rf) if len(shape) == 4 else (shape[0], shape[1])
            lim = float(np.sqrt(6.0 / (fan_in + fan_out)))
            return ((torch.rand(shape, generator=g) * 2 - 1) * lim).to(self.device, dtype)

        z = lambda n: torch.zeros(n, device=self.device, dtype=dtype)  # noqa: E731
        self.stem = (glorot(width, 3, 5, 5), z(width))
        self.tower = [dict(res=(glorot(width, width, 1, 1), z(width)), c1=(glorot(width, width, 3, 3), z(width)),
                           c2=(glorot(width, width, 3, 3), z(width))) for _ in range(blocks)]
        self.vconv, self.pconv = (glorot(4, width, 1, 1), z(4)), (glorot(16, width, 1, 1), z(16))
        self.vfc1, self.vfc2 = (glorot(4 * C, 64), z(64)), (glorot(64, 1), z(1))
        self.pfc = (glorot(16 * C, C), z(C))
        self._pack_version = 0
        self._evaluators = weakref.WeakSet()     # live evaluators: an evaluator dropped without close() frees its tower by itself
        self._eval_lock = threading.Lock()       # eval(): one evaluator of the net's own, its outputs copied out before the next call
        self._own_eval = None

    @property
    def version(self):
        """The pack counter: moves with every weight update (what Player._weights_version keys its captured graph on)."""
        return self._pack_version

    def _towers(self):
        """Every live tower over this net: the primary one (select_backend) and those of the evaluators handed out."""
        out = []
        for tw in [getattr(self, "_tower", None)] + [e.tower for e in list(getattr(self, "_evaluators", ()))]:
            if tw is not None and tw._h and all(tw is not o for o in out):
                out.append(tw)
        return out

    # ---- weights by name ----
    def variable_shapes(self):
        return variable_shapes(self.board_size, self.blocks, self.width)

    def _named(self):
        """name -> (holder, key, index) of the tensor behind it: self.stem / self.tower[b][...] / the heads stay the storage
        (callers replace those tuples directly), so a name is resolved when it is used."""
        out = collections.OrderedDict()
        out["stem/kernel"], out["stem/bias"] = (self.__dict__, "stem", 0), (self.__dict__, "stem", 1)
        for b, blk in enumerate(self.tower):
            for layer, key in (("conv1", "c1"), ("conv2", "c2"), ("res", "res")):
                out["tower/block%d_%s/kernel" % (b, layer)] = (blk, key, 0)
                out["tower/block%d_%s/bias" % (b, layer)] = (blk, key, 1)
        for layer, key in (("value/conv", "vconv"), ("policy/conv", "pconv"), ("value/fc1", "vfc1"), ("value/fc2", "vfc2"),
                           ("policy/fc", "pfc")):
            out[layer + "/kernel"], out[layer + "/bias"] = (self.__dict__, key, 0), (self.__dict__, key, 1)
        return out

    def _tensor(self, ref):
        holder, key, i = ref
        return holder[key][i]

    @property
    def variables(self):
        """{name: float32 host array} in variable_shapes() order: the values the evaluators use (bf16-rounded on a bf16 net)."""
        return collections.OrderedDict((k, self._tensor(r).detach().float().cpu().numpy().copy()) for k, r in self._named().items())

    def _checked(self, variables):
        shapes = self.variable_shapes()
        for name, shape in shapes.items():
            if name not in variables:
                raise KeyError("missing variable %s" % name)
            if tuple(variables[name].shape) != tuple(shape):
                raise ValueError("variable %s has shape %s, expected %s" % (name, tuple(variables[name].shape), tuple(shape)))
        return shapes

    def set_variables(self, variables):
        """The host path: values (arrays or tensors, variable_shapes() names and shapes) -> the net's tensors in self.dtype; if a hip
        backend is selected the host setters re-pack them into the tower it has, in place (they synchronise the device): the same
        handle, buffers and bound outputs, so the evaluator handed out and a graph captured over it stay valid."""
        new = {}
        for name in self._checked(variables):
            v = variables[name]
            v = v.detach() if torch.is_tensor(v) else torch.from_numpy(np.ascontiguousarray(v, np.float32))
            new[name] = v.to(device=self.device, dtype=self.dtype).contiguous()
        for name, (holder, key, i) in self._named().items():
            holder[key] = tuple(new[name] if k == i else t for k, t in enumerate(holder[key]))
        for tower in self._towers():
            for b, blk in enumerate(self.tower):
                tower.set_block(b, blk)
            tower.set_stem(self.stem)
            tower.set_heads(self.vconv, self.pconv)
            tower.set_dense(self.vfc1 + self.vfc2 + self.pfc)
        self._pack_version = getattr(self, "_pack_version", 0) + 1

    @torch.no_grad()
    def set_variables_device(self, tensors, calibrate_on=None, margin=1.0):
        """set_variables without the host: `tensors` maps every name to a float32 tensor (a deep Trainer's parameters:
        train.Trainer.device_variables()).  With a hip backend selected the net's own tensors take the values in self.dtype in place
        (one copy_ per variable, so eval_device follows), and HipTower.load_device packs in place, stream-ordered, with no wait:
        the kernels straight from the caller's tensors — the packed buffers are the snapshot, no weight tensor is cloned — and the
        biases from small fp32 temporaries made of the net's rounded copies.  The tower adds the stem's, blocks' and head
        convolutions' biases in fp32 as given, so handing over the rounded values is what makes host path and device path pack
        the same values and give the same bits.  A cpu net, or one without a hip backend, does what set_variables does.

        calibrate_on: planes (float32 [B,3,11,11] on the device) to re-calibrate the int8 evaluators' activation scales on, behind
        load_device on the same stream (calibrate_int8_device without a second version bump): the whole hand-over stays launches
        only, and an int8 evaluator follows the new net with scales measured on it.  None (default): the scales stay as they are —
        today's behaviour and bits.  The host path ignores it (there is no tower to calibrate)."""
        towers = self._towers()
        if self.device.type != "cuda" or not towers:
            self.set_variables(tensors)
            return
        if calibrate_on is not None:
            from . import tower_hip
            tower_hip.check_calibration("int8", self.board_size, margin)     # refused before anything is written
        src = collections.OrderedDict()
        for name in self._checked(tensors):
            src[name] = tensors[name].detach().to(device=self.device, dtype=torch.float32).contiguous()   # no copy if it already is
        for name, ref in self._named().items():
            own = self._tensor(ref)
            own.copy_(src[name])
            if name.endswith("bias"):
                src[name] = own.float()
        for tower in towers:
            tower.load_device(src)
        if calibrate_on is not None:
            for tower in towers:
                if tower.precision == "int8":
                    tower.calibrate_i8(calibrate_on, margin)
        self._pack_version = getattr(self, "_pack_version", 0) + 1

    def save_npz(self, path):
        np.savez(path, **self.variables)

    def load_npz(self, path):
        with np.load(path) as z:
            self.set_variables({k: z[k] for k in z.files})

    def flops_per_position(self):
        HW, w = self.board_size ** 2, self.width
        mac = 75 * w * HW + self.blocks * (w * w + 18 * w * w) * HW + (4 + 16) * w * HW + 4 * HW * 64 + 64 + 16 * HW * HW
        return 2 * mac

    @torch.no_grad()
    def eval_device(self, x, dtype=None):
        """All-PyTorch evaluation in self.dtype (bf16), or — dtype=torch.float32 — of the SAME (bf16-valued) weights in fp32
        arithmetic with fp32 activations: the yardstick both bf16 paths' errors are measured against (tests/test_gpu_realnet.py)."""
        dt = self.dtype if dtype is None else dtype
        c = (lambda wb: (wb[0].to(dt), wb[1].to(dt)))
        B = x.shape[0]
        h = F.elu(F.conv2d(x.to(dt), *c(self.stem), padding=2))
        for blk in self.tower:
            r = F.conv2d(h, *c(blk["res"]))
            g = F.elu(F.conv2d(h, *c(blk["c1"]), padding=1))
            h = F.elu(r + F.conv2d(g, *c(blk["c2"]), padding=1))
        v = F.elu(F.conv2d(h, *c(self.vconv))).reshape(B, -1)
        v = F.elu(v @ self.vfc1[0].to(dt) + self.vfc1[1].to(dt))
        v = torch.tanh((v @ self.vfc2[0].to(dt) + self.vfc2[1].to(dt)).float() / 2).squeeze(1)
        p = F.elu(F.conv2d(h, *c(self.pconv))).reshape(B, -1)
        p = torch.softmax((p @ self.pfc[0].to(dt) + self.pfc[1].to(dt)).float(), dim=1)
        return p, v

    # ---- hand-written tower (csrc/af_tower_bf16.hip) ----
    def select_backend(self, name, max_batch, precision="bf16", act_scales=None):
        """"hip": the whole forward on the hand-written kernels (raises if libaf_tower.so is missing), the residual blocks in
        `precision` — "bf16" (default: today's kernels and bits) or "int8" with act_scales (see evaluator);
        "torch": the all-PyTorch path."""
        if name == "torch":
            return self.eval_device
        if name != "hip":
            raise ValueError(name)
        ev = self.evaluator(max_batch, precision=precision, act_scales=act_scales)   # the net's primary evaluator: its tower is what eval_hip(x) runs on
        self._pack_version = getattr(self, "_pack_version", 0) + 1
        self._tower = ev.tower
        return ev

    def evaluator(self, max_batch, precision="bf16", act_scales=None):
        """A new evaluator with a tower of its own, packed from the net's current tensors: one per consumer, so that two Players,
        or a Player and a self-play engine, share the net and not each other's buffers.  It follows set_variables /
        set_variables_device / load_npz in place until its close() (or the net's).

        precision="int8" (11x11 nets): the residual blocks run with int8 weights and int8 stored activations
        (csrc/af_tower_i8.hip, specified by alphafive_amd/tower_i8.py); stem, heads and dense layers stay bf16.  act_scales are
        the 2 * blocks activation scales of calibrate_int8.  An int8 evaluator has the two forms a bf16 one has — the tile-parallel
        kernel up to HipTower.small_batch_i8, the persistent kernels above — with the same bits (integer accumulation is exact in
        any order), so a position's bits do not depend on the batch it is evaluated in.  Weight updates
        re-quantise the weights in place like the bf16 ones; the ACTIVATION scales stay as calibrated until the caller calibrates
        again, which needs the host no more than the weights do: calibrate_int8_device(planes), or
        set_variables_device(tensors, calibrate_on=planes) in one go, measures the new net's activations on the device and installs
        the scales in place, launches only (the host route — calibrate_int8, then evaluator.tower.enable_i8(scales) — remains)."""
        from . import tower_hip, tower_i8
        tower_hip.check_precision(precision, self.board_size, act_scales)
        if precision == "int8":
            act_scales = tower_i8.check_scales(act_scales, self.blocks)
        tower = tower_hip.HipTower(self.tower, self.board_size, self.width, max_batch, self.device, stem=self.stem,
                                   vconv=self.vconv, pconv=self.pconv, dense=self.vfc1 + self.vfc2 + self.pfc,
                                   precision=precision, act_scales=act_scales)
        ev = _HipEvaluator(self, tower)
        self._evaluators.add(ev)
        return ev

    @torch.no_grad()
    def eval_hip(self, x, tower=None):
        """The whole forward on hand-written kernels: af_tower_stem -> af_tower_forward[_small] (an int8 tower:
        af_tower_forward_i8[_small]) -> af_tower_heads (the 1x1 convs) -> af_tower_dense (the three dense layers + softmax on the
        MFMA), on `tower` (default: the primary evaluator's).
        The one place that chooses the tower's form: the tile-parallel kernel up to the batch the library measured it faster at
        (HipTower.small_batch, for an int8 tower HipTower.small_batch_i8), the persistent kernels above; the bits are the same
        either way."""
        tw = self._tower if tower is None else tower
        B = x.shape[0]
        tw.stem(x.contiguous())
        if tw.precision == "int8":
            if B <= tw.small_batch_i8:
                tw.forward_i8_small(B)
            else:
                tw.forward_i8(B)
        elif B <= tw.small_batch:
            tw.forward_small(B)
        else:
            tw.forward(B)
        tw.heads(B)
        return tw.dense(B)

    @torch.no_grad()
    def calibrate_int8(self, planes, margin=1.0):
        """Activation scales for precision="int8": the fp32 torch path (eval_device's arithmetic, the net's weights in fp32) layer
        by layer over the caller's positions — planes float32 [B,3,S,S], array or tensor — on PyTorch ops only, no hand-written
        kernel.  -> float32 [2 * blocks] in tower_i8's order h_0, g_0, h_1, g_1, ...: fp32(absmax * margin / 127) of every
        block's input and mid activation over all positions (a tensor that is zero everywhere gets scale 1).  Deterministic."""
        x = planes if torch.is_tensor(planes) else torch.from_numpy(np.ascontiguousarray(planes, np.float32))
        c = (lambda wb: (wb[0].float(), wb[1].float()))
        h = F.elu(F.conv2d(x.to(self.device, torch.float32), *c(self.stem), padding=2))
        out = []
        for blk in self.tower:
            g = F.elu(F.conv2d(h, *c(blk["c1"]), padding=1))
            out += [h.abs().max(), g.abs().max()]
            h = F.elu(F.conv2d(h, *c(blk["res"])) + F.conv2d(g, *c(blk["c2"]), padding=1))
        amax = torch.stack(out).double().cpu().numpy()
        scales = (amax * float(margin) / 127.0).astype(np.float32)
        scales[scales == 0] = 1.0
        return scales

    @torch.no_grad()
    def calibrate_int8_device(self, planes, margin=1.0, evaluators=None):
        """calibrate_int8 + enable_i8 without the host (HipTower.calibrate_i8): planes float32 [B,3,11,11] on the net's device;
        every int8 evaluator of the net — or those given — measures the activations of its own bf16 kernels over them, on its own
        handle (towers are independent), turns the maxima into scales on the device and re-packs its int8 weights under them, on
        torch's current stream with no wait.  What is measured is the bf16 tower, not calibrate_int8's fp32 path
        (alphafive_amd/tower_i8.py).  Whether a tower installed its scales: evaluator.tower.calibration_status().  ValueError,
        before anything touches the GPU, for a bad margin, a 15x15 net, a bf16 evaluator among those given, or no int8 evaluator."""
        from . import tower_hip
        tower_hip.check_calibration("int8", self.board_size, margin)
        if evaluators is None:
            towers = [tw for tw in self._towers() if tw.precision == "int8"]
        else:
            towers = [ev.tower for ev in evaluators]
        if not towers:
            raise ValueError("calibrate_int8_device: the net has no int8 evaluator")
        for tw in towers:
            tower_hip.check_calibration(tw.precision, tw.S, margin)
        for tw in towers:
            tw.calibrate_i8(planes, margin)
        self._pack_version = getattr(self, "_pack_version", 0) + 1

    def eval(self, inputs):
        """network.py:90-97, as ResNet.eval: numpy float32[B,3,S,S] -> (prob[B,S*S], value[B]) numpy.  A cuda net evaluates on the
        hand-written kernels through an evaluator of its own, made at the first call (and again for a larger batch); a cpu net
        through eval_device."""
        x = torch.from_numpy(np.ascontiguousarray(inputs, np.float32))
        if self.device.type != "cuda":
            p, v = self.eval_device(x)
            return p.float().numpy(), v.float().numpy()
        with self._eval_lock:
            ev = self._own_eval
            if ev is None or ev.tower is None or not ev.tower._h or ev.tower.max_batch < x.shape[0]:
                if ev is not None:
                    ev.close()
                ev = self._own_eval = self.evaluator(max(int(x.shape[0]), 1))
            p, v = ev(x.to(self.device))
            return p.cpu().numpy(), v.cpu().numpy()

    def close(self):
        """Closes every evaluator the net handed out (their towers: handles, packed weights, buffers), the primary one included."""
        for ev in list(self._evaluators):
            ev.close()
        self._own_eval = None
        tower = getattr(self, "_tower", None)
        if tower is not None:
            tower.close()
            self._tower = None
        self._pack_version = getattr(self, "_pack_version", 0) + 1      # a graph captured over released buffers must not replay

    @torch.no_grad()
    def eval_hip_torch_dense(self, x):
        """A/B reference for af_tower_dense: the same pipeline with the dense layers on PyTorch ops."""
        B, tw = x.shape[0], self._tower
        tw.stem(x.contiguous())
        tw.forward(B)
        vin, pin = tw.heads(B)
        v = F.elu(vin @ self.vfc1[0] + self.vfc1[1])
        v = torch.tanh((v @ self.vfc2[0] + self.vfc2[1]).float() / 2).squeeze(1)
        p = torch.softmax((pin @ self.pfc[0] + self.pfc[1]).float(), dim=1)
        return p, v

    @torch.no_grad()
    def eval_hip_torch_ends(self, x):
        """The hand-written tower between PyTorch stem and heads (A/B reference for the stem / heads kernels)."""
        B, tw = x.shape[0], self._tower
        tw.load_nchw(F.elu(F.conv2d(x.to(self.dtype), self.stem[0], self.stem[1], padding=2)))
        tw.forward(B)
        h = tw.store_nchw(B)
        v = F.elu(F.conv2d(h, *self.vconv)).reshape(B, -1)
        v = F.elu(v @ self.vfc1[0] + self.vfc1[1])
        v = torch.tanh((v @ self.vfc2[0] + self.vfc2[1]).float() / 2).squeeze(1)
        p = F.elu(F.conv2d(h, *self.pconv)).reshape(B, -1)
        p = torch.softmax((p @ self.pfc[0] + self.pfc[1]).float(), dim=1)
        return p, v

    @torch.no_grad()
    def tower_reference(self, h):
        """The tower alone on PyTorch ops (bf16 in/out NCHW) — what af_tower_forward replaces."""
        for blk in self.tower:
            r = F.conv2d(h, *blk["res"])
            g = F.elu(F.conv2d(h, *blk["c1"], padding=1))
            h = F.elu(r + F.conv2d(g, *blk["c2"], padding=1))
        return h
