"""ctypes binding of libaf_tower.so (include/af_tower_bf16.h): the hand-written bf16 MFMA residual tower of
BASELINE configs[4].  Raises if the library is missing — DeepResNet.select_backend decides what to do then."""
import ctypes as C
import os

import numpy as np
import torch

_PKG = os.path.dirname(os.path.abspath(__file__))
_LIBPATH = os.environ.get("AF_TOWER_LIB") or os.path.join(_PKG, "_lib", "libaf_tower.so")
_lib = None


class TowerError(RuntimeError):
    """`code`: the AF_TOWER_ERR_* value of include/af_tower_bf16.h the library returned; AF_TOWER_ERR_ARG (-1) for what the binding
    itself refuses before calling in (a missing tensor, a wrong count, dtype, layout or device)."""

    def __init__(self, message, code=-1):
        super().__init__(message)
        self.code = int(code)


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(_LIBPATH):
            raise ImportError(f"{_LIBPATH} not built (python -m alphafive_amd.build)")
        import torch  # noqa: F401  (torch first: see engine.py:lib)
        L = C.CDLL(_LIBPATH)
        vp, fp = C.c_void_p, C.POINTER(C.c_float)
        L.af_tower_create.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(vp)]
        L.af_tower_destroy.argtypes = [vp]
        L.af_tower_destroy.restype = None
        L.af_tower_set_block.argtypes = [vp, C.c_int32, fp, fp, fp, fp, fp, fp]
        L.af_tower_set_stem.argtypes = [vp, fp, fp]
        L.af_tower_set_heads.argtypes = [vp, fp, fp, fp, fp]
        L.af_tower_stem.argtypes = [vp, vp, vp, vp, C.c_int32]
        L.af_tower_heads.argtypes = [vp, vp, vp, vp, vp, C.c_int32]
        L.af_tower_set_dense.argtypes = [vp, fp, fp, fp, fp, fp, fp]
        L.af_tower_dense.argtypes = [vp, vp, vp, vp, vp, vp, C.c_int32]
        L.af_tower_pix.argtypes = [vp]
        L.af_tower_plane_elems.argtypes = [vp]
        L.af_tower_plane_elems.restype = C.c_int64
        L.af_tower_forward.argtypes = [vp, vp, vp, vp, C.c_int32]
        L.af_tower_forward_small.argtypes = [vp, vp, vp, vp, C.c_int32]
        L.af_tower_small_batch.argtypes = [vp]
        L.af_tower_small_batch.restype = C.c_int32
        L.af_tower_flops_per_position.argtypes = [vp]
        L.af_tower_flops_per_position.restype = C.c_int64
        L.af_tower_tune.argtypes = [C.c_int32, C.c_int32]
        L.af_tower_update_device.argtypes = [vp, vp, C.POINTER(vp), C.POINTER(C.c_int64), C.c_int32]
        L.af_tower_debug_weights.argtypes = [vp, C.c_int32, vp, C.c_int64]
        L.af_tower_debug_weights.restype = C.c_int64
        # the int8 residual blocks (csrc/af_tower_i8.hip)
        L.af_tower_i8_enable.argtypes = [vp, fp, C.c_int32]
        L.af_tower_i8_plane_bytes.argtypes = [vp]
        L.af_tower_i8_plane_bytes.restype = C.c_int64
        L.af_tower_forward_i8.argtypes = [vp, vp, vp, vp, vp, C.c_int32]
        L.af_tower_conv_i8.argtypes = [vp, vp, C.c_int32, C.c_int32, vp, vp, vp, C.c_int32, C.c_int32]
        L.af_tower_quantize_i8.argtypes = [vp, vp, vp, vp, C.c_int32]
        L.af_tower_forward_i8_small.argtypes = [vp, vp, vp, vp, vp, C.c_int32]
        L.af_tower_conv_i8_small.argtypes = [vp, vp, C.c_int32, C.c_int32, vp, vp, vp, C.c_int32, C.c_int32]
        L.af_tower_i8_small_batch.argtypes = [vp]
        L.af_tower_i8_small_batch.restype = C.c_int32
        L.af_tower_i8_debug_weights.argtypes = [vp, C.c_int32, vp, C.c_int64]
        L.af_tower_i8_debug_weights.restype = C.c_int64
        L.af_tower_i8_calibrate.argtypes = [vp, vp, vp, vp, C.c_int32, C.c_float]
        L.af_tower_i8_calibration_status.argtypes = [vp, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
        L.af_tower_i8_absmax.argtypes = [vp, vp, vp, C.c_int32, vp]
        L.af_tower_strerror.argtypes = [C.c_int]
        L.af_tower_strerror.restype = C.c_char_p
        _lib = L
    return _lib


def _check(rc, what):
    if rc < 0:
        raise TowerError(f"{what}: {lib().af_tower_strerror(rc).decode()} (code {rc})", rc)


def update_names(blocks):
    """The tensors of af_tower_update_device in its order (include/af_tower_bf16.h), by DeepResNet's variable names."""
    names = ["stem/kernel", "stem/bias"]
    for b in range(blocks):
        names += ["tower/block%d_%s/%s" % (b, layer, part) for layer in ("conv1", "conv2", "res") for part in ("kernel", "bias")]
    for layer in ("value/conv", "policy/conv", "value/fc1", "value/fc2", "policy/fc"):
        names += [layer + "/kernel", layer + "/bias"]
    return names


PRECISIONS = ("bf16", "int8")


def check_precision(precision, board_size, act_scales):
    """What a tower can be built with, checked before anything touches the GPU: ValueError for an unknown precision, for int8 on
    a board other than 11x11 (the int8 kernels exist for that size only) and for int8 without activation scales."""
    if precision not in PRECISIONS:
        raise ValueError("unknown precision %r: expected one of %s" % (precision, ", ".join(PRECISIONS)))
    if precision == "int8":
        if board_size != 11:
            raise ValueError("precision='int8' is built for 11x11 boards only, not %dx%d" % (board_size, board_size))
        if act_scales is None:
            raise ValueError("precision='int8' needs act_scales (DeepResNet.calibrate_int8)")
    elif act_scales is not None:
        raise ValueError("act_scales given with precision=%r" % (precision,))


def check_calibration(precision, board_size, margin):
    """What a device calibration (HipTower.calibrate_i8) can be asked for, checked before anything touches the GPU: ValueError
    for a tower that is not int8, for a board other than 11x11 and for a margin that is not a finite positive number."""
    if precision != "int8":
        raise ValueError("device calibration needs a precision='int8' tower, not %r" % (precision,))
    if board_size != 11:
        raise ValueError("precision='int8' is built for 11x11 boards only, not %dx%d" % (board_size, board_size))
    m = float(margin)
    if not (np.isfinite(m) and m > 0):
        raise ValueError("device calibration: margin must be finite and positive, not %r" % (margin,))


def tune(key, value):
    _check(lib().af_tower_tune(key, value), "af_tower_tune")


class HipTower(object):
    """blocks = list of dicts with torch tensors res/c1/c2 = (weight OIHW, bias), as DeepResNet.tower holds them.
    precision="int8" (11x11 only) with act_scales = the 2 * blocks activation scales of alphafive_amd/tower_i8.py: the handle is
    enabled for int8 BEFORE the weights are set, so every pack path — the setters here, load_device — also packs the int8
    weights from the same fp32 sources, and the tower owns the two int8 activation buffers forward_i8 runs through."""

    def __init__(self, blocks, board_size, width, max_batch, device, stem=None, vconv=None, pconv=None, dense=None,
                 precision="bf16", act_scales=None):
        check_precision(precision, board_size, act_scales)
        self.S, self.width, self.max_batch, self.device = board_size, width, max_batch, torch.device(device)
        self._h = C.c_void_p()
        self.blocks = len(blocks)
        self.precision = precision
        # int8: the scales last given to enable_i8, a float32 copy — the last HOST-given ones: a device calibration
        # (calibrate_i8) replaces the scales on the device without telling the host; read_act_scales() reads those back
        self.act_scales = None
        idx = self.device.index if self.device.index is not None else torch.cuda.current_device()
        _check(lib().af_tower_create(board_size, width, len(blocks), idx, C.byref(self._h)), "af_tower_create")
        if precision == "int8":
            self.enable_i8(act_scales)
            plane = int(lib().af_tower_i8_plane_bytes(self._h))
            # C16 activations [B][width/16][PIX][16]; zero borders are never written by the kernels
            self.xq = torch.zeros((max_batch, width // 16, plane // (width // 16) // 16, 16), dtype=torch.int8, device=self.device)
            self.gq = torch.zeros_like(self.xq)
        for b, blk in enumerate(blocks):
            self.set_block(b, blk)
        if stem is not None:
            self.set_stem(stem)
        if vconv is not None:
            self.set_heads(vconv, pconv)
        self.has_dense = dense is not None
        if dense is not None:                          # (vfc1_w [4C][64], vfc1_b, vfc2_w [64][1], vfc2_b, pfc_w [16C][C], pfc_b)
            self.set_dense(dense)
        self.policy = torch.empty((max_batch, board_size ** 2), dtype=torch.float32, device=self.device)
        self.value = torch.empty((max_batch,), dtype=torch.float32, device=self.device)
        self.vin = torch.empty((max_batch, 4 * board_size ** 2), dtype=torch.bfloat16, device=self.device)
        self.pin = torch.empty((max_batch, 16 * board_size ** 2), dtype=torch.bfloat16, device=self.device)
        self.pix = int(lib().af_tower_pix(self._h))
        self.flops_per_position = int(lib().af_tower_flops_per_position(self._h))
        self.small_batch = int(lib().af_tower_small_batch(self._h))       # forward_small is the faster form up to this batch (0: never)
        self.small_batch_i8 = int(lib().af_tower_i8_small_batch(self._h))  # ... and forward_i8_small against forward_i8 (0: never, and at 15x15)
        # C8 activations [B][width/8][PIX][8]; zero borders are never written by the kernels
        self.x = torch.zeros((max_batch, width // 8, self.pix, 8), dtype=torch.bfloat16, device=self.device)
        self.g = torch.zeros_like(self.x)
        S = board_size
        self._xin = self.x[:, :, S:S + S * S, :].unflatten(2, (S, S))      # [B, width/8, S, S, 8] view of the board pixels

    # ---- host setters: fp32 host copies, staged on the device and packed in place by the kernels load_device runs; they
    # synchronise the device (not stream-ordered, illegal inside a capture) and keep every buffer's address ----
    @staticmethod
    def _host(tensors):
        keep = [np.ascontiguousarray(t.detach().float().cpu().numpy(), np.float32) for t in tensors]
        return keep, [a.ctypes.data_as(C.POINTER(C.c_float)) for a in keep]

    def set_block(self, b, blk):
        keep, ptrs = self._host([blk[k][i] for k in ("c1", "c2", "res") for i in (0, 1)])
        _check(lib().af_tower_set_block(self._h, b, *ptrs), f"af_tower_set_block({b})")

    def set_stem(self, stem):
        keep, ptrs = self._host(stem)
        _check(lib().af_tower_set_stem(self._h, *ptrs), "af_tower_set_stem")

    def set_heads(self, vconv, pconv):
        keep, ptrs = self._host((vconv[0], vconv[1], pconv[0], pconv[1]))
        _check(lib().af_tower_set_heads(self._h, *ptrs), "af_tower_set_heads")

    def set_dense(self, dense):
        keep, ptrs = self._host(dense)
        _check(lib().af_tower_set_dense(self._h, *ptrs), "af_tower_set_dense")
        self.has_dense = True

    def load_nchw(self, h):
        """h: bf16 [B, width, S, S] -> interior of the C8 buffer."""
        B = h.shape[0]
        self._xin[:B].copy_(h.view(B, self.width // 8, 8, self.S, self.S).permute(0, 1, 3, 4, 2))

    def store_nchw(self, B):
        return self._xin[:B].permute(0, 1, 4, 2, 3).reshape(B, self.width, self.S, self.S)

    def scratch_nchw(self, B):
        """bf16 [B, width, S, S]: what the last convolution that wrote the scratch buffer left there — after forward() on a
        single-block tower, the block's mid activation g = ELU(conv3x3(h) + b1).  Like load_nchw / store_nchw it reads the C8 layout
        of include/af_tower_bf16.h, which is the same rule at every board size (15x15 runs its convolutions in half boards, but
        reads and writes whole planes in this layout)."""
        S = self.S
        gin = self.g[:, :, S:S + S * S, :].unflatten(2, (S, S))
        return gin[:B].permute(0, 1, 4, 2, 3).reshape(B, self.width, S, S)

    def stem(self, planes):
        """planes fp32 [B,3,S,S] (contiguous) -> the C8 buffer (af_tower_stem_kernel)."""
        B = planes.shape[0]
        assert planes.is_contiguous() and planes.dtype == torch.float32 and B <= self.max_batch
        stream = torch.cuda.current_stream(self.device).cuda_stream
        _check(lib().af_tower_stem(self._h, stream, planes.data_ptr(), self.x.data_ptr(), B), "af_tower_stem")

    def heads(self, B):
        """-> (vin bf16 [B, 4*S*S], pin bf16 [B, 16*S*S]) = ELU(1x1 conv) of the tower output, flattened NCHW."""
        stream = torch.cuda.current_stream(self.device).cuda_stream
        _check(lib().af_tower_heads(self._h, stream, self.x.data_ptr(), self.vin.data_ptr(), self.pin.data_ptr(), B),
               "af_tower_heads")
        return self.vin[:B], self.pin[:B]

    def dense(self, B):
        """vin / pin of heads() -> (policy fp32 [B, S*S] softmax, value fp32 [B]) on the MFMA dense kernel."""
        stream = torch.cuda.current_stream(self.device).cuda_stream
        _check(lib().af_tower_dense(self._h, stream, self.vin.data_ptr(), self.pin.data_ptr(), self.policy.data_ptr(),
                                    self.value.data_ptr(), B), "af_tower_dense")
        return self.policy[:B], self.value[:B]

    def bind_outputs(self, policy, value):
        """Write results straight into caller-owned device tensors (the engine's: no copy on the tick path)."""
        assert policy.is_contiguous() and value.is_contiguous() and policy.dtype == torch.float32
        self.policy, self.value = policy, value

    def forward(self, B):
        stream = torch.cuda.current_stream(self.device).cuda_stream
        _check(lib().af_tower_forward(self._h, stream, self.x.data_ptr(), self.g.data_ptr(), B), "af_tower_forward")

    # ---- int8 residual blocks ----
    def enable_i8(self, act_scales):
        """af_tower_i8_enable: stores the activation scales; called again with new ones it re-packs the int8 weights in place
        (synchronises the device)."""
        a = np.ascontiguousarray(np.asarray(act_scales, np.float32).reshape(-1))
        _check(lib().af_tower_i8_enable(self._h, a.ctypes.data_as(C.POINTER(C.c_float)), a.shape[0]), "af_tower_i8_enable")
        self.act_scales = a.copy()

    def calibrate_i8(self, planes, margin=1.0):
        """Activation scales from the device's own activations, in place (af_tower_i8_calibrate): runs the stem over planes —
        float32 [B,3,11,11], contiguous, on this device — then the bf16 blocks with the absmax of every h_b and g_b measured on the
        way, turns the 2 * blocks maxima into scales on the device (tower_i8.scales_from_absmax), installs them if they are all
        usable (calibration_status() tells) and re-packs the int8 weights under them.  Launches only on torch's current stream: no
        allocation, no copy to the host, no wait, so with B <= max_batch — the tower's own x / g — it is legal inside a stream
        capture, and an int8 forward captured earlier replays with the new scales.  A larger B runs through scratch buffers
        allocated for the call: NOT for use under capture.  x (and the scratch g) are left holding the bf16 tower's activations."""
        check_calibration(self.precision, self.S, margin)
        if not (torch.is_tensor(planes) and planes.is_cuda and planes.dtype == torch.float32 and planes.is_contiguous()
                and planes.dim() == 4 and tuple(planes.shape[1:]) == (3, self.S, self.S) and planes.shape[0] >= 1):
            raise TowerError("calibrate_i8: planes must be a contiguous float32 [B,3,%d,%d] tensor on %s" % (self.S, self.S, self.device))
        B = planes.shape[0]
        stream = torch.cuda.current_stream(self.device).cuda_stream
        if B <= self.max_batch:
            x, g = self.x, self.g
        else:
            x = torch.zeros((B,) + tuple(self.x.shape[1:]), dtype=torch.bfloat16, device=self.device)
            g = torch.zeros_like(x)
        _check(lib().af_tower_stem(self._h, stream, planes.data_ptr(), x.data_ptr(), B), "af_tower_stem")
        _check(lib().af_tower_i8_calibrate(self._h, stream, x.data_ptr(), g.data_ptr(), B, float(margin)), "af_tower_i8_calibrate")

    def calibration_status(self):
        """-> (status, count) of af_tower_i8_calibration_status: 0 if the last calibrate_i8 installed its scales, 1 if it refused
        them (a NaN or an infinity among the activations) and left the old ones; how many have been installed.  Synchronises."""
        st, n = C.c_int32(), C.c_int32()
        _check(lib().af_tower_i8_calibration_status(self._h, C.byref(st), C.byref(n)), "af_tower_i8_calibration_status")
        return st.value, n.value

    def read_act_scales(self):
        """The activation scales as the device holds them now, float32 [2 * blocks] in tower_i8's order — after a calibrate_i8
        these are not act_scales any more.  Synchronises the device."""
        size = lib().af_tower_i8_debug_weights(self._h, 4 * self.blocks, None, 0)
        _check(size, "af_tower_i8_debug_weights")
        buf = np.empty(size, np.uint8)
        _check(lib().af_tower_i8_debug_weights(self._h, 4 * self.blocks, buf.ctypes.data_as(C.c_void_p), size), "af_tower_i8_debug_weights")
        return buf.view(np.float32)[:2 * self.blocks].copy()

    def absmax(self, x, B):
        """Tests: the absmax kernel alone over the board pixels of the first B positions of a bf16 C8 tensor -> the largest
        magnitude's bit pattern (bits & 0x7fff), an int.  Synchronises."""
        word = torch.zeros(1, dtype=torch.int32, device=self.device)
        stream = torch.cuda.current_stream(self.device).cuda_stream
        _check(lib().af_tower_i8_absmax(self._h, stream, x.data_ptr(), B, word.data_ptr()), "af_tower_i8_absmax")
        return int(word.item())

    def forward_i8(self, B):
        """The blocks in int8: quantises the stem's output in self.x, runs every block through xq / gq and leaves the last block's
        bf16 output in self.x, where heads() reads it.  The persistent kernels at every batch (forward_i8_small: the tile-parallel form)."""
        if self.precision != "int8":
            raise TowerError("forward_i8: this tower was built with precision=%r" % (self.precision,), -3)
        stream = torch.cuda.current_stream(self.device).cuda_stream
        _check(lib().af_tower_forward_i8(self._h, stream, self.x.data_ptr(), self.xq.data_ptr(), self.gq.data_ptr(), B),
               "af_tower_forward_i8")

    def forward_i8_small(self, B):
        """forward_i8() on the tile-parallel int8 kernel (af_tower_forward_i8_small): the same bits at any batch, the form
        DeepResNet.eval_hip takes up to small_batch_i8."""
        if self.precision != "int8":
            raise TowerError("forward_i8_small: this tower was built with precision=%r" % (self.precision,), -3)
        stream = torch.cuda.current_stream(self.device).cuda_stream
        _check(lib().af_tower_forward_i8_small(self._h, stream, self.x.data_ptr(), self.xq.data_ptr(), self.gq.data_ptr(), B),
               "af_tower_forward_i8_small")

    def conv_i8_small(self, block, second, inp, inp2, out, B):
        """Tests: one int8 layer on the tile-parallel kernel (af_tower_conv_i8_small); arguments as conv_i8."""
        stream = torch.cuda.current_stream(self.device).cuda_stream
        _check(lib().af_tower_conv_i8_small(self._h, stream, block, int(second), inp.data_ptr(), inp2.data_ptr() if inp2 is not None else None,
                                            out.data_ptr(), int(out.dtype == torch.bfloat16), B), "af_tower_conv_i8_small")

    def quantize_i8(self, x, xq, B):
        """Tests: the entry quantiser alone, bf16 C8 tensor x -> int8 C16 tensor xq."""
        stream = torch.cuda.current_stream(self.device).cuda_stream
        _check(lib().af_tower_quantize_i8(self._h, stream, x.data_ptr(), xq.data_ptr(), B), "af_tower_quantize_i8")

    def conv_i8(self, block, second, inp, inp2, out, B):
        """Tests: one int8 layer (af_tower_conv_i8); out int8 C16 or bf16 C8, by its dtype."""
        stream = torch.cuda.current_stream(self.device).cuda_stream
        _check(lib().af_tower_conv_i8(self._h, stream, block, int(second), inp.data_ptr(), inp2.data_ptr() if inp2 is not None else None,
                                      out.data_ptr(), int(out.dtype == torch.bfloat16), B), "af_tower_conv_i8")

    def debug_weights_i8(self):
        """Tests: the int8 weight-derived buffers as bytes, in af_tower_i8_debug_weights' order (4 per block, then the scales)."""
        out = []
        for i in range(4 * self.blocks + 1):
            size = lib().af_tower_i8_debug_weights(self._h, i, None, 0)
            _check(size, "af_tower_i8_debug_weights")
            buf = np.empty(size, np.uint8)
            _check(lib().af_tower_i8_debug_weights(self._h, i, buf.ctypes.data_as(C.c_void_p), size), "af_tower_i8_debug_weights")
            out.append(buf)
        return out

    def forward_small(self, B):
        """forward() on the tile-parallel kernel (af_tower_forward_small): the same bits at any batch, faster up to small_batch."""
        stream = torch.cuda.current_stream(self.device).cuda_stream
        _check(lib().af_tower_forward_small(self._h, stream, self.x.data_ptr(), self.g.data_ptr(), B), "af_tower_forward_small")

    def load_device(self, tensors):
        """Weight update without the host (af_tower_update_device): `tensors` is a list in the ABI's order or a dict by the names
        of update_names(blocks); each a contiguous float32 tensor on this handle's device, OIHW convolutions and [in][out] dense
        layers.  Kernels re-pack them in place into the buffers the handle owns, on torch's current stream, behind the forwards
        already queued there: launches only, no wait, legal inside a stream capture.  The tensors must hold their values until
        the pack kernels have run — a producer on the same stream is ordered.  Every host setter must have run once before (the
        constructor's, when it got all four groups): TowerError with code -3 otherwise."""
        names = update_names(self.blocks)
        if isinstance(tensors, dict):
            missing = [k for k in names if k not in tensors]
            if missing:
                raise TowerError("load_device: missing %s" % ", ".join(missing))
            tensors = [tensors[k] for k in names]
        tensors = list(tensors)
        if len(tensors) != len(names):
            raise TowerError("load_device: %d tensors, expected %d (12 + 6 * blocks)" % (len(tensors), len(names)))
        idx = self.device.index if self.device.index is not None else torch.cuda.current_device()
        for name, t in zip(names, tensors):
            if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
                raise TowerError(f"load_device({name}): a contiguous float32 tensor on {self.device} is required")
            if t.device.index != idx:
                raise TowerError(f"load_device({name}): tensor on {t.device}, handle on {self.device}")
        n = len(names)
        stream = torch.cuda.current_stream(self.device).cuda_stream
        _check(lib().af_tower_update_device(self._h, stream, (C.c_void_p * n)(*[t.data_ptr() for t in tensors]),
                                            (C.c_int64 * n)(*[t.numel() for t in tensors]), n), "af_tower_update_device")

    def debug_weights(self):
        """Tests: every weight-derived device buffer of the handle as bytes, in af_tower_debug_weights' order (synchronises);
        None for a buffer of a group (a block, stem, heads, dense) whose host setter has not run."""
        out = []
        for i in range(4 * self.blocks + 12):
            size = lib().af_tower_debug_weights(self._h, i, None, 0)
            if size == -3:                              # AF_TOWER_ERR_STATE
                out.append(None)
                continue
            _check(size, "af_tower_debug_weights")
            buf = np.empty(size, np.uint8)
            _check(lib().af_tower_debug_weights(self._h, i, buf.ctypes.data_as(C.c_void_p), size), "af_tower_debug_weights")
            out.append(buf)
        return out

    def close(self):
        if getattr(self, "_h", None):
            try:
                lib().af_tower_destroy(self._h)
            except Exception:       # interpreter shutdown
                pass
            self._h = None

    __del__ = close
