"""ctypes binding of libaf_sym.so (include/af_sym.h): the board-symmetry kernels around an evaluator — expand / reduce for the
symmetry-averaged evaluation, apply / restore for one symmetry drawn per leaf.  Raises if the library is missing.
alphafive_amd/symmetry.py holds the numpy specification and the evaluator built on this binding."""
import ctypes as C
import os

import numpy as np
import torch

_PKG = os.path.dirname(os.path.abspath(__file__))
_LIBPATH = os.environ.get("AF_SYM_LIB") or os.path.join(_PKG, "_lib", "libaf_sym.so")
_lib = None

ABI_VERSION = 1


class SymError(RuntimeError):
    """`code`: the AF_SYM_ERR_* value of include/af_sym.h the library returned; AF_SYM_ERR_ARG (-1) for what the binding itself
    refuses before calling in (a wrong dtype, layout, shape or device)."""

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
        vp = C.c_void_p
        L.af_sym_abi_version.argtypes = []
        L.af_sym_create.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_uint64, C.POINTER(vp)]
        L.af_sym_destroy.argtypes = [vp]
        L.af_sym_destroy.restype = None
        L.af_sym_expand.argtypes = [vp, vp, vp, vp, C.c_int32]
        L.af_sym_reduce.argtypes = [vp, vp, vp, vp, vp, vp, C.c_int32]
        L.af_sym_apply.argtypes = [vp, vp, vp, vp, C.c_int32]
        L.af_sym_restore.argtypes = [vp, vp, vp, vp, vp, vp, C.c_int32]
        L.af_sym_set_counter.argtypes = [vp, vp, C.c_uint64]
        L.af_sym_state.argtypes = [vp, vp, C.POINTER(C.c_uint64), C.POINTER(C.c_int32), C.c_int32]
        L.af_sym_strerror.argtypes = [C.c_int]
        L.af_sym_strerror.restype = C.c_char_p
        if L.af_sym_abi_version() != ABI_VERSION:
            raise ImportError(f"{_LIBPATH}: ABI version {L.af_sym_abi_version()}, this binding is written for {ABI_VERSION}")
        _lib = L
    return _lib


def _check(rc, what):
    if rc < 0:
        raise SymError(f"{what}: {lib().af_sym_strerror(rc).decode()} (code {rc})", rc)


class HipSym(object):
    """One af_sym handle: the four work calls on torch's current stream (launches only: legal under stream capture), the
    random mode's counter and stored symmetries on the device.  Tensors are contiguous float32 on the handle's device; `batch`
    rows of them are read and written, whatever their leading dimension."""

    def __init__(self, board_size, max_batch, device="cuda:0", seed=0):
        self.S, self.C, self.max_batch = int(board_size), int(board_size) ** 2, int(max_batch)
        self.device = torch.device(device)
        self.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        self._h = C.c_void_p()
        idx = self.device.index if self.device.index is not None else torch.cuda.current_device()
        _check(lib().af_sym_create(self.S, self.max_batch, idx, self.seed, C.byref(self._h)), "af_sym_create")

    def _stream(self):
        return torch.cuda.current_stream(self.device).cuda_stream

    def _ptr(self, what, t, rows, *tail):
        if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
            raise SymError(f"{what}: a contiguous float32 tensor on {self.device} is required")
        if t.numel() < rows * int(np.prod(tail, dtype=np.int64)):
            raise SymError(f"{what}: {tuple(t.shape)} holds fewer than {rows} rows of {tail}")
        return t.data_ptr()

    def expand(self, planes, planes8, batch):
        """planes [batch,3,S,S] -> planes8 [8 * batch,3,S,S], row 8 b + s = transform(planes[b], s)."""
        S = self.S
        _check(lib().af_sym_expand(self._h, self._stream(), self._ptr("planes", planes, batch, 3, S, S),
                                   self._ptr("planes8", planes8, 8 * batch, 3, S, S), batch), "af_sym_expand")

    def reduce(self, policy8, value8, policy, value, batch):
        """(policy8 [8 * batch,C], value8 [8 * batch]) -> (policy [batch,C], value [batch]): symmetry.reduce_reference."""
        _check(lib().af_sym_reduce(self._h, self._stream(), self._ptr("policy8", policy8, 8 * batch, self.C),
                                   self._ptr("value8", value8, 8 * batch), self._ptr("policy", policy, batch, self.C),
                                   self._ptr("value", value, batch), batch), "af_sym_reduce")

    def apply(self, planes, planes_t, batch):
        """planes -> planes_t, row b under the symmetry drawn for it at the handle's counter (symmetry.draw_reference)."""
        S = self.S
        _check(lib().af_sym_apply(self._h, self._stream(), self._ptr("planes", planes, batch, 3, S, S),
                                  self._ptr("planes_t", planes_t, batch, 3, S, S), batch), "af_sym_apply")

    def restore(self, policy_t, value_t, policy, value, batch):
        """policy_t -> policy under the inverse of the symmetries apply() stored; the value moves if the tensors differ; the
        counter advances by one."""
        _check(lib().af_sym_restore(self._h, self._stream(), self._ptr("policy_t", policy_t, batch, self.C),
                                    self._ptr("value_t", value_t, batch), self._ptr("policy", policy, batch, self.C),
                                    self._ptr("value", value, batch), batch), "af_sym_restore")

    def set_counter(self, counter):
        _check(lib().af_sym_set_counter(self._h, self._stream(), int(counter) & 0xFFFFFFFFFFFFFFFF), "af_sym_set_counter")

    def state(self, batch=None):
        """Tests: (counter, int32 [batch] stored symmetries) as the device holds them (synchronises the stream)."""
        n = self.max_batch if batch is None else int(batch)
        ctr = C.c_uint64()
        syms = np.zeros(n, np.int32)
        _check(lib().af_sym_state(self._h, self._stream(), C.byref(ctr), syms.ctypes.data_as(C.POINTER(C.c_int32)), n), "af_sym_state")
        return int(ctr.value), syms

    def close(self):
        if getattr(self, "_h", None):
            try:
                lib().af_sym_destroy(self._h)
            except Exception:       # interpreter shutdown
                pass
            self._h = None

    __del__ = close
