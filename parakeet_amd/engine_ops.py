"""The engine's shared GEMMs exactly as the models launch them (``pk_op_gemm``, ``pk_op_rowgemm``, ``pk_op_row_amax``).

Thin wrappers over the C ABI: every keyword is the field of ``pk_op_gemm_cfg`` / ``pk_op_rowgemm_cfg`` of that name
(include/pk_synth.h).  Device-side fields take a device tensor (or anything ``Context.to_device`` accepts), host-side
fields a numpy array; ``None`` switches the feature off.  Output tensors are given by the caller, who sizes them and may
pre-fill them, so that what a kernel leaves untouched can be seen.
"""
import ctypes as C

import numpy as np
import torch

from . import _capi
from .runtime import Context, to_numpy_f32

KERNELS = ("fp32", "h3-64", "h3-128")
MATH_F32, MATH_F16X3 = 0, 1
ACT_NONE, ACT_RELU, ACT_TANH = 0, 1, 2
EPI_STD, EPI_GATE, EPI_GATE_PROJ = 0, 1, 2
RES_AFTER_ACT, RES_AFTER_AFFINE, RES_BEFORE_ACT = 0, 1, 2

_GEMM_DEV_F32 = ("A", "A2", "res", "a_amax", "a2_amax")
_GEMM_DEV_I32 = ("rowvalid", "out_rowmap")
_GEMM_OUT = ("C", "C2")
_GEMM_HOST = ("W", "bias", "cscale", "cshift", "W2", "bias2")
_ROW_DEV_F32 = ("x", "res")
_ROW_DEV_I32 = ("stop_minlen", "stop_maxlen")
_ROW_OUT = ("y", "lstm_c", "lstm_h1", "lstm_h2", "stop_probs", "stop_len", "stop_ndone")
_ROW_HOST = ("W", "bias", "ln_g", "ln_b", "stop_w")


def _fill(cfg, ctx, kw, dev_f32, dev_i32, outs, host):
    keep = []                                     # whatever the pointers refer to, alive until the call returns
    names = {n for n, _ in cfg._fields_}
    for k, v in kw.items():
        if k not in names:
            raise TypeError(f"unknown field {k!r}")
        if v is None:
            continue
        if k in dev_f32 or k in dev_i32:
            t = ctx.to_device(v, torch.float32 if k in dev_f32 else torch.int32)
            keep.append(t)
            setattr(cfg, k, t.data_ptr())
        elif k in outs:
            if not (isinstance(v, torch.Tensor) and v.is_cuda and v.is_contiguous()):
                raise TypeError(f"{k} must be a contiguous device tensor")
            setattr(cfg, k, v.data_ptr())
        elif k in host:
            a = to_numpy_f32(v)
            keep.append(a)
            setattr(cfg, k, a.ctypes.data)
        elif k in ("tap_off", "tap_w"):
            for i, x in enumerate(v):
                getattr(cfg, k)[i] = int(x)
        elif k == "drop_seeds":
            t = ctx.to_device(np.asarray(v, dtype=np.uint64).view(np.int64), torch.int64)
            keep.append(t)
            cfg.drop_seeds = t.data_ptr()
        else:
            setattr(cfg, k, v)
    return keep


def gemm(**kw):
    """Run ``pk_op_gemm``; returns the name of the kernel that ran (one of KERNELS).  Raises as ``_capi.check`` does."""
    ctx = Context.get()
    cfg = _capi.OpGemmCfg()
    cfg.kernel = -1
    keep = _fill(cfg, ctx, kw, _GEMM_DEV_F32, _GEMM_DEV_I32, _GEMM_OUT, _GEMM_HOST)
    _capi.check(ctx.lib.pk_op_gemm(ctx.handle, C.byref(cfg)))
    del keep
    if not 0 <= cfg.kernel < len(KERNELS):
        raise RuntimeError(f"pk_op_gemm reported kernel {cfg.kernel}")
    return KERNELS[cfg.kernel]


def rowgemm(**kw):
    """Run ``pk_op_rowgemm``."""
    ctx = Context.get()
    cfg = _capi.OpRowgemmCfg()
    cfg.ln_eps, cfg.drop_J, cfg.drop_scale, cfg.stop_thr = 1e-5, 1, 1.0, 0.5
    keep = _fill(cfg, ctx, kw, _ROW_DEV_F32, _ROW_DEV_I32, _ROW_OUT, _ROW_HOST)
    _capi.check(ctx.lib.pk_op_rowgemm(ctx.handle, C.byref(cfg)))
    del keep


def row_amax(A, lda, C_, r0, r1, amax, base_row=0, amax_base=0):
    """``pk_op_row_amax`` on device tensors: row 0 of the matrix is row ``base_row`` of the 2-D tensor ``A`` (so r0 may be
    negative), entry 0 of the result is element ``amax_base`` of the 1-D tensor ``amax``.  Synchronises."""
    ctx = Context.get()
    assert A.is_cuda and amax.is_cuda and A.dtype == amax.dtype == torch.float32
    assert base_row + r0 >= 0 and (base_row + r1 - 1) * lda + C_ <= A.numel() and amax_base + r0 >= 0 and \
        amax_base + r1 <= amax.numel(), "rows outside the tensors"
    _capi.check(ctx.lib.pk_op_row_amax(ctx.handle, C.c_void_p(A.data_ptr() + 4 * base_row * lda), int(lda), int(C_),
                                       int(r0), int(r1), C.c_void_p(amax.data_ptr() + 4 * amax_base)))
    ctx.sync()
