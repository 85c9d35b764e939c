"""ctypes binding of libqvit_hip.so (include/qvit_hip.h) plus thin torch-tensor wrappers.

This is the only place the Python side touches the C-ABI. There is no fallback: if the
library is missing or a GPU is required and absent, calls raise. Tensors are passed as raw
device pointers; every call is enqueued on torch's current HIP stream.
"""
from __future__ import annotations

import ctypes
import os
import threading
from typing import NamedTuple, Optional, Tuple

import numpy as np
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
# QVIT_LIB: another build of the library (diagnostic A/B runs of the same tests on one box)
LIB_PATH = os.environ.get("QVIT_LIB") or os.path.join(_HERE, "libqvit_hip.so")

# ---- constants mirrored from include/qvit_hip.h ---------------------------------------------
QT_LINEAR = 0
QT_NONLINEAR = 1
QT_ULTRA_ACT = 2
QT_FORCE_CAREFUL = 0x100  # test-only: disable the guarded fast path

W4 = 4
W8 = 8
W4R = 40  # qvit_gemm / qvit_gemm_qkv_split only: a W4 image re-ordered by qvit_pack_weight_w4r
W8R = 80  # qvit_gemm / qvit_gemm_qkv_split only: a W4 image as 16x-scaled int8 operands (qvit_pack_weight_w8r)
W16 = 16  # qvit_gemm_wonly only: balanced base-256 digits as W8 images, two (|k| <= 32639) or
W24 = 24  # three (|k| < 2^23)

EPI_F32 = 0
EPI_F32_RESID = 1
EPI_I8_GELU = 2
EPI_I8 = 3
EPI_I32 = 4
EPI_QKV_SPLIT = 5   # qvit_gemm_qkv_split only

ATT_F32 = 0
ATT_I8 = 1

ULTRA_CODES = 0
ULTRA_CODES_POOL = 1
ULTRA_F32 = 2

EPI_TABLE_MAX_NB = 3800

QAT_SGD, QAT_ADAM, QAT_ADAMW = 0, 1, 2
QAT_WARMUP, QAT_RANGE, QAT_FIX = 0, 1, 2
QAT_CHUNK = 4096          # elements of one chunk of qvit_qat_step
QAT_TENSOR_BYTES = 48     # its tensor descriptor, and the (layer, side) descriptor of qvit_qat_quant_step
QAT_QUANT_BYTES = 64
PRUNE_GROUP_BYTES = 64    # the group, member and item descriptors of the qvit_prune_* entry points
PRUNE_MEMBER_BYTES = 48
PRUNE_ITEM_BYTES = 16
PRUNE_IMPORTANT, PRUNE_REDUNDANT, PRUNE_PRUNED = 0, 1, 2

# The descriptors as numpy dtypes: the Python statement of the structs' layouts (their fields, in their order; natural
# alignment leaves no padding). The host tables are arrays of these and reach the device byte for byte.
_P, _I = "<i8", "<i4"   # a device pointer or int64_t, an int32_t
QAT_TENSOR_DTYPE = np.dtype([("p", _P), ("grad", _P), ("m", _P), ("v", _P), ("numel", _P), ("lr_class", _I),
                             ("flags", _I)])
QAT_CHUNK_DTYPE = np.dtype([("tensor", _I), ("index", _I)])
QAT_QUANT_DTYPE = np.dtype([("s", _P, (3,)), ("g", _P, (3,)), ("mom", _P), ("side", _I), ("flags", _I)])
PRUNE_GROUP_DTYPE = np.dtype([("d", _P), ("qm", _P), ("t", _P), ("member_begin", _I), ("member_count", _I),
                              ("rows", _I), ("joint", _I), ("red_begin", _I), ("red_count", _I), ("elems", _P),
                              ("sections", _I), ("unit_rows", _I)])
PRUNE_MEMBER_DTYPE = np.dtype([("p", _P), ("grad", _P), ("m", _P), ("v", _P), ("width", _P), ("quantized", _I),
                               ("flags", _I)])
PRUNE_ITEM_DTYPE = np.dtype([("group", _I), ("row", _I), ("state", _I), ("link", _I)])
for _dt, _n in ((QAT_TENSOR_DTYPE, QAT_TENSOR_BYTES), (QAT_CHUNK_DTYPE, 8), (QAT_QUANT_DTYPE, QAT_QUANT_BYTES),
                (PRUNE_GROUP_DTYPE, PRUNE_GROUP_BYTES), (PRUNE_MEMBER_DTYPE, PRUNE_MEMBER_BYTES),
                (PRUNE_ITEM_DTYPE, PRUNE_ITEM_BYTES)):
    assert _dt.itemsize == _n, (_dt, _n)


class Hyper(NamedTuple):
    """The hyper-parameters of one step, in the order the qvit_qat_* and qvit_prune_* entry points take them."""
    variant: int
    first_step: int
    lr: float
    lr_quant: float
    first_momentum: float
    second_momentum: float
    alpha1: float
    alpha2: float
    weight_decay: float
    bias_correction1: float
    bias_correction2: float
    clip_lo: float
    clip_hi: float


U8_NCHW = 0
U8_NHWC = 1
U8_MAX_C = 16   # channels whose [C][256] tables the uint8 kernels hold in LDS

TILE_N = 256
TILE_K = 128


def round_up(v: int, m: int) -> int:
    return (v + m - 1) // m * m


# Which of a layer's two backward contractions run on the project's kernels, by the value of its switch
# (quant_layers.BACKWARD_GEMM / CONV_BACKWARD_GEMM, quant_ultra.ULTRA_BWD; the rules on top stay with the switches).
BACKWARD_OPS = {"hip": ("dgrad", "wgrad"), "torch": (), "dgrad": ("dgrad",), "wgrad": ("wgrad",)}


def backward_ops(value, what: str) -> tuple:
    """BACKWARD_OPS[value]. `what` names where the value came from, for the error: an environment variable
    (QVIT_..., checked at import, reported as NAME='v') or a module attribute (looked up at every use, since a caller
    may have assigned it; reported as NAME = 'v')."""
    try:
        return BACKWARD_OPS[value]
    except KeyError:
        sep = "=" if what.startswith("QVIT_") else " = "
        raise ValueError(f"{what}{sep}{value!r}: expected hip, torch, dgrad or wgrad") from None


_c_p =ctypes.c_void_p
_i64 = ctypes.c_int64
_i32 = ctypes.c_int
_f32 = ctypes.c_float
_f64 = ctypes.c_double

# name -> argtypes (restype is int for all but the string getters)
_SIGNATURES = {
    "qvit_quantize_act_i8": [_c_p, _i64, _i64, _i64, _i32, _c_p, _c_p, _c_p, _i32, _c_p, _i64, _i64, _c_p],
    "qvit_fake_quant_f32": [_c_p, _i64, _i32, _c_p, _c_p, _c_p, _i32, _c_p, _c_p],
    "qvit_quant_backward": [_c_p, _c_p, _i64, _i32, _c_p, _c_p, _c_p, _f32, _f32, _f32, _c_p, _c_p, _c_p, _i64, _c_p],
    "qvit_quant_error": [_c_p, _i64, _i64, _i64, _i32, _c_p, _c_p, _c_p, _i32, _i32, _c_p, _c_p, _c_p, _i64, _c_p],
    "qvit_qat_step": [_c_p, _i32, _c_p, _i64, _i32, _i32] + [_f32] * 11 + [_c_p],
    "qvit_qat_quant_step": [_c_p, _i32, _c_p, _i32, _i32, _i32, _i32] + [_f32] * 11 + [_i32] * 4 + [_c_p],
    "qvit_prune_scores": [_c_p, _i32, _c_p, _i32, _c_p, _i64, _c_p, _i32, _i32] + [_f32] * 11 + [_c_p],
    "qvit_prune_scores_fold": [_c_p, _i32, _c_p, _i64, _c_p, _c_p, _i64, _c_p, _c_p],
    "qvit_prune_scores_finish": [_c_p, _i32, _c_p, _i64, _c_p] + [_f64] * 5 + [_c_p, _c_p],
    "qvit_prune_joint_scalars": [_c_p, _i32, _i32, _i32] + [_f32] * 11 + [_i32, _i32, _c_p],
    "qvit_prune_joint_reduce": [_c_p, _i32, _c_p, _i32, _c_p, _i64, _c_p, _i32, _i32] + [_f32] * 11 + [_c_p],
    "qvit_prune_joint_finish": [_c_p, _i32, _c_p, _i64, _f64, _i32, _i32, _i32, _i32, _c_p, _c_p, _c_p],
    "qvit_prune_joint_apply": [_c_p, _i32, _c_p, _i32, _c_p, _i64, _c_p, _i32, _i32] + [_f32] * 11 + [_c_p],
    "qvit_gelu_f32": [_c_p, _i64, _c_p, _c_p],
    "qvit_layernorm_quant_backward": [_c_p, _i64, _i64, _i64, _c_p, _c_p, _f32, _i32, _c_p, _c_p, _c_p, _f32, _f32,
                                      _c_p, _i64, _c_p, _i64, _c_p, _c_p, _c_p, _c_p, _i64, _c_p],
    "qvit_gelu_quant_i8": [_c_p, _i64, _i64, _i64, _i32, _c_p, _c_p, _c_p, _i32, _c_p, _i64, _i64, _c_p],
    "qvit_gelu_quant_backward": [_c_p, _c_p, _i64, _i32, _c_p, _c_p, _c_p, _f32, _f32, _c_p, _c_p, _c_p, _i64, _c_p],
    "qvit_pack_weight": [_c_p, _i64, _i64, _i64, _i32, _c_p, _c_p, _c_p, _i32, _c_p, _i64, _i64, _c_p, _c_p],
    "qvit_pad_bias": [_c_p, _i64, _c_p, _i64, _c_p],
    "qvit_pack_weight_w4r": [_c_p, _i64, _i64, _c_p, _c_p],
    "qvit_pack_weight_w8r": [_c_p, _i64, _i64, _c_p, _c_p],
    "qvit_im2col_quant_i8": [_c_p, _i64, _i64, _i64, _i64, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32,
                             _i32, _c_p, _c_p, _c_p, _i32, _c_p, _i64, _i64, _c_p],
    "qvit_im2col_u8_i8": [_c_p, _i64, _i64, _i64, _i64, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32,
                          _c_p, _c_p, _i64, _i64, _c_p],
    "qvit_u8_normalize_f32": [_c_p, _i64, _i64, _i64, _i64, _i32, _c_p, _c_p, _c_p],
    "qvit_layernorm_quant_i8": [_c_p, _i64, _i64, _i64, _c_p, _c_p, _f32, _i32, _c_p, _c_p, _c_p, _i32,
                                _c_p, _i64, _i64, _c_p, _c_p],
    "qvit_gemm": [_c_p, _i64, _i64, _i64, _c_p, _i32, _i64, _i64, _c_p, _c_p, _c_p, _i32, _c_p, _i64,
                  _i32, _c_p, _c_p, _c_p, _i32, _c_p, _c_p],
    "qvit_layernorm_quant_i8_t32": [_c_p, _i64, _i64, _i64, _c_p, _c_p, _f32, _i32, _c_p, _c_p, _c_p, _i32, _c_p,
                                    _i64, _c_p, _c_p],
    "qvit_gemm_a32_fits": [_i64, _i32, _i64, _i64, _i32],
    "qvit_gemm_a32": [_c_p, _i64, _i64, _c_p, _i32, _i64, _i64, _c_p, _c_p, _c_p, _i32, _c_p, _i64, _i32, _c_p, _c_p,
                      _c_p, _i32, _c_p, _c_p],
    "qvit_gemm_wonly": [_c_p, _i64, _i64, _i64, _c_p, _i32, _i64, _i64, _c_p, _c_p, _c_p, _i64, _c_p, _i64, _c_p],
    "qvit_gemm_wgrad": [_c_p, _i64, _i64, _i64, _c_p, _i64, _i64, _c_p, _c_p, _i64, _c_p, _i64, _c_p],
    "qvit_col2im_quant_backward": [_c_p, _i64, _c_p, _i64, _i64, _i64, _i64, _i32, _i32, _i32, _i32, _i32, _i32, _i32,
                                   _i32, _i32, _c_p, _c_p, _c_p, _f32, _f32, _c_p, _c_p, _c_p, _i64, _c_p],
    "qvit_conv_wonly": [_c_p, _i64, _i64, _i64, _i64, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _c_p, _i32,
                        _i64, _i64, _i64, _c_p, _c_p, _c_p, _c_p, _i64, _c_p],
    "qvit_conv_wonly_bn_act": [_c_p, _i64, _i64, _i64, _i64, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _c_p,
                               _i32, _i64, _i64, _i64, _c_p, _c_p, _c_p, _c_p, _i32, _c_p, _c_p],
    "qvit_conv_wonly_narrow": [_i32],
    "qvit_epi_table_build": [_i32, _i32, _c_p, _c_p, _c_p, _i32, _f32, _f32, _i64, _c_p, _c_p],
    "qvit_gemm_resid_ln": [_c_p, _i64, _i64, _i64, _c_p, _i32, _i64, _i64, _c_p, _c_p, _c_p, _c_p, _i64, _c_p, _c_p,
                           _f32, _i32, _c_p, _c_p, _c_p, _i32, _c_p, _c_p, _i64, _i64, _c_p, _c_p],
    "qvit_ultra_weight_codes": [_c_p, _i64, _i64, _i64, _i32, _c_p, _i64, _i64, _c_p, _c_p, _c_p],
    "qvit_ultra_bn_fold": [_c_p, _c_p, _c_p, _c_p, _f32, _i64, _c_p, _c_p, _c_p],
    "qvit_ultra_conv0": [_c_p, _i64, _i64, _i64, _c_p, _c_p, _c_p, _i32, _c_p, _c_p],
    "qvit_ultra_conv": [_c_p, _i64, _i64, _i64, _i64, _i64, _c_p, _i64, _i64, _i32, _i32, _c_p, _c_p, _i32, _c_p,
                        _i64, _c_p],
    "qvit_ultra_tail": [_c_p, _i64, _i64, _i64, _c_p, _i64, _c_p, _c_p, _c_p, _i64, _c_p, _i64, _i32, _i32, _c_p,
                        _i64, _c_p, _i64, _i64, _f32, _c_p, _c_p, _c_p],
    "qvit_ultra_conv0_int": [_c_p, _i64, _i64, _i64, _c_p, _c_p, _c_p, _i32, _i32, _c_p, _c_p],
    "qvit_ultra_conv_int": [_c_p, _i64, _i64, _i64, _i64, _i64, _c_p, _i64, _i64, _c_p, _c_p, _i32, _i32, _i32,
                            _c_p, _i64, _c_p],
    "qvit_yolo_decode": [_c_p, _i64, _i64, _i64, _i64, _i64, _i64, _c_p, _f32, _c_p, _c_p, _c_p],
    "qvit_ultra_weight_quant_backward": [_c_p, _c_p, _i64, _i32, _c_p, _c_p, _i64, _c_p],
    "qvit_ultra_act_quant_backward": [_c_p, _c_p, _i64, _c_p, _c_p],
    "qvit_conv_wgrad": [_c_p, _c_p, _i64, _i64, _i64, _i64, _i64, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32,
                        _i32, _c_p, _c_p, _i64, _c_p],
    "qvit_bn_stats": [_c_p, _i64, _i64, _i64, _i64, _f64, _f64, _c_p, _c_p, _c_p, _c_p, _c_p, _c_p, _i64, _c_p],
    "qvit_bn_act_pool_forward": [_c_p, _i64, _i64, _i64, _i64, _c_p, _c_p, _c_p, _c_p, _i32, _i32, _c_p, _c_p, _c_p],
    "qvit_bn_act_pool_backward_reduce": [_c_p, _c_p, _c_p, _i64, _i64, _i64, _i64, _c_p, _c_p, _i32, _c_p, _c_p, _i64,
                                         _c_p],
    "qvit_bn_act_pool_backward_dx": [_c_p, _c_p, _c_p, _i64, _i64, _i64, _i64, _c_p, _c_p, _c_p, _c_p, _i32, _c_p,
                                     _c_p, _c_p, _c_p],
    "qvit_attention": [_c_p, _i64, _i64, _i64, _i64, _i64, _f32, _f32, _i32, _c_p, _i64, _i32, _c_p, _c_p, _c_p,
                       _i32, _c_p],
    "qvit_gemm_qkv_split": [_c_p, _i64, _i64, _i64, _c_p, _i32, _i64, _i64, _c_p, _c_p, _c_p, _i64, _f32, _c_p,
                            _c_p, _c_p],
    "qvit_gemm_qkv_split_hd": [_c_p, _i64, _i64, _i64, _c_p, _i32, _i64, _i64, _c_p, _c_p, _c_p, _i64, _i64, _f32, _c_p,
                               _c_p, _c_p],
    "qvit_qkv_attention": [_c_p, _i64, _i64, _i64, _i64, _c_p, _i32, _i64, _c_p, _c_p, _c_p, _i64, _i64, _f32, _f32,
                           _i32, _c_p, _i64, _i32, _c_p, _c_p, _c_p, _i32, _c_p, _c_p],
    "qvit_qkv_attention_q": [_c_p, _i64, _i64, _i64, _i64, _i64, _c_p, _i32, _i64, _c_p, _c_p, _c_p, _i64, _i64, _f32,
                             _f32, _i32, _c_p, _i64, _i32, _c_p, _c_p, _c_p, _i32, _c_p, _c_p],
    "qvit_attention_split": [_c_p, _c_p, _i64, _i64, _i64, _i64, _f32, _f32, _i32, _c_p, _i64, _i32, _c_p, _c_p,
                             _c_p, _i32, _c_p, _c_p],
    "qvit_attention_backward": [_c_p, _c_p, _c_p, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _f32, _f32, _f32, _c_p,
                                _i64, _c_p, _i64, _c_p],
}
# name -> argtypes of the entry points returning int64_t
INT64_FUNCS = {
    "qvit_quant_backward_workspace_bytes": [_i64],
    "qvit_quant_error_workspace_bytes": [_i64, _i64, _i32],
    "qvit_layernorm_quant_backward_workspace_bytes": [_i64, _i64],
    "qvit_gelu_quant_backward_workspace_bytes": [_i64],
    "qvit_attention_backward_workspace_bytes": [_i64, _i64, _i64],
    "qvit_gemm_wgrad_workspace_bytes": [_i64, _i64, _i64],
    "qvit_col2im_quant_backward_workspace_bytes": [_i64, _i64, _i64, _i64, _i32, _i32, _i32, _i32, _i32, _i32, _i32,
                                                   _i32],
    "qvit_ultra_weight_quant_backward_workspace_bytes": [_i64],
    "qvit_conv_wgrad_workspace_bytes": [_i64, _i64, _i64, _i64, _i64, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32],
    "qvit_bn_stats_workspace_bytes": [_i64, _i64, _i64, _i64],
    "qvit_bn_act_pool_backward_workspace_bytes": [_i64, _i64, _i64, _i64, _i32],
}
STRING_FUNCS = {"qvit_strerror": [_i32], "qvit_version": []}
EXPORTED_SYMBOLS = sorted(list(_SIGNATURES) + list(INT64_FUNCS) + list(STRING_FUNCS))

_lock = threading.Lock()
_lib: Optional[ctypes.CDLL] = None


class QvitError(RuntimeError):
    pass


def load(path: str = LIB_PATH) -> ctypes.CDLL:
    """Loads libqvit_hip.so (no compute). Raises if it is absent: there is no fallback path."""
    global _lib
    with _lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(path):
            raise QvitError(
                f"{path} is missing: build it with `python -m quantized_vit_amd.build` "
                "(the HIP extension is required; there is no CPU fallback)")
        lib = ctypes.CDLL(path, mode=ctypes.RTLD_GLOBAL)
        for name, args in _SIGNATURES.items():
            if path != LIB_PATH and not hasattr(lib, name):
                continue  # an older build loaded for a same-box A/B (tools/lib_ab.sh): its entry points only
            fn = getattr(lib, name)
            fn.argtypes = args
            fn.restype = ctypes.c_int
        for name, args in INT64_FUNCS.items():
            if path != LIB_PATH and not hasattr(lib, name):
                continue
            fn = getattr(lib, name)
            fn.argtypes = args
            fn.restype = ctypes.c_int64
        for name, args in STRING_FUNCS.items():
            fn = getattr(lib, name)
            fn.argtypes = args
            fn.restype = ctypes.c_char_p
        _lib = lib
        return lib


def version() -> str:
    return load().qvit_version().decode()


def build_id(path: Optional[str] = None) -> Optional[str]:
    """Identity of a library build: the digest of its build inputs (sources, headers, build script, flags and
    defines; build.py writes it beside the library as <lib>.srcsha), so a rebuild from the same inputs keeps its
    id. Profile JSONs record the build they were measured on, and bench.py merges their counters
    only into a line timed on that same build. A library without a digest file falls back to its bytes' sha256."""
    import hashlib
    p = path or (getattr(_lib, "_name", None) if _lib is not None else None) or LIB_PATH
    try:
        with open(p + ".srcsha") as f:
            digest = f.read().strip()
        if digest:
            return "src-" + digest[:16]
    except OSError:
        pass
    try:
        with open(p, "rb") as f:
            return hashlib.sha256(f.read()).hexdigest()[:16]
    except OSError:
        return None


def _check(code: int, what: str) -> None:
    if code != 0:
        msg = load().qvit_strerror(code).decode()
        raise QvitError(f"{what} failed: {msg} (status {code})")


def _ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def _stream(dev: torch.device) -> int:
    return torch.cuda.current_stream(dev).cuda_stream


def _require_gpu(t: torch.Tensor, name: str) -> None:
    if not t.is_cuda:
        raise QvitError(f"{name} must be a ROCm device tensor (got {t.device}); the HIP path has no CPU fallback")


# ---- wrappers -------------------------------------------------------------------------------
def quantize_act_i8(x2d: torch.Tensor, qtype: int, d: Optional[torch.Tensor], qm: Optional[torch.Tensor],
                    t: Optional[torch.Tensor], levels: int, out: torch.Tensor, kpad: int) -> torch.Tensor:
    _require_gpu(x2d, "input")
    assert x2d.dtype == torch.float32 and x2d.dim() == 2 and x2d.stride(1) == 1
    rows, cols = x2d.shape
    _check(load().qvit_quantize_act_i8(_ptr(x2d), rows, cols, x2d.stride(0), qtype, _ptr(d), _ptr(qm), _ptr(t),
                                       levels, _ptr(out), out.stride(0), kpad, _stream(x2d.device)),
           "qvit_quantize_act_i8")
    return out


def fake_quant_f32(x: torch.Tensor, qtype: int, d: Optional[torch.Tensor], qm: Optional[torch.Tensor],
                   t: Optional[torch.Tensor], levels: int = 0) -> torch.Tensor:
    _require_gpu(x, "input")
    xc = x.contiguous().float()
    y = torch.empty_like(xc)
    _check(load().qvit_fake_quant_f32(_ptr(xc), xc.numel(), qtype, _ptr(d), _ptr(qm), _ptr(t), levels, _ptr(y),
                                      _stream(x.device)), "qvit_fake_quant_f32")
    return y


def quant_backward(x: torch.Tensor, grad_out: torch.Tensor, qtype: int, d: torch.Tensor, qm: torch.Tensor,
                   t: Optional[torch.Tensor], clip_lo: float, clip_hi: float, dge_k: float = 0.0,
                   grad_x: Optional[torch.Tensor] = None):
    """Backward of the fake quantizer over x (qvit_quant_backward). Returns (grad_x, scalars): grad_x shaped as x
    (written into `grad_x` when given; it may be grad_out itself) and the float32 [3] sums for d_quant, q_m and
    t_quant, on the device (no host sync)."""
    _require_gpu(x, "input")
    _require_gpu(grad_out, "grad_out")
    xc = x.detach().contiguous().float()
    gc = grad_out.detach().contiguous().float()
    if xc.numel() != gc.numel():
        raise QvitError(f"quant_backward: grad_out has {gc.numel()} elements for an input of {xc.numel()}")
    if grad_x is None:
        grad_x = torch.empty_like(xc)
    assert grad_x.is_cuda and grad_x.dtype == torch.float32 and grad_x.is_contiguous() and \
        grad_x.numel() == xc.numel()
    n = xc.numel()
    lib = load()
    nbytes = int(lib.qvit_quant_backward_workspace_bytes(n))
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device=xc.device)
    scalars = torch.empty(3, dtype=torch.float32, device=xc.device)
    _check(lib.qvit_quant_backward(_ptr(xc), _ptr(gc), n, qtype, _ptr(d), _ptr(qm), _ptr(t), float(clip_lo),
                                   float(clip_hi), float(dge_k), _ptr(grad_x), _ptr(scalars), _ptr(ws), nbytes,
                                   _stream(xc.device)), "qvit_quant_backward")
    return grad_x, scalars


QUANT_ERROR_MAX_CAND = 64


def quant_error(x2d: torch.Tensor, qtype: int, d: torch.Tensor, q_m: torch.Tensor, t: Optional[torch.Tensor],
                err: Optional[torch.Tensor] = None, nclip: Optional[torch.Tensor] = None, accumulate: bool = False):
    """Squared quantization error and clip count of x2d (fp32 [rows, cols], unit column stride, any row stride) under
    the candidates (d[c], q_m[c]) at one t (qvit_quant_error). Returns (err float64 [ncand], nclip int64 [ncand]) on
    the device, no host sync; given buffers are written, or added to under `accumulate`."""
    _require_gpu(x2d, "input")
    if x2d.dtype != torch.float32 or x2d.dim() != 2 or (x2d.shape[1] > 1 and x2d.stride(1) != 1):
        raise QvitError(f"quant_error: the input must be a float32 matrix with unit column stride (got {x2d.dtype}, "
                        f"shape {tuple(x2d.shape)}, strides {tuple(x2d.stride())})")
    dev = x2d.device
    ncand = d.numel()
    for name, v in (("d", d), ("q_m", q_m)):
        if not (v.is_cuda and v.dtype == torch.float32 and v.dim() == 1 and v.is_contiguous() and v.numel() == ncand):
            raise QvitError(f"quant_error: {name} must be a contiguous float32 device vector of {ncand} candidates")
    if accumulate and (err is None or nclip is None):
        raise QvitError("quant_error: accumulate needs the err and nclip buffers to add to")
    if err is None:
        err = torch.empty(ncand, dtype=torch.float64, device=dev)
    if nclip is None:
        nclip = torch.empty(ncand, dtype=torch.int64, device=dev)
    for name, v, dt in (("err", err, torch.float64), ("nclip", nclip, torch.int64)):
        if not (v.is_cuda and v.dtype == dt and v.is_contiguous() and v.numel() == ncand):
            raise QvitError(f"quant_error: {name} must be a contiguous {dt} device vector of {ncand} elements")
    rows, cols = x2d.shape
    ldx = x2d.stride(0) if rows > 1 else max(cols, x2d.stride(0))
    lib = load()
    ws = _workspace(int(lib.qvit_quant_error_workspace_bytes(rows, cols, ncand)), "qvit_quant_error_workspace_bytes",
                    None, dev)
    _check(lib.qvit_quant_error(_ptr(x2d) if x2d.numel() else None, rows, cols, ldx, qtype, _ptr(d), _ptr(q_m), _ptr(t),
                                ncand, int(bool(accumulate)), _ptr(err), _ptr(nclip), _ptr(ws),
                                ws.numel() * ws.element_size(), _stream(dev)), "qvit_quant_error")
    return err, nclip


def qat_step(tensors: torch.Tensor, ntensors: int, chunks: torch.Tensor, nchunks: int, hyper: tuple) -> None:
    """One dense optimizer step over the device descriptor table (qvit_qat_step). `hyper`: (variant, first_step, lr,
    lr_quant, first_momentum, second_momentum, alpha1, alpha2, weight_decay, bias_correction1, bias_correction2,
    clip_lo, clip_hi) as include/qvit_hip.h lists them."""
    _require_gpu(tensors, "tensor table")
    _require_gpu(chunks, "chunk list")
    _check(load().qvit_qat_step(_ptr(tensors), ntensors, _ptr(chunks), nchunks, *hyper, _stream(tensors.device)),
           "qvit_qat_step")


def qat_quant_step(quants: torch.Tensor, nquants: int, bits: torch.Tensor, stage: int, first_fix: bool, hyper: tuple,
                   bit_ranges: tuple) -> None:
    """The quantizer scalars' step and projection (qvit_qat_quant_step). `bit_ranges`: (min_bit_wt, max_bit_wt,
    min_bit_act, max_bit_act)."""
    _require_gpu(quants, "quantizer table")
    assert bits.is_cuda and bits.dtype == torch.int32 and bits.is_contiguous() and bits.numel() >= nquants
    _check(load().qvit_qat_quant_step(_ptr(quants), nquants, _ptr(bits), stage, int(bool(first_fix)), *hyper,
                                      *bit_ranges, _stream(quants.device)), "qvit_qat_quant_step")


def prune_scores(groups: torch.Tensor, ngroups: int, members: torch.Tensor, nmembers: int, items: torch.Tensor,
                 nitems: int, sums: torch.Tensor, weights: tuple, scores: torch.Tensor, hyper: tuple,
                 units: Optional[torch.Tensor] = None, nunits: int = 0,
                 unit_sums: Optional[torch.Tensor] = None) -> None:
    """The saliency score of every listed row (qvit_prune_scores, then qvit_prune_scores_finish). `weights`: the five
    criteria weights in the header's order; `sums` float64 [nitems, 3] and `scores` float32 [nitems] are written.
    With `units` (some group's unit is a set of rows) qvit_prune_scores_fold runs between the two: `unit_sums`
    float64 [nunits, 3] and `scores` float32 [nunits] are written."""
    _require_gpu(groups, "group table")
    nscores = nitems if units is None else nunits
    assert sums.dtype == torch.float64 and sums.numel() >= 3 * nitems and scores.dtype == torch.float32 and \
        scores.numel() >= nscores
    lib, st = load(), _stream(groups.device)
    _check(lib.qvit_prune_scores(_ptr(groups), ngroups, _ptr(members), nmembers, _ptr(items), nitems, _ptr(sums),
                                 *hyper, st), "qvit_prune_scores")
    if units is not None:
        assert unit_sums is not None and unit_sums.dtype == torch.float64 and unit_sums.numel() >= 3 * nunits
        _check(lib.qvit_prune_scores_fold(_ptr(groups), ngroups, _ptr(items), nitems, _ptr(sums), _ptr(units), nunits,
                                          _ptr(unit_sums), st), "qvit_prune_scores_fold")
        items, nitems, sums = units, nunits, unit_sums
    _check(lib.qvit_prune_scores_finish(_ptr(groups), ngroups, _ptr(items), nitems, _ptr(sums),
                                        *[float(w) for w in weights], _ptr(scores), st), "qvit_prune_scores_finish")


def prune_joint_scalars(quants: torch.Tensor, nquants: int, hyper: tuple, min_bit_act: int, max_bit_act: int) -> None:
    """The quantizer scalars of the joint groups' layers (qvit_prune_joint_scalars)."""
    _require_gpu(quants, "quantizer table")
    _check(load().qvit_prune_joint_scalars(_ptr(quants), nquants, *hyper, min_bit_act, max_bit_act,
                                           _stream(quants.device)), "qvit_prune_joint_scalars")


def prune_joint_reduce(groups: torch.Tensor, ngroups: int, members: torch.Tensor, nmembers: int, items: torch.Tensor,
                       nitems: int, partials: torch.Tensor, hyper: tuple) -> None:
    _require_gpu(groups, "group table")
    assert partials.dtype == torch.float64 and partials.numel() >= 6 * nitems
    _check(load().qvit_prune_joint_reduce(_ptr(groups), ngroups, _ptr(members), nmembers, _ptr(items), nitems,
                                          _ptr(partials), *hyper, _stream(groups.device)), "qvit_prune_joint_reduce")


def prune_joint_finish(groups: torch.Tensor, ngroups: int, partials: torch.Tensor, npartials: int, lr: float,
                       period: int, t_in_period: int, min_bit_wt: int, max_bit_wt: int, gamma: torch.Tensor,
                       info: torch.Tensor) -> None:
    _require_gpu(groups, "group table")
    assert partials.dtype == torch.float64 and partials.numel() >= 6 * npartials
    assert gamma.dtype == torch.float32 and gamma.numel() >= ngroups and info.dtype == torch.int32 and \
        info.numel() >= ngroups
    _check(load().qvit_prune_joint_finish(_ptr(groups), ngroups, _ptr(partials), npartials, float(lr), period,
                                          t_in_period, min_bit_wt, max_bit_wt, _ptr(gamma), _ptr(info),
                                          _stream(groups.device)), "qvit_prune_joint_finish")


def prune_joint_apply(groups: torch.Tensor, ngroups: int, members: torch.Tensor, nmembers: int, items: torch.Tensor,
                      nitems: int, gamma: torch.Tensor, hyper: tuple) -> None:
    _require_gpu(groups, "group table")
    assert gamma.dtype == torch.float32 and gamma.numel() >= ngroups
    _check(load().qvit_prune_joint_apply(_ptr(groups), ngroups, _ptr(members), nmembers, _ptr(items), nitems,
                                         _ptr(gamma), *hyper, _stream(groups.device)), "qvit_prune_joint_apply")


def gelu_f32(x: torch.Tensor) -> torch.Tensor:
    """nn.GELU() bit-identical to torch's ATen CPU kernel (qvit_gelu_f32)."""
    _require_gpu(x, "input")
    xc = x.contiguous().float()
    y = torch.empty_like(xc)
    _check(load().qvit_gelu_f32(_ptr(xc), xc.numel(), _ptr(y), _stream(x.device)), "qvit_gelu_f32")
    return y


LN_BWD_MAX_COLS = 2048   # train_fuse.hip kLnMaxCols: a row of the LayerNorm backward stays in one wave's registers


def _rows_ok(t: torch.Tensor) -> bool:
    """fp32 device rows the train-fusion kernels take: unit column stride, row stride % 4, 16-byte base."""
    return (t.is_cuda and t.dtype == torch.float32 and t.dim() == 2 and t.stride(1) == 1 and t.stride(0) % 4 == 0
            and t.stride(0) >= t.shape[1] and t.data_ptr() % 16 == 0)


def layernorm_quant_backward_fits(x2d: torch.Tensor, gamma: Optional[torch.Tensor],
                                  beta: Optional[torch.Tensor]) -> bool:
    """Whether qvit_layernorm_quant_backward takes these rows (its alignment rules; else QVIT_EALIGN)."""
    cols = x2d.shape[1] if x2d.dim() == 2 else 0
    vec = lambda v: (v is not None and v.is_cuda and v.dtype == torch.float32 and v.is_contiguous()
                     and v.numel() == cols and v.data_ptr() % 16 == 0)
    return _rows_ok(x2d) and cols % 4 == 0 and 0 < cols <= LN_BWD_MAX_COLS and vec(gamma) and vec(beta)


def layernorm_quant_backward(x2d: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, eps: float, qtype: int,
                             d: torch.Tensor, qm: torch.Tensor, t: Optional[torch.Tensor], clip_lo: float,
                             clip_hi: float, grad_y: torch.Tensor, grad_x: Optional[torch.Tensor] = None,
                             want_gamma: bool = True, want_beta: bool = True):
    """Backward of layernorm_quant_i8 (qvit_layernorm_quant_backward): x2d the LayerNorm input [rows, cols], grad_y
    the gradient with respect to the quantizer's output. Returns (grad_x, grad_gamma, grad_beta, scalars): grad_x
    [rows, cols] (written into `grad_x` when given; it may be grad_y itself), the affine gradients (None where not
    wanted: that reduction is skipped) and the float32 [3] sums for d_quant, q_m, t_quant, all on the device."""
    _require_gpu(x2d, "input")
    _require_gpu(grad_y, "grad_y")
    assert x2d.dtype == torch.float32 and grad_y.dtype == torch.float32 and x2d.dim() == 2
    assert x2d.stride(1) == 1 and grad_y.stride(1) == 1 and tuple(grad_y.shape) == tuple(x2d.shape)
    rows, cols = x2d.shape
    if grad_x is None:
        grad_x = torch.empty((rows, cols), dtype=torch.float32, device=x2d.device)
    assert grad_x.is_cuda and grad_x.dtype == torch.float32 and grad_x.stride(1) == 1 and \
        tuple(grad_x.shape) == (rows, cols)
    lib = load()
    nbytes = int(lib.qvit_layernorm_quant_backward_workspace_bytes(rows, cols))
    if nbytes < 0:
        _check(nbytes, "qvit_layernorm_quant_backward_workspace_bytes")
    ws = torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=x2d.device)
    gg = torch.empty(cols, dtype=torch.float32, device=x2d.device) if want_gamma else None
    gb = torch.empty(cols, dtype=torch.float32, device=x2d.device) if want_beta else None
    scalars = torch.empty(3, dtype=torch.float32, device=x2d.device)
    _check(lib.qvit_layernorm_quant_backward(_ptr(x2d), rows, cols, x2d.stride(0), _ptr(gamma), _ptr(beta),
                                             float(eps), qtype, _ptr(d), _ptr(qm), _ptr(t), float(clip_lo),
                                             float(clip_hi), _ptr(grad_y), grad_y.stride(0), _ptr(grad_x),
                                             grad_x.stride(0), _ptr(gg), _ptr(gb), _ptr(scalars), _ptr(ws),
                                             ws.numel() * 8, _stream(x2d.device)), "qvit_layernorm_quant_backward")
    return grad_x, gg, gb, scalars


def gelu_quant_i8(h2d: torch.Tensor, qtype: int, d: Optional[torch.Tensor], qm: Optional[torch.Tensor],
                  t: Optional[torch.Tensor], levels: int, out: torch.Tensor, kpad: int) -> torch.Tensor:
    """codes = quantize(GELU(h)) (qvit_gelu_quant_i8): quantize_act_i8(gelu_f32(h)) byte for byte, in one pass."""
    _require_gpu(h2d, "input")
    assert h2d.dtype == torch.float32 and h2d.dim() == 2 and h2d.stride(1) == 1
    rows, cols = h2d.shape
    _check(load().qvit_gelu_quant_i8(_ptr(h2d), rows, cols, h2d.stride(0), qtype, _ptr(d), _ptr(qm), _ptr(t), levels,
                                     _ptr(out), out.stride(0), kpad, _stream(h2d.device)), "qvit_gelu_quant_i8")
    return out


def gelu_quant_backward(h: torch.Tensor, grad_y: torch.Tensor, qtype: int, d: torch.Tensor, qm: torch.Tensor,
                        t: Optional[torch.Tensor], clip_lo: float, clip_hi: float,
                        grad_h: Optional[torch.Tensor] = None):
    """Backward of gelu_quant_i8 (qvit_gelu_quant_backward) over contiguous h: (grad_h, scalars) as quant_backward
    (grad_h may be grad_y itself)."""
    _require_gpu(h, "input")
    _require_gpu(grad_y, "grad_y")
    assert h.dtype == torch.float32 and grad_y.dtype == torch.float32 and h.is_contiguous() and \
        grad_y.is_contiguous() and h.numel() == grad_y.numel()
    if grad_h is None:
        grad_h = torch.empty_like(h)
    assert grad_h.is_cuda and grad_h.dtype == torch.float32 and grad_h.is_contiguous() and \
        grad_h.numel() == h.numel()
    n = h.numel()
    lib = load()
    nbytes = int(lib.qvit_gelu_quant_backward_workspace_bytes(n))
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device=h.device)
    scalars = torch.empty(3, dtype=torch.float32, device=h.device)
    _check(lib.qvit_gelu_quant_backward(_ptr(h), _ptr(grad_y), n, qtype, _ptr(d), _ptr(qm), _ptr(t), float(clip_lo),
                                        float(clip_hi), _ptr(grad_h), _ptr(scalars), _ptr(ws), nbytes,
                                        _stream(h.device)), "qvit_gelu_quant_backward")
    return grad_h, scalars


def pack_weight(w2d: torch.Tensor, qtype: int, d: torch.Tensor, qm: torch.Tensor, t: Optional[torch.Tensor],
                wfmt: int, npad: int, kpad: int, overflow: Optional[torch.Tensor]) -> torch.Tensor:
    _require_gpu(w2d, "weight")
    assert w2d.dtype == torch.float32 and w2d.stride(1) == 1
    n, k = w2d.shape
    nbytes = npad * kpad // 2 if wfmt == W4 else npad * kpad
    packed = torch.empty(nbytes, dtype=torch.uint8, device=w2d.device)
    _check(load().qvit_pack_weight(_ptr(w2d), n, k, w2d.stride(0), qtype, _ptr(d), _ptr(qm), _ptr(t), wfmt,
                                   _ptr(packed), npad, kpad, _ptr(overflow), _stream(w2d.device)),
           "qvit_pack_weight")
    return packed


def code_quantizer(device: torch.device) -> tuple:
    """(qtype, d, q_m, t) under which qvit_pack_weight reproduces integer-valued inputs exactly: the linear
    quantizer at d = 1 rounds an integer to itself, and q_m = 1024 exceeds every int8 code, so nothing is clipped."""
    return QT_LINEAR, torch.ones(1, device=device), torch.full((1,), 1024.0, device=device), None


def pack_codes(codes: torch.Tensor, wfmt: int, npad: int, kpad: int,
               overflow: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The W4 / W8 image of integer weight codes (fp32 [n, k] rows on the device), exact. `overflow`: the int32
    word a code outside the format is counted in; without one a fresh word is used and nothing is read back."""
    if overflow is None:
        overflow = torch.zeros(1, dtype=torch.int32, device=codes.device)
    return pack_weight(codes, *code_quantizer(codes.device), wfmt, npad, kpad, overflow)


def pack_weight_w4r(packed: torch.Tensor, npad: int, kpad: int) -> torch.Tensor:
    """The register-weight image (wfmt W4R) of a W4 image from pack_weight (qvit_pack_weight_w4r): same bytes,
    re-ordered per GEMM lane; qvit_gemm gives the W4 results on it."""
    _require_gpu(packed, "packed weights")
    assert packed.dtype == torch.uint8 and packed.is_contiguous() and packed.numel() == npad * kpad // 2
    out = torch.empty_like(packed)
    _check(load().qvit_pack_weight_w4r(_ptr(packed), npad, kpad, _ptr(out), _stream(packed.device)),
           "qvit_pack_weight_w4r")
    return out


def pack_weight_w8r(packed: torch.Tensor, npad: int, kpad: int) -> torch.Tensor:
    """The int8 register image (wfmt W8R) of a W4 image from pack_weight (qvit_pack_weight_w8r): npad * kpad
    bytes, each code as the byte 16 k in the GEMM lanes' operand order; qvit_gemm gives the W4 results on it."""
    _require_gpu(packed, "packed weights")
    assert packed.dtype == torch.uint8 and packed.is_contiguous() and packed.numel() == npad * kpad // 2
    out = torch.empty(npad * kpad, dtype=torch.uint8, device=packed.device)
    _check(load().qvit_pack_weight_w8r(_ptr(packed), npad, kpad, _ptr(out), _stream(packed.device)),
           "qvit_pack_weight_w8r")
    return out


def pack_weight_wide(codes: torch.Tensor, npad: int, kpad: int):
    """Packs integer weight codes beyond int8 ([n, k] float, on the device) for qvit_gemm_wonly as balanced
    base-256 digits, one W8 image per digit, most significant first: W16 (k = 256 h + l, |k| <= 32639) or W24
    (k = 65536 a + 256 h + l, |k| < 2^23). Returns (packed, wfmt)."""
    _require_gpu(codes, "weight codes")
    c = codes.detach().float().contiguous()
    cmax = float(c.abs().max()) if c.numel() else 0.0
    if cmax >= 2 ** 23:
        raise QvitError("pack_weight_wide: a weight code reaches 2^23")
    ndig = 2 if cmax <= 32639 else 3
    digits = []
    r = c
    for _ in range(ndig):
        d = torch.remainder(r + 128.0, 256.0) - 128.0   # in [-128, 127]
        digits.append(d)
        r = (r - d) / 256.0                              # exact: r - d is a multiple of 256
    if float(r.abs().max()) if r.numel() else 0.0:
        raise QvitError("pack_weight_wide: codes do not fit the digits")
    exact = code_quantizer(c.device)   # one pair of scalars and one overflow word for all the digits
    ovf = torch.zeros(1, dtype=torch.int32, device=c.device)
    imgs = [pack_weight(d.contiguous(), *exact, W8, npad, kpad, ovf) for d in reversed(digits)]
    if int(ovf.item()) != 0:
        raise QvitError("pack_weight_wide: a digit left the int8 range")
    return torch.cat(imgs), (W16 if ndig == 2 else W24)


def pad_bias(bias: Optional[torch.Tensor], n: int, npad: int, device: torch.device) -> torch.Tensor:
    out = torch.empty(npad, dtype=torch.float32, device=device)
    b = None if bias is None else bias.detach().contiguous().float()
    _check(load().qvit_pad_bias(_ptr(b), n, _ptr(out), npad, _stream(device)), "qvit_pad_bias")
    return out


def im2col_quant_i8(x: torch.Tensor, kh: int, kw: int, sh: int, sw: int, ph: int, pw: int, dh: int, dw: int,
                    qtype: int, d, qm, t, levels: int, out: torch.Tensor, kpad: int) -> torch.Tensor:
    _require_gpu(x, "input")
    assert x.dtype == torch.float32 and x.is_contiguous() and x.dim() == 4
    B, C, H, W = x.shape
    _check(load().qvit_im2col_quant_i8(_ptr(x), B, C, H, W, kh, kw, sh, sw, ph, pw, dh, dw, qtype, _ptr(d),
                                       _ptr(qm), _ptr(t), levels, _ptr(out), out.stride(0), kpad,
                                       _stream(x.device)), "qvit_im2col_quant_i8")
    return out


def u8_image_layout(img: torch.Tensor) -> Tuple[torch.Tensor, int]:
    """(tensor, layout) the uint8 kernels read for a [B, C, H, W] uint8 image: a contiguous tensor as it is (NCHW), a
    channels_last one in place (NHWC: a decoder's [B, H, W, C] output seen through permute), anything else after
    one contiguous copy."""
    assert img.dtype == torch.uint8 and img.dim() == 4
    if img.is_contiguous():
        return img, U8_NCHW
    if img.is_contiguous(memory_format=torch.channels_last):
        return img, U8_NHWC
    return img.contiguous(), U8_NCHW


def im2col_u8_i8(img: torch.Tensor, kh: int, kw: int, sh: int, sw: int, ph: int, pw: int, dh: int, dw: int,
                 code_table: torch.Tensor, out: torch.Tensor, kpad: int) -> torch.Tensor:
    """im2col codes of a uint8 [B, C, H, W] image through the int8 [C, 256] code table (qvit_im2col_u8_i8)."""
    _require_gpu(img, "input")
    img, layout = u8_image_layout(img)
    B, C, H, W = img.shape
    assert code_table.dtype == torch.int8 and code_table.is_contiguous() and tuple(code_table.shape) == (C, 256)
    _check(load().qvit_im2col_u8_i8(_ptr(img), B, C, H, W, layout, kh, kw, sh, sw, ph, pw, dh, dw, _ptr(code_table),
                                    _ptr(out), out.stride(0), kpad, _stream(img.device)), "qvit_im2col_u8_i8")
    return out


def u8_normalize_f32(img: torch.Tensor, value_table: torch.Tensor) -> torch.Tensor:
    """value_table[c][img[b, c, y, x]] as a contiguous fp32 NCHW tensor (qvit_u8_normalize_f32)."""
    _require_gpu(img, "input")
    img, layout = u8_image_layout(img)
    B, C, H, W = img.shape
    assert value_table.dtype == torch.float32 and value_table.is_contiguous() and \
        tuple(value_table.shape) == (C, 256)
    out = torch.empty((B, C, H, W), dtype=torch.float32, device=img.device)
    _check(load().qvit_u8_normalize_f32(_ptr(img), B, C, H, W, layout, _ptr(value_table), _ptr(out),
                                        _stream(img.device)), "qvit_u8_normalize_f32")
    return out


def layernorm_quant_i8(x2d: torch.Tensor, gamma: Optional[torch.Tensor], beta: Optional[torch.Tensor], eps: float,
                       qtype: int, d, qm, t, levels: int, out: torch.Tensor, kpad: int,
                       code_table: Optional[torch.Tensor] = None) -> torch.Tensor:
    """LayerNorm + activation quantizer -> int8 codes (code_table: EPI_I8 table of the quantizer, optional)."""
    _require_gpu(x2d, "input")
    assert x2d.dtype == torch.float32 and x2d.stride(1) == 1
    rows, cols = x2d.shape
    _check(load().qvit_layernorm_quant_i8(_ptr(x2d), rows, cols, x2d.stride(0), _ptr(gamma), _ptr(beta), eps, qtype,
                                          _ptr(d), _ptr(qm), _ptr(t), levels, _ptr(out), out.stride(0), kpad,
                                          _ptr(code_table), _stream(x2d.device)), "qvit_layernorm_quant_i8")
    return out


def gemm(A: torch.Tensor, M: int, K: int, packed: torch.Tensor, wfmt: int, N: int, npad: int,
         d_act: Optional[torch.Tensor], d_wt: Optional[torch.Tensor], bias_pad: Optional[torch.Tensor],
         epilogue: int, C: torch.Tensor, out_qtype: int = 0, out_d=None, out_qm=None, out_t=None,
         out_levels: int = 0, epi_table: Optional[torch.Tensor] = None) -> torch.Tensor:
    _require_gpu(A, "codes")
    _check(load().qvit_gemm(_ptr(A), M, K, A.stride(0), _ptr(packed), wfmt, N, npad, _ptr(d_act), _ptr(d_wt),
                            _ptr(bias_pad), epilogue, _ptr(C), C.stride(0), out_qtype, _ptr(out_d), _ptr(out_qm),
                            _ptr(out_t), out_levels, _ptr(epi_table), _stream(A.device)), "qvit_gemm")
    return C


def t32_rows(M: int) -> int:
    """Rows a QVIT_ACT_T32 code buffer holds for M rows (whole 64-row wave tiles of qvit_gemm_a32)."""
    return (M + 63) // 64 * 64


def t32_to_rows(codes_t32: torch.Tensor, M: int, kpad: int) -> torch.Tensor:
    """QVIT_ACT_T32 codes -> row-major [M, kpad] (a view permutation; tests and code tracing only)."""
    R = t32_rows(M)
    t = codes_t32.view(-1)[:R * kpad].view(R // 32, kpad // 32, 2, 32, 16)   # [rb][kb][half][row][16]
    return t.permute(0, 3, 1, 2, 4).reshape(R, kpad)[:M]


def rows_to_t32(codes: torch.Tensor, kpad: int) -> torch.Tensor:
    """Row-major [M, >= kpad] codes -> a QVIT_ACT_T32 buffer (rows padded with zeros; tests only)."""
    M = codes.shape[0]
    R = t32_rows(M)
    full = torch.zeros((R, kpad), dtype=torch.int8, device=codes.device)
    full[:M] = codes[:, :kpad]
    return full.view(R // 32, 32, kpad // 32, 2, 16).permute(0, 2, 3, 1, 4).contiguous().view(-1)


def layernorm_quant_i8_t32(x2d: torch.Tensor, gamma: Optional[torch.Tensor], beta: Optional[torch.Tensor], eps: float,
                           qtype: int, d, qm, t, levels: int, out: torch.Tensor, kpad: int,
                           code_table: Optional[torch.Tensor] = None) -> torch.Tensor:
    """layernorm_quant_i8 with the codes in QVIT_ACT_T32 order (out: int8, >= t32_rows(M) * kpad bytes)."""
    _require_gpu(x2d, "input")
    assert x2d.dtype == torch.float32 and x2d.stride(1) == 1
    rows, cols = x2d.shape
    assert out.numel() >= t32_rows(rows) * kpad
    _check(load().qvit_layernorm_quant_i8_t32(_ptr(x2d), rows, cols, x2d.stride(0), _ptr(gamma), _ptr(beta), eps,
                                              qtype, _ptr(d), _ptr(qm), _ptr(t), levels, _ptr(out), kpad,
                                              _ptr(code_table), _stream(x2d.device)), "qvit_layernorm_quant_i8_t32")
    return out


def gemm_a32_fits(K: int, wfmt: int, N: int, npad: int, epilogue: int) -> bool:
    lib = load()
    if not hasattr(lib, "qvit_gemm_a32_fits"):  # (an older build in a same-box A/B)
        return False
    return bool(lib.qvit_gemm_a32_fits(K, wfmt, N, npad, epilogue))


def gemm_a32(A: torch.Tensor, M: int, K: int, packed: torch.Tensor, wfmt: int, N: int, npad: int, d_act, d_wt,
             bias_pad: Optional[torch.Tensor], epilogue: int, C: torch.Tensor, out_qtype: int = 0, out_d=None,
             out_qm=None, out_t=None, out_levels: int = 0, epi_table: Optional[torch.Tensor] = None) -> torch.Tensor:
    """qvit_gemm_a32: the int8-code GEMM on QVIT_ACT_T32 activations (weight-stationary fc1 schedule)."""
    _require_gpu(A, "codes")
    assert A.numel() >= t32_rows(M) * K
    _check(load().qvit_gemm_a32(_ptr(A), M, K, _ptr(packed), wfmt, N, npad, _ptr(d_act), _ptr(d_wt), _ptr(bias_pad),
                                epilogue, _ptr(C), C.stride(0), out_qtype, _ptr(out_d), _ptr(out_qm), _ptr(out_t),
                                out_levels, _ptr(epi_table), _stream(A.device)), "qvit_gemm_a32")
    return C


WONLY_WS_MAX = 64 << 20   # bytes of split-K partials per call (small-M weight-only layers)


def wonly_workspace(device: torch.device, M: int, npad: int) -> Optional[torch.Tensor]:
    """Split-K workspace of qvit_gemm_wonly for M rows (at most 256 partial sets). A fresh buffer per call from
    torch's caching allocator, which ties it to the current stream: launches on different streams never share
    partials."""
    need = min(256 * M * npad * 4, WONLY_WS_MAX)
    return torch.empty(need // 4 + 4, dtype=torch.float32, device=device)


def gemm_wonly(X: torch.Tensor, M: int, K: int, packed: torch.Tensor, wfmt: int, N: int, npad: int,
               d_wt: torch.Tensor, bias_pad: Optional[torch.Tensor], Y: torch.Tensor, split: bool = True) -> torch.Tensor:
    """Y = d_wt * (X @ codes^T) + bias with fp32 X (qvit_gemm_wonly: weight-only QuantizeLinear); small M
    splits the K range over several workgroups through a cached workspace (split=False: never)."""
    _require_gpu(X, "activations")
    small = (npad // 256) * ((M + 63) // 64) < 128   # the kernel splits K only for fewer tiles than this
    ws = wonly_workspace(X.device, M, npad) if (split and small) else None
    _check(load().qvit_gemm_wonly(_ptr(X), M, K, X.stride(0), _ptr(packed), wfmt, N, npad, _ptr(d_wt),
                                  _ptr(bias_pad), _ptr(Y), Y.stride(0), _ptr(ws), 0 if ws is None else ws.numel() * 4,
                                  _stream(X.device)), "qvit_gemm_wonly")
    return Y


def gemm_wonly_rows(x2: torch.Tensor, k: int, kpad: int, packed: torch.Tensor, wfmt: int, n: int, npad: int,
                    d_wt: torch.Tensor, bias_pad: Optional[torch.Tensor]) -> torch.Tensor:
    """d_wt * (x2[:, :k] @ codes^T) + bias as [M, n] on qvit_gemm_wonly, for the rows of a layer's forward or the
    output gradient of its backward against the (transposed) packed image. The rows are read in place when the kernel
    can take them: fp32, unit column stride, at least kpad columns (those past k multiply zero codes), a row stride
    that is a multiple of 4 and a 16-byte aligned base; otherwise their first k columns are copied into fresh
    zero-padded [M, kpad] rows. The result is a view of rows of round_up(n, 4) floats when n is no multiple of 4.
    It launches whenever it is called, on no rows too: a caller that must not checks M itself.

    This one predicate is what each caller used to spell for the operands it can see: a gradient's width n never
    exceeds kpad_t = round_up(n, TILE_K), and a layer's in_features never exceed its kpad, so `shape[1] >= kpad`
    is `shape[1] == kpad` there; and a contiguous [M, kpad_t] matrix has a row stride that is a multiple of 4, so the
    site that left the stride test out lost nothing."""
    M = x2.shape[0]
    if (x2.dtype != torch.float32 or x2.stride(-1) != 1 or x2.shape[1] < kpad or x2.stride(0) % 4
            or x2.data_ptr() % 16):
        rows = torch.zeros((M, kpad), dtype=torch.float32, device=x2.device)
        rows[:, :k] = x2[:, :k]
        x2 = rows
    ldy = round_up(n, 4)
    y = torch.empty((M, ldy), dtype=torch.float32, device=x2.device)
    gemm_wonly(x2, M, kpad, packed, wfmt, n, npad, d_wt, bias_pad, y)
    return y if ldy == n else y[:, :n]


def gemm_wgrad_splits(M: int, N: int, K: int) -> int:
    """Workgroups per output tile over which qvit_gemm_wgrad splits the M range (from its workspace query)."""
    r = lambda v: (v + 127) // 128 * 128
    nbytes = int(load().qvit_gemm_wgrad_workspace_bytes(M, N, K))
    if nbytes < 0:
        raise QvitError(f"qvit_gemm_wgrad_workspace_bytes({M}, {N}, {K}) failed (status {nbytes})")
    return nbytes // (r(N) * r(K) * 4)


def gemm_wgrad(G: torch.Tensor, codes: torch.Tensor, K: int, d_act: torch.Tensor,
               out: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """dW[N, K] = d_act * G^T @ codes[:, :K] (qvit_gemm_wgrad): G fp32 [M, N], codes int8 [M, >= K] (the forward's
    activation codes). An operand off the kernel's alignment (row stride of G not a multiple of 4, of the codes not
    a multiple of 16, base not 16-byte aligned) is copied into a padded buffer first. `out`: fp32 [N, >= K] rows
    (columns past K stay untouched); `workspace`: float32, at least the query's bytes (contents irrelevant)."""
    _require_gpu(G, "grad_out")
    _require_gpu(codes, "codes")
    assert G.dim() == 2 and codes.dim() == 2 and codes.dtype == torch.int8 and codes.shape[0] == G.shape[0]
    assert codes.shape[1] >= K >= 1
    M, N = G.shape
    if G.dtype != torch.float32 or G.stride(1) != 1 or G.stride(0) % 4 or G.stride(0) < N or G.data_ptr() % 16:
        gp = torch.zeros((M, (N + 3) // 4 * 4), dtype=torch.float32, device=G.device)
        gp[:, :N] = G
        G = gp
    if codes.stride(1) != 1 or codes.stride(0) % 16 or codes.stride(0) < K or codes.data_ptr() % 16:
        cp = torch.zeros((M, (K + 15) // 16 * 16), dtype=torch.int8, device=codes.device)
        cp[:, :K] = codes[:, :K]
        codes = cp
    if out is None:
        out = torch.empty((N, K), dtype=torch.float32, device=G.device)
    assert out.dtype == torch.float32 and out.shape[0] == N and out.shape[1] >= K and out.stride(1) == 1
    if M == 0:   # (an empty tensor has no device pointer to hand over)
        out[:, :K] = 0
        return out
    lib = load()
    nbytes = int(lib.qvit_gemm_wgrad_workspace_bytes(M, N, K))
    if nbytes < 0:
        _check(nbytes, "qvit_gemm_wgrad_workspace_bytes")
    if workspace is None:
        workspace = torch.empty(nbytes // 4, dtype=torch.float32, device=G.device)
    _check(lib.qvit_gemm_wgrad(_ptr(G), M, N, G.stride(0), _ptr(codes), K, codes.stride(0), _ptr(d_act), _ptr(out),
                               out.stride(0), _ptr(workspace), workspace.numel() * workspace.element_size(),
                               _stream(G.device)), "qvit_gemm_wgrad")
    return out


def conv_out_hw(H: int, W: int, kernel_size, stride, padding, dilation) -> Tuple[int, int]:
    """(OH, OW) of a convolution on an H x W image, as torch and qvit_common.h's qvit_conv_shape count them. (A
    padded image smaller than the dilated kernel is the library's to reject: it checks the extents itself.)"""
    (kh, kw), (sh, sw), (ph, pw), (dh, dw) = kernel_size, stride, padding, dilation
    return (H + 2 * ph - dh * (kh - 1) - 1) // sh + 1, (W + 2 * pw - dw * (kw - 1) - 1) // sw + 1


def col2im_quant_backward(P: torch.Tensor, x: Optional[torch.Tensor], xshape, kernel_size, stride, padding, dilation,
                          qtype: int = QT_LINEAR, d: Optional[torch.Tensor] = None, qm: Optional[torch.Tensor] = None,
                          t: Optional[torch.Tensor] = None, clip_lo: float = 0.0, clip_hi: float = 0.0,
                          grad_x: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None):
    """col2im of the patch-row gradient P (fp32 [B*OH*OW, >= C*kh*kw] rows in im2col_quant_i8's column order, any
    row stride) into an image of shape `xshape`, fused with the backward of the activation quantizer over the
    layer's input x (qvit_col2im_quant_backward). Returns (grad_x, scalars) as quant_backward does, on the device
    with no host sync. Fold-only form: x = None returns (grad_xq, None) and takes no quantizer arguments. `grad_x`
    (fp32, contiguous, of shape xshape) must not share memory with P; `workspace`: float64, at least the query's
    bytes (contents irrelevant)."""
    _require_gpu(P, "P")
    B, C, H, W = (int(v) for v in xshape)
    (kh, kw), (sh, sw), (ph, pw), (dh, dw) = kernel_size, stride, padding, dilation
    geo = (B, C, H, W, kh, kw, sh, sw, ph, pw, dh, dw)
    OH, OW = conv_out_hw(H, W, kernel_size, stride, padding, dilation)
    K = C * kh * kw
    if P.dim() != 2 or P.shape[0] != B * OH * OW or P.shape[1] < K:
        raise QvitError(f"col2im_quant_backward: P of shape {tuple(P.shape)} for {B * OH * OW} patch rows of {K}")
    if P.dtype != torch.float32 or P.stride(1) != 1 or (P.shape[0] > 1 and P.stride(0) < K):
        P = P.detach().float().contiguous()
    dev = P.device
    if x is not None:
        _require_gpu(x, "input")
        x = x.detach()
        if x.dtype != torch.float32 or not x.is_contiguous():
            x = x.float().contiguous()
        if tuple(x.shape) != (B, C, H, W):
            raise QvitError(f"col2im_quant_backward: input of shape {tuple(x.shape)} for an image of {(B, C, H, W)}")
    if grad_x is None:
        grad_x = torch.empty((B, C, H, W), dtype=torch.float32, device=dev)
    assert grad_x.is_cuda and grad_x.dtype == torch.float32 and grad_x.is_contiguous() and \
        tuple(grad_x.shape) == (B, C, H, W)
    lib = load()
    scalars, nbytes = None, 0
    if x is not None:
        nbytes = int(lib.qvit_col2im_quant_backward_workspace_bytes(*geo))
        workspace = _workspace(nbytes, "qvit_col2im_quant_backward_workspace_bytes", workspace, dev)
        nbytes = workspace.numel() * workspace.element_size()
        scalars = torch.empty(3, dtype=torch.float32, device=dev)
    ldp = P.stride(0) if P.shape[0] > 1 else max(P.shape[1], 1)
    _check(lib.qvit_col2im_quant_backward(_ptr(P), ldp, _ptr(x), *geo, qtype, _ptr(d), _ptr(qm), _ptr(t),
                                          float(clip_lo), float(clip_hi), _ptr(grad_x), _ptr(scalars),
                                          _ptr(workspace) if x is not None else None, nbytes, _stream(dev)),
           "qvit_col2im_quant_backward")
    return grad_x, scalars


def conv_wonly(x: torch.Tensor, kernel_size, stride, padding, dilation, packed: torch.Tensor, wfmt: int, N: int,
               npad: int, kpad: int, d_wt: torch.Tensor, bias_pad: Optional[torch.Tensor],
               split: bool = True) -> torch.Tensor:
    """F.conv2d(x, d_wt * codes, bias) (groups 1, zero padding) with fp32 NCHW x on qvit_conv_wonly: an implicit
    GEMM against the packed codes ([N][C kh kw] in the weight's flattening order). Returns NCHW fp32. Few output
    pixels on the wide schedule split K through a workspace (split=False: never)."""
    _require_gpu(x, "activations")
    if x.dtype != torch.float32 or not x.is_contiguous():
        x = x.float().contiguous()
    B, C, H, W = x.shape
    (kh, kw), (sh, sw), (ph, pw), (dh, dw) = kernel_size, stride, padding, dilation
    OH, OW = conv_out_hw(H, W, kernel_size, stride, padding, dilation)
    y = torch.empty((B, N, OH, OW), dtype=torch.float32, device=x.device)
    M = B * OH * OW
    small = split and (npad // 256) * ((M + 63) // 64) < 128 and not narrow_conv_fits(wfmt, N, C * kh * kw, H, W)
    ws = wonly_workspace(x.device, M, npad) if small else None
    _check(load().qvit_conv_wonly(_ptr(x), B, C, H, W, kh, kw, sh, sw, ph, pw, dh, dw, _ptr(packed), wfmt, N, npad,
                                  kpad, _ptr(d_wt), _ptr(bias_pad), _ptr(y), _ptr(ws),
                                  0 if ws is None else ws.numel() * 4, _stream(x.device)), "qvit_conv_wonly")
    return y


def conv_wonly_bn_act(x: torch.Tensor, kernel_size, stride, padding, dilation, packed: torch.Tensor, wfmt: int,
                      N: int, npad: int, kpad: int, d_wt: torch.Tensor, bias_pad: Optional[torch.Tensor],
                      bn_alpha: torch.Tensor, bn_shift: torch.Tensor, a_levels: int) -> Optional[torch.Tensor]:
    """conv_wonly -> BatchNorm2d(eval) as y alpha + shift (ultra_bn_fold) -> activation_quantize_fn values
    round(clamp(., 0, 1) levels) / levels, in one launch (qvit_conv_wonly_bn_act, the narrow schedule). None when
    the layer is outside that schedule (more than 64 channels, codes wider than int8, a weight panel past 24 KiB):
    the caller runs the modules one by one."""
    _require_gpu(x, "activations")
    (kh, kw), (sh, sw), (ph, pw), (dh, dw) = kernel_size, stride, padding, dilation
    if not narrow_conv_fits(wfmt, N, x.shape[1] * kh * kw, x.shape[2], x.shape[3]):
        return None
    if x.dtype != torch.float32 or not x.is_contiguous():
        x = x.float().contiguous()
    B, C, H, W = x.shape
    OH, OW = conv_out_hw(H, W, kernel_size, stride, padding, dilation)
    y = torch.empty((B, N, OH, OW), dtype=torch.float32, device=x.device)
    _check(load().qvit_conv_wonly_bn_act(_ptr(x), B, C, H, W, kh, kw, sh, sw, ph, pw, dh, dw, _ptr(packed), wfmt, N,
                                       npad, kpad, _ptr(d_wt), _ptr(bias_pad), _ptr(bn_alpha), _ptr(bn_shift),
                                       a_levels, _ptr(y), _stream(x.device)), "qvit_conv_wonly_bn_act")
    return y


NARROW_W_MAX = 24 * 1024   # gemm_wonly.hip NW_WMAX: the narrow schedule's LDS weight panel
NARROW_K_MAX = 1024        # gemm_wonly.hip NW_KMAX: its tap table


def narrow_conv_fits(wfmt: int, N: int, kreal: int, H: int = 0, W: int = 0) -> bool:
    """Whether qvit_conv_wonly runs the narrow schedule (gemm_wonly.hip narrow_geo): N <= 64 channels, int4 / int8
    codes, the K stages up to C kh kw (<= NARROW_K_MAX taps) of 16 ceil(N / 16) rows within NARROW_W_MAX, input
    sides below 32767, the schedule enabled."""
    if N > 64 or wfmt not in (W4, W8) or not conv_wonly_narrow(-1) or H >= 32767 or W >= 32767:
        return False
    nke = (kreal + 63) // 64
    return (nke * 64 <= NARROW_K_MAX
            and nke * 16 * ((N + 15) // 16) * (32 if wfmt == W4 else 64) <= NARROW_W_MAX)


def conv_wonly_narrow(enable: int = -1) -> bool:
    """The narrow convolution schedule of qvit_conv_wonly (N <= 64) on (1) / off (0) for this process; -1 queries.
    Returns the previous setting (tests compare the two schedules)."""
    return bool(load().qvit_conv_wonly_narrow(int(enable)))


def resid_ln_counters(device: torch.device, rows: int, npad: int) -> torch.Tensor:
    """Arrival counters of qvit_gemm_resid_ln for `rows` rows: one int32 per 128-row block. The call zeroes them
    on its stream; a fresh buffer per call (caching allocator, stream-bound) so concurrent launches never share."""
    return torch.empty(max((rows + 127) // 128, 1), dtype=torch.int32, device=device)


def gemm_resid_ln(A: torch.Tensor, M: int, K: int, packed: torch.Tensor, wfmt: int, N: int, npad: int,
                  d_act, d_wt, bias_pad, C: torch.Tensor, gamma, beta, eps: float, out_qtype: int, out_d, out_qm,
                  out_t, out_levels: int, ln_table, codes: torch.Tensor, kpad_codes: int) -> torch.Tensor:
    """C += contraction (QVIT_EPI_F32_RESID), then LayerNorm + quantizer of the updated rows -> codes
    (qvit_gemm_resid_ln)."""
    _require_gpu(A, "codes")
    cnt = resid_ln_counters(A.device, M, npad)
    _check(load().qvit_gemm_resid_ln(_ptr(A), M, K, A.stride(0), _ptr(packed), wfmt, N, npad, _ptr(d_act),
                                     _ptr(d_wt), _ptr(bias_pad), _ptr(C), C.stride(0), _ptr(gamma), _ptr(beta), eps,
                                     out_qtype, _ptr(out_d), _ptr(out_qm), _ptr(out_t), out_levels, _ptr(ln_table),
                                     _ptr(codes), codes.stride(0), kpad_codes, _ptr(cnt), _stream(A.device)),
           "qvit_gemm_resid_ln")
    return codes


def epi_table_build(epilogue: int, out_qtype: int, out_d, out_qm, out_t, out_levels: int, v_lo: float, w: float,
                    nb: int, device: torch.device) -> torch.Tensor:
    """Code table of an int8 GEMM epilogue (qvit_epi_table_build); validity is decided on the device."""
    table = torch.zeros((16 + 8 * nb + 1023) // 1024 * 1024, dtype=torch.uint8, device=device)  # 1-KiB pieces
    _check(load().qvit_epi_table_build(epilogue, out_qtype, _ptr(out_d), _ptr(out_qm), _ptr(out_t), out_levels,
                                       v_lo, w, nb, _ptr(table), _stream(device)), "qvit_epi_table_build")
    return table


def attention(qkv: torch.Tensor, B: int, N: int, H: int, head_dim: int, scale: float, out: torch.Tensor,
              out_mode: int = ATT_F32, in_scale: float = 1.0, out_qtype: int = 0, out_d=None, out_qm=None,
              out_t=None, out_levels: int = 0) -> torch.Tensor:
    """softmax(q k^T * scale) v per (image, head) on a [B*N, >= 3*H*hd] fp32 qkv projection; hd 64, or 80 with
    ATT_F32 (anything else is QVIT_EINVAL)."""
    _require_gpu(qkv, "qkv")
    assert qkv.dtype == torch.float32 and qkv.stride(1) == 1
    _check(load().qvit_attention(_ptr(qkv), B, N, H, head_dim, qkv.stride(0), scale, in_scale, out_mode, _ptr(out),
                                 out.stride(0), out_qtype, _ptr(out_d), _ptr(out_qm), _ptr(out_t), out_levels,
                                 _stream(qkv.device)), "qvit_attention")
    return out


def attention_backward_workspace_bytes(B: int, N: int, H: int) -> int:
    return int(load().qvit_attention_backward_workspace_bytes(B, N, H))


def attention_backward(qkv: torch.Tensor, out: torch.Tensor, grad_out: torch.Tensor, B: int, N: int, H: int,
                       head_dim: int, scale: float, in_scale: float = 1.0, g_scale: float = 1.0,
                       grad_qkv: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Gradient of attention() with respect to qkv (qvit_attention_backward; hd 64 or 80): qkv [B*N, >= 3*H*hd], out and
    grad_out [B*N, >= H*hd], all fp32 with unit column stride. Returns grad_qkv shaped like qkv's [B*N, 3*H*hd]
    columns (written into `grad_qkv` when given; columns past 3*H*hd are left alone)."""
    for t, name in ((qkv, "qkv"), (out, "out"), (grad_out, "grad_out")):
        _require_gpu(t, name)
        assert t.dtype == torch.float32 and t.dim() == 2 and t.stride(1) == 1 and t.shape[0] == B * N, name
    if grad_qkv is None:
        grad_qkv = torch.empty((B * N, 3 * H * head_dim), dtype=torch.float32, device=qkv.device)
    _require_gpu(grad_qkv, "grad_qkv")
    assert grad_qkv.dtype == torch.float32 and grad_qkv.dim() == 2 and grad_qkv.stride(1) == 1
    lib = load()
    nbytes = int(lib.qvit_attention_backward_workspace_bytes(B, N, H))
    if nbytes < 0:
        _check(nbytes, "qvit_attention_backward_workspace_bytes")
    ws = torch.empty(max(nbytes, 16) // 4, dtype=torch.float32, device=qkv.device)
    _check(lib.qvit_attention_backward(_ptr(qkv), _ptr(out), _ptr(grad_out), B, N, H, head_dim, qkv.stride(0),
                                       out.stride(0), grad_out.stride(0), scale, in_scale, g_scale, _ptr(grad_qkv),
                                       grad_qkv.stride(0), _ptr(ws), nbytes, _stream(qkv.device)),
           "qvit_attention_backward")
    return grad_qkv


def gemm_qkv_split(A: torch.Tensor, M: int, K: int, packed: torch.Tensor, wfmt: int, N: int, npad: int,
                   d_act: torch.Tensor, d_wt: torch.Tensor, bias_pad: Optional[torch.Tensor], seq: int,
                   in_scale: float, hi: torch.Tensor, lo: torch.Tensor, head_dim: int = 64):
    """qkv projection as fp16 hi/lo planes [B][N/head_dim][seq][head_dim] of in_scale * x (qvit_gemm_qkv_split;
    qvit_gemm_qkv_split_hd for a head_dim other than 64)."""
    _require_gpu(A, "codes")
    assert hi.dtype == torch.float16 and lo.dtype == torch.float16 and hi.is_contiguous() and lo.is_contiguous()
    assert hi.numel() >= M * N and lo.numel() >= M * N
    if head_dim != 64:
        _check(load().qvit_gemm_qkv_split_hd(_ptr(A), M, K, A.stride(0), _ptr(packed), wfmt, N, npad, _ptr(d_act),
                                             _ptr(d_wt), _ptr(bias_pad), seq, head_dim, in_scale, _ptr(hi), _ptr(lo),
                                             _stream(A.device)), "qvit_gemm_qkv_split_hd")
        return hi, lo
    _check(load().qvit_gemm_qkv_split(_ptr(A), M, K, A.stride(0), _ptr(packed), wfmt, N, npad, _ptr(d_act),
                                      _ptr(d_wt), _ptr(bias_pad), seq, in_scale, _ptr(hi), _ptr(lo),
                                      _stream(A.device)), "qvit_gemm_qkv_split")
    return hi, lo


def attention_split(hi: torch.Tensor, lo: torch.Tensor, B: int, N: int, H: int, head_dim: int, scale: float,
                    out: torch.Tensor, out_mode: int = ATT_F32, in_scale: float = 1.0, out_qtype: int = 0,
                    out_d=None, out_qm=None, out_t=None, out_levels: int = 0,
                    epi_table: Optional[torch.Tensor] = None) -> torch.Tensor:
    """qvit_attention on the split planes of gemm_qkv_split (epi_table: EPI_I8 code table of the output
    quantizer, optional)."""
    _require_gpu(hi, "qkv_hi")
    assert hi.dtype == torch.float16 and lo.dtype == torch.float16
    assert hi.numel() >= B * 3 * H * N * head_dim and lo.numel() >= B * 3 * H * N * head_dim
    _check(load().qvit_attention_split(_ptr(hi), _ptr(lo), B, N, H, head_dim, scale, in_scale, out_mode, _ptr(out),
                                       out.stride(0), out_qtype, _ptr(out_d), _ptr(out_qm), _ptr(out_t), out_levels,
                                       _ptr(epi_table), _stream(hi.device)), "qvit_attention_split")
    return out


QKV_ATT_MAX_N = 208
QKV_ATT_MAX_C = 768   # H * 64 (the bias of the qkv layer stays in LDS)


def qkv_attention(codes: torch.Tensor, B: int, N: int, K: int, packed: torch.Tensor, npad: int,
                  d_act: torch.Tensor, d_wt: torch.Tensor, bias_pad: Optional[torch.Tensor], H: int, scale: float,
                  out: torch.Tensor, out_mode: int = ATT_F32, in_scale: float = 1.0, out_qtype: int = 0,
                  out_d=None, out_qm=None, out_t=None, out_levels: int = 0,
                  epi_table: Optional[torch.Tensor] = None, wfmt: int = W4) -> torch.Tensor:
    """qkv projection (W4 codes) + attention core in one kernel (qvit_qkv_attention), N <= 208."""
    _require_gpu(codes, "codes")
    _check(load().qvit_qkv_attention(_ptr(codes), B, N, K, codes.stride(0), _ptr(packed), wfmt, npad, _ptr(d_act),
                                     _ptr(d_wt), _ptr(bias_pad), H, 64, scale, in_scale, out_mode, _ptr(out),
                                     out.stride(0), out_qtype, _ptr(out_d), _ptr(out_qm), _ptr(out_t), out_levels,
                                     _ptr(epi_table), _stream(codes.device)), "qvit_qkv_attention")
    return out


QKV_ATT_MAX_NQ = 32


def qkv_attention_q(codes: torch.Tensor, B: int, N: int, NQ: int, K: int, packed: torch.Tensor, npad: int,
                    d_act: torch.Tensor, d_wt: torch.Tensor, bias_pad: Optional[torch.Tensor], H: int, scale: float,
                    out: torch.Tensor, out_mode: int = ATT_F32, in_scale: float = 1.0, out_qtype: int = 0,
                    out_d=None, out_qm=None, out_t=None, out_levels: int = 0,
                    epi_table: Optional[torch.Tensor] = None, wfmt: int = W4) -> torch.Tensor:
    """qkv_attention for the first NQ <= 32 tokens of each image (qvit_qkv_attention_q): `out` is the compact
    [B*NQ, ldo], its row b*NQ + i the same bits as row b*N + i of qkv_attention."""
    _require_gpu(codes, "codes")
    _check(load().qvit_qkv_attention_q(_ptr(codes), B, N, NQ, K, codes.stride(0), _ptr(packed), wfmt, npad,
                                       _ptr(d_act), _ptr(d_wt), _ptr(bias_pad), H, 64, scale, in_scale, out_mode,
                                       _ptr(out), out.stride(0), out_qtype, _ptr(out_d), _ptr(out_qm), _ptr(out_t),
                                       out_levels, _ptr(epi_table), _stream(codes.device)), "qvit_qkv_attention_q")
    return out


# ---- UltraNet ---------------------------------------------------------------------------------------
def ultra_weight_codes(w: torch.Tensor, w_bit: int, kpad: int, cout_pad: int, values: bool = False):
    """Conv weight [cout][cin][ks][ks] -> int8 codes [cout_pad][kpad] in K order (ky, kx, c)
    (and, with values=True, also the fake-quant weight k/(2^(w_bit-1)-1) in w's layout)."""
    _require_gpu(w, "weight")
    w = w.detach().float().contiguous()
    cout, cin, ks, ks2 = w.shape
    assert ks == ks2
    codes = torch.empty((cout_pad, kpad), dtype=torch.int8, device=w.device)
    vals = torch.empty_like(w) if values else None
    ws = torch.empty(1, dtype=torch.int32, device=w.device)
    _check(load().qvit_ultra_weight_codes(_ptr(w), cout, cin, ks, w_bit, _ptr(codes), kpad, cout_pad, _ptr(vals),
                                          _ptr(ws), _stream(w.device)), "qvit_ultra_weight_codes")
    return (codes, vals) if values else codes


def ultra_bn_fold(bn, device) -> tuple:
    n = bn.num_features
    alpha = torch.empty(n, device=device)
    shift = torch.empty(n, device=device)
    g = bn.weight.detach().float().contiguous() if bn.weight is not None else None
    b = bn.bias.detach().float().contiguous() if bn.bias is not None else None
    _check(load().qvit_ultra_bn_fold(_ptr(g), _ptr(b), _ptr(bn.running_mean), _ptr(bn.running_var), float(bn.eps), n,
                                     _ptr(alpha), _ptr(shift), _stream(device)), "qvit_ultra_bn_fold")
    return alpha, shift


def ultra_conv0(img: torch.Tensor, wvals: torch.Tensor, alpha, shift, a_bit: int) -> torch.Tensor:
    """Layer 0: float image NCHW -> conv3x3 with fake-quant weights wvals [16][3][3][3] -> BN -> quantizer
    -> 2x2 max pool -> NHWC codes [B][H/2][W/2][16]."""
    _require_gpu(img, "image")
    assert img.dtype == torch.float32 and img.is_contiguous() and img.shape[1] == 3
    assert wvals.shape == (16, 3, 3, 3) and wvals.is_contiguous()
    B, _, H, W = img.shape
    out = torch.empty((B, H // 2, W // 2, 16), dtype=torch.int8, device=img.device)
    _check(load().qvit_ultra_conv0(_ptr(img), B, H, W, _ptr(wvals), _ptr(alpha), _ptr(shift), a_bit, _ptr(out),
                                   _stream(img.device)), "qvit_ultra_conv0")
    return out


def ultra_conv(x: torch.Tensor, ks: int, wcodes: torch.Tensor, cout: int, w_bit: int, a_bit: int, alpha, shift,
               mode: int) -> torch.Tensor:
    """NHWC codes [B][H][W][cin] -> NHWC codes (mode ULTRA_CODES / ULTRA_CODES_POOL) or fp32 (ULTRA_F32)."""
    _require_gpu(x, "codes")
    assert x.dtype == torch.int8 and x.is_contiguous()
    B, H, W, cin = x.shape
    if mode == ULTRA_CODES_POOL:
        out = torch.empty((B, H // 2, W // 2, cout), dtype=torch.int8, device=x.device)
    elif mode == ULTRA_CODES:
        out = torch.empty((B, H, W, cout), dtype=torch.int8, device=x.device)
    else:
        out = torch.empty((B, H, W, cout), dtype=torch.float32, device=x.device)
    _check(load().qvit_ultra_conv(_ptr(x), B, H, W, cin, ks, _ptr(wcodes), wcodes.shape[1], cout, w_bit, a_bit,
                                  _ptr(alpha), _ptr(shift), mode, _ptr(out), cout, _stream(x.device)),
           "qvit_ultra_conv")
    return out


def ultra_tail(x: torch.Tensor, wcodes, alphas, shifts, hcodes: torch.Tensor, hbias: torch.Tensor, hout: int,
               w_bit: int, a_bit: int, decode=None):
    """UltraNet layers.16-28 in one launch (qvit_ultra_tail): NHWC codes [B][H][W][64] (H, W <= 26) through four
    3x3 64 -> 64 blocks and the 1x1 head -> fp32 NHWC [B][H][W][hout]; with decode = (anchors, na, no, stride)
    the YOLO decode runs in the kernel and (io [B, na*H*W, no], p [B, na, H, W, no]) is returned instead."""
    _require_gpu(x, "codes")
    assert x.dtype == torch.int8 and x.is_contiguous() and x.shape[3] == 64
    B, H, W, _ = x.shape
    arr = lambda ts: (ctypes.c_void_p * 4)(*[t.data_ptr() for t in ts])
    if decode is None:
        out = torch.empty((B, H, W, hout), dtype=torch.float32, device=x.device)
        io = p = anchors = None
        na = no = 0
        stride = 0.0
    else:
        anchors, na, no, stride = decode
        out = None
        io = torch.empty((B, na, H, W, no), device=x.device)
        p = torch.empty_like(io)
    _check(load().qvit_ultra_tail(_ptr(x), B, H, W, arr(wcodes), wcodes[0].shape[1], arr(alphas), arr(shifts),
                                  _ptr(hcodes), hcodes.shape[1], _ptr(hbias), hout, w_bit, a_bit, _ptr(out), hout,
                                  _ptr(anchors), na, no, float(stride), _ptr(io), _ptr(p), _stream(x.device)),
           "qvit_ultra_tail")
    return out if decode is None else (io.view(B, -1, no), p)


def ultra_conv0_int(img_u8: torch.Tensor, wcodes: torch.Tensor, inc: torch.Tensor, bias: torch.Tensor,
                    shift_bits: int, out_bit: int) -> torch.Tensor:
    """Integer deploy layer 0: uint8 image NCHW -> conv3x3 (weight codes [16][3][3][3]) -> integer BN/act
    threshold -> 2x2 max pool -> NHWC codes [B][H/2][W/2][16]."""
    _require_gpu(img_u8, "image")
    assert img_u8.dtype == torch.uint8 and img_u8.is_contiguous() and img_u8.shape[1] == 3
    assert wcodes.shape == (16, 3, 3, 3) and wcodes.dtype == torch.int8 and wcodes.is_contiguous()
    assert inc.dtype == torch.int32 and bias.dtype == torch.int32 and inc.numel() >= 16 and bias.numel() >= 16
    B, _, H, W = img_u8.shape
    out = torch.empty((B, H // 2, W // 2, 16), dtype=torch.int8, device=img_u8.device)
    _check(load().qvit_ultra_conv0_int(_ptr(img_u8), B, H, W, _ptr(wcodes), _ptr(inc), _ptr(bias), shift_bits,
                                       out_bit, _ptr(out), _stream(img_u8.device)), "qvit_ultra_conv0_int")
    return out


def ultra_conv_int(x: torch.Tensor, ks: int, wcodes: torch.Tensor, cout: int, inc: torch.Tensor, bias: torch.Tensor,
                   shift_bits: int, out_bit: int, pool: bool) -> torch.Tensor:
    """Integer deploy layers 1..7: NHWC codes [B][H][W][cin] -> NHWC codes (2x2 max-pooled when pool)."""
    _require_gpu(x, "codes")
    assert x.dtype == torch.int8 and x.is_contiguous()
    assert inc.dtype == torch.int32 and bias.dtype == torch.int32 and inc.numel() >= cout and bias.numel() >= cout
    B, H, W, cin = x.shape
    shape = (B, H // 2, W // 2, cout) if pool else (B, H, W, cout)
    out = torch.empty(shape, dtype=torch.int8, device=x.device)
    _check(load().qvit_ultra_conv_int(_ptr(x), B, H, W, cin, ks, _ptr(wcodes), wcodes.shape[1], cout, _ptr(inc),
                                      _ptr(bias), shift_bits, out_bit, 1 if pool else 0, _ptr(out), cout,
                                      _stream(x.device)), "qvit_ultra_conv_int")
    return out


def yolo_decode(head: torch.Tensor, na: int, no: int, anchors: torch.Tensor, stride: float):
    """head NHWC fp32 [B][ny][nx][na*no] -> (io [B, na*ny*nx, no], p [B, na, ny, nx, no])."""
    _require_gpu(head, "head")
    B, ny, nx, C = head.shape
    io = torch.empty((B, na, ny, nx, no), device=head.device)
    p = torch.empty_like(io)
    _check(load().qvit_yolo_decode(_ptr(head), B, ny, nx, na, no, C, _ptr(anchors), stride, _ptr(io), _ptr(p),
                                   _stream(head.device)), "qvit_yolo_decode")
    return io.view(B, -1, no), p


# ---- UltraNet training (ultra_backward.hip) -----------------------------------------------------------
def ultra_weight_quant_backward(w: torch.Tensor, grad_out: torch.Tensor, w_bit: int,
                                grad_w: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Backward of weight_quantize_fn (2 <= w_bit <= 8) over the weight w given the gradient of its fake-quant
    values (qvit_ultra_weight_quant_backward); shaped as w (written into `grad_w` when given; it may be grad_out)."""
    _require_gpu(w, "weight")
    _require_gpu(grad_out, "grad_out")
    wc = w.detach().contiguous().float()
    gc = grad_out.detach().contiguous().float()
    if wc.numel() != gc.numel():
        raise QvitError(f"ultra_weight_quant_backward: grad_out has {gc.numel()} elements for {wc.numel()} weights")
    if grad_w is None:
        grad_w = torch.empty_like(wc)
    assert grad_w.is_cuda and grad_w.dtype == torch.float32 and grad_w.is_contiguous() and \
        grad_w.numel() == wc.numel()
    n = wc.numel()
    lib = load()
    nbytes = int(lib.qvit_ultra_weight_quant_backward_workspace_bytes(n))
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device=wc.device)
    _check(lib.qvit_ultra_weight_quant_backward(_ptr(wc), _ptr(gc), n, w_bit, _ptr(grad_w), _ptr(ws), nbytes,
                                                _stream(wc.device)), "qvit_ultra_weight_quant_backward")
    return grad_w


def ultra_act_quant_backward(x: torch.Tensor, grad_out: torch.Tensor,
                             grad_x: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Backward of activation_quantize_fn over its input x: grad_out where 0 <= x <= 1, else 0
    (qvit_ultra_act_quant_backward); shaped as x (written into `grad_x` when given; it may be grad_out)."""
    _require_gpu(x, "input")
    _require_gpu(grad_out, "grad_out")
    xc = x.detach().contiguous().float()
    gc = grad_out.detach().contiguous().float()
    if xc.numel() != gc.numel():
        raise QvitError(f"ultra_act_quant_backward: grad_out has {gc.numel()} elements for an input of {xc.numel()}")
    if xc.data_ptr() % 16:
        xc = xc.clone()
    if gc.data_ptr() % 16:
        gc = gc.clone()
    if grad_x is None:
        grad_x = torch.empty_like(xc)
    assert grad_x.is_cuda and grad_x.dtype == torch.float32 and grad_x.is_contiguous() and \
        grad_x.numel() == xc.numel()
    if xc.numel():
        _check(load().qvit_ultra_act_quant_backward(_ptr(xc), _ptr(gc), xc.numel(), _ptr(grad_x),
                                                    _stream(xc.device)), "qvit_ultra_act_quant_backward")
    return grad_x


def conv_wgrad(G: torch.Tensor, x: torch.Tensor, kernel_size, stride, padding, dilation, levels: int,
               out: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Weight gradient [N, C, kh, kw] of F.conv2d(x, w) (groups 1, zero padding) given the output's gradient G
    [B, N, OH, OW], for an x that holds k / levels with integer 0 <= k <= levels (activation_quantize_fn's output):
    qvit_conv_wgrad, an implicit GEMM of G against the integer codes. `out`: a contiguous fp32 [N, C, kh, kw];
    `workspace`: float32, at least the query's bytes (contents irrelevant)."""
    _require_gpu(G, "grad_out")
    _require_gpu(x, "input")
    assert G.dim() == 4 and x.dim() == 4 and G.shape[0] == x.shape[0]
    if G.dtype != torch.float32 or not G.is_contiguous():
        G = G.float().contiguous()
    if x.dtype != torch.float32 or not x.is_contiguous():
        x = x.float().contiguous()
    B, C, H, W = x.shape
    N = G.shape[1]
    (kh, kw), (sh, sw), (ph, pw), (dh, dw) = kernel_size, stride, padding, dilation
    OH, OW = conv_out_hw(H, W, kernel_size, stride, padding, dilation)
    if tuple(G.shape) != (B, N, OH, OW):
        raise QvitError(f"conv_wgrad: grad_out {tuple(G.shape)} for an output of {(B, N, OH, OW)}")
    if out is None:
        out = torch.empty((N, C, kh, kw), dtype=torch.float32, device=G.device)
    assert out.dtype == torch.float32 and out.is_contiguous() and tuple(out.shape) == (N, C, kh, kw)
    if B == 0:   # (an empty tensor has no device pointer to hand over)
        return out.zero_()
    lib = load()
    nbytes = int(lib.qvit_conv_wgrad_workspace_bytes(B, C, H, W, N, kh, kw, sh, sw, ph, pw, dh, dw))
    if nbytes < 0:
        _check(nbytes, "qvit_conv_wgrad_workspace_bytes")
    if workspace is None:
        workspace = torch.empty(nbytes // 4, dtype=torch.float32, device=G.device)
    _check(lib.qvit_conv_wgrad(_ptr(G), _ptr(x), B, C, H, W, N, kh, kw, sh, sw, ph, pw, dh, dw, int(levels),
                               _ptr(out), _ptr(workspace), workspace.numel() * workspace.element_size(),
                               _stream(G.device)), "qvit_conv_wgrad")
    return out


# ---- UltraNet training: BatchNorm2d -> quantizer -> max pool (ultra_bn_fuse.hip) ------------------------------
def _f32c(t: torch.Tensor, name: str) -> torch.Tensor:
    _require_gpu(t, name)
    t = t.detach()
    return t if t.dtype == torch.float32 and t.is_contiguous() else t.float().contiguous()


def _workspace(nbytes: int, what: str, workspace: Optional[torch.Tensor], dev) -> torch.Tensor:
    if nbytes < 0:
        _check(nbytes, what)
    if workspace is None:
        workspace = torch.empty(nbytes // 8, dtype=torch.float64, device=dev)
    return workspace


def bn_stats(x: torch.Tensor, eps: float, factor: float = 0.0, running_mean: Optional[torch.Tensor] = None,
             running_var: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None):
    """Batch statistics of x [B, C, H, W] per channel (qvit_bn_stats): (mean, biased var, invstd), fp32 [C] each;
    the running tensors, when given, are updated in place as nn.BatchNorm2d does with `factor`."""
    x = _f32c(x, "input")
    B, C, H, W = x.shape
    lib = load()
    ws = _workspace(int(lib.qvit_bn_stats_workspace_bytes(B, C, H, W)), "qvit_bn_stats_workspace_bytes", workspace,
                    x.device)
    for r in (running_mean, running_var):
        assert r is None or (r.is_cuda and r.dtype == torch.float32 and r.is_contiguous() and r.numel() == C)
    stats = torch.empty((3, C), dtype=torch.float32, device=x.device)
    _check(lib.qvit_bn_stats(_ptr(x), B, C, H, W, float(eps), float(factor), _ptr(running_mean), _ptr(running_var),
                             _ptr(stats[0]), _ptr(stats[1]), _ptr(stats[2]), _ptr(ws),
                             ws.numel() * ws.element_size(), _stream(x.device)), "qvit_bn_stats")
    return stats[0], stats[1], stats[2]


def bn_act_pool_forward(x: torch.Tensor, mean: torch.Tensor, invstd: torch.Tensor, gamma: Optional[torch.Tensor],
                        beta: Optional[torch.Tensor], levels: int, pool: bool):
    """quantizer(batch_norm(x)) on the given statistics, max-pooled 2 x 2 when `pool` (qvit_bn_act_pool_forward):
    (values k / levels, flag bytes), both shaped as the output."""
    x = _f32c(x, "input")
    B, C, H, W = x.shape
    shape = (B, C, H // 2, W // 2) if pool else (B, C, H, W)
    out = torch.empty(shape, dtype=torch.float32, device=x.device)
    flags = torch.empty(shape, dtype=torch.uint8, device=x.device)
    gamma = None if gamma is None else _f32c(gamma, "gamma")
    beta = None if beta is None else _f32c(beta, "beta")
    _check(load().qvit_bn_act_pool_forward(_ptr(x), B, C, H, W, _ptr(mean), _ptr(invstd), _ptr(gamma), _ptr(beta),
                                           int(levels), int(bool(pool)), _ptr(out), _ptr(flags), _stream(x.device)),
           "qvit_bn_act_pool_forward")
    return out, flags


def bn_act_pool_backward(x: torch.Tensor, grad_out: torch.Tensor, flags: torch.Tensor, mean: torch.Tensor,
                         invstd: torch.Tensor, gamma: Optional[torch.Tensor], pool: bool, want_dgamma: bool = True,
                         want_dbeta: bool = True, workspace: Optional[torch.Tensor] = None):
    """Backward of bn_act_pool_forward over x given its flag bytes (qvit_bn_act_pool_backward_reduce, then
    qvit_bn_act_pool_backward_dx): (dx, dgamma or None, dbeta or None, sums [2, C] float64 = S1, S2)."""
    x = _f32c(x, "input")
    g = _f32c(grad_out, "grad_out")
    B, C, H, W = x.shape
    pool = int(bool(pool))
    if tuple(g.shape) != tuple(flags.shape) or tuple(g.shape) != ((B, C, H // 2, W // 2) if pool else (B, C, H, W)):
        raise QvitError(f"bn_act_pool_backward: grad_out {tuple(g.shape)}, flags {tuple(flags.shape)} for an input "
                        f"of {tuple(x.shape)}, pool {pool}")
    lib = load()
    ws = _workspace(int(lib.qvit_bn_act_pool_backward_workspace_bytes(B, C, H, W, pool)),
                    "qvit_bn_act_pool_backward_workspace_bytes", workspace, x.device)
    sums = torch.empty((2, C), dtype=torch.float64, device=x.device)
    _check(lib.qvit_bn_act_pool_backward_reduce(_ptr(x), _ptr(g), _ptr(flags), B, C, H, W, _ptr(mean), _ptr(invstd),
                                                pool, _ptr(sums), _ptr(ws), ws.numel() * ws.element_size(),
                                                _stream(x.device)), "qvit_bn_act_pool_backward_reduce")
    dx = torch.empty_like(x)
    dgamma = torch.empty(C, dtype=torch.float32, device=x.device) if want_dgamma else None
    dbeta = torch.empty(C, dtype=torch.float32, device=x.device) if want_dbeta else None
    gamma = None if gamma is None else _f32c(gamma, "gamma")
    _check(lib.qvit_bn_act_pool_backward_dx(_ptr(x), _ptr(g), _ptr(flags), B, C, H, W, _ptr(mean), _ptr(invstd),
                                            _ptr(gamma), _ptr(sums), pool, _ptr(dx), _ptr(dgamma), _ptr(dbeta),
                                            _stream(x.device)), "qvit_bn_act_pool_backward_dx")
    return dx, dgamma, dbeta, sums
