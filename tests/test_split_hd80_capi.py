"""Argument checks of the split inference path at head_dim 80: qvit_attention_split's new width and the new entry point
qvit_gemm_qkv_split_hd. As in test_capi_rejections.py every call is answered by the host checks alone (nothing is
dereferenced, nothing is launched), a row is (overrides of a valid call, status), and a row that expects QVIT_OK
zeroes the size on which the entry point returns before its launch."""
import pytest

from quantized_vit_amd import _lib, build
from test_capi_rejections import (A0, A1, A2, A3, A4, A5, A6, EALIGN, EINVAL, ENULL, GEMM_QKV_SPLIT, OK, _p,
                                  attention_split)


@pytest.fixture(scope="module")
def lib():
    build.build()
    return _lib.load()


def test_library_exports_the_head_dim_entry_point(lib):
    assert hasattr(lib, "qvit_gemm_qkv_split_hd")


# head_dim 80 takes H * 80 output columns (ldo = 160 for the valid call's two heads)
ATTENTION_SPLIT_HD80 = [
    (dict(hd=80, ldo=160, B=0), OK), (dict(hd=80, ldo=160, B=0, mode=0), OK), (dict(hd=80, ldo=160, B=0, table=A5), OK),
    (dict(hd=96, ldo=192), EINVAL), (dict(hd=32), EINVAL), (dict(hd=96, ldo=192, B=0), EINVAL),
    (dict(hd=80, ldo=156), EINVAL), (dict(hd=80, ldo=128), EINVAL),       # ldo < H * 80 (128 holds two 64-wide heads)
    (dict(hd=80, ldo=160, lo=A4 + 8), EALIGN), (dict(hd=80, ldo=160, hi=A0 + 8, B=0), EALIGN),
    (dict(hd=80, ldo=162, B=0), EALIGN),
    # the order of the rules is the width-64 order: NULL, the table's alignment, head_dim, sizes, alignment
    (dict(hd=80, ldo=160, out=None, lo=A4 + 8), ENULL), (dict(hd=96, ldo=192, table=A5 + 8), EALIGN),
    (dict(hd=96, ldo=192, lo=A4 + 8), EINVAL), (dict(hd=80, ldo=156, lo=A4 + 8), EINVAL),
    (dict(hd=80, ldo=160, qtype=7, B=0), EINVAL), (dict(hd=80, ldo=160, mode=2, B=0), EINVAL),
]


@pytest.mark.parametrize("over,want", ATTENTION_SPLIT_HD80, ids=[str(o) for o, _ in ATTENTION_SPLIT_HD80])
def test_attention_split_head_dim_80(lib, over, want):
    assert attention_split(lib, **over) == want


def gemm_qkv_split_hd(lib, A=A0, M=10, K=128, lda=128, Wp=A1, wfmt=_lib.W4, N=64, npad=256, d_act=A2, d_wt=A3, bias=None,
                      seq=5, hd=64, in_scale=1.0, hi=A4, lo=A5):
    return lib.qvit_gemm_qkv_split_hd(_p(A), M, K, lda, _p(Wp), wfmt, N, npad, _p(d_act), _p(d_wt), _p(bias), seq, hd,
                                      in_scale, _p(hi), _p(lo), None)


HD80 = dict(N=480, npad=512, hd=80)
GEMM_QKV_SPLIT_HD = [
    (dict(hd=96, N=96), EINVAL), (dict(hd=32), EINVAL), (dict(N=480, npad=512, hd=64), EINVAL),      # 480 % 64 != 0
    (dict(HD80, M=0), OK), (dict(M=0), OK), (dict(N=80, hd=80, M=0), OK), (dict(N=160, hd=80, M=0), OK),
    (dict(HD80, N=448), EINVAL),                                                           # 448 % 64 == 0, % 80 != 0
    # head_dim is looked at after NULL and wfmt, with the sizes, before seq and before every alignment rule
    (dict(hd=96, lo=None), ENULL), (dict(hd=96, wfmt=5), EINVAL), (dict(hd=96, hi=A4 + 8), EINVAL),
    (dict(hd=96, lda=136), EINVAL), (dict(HD80, lda=136), EALIGN), (dict(HD80, seq=3, A=A0 + 8), EINVAL),
    (dict(HD80, lo=None), ENULL), (dict(HD80, d_act=None, N=482), ENULL), (dict(HD80, in_scale=0.0), EINVAL),
    (dict(HD80, M=0, bias=A6 + 8), EALIGN), (dict(HD80, M=0, lo=A5 + 8), EALIGN), (dict(HD80, hi=A4 + 8, N=482), EINVAL),
]


@pytest.mark.parametrize("over,want", GEMM_QKV_SPLIT + GEMM_QKV_SPLIT_HD,
                         ids=[str(o) for o, _ in GEMM_QKV_SPLIT + GEMM_QKV_SPLIT_HD])
def test_gemm_qkv_split_hd(lib, over, want):
    """GEMM_QKV_SPLIT: at head_dim 64 the new entry point answers every row of the existing one's table alike."""
    assert gemm_qkv_split_hd(lib, **over) == want
