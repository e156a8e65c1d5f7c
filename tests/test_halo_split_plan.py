"""Host-side check of the halo-tiled split-product conv's plan (csrc/conv_halo_split.hip,
clskd_conv_halo_split_plan): the only way the kernel can fault is a staging load outside its
segment, so every tile, chunk and staging slot is walked on the host — with the kernel's index
arithmetic — and the touched offsets must lie inside each segment's extent; the LDS footprint
must fit 160 KiB.  No GPU is used: pointers are placeholders that are never dereferenced."""
import ctypes as C

import pytest

from clskd import _lib
from halo_split_cases import CASES, STUDENT, STUDENT_T, T


def _desc(B, segc, N, taps, sf, Fi, Fo, of_mul, of_add, Tn, accumulate=0):
    d = _lib.ConvDesc()
    K = len(taps) * sum(segc)
    d.B, d.Fo, d.To, d.N, d.K = B, Fo, Tn, N, -(-K // 16) * 16
    d.stride_f, d.stride_t, d.nseg = sf, 1, len(segc)
    for i in range(_lib.MAX_SEGS):
        c = segc[min(i, len(segc) - 1)]
        d.seg[i] = _lib.Seg(0x100000 * (i + 1), Fi * Tn * c, Tn * c, c, Fi, Tn)
    d.vec4, d.kvec = 1, 4
    d.weight, d.out = 0x1000000, 0x2000000
    Fout = Fo * of_mul
    d.oB, d.oF, d.oT, d.oNhi, d.oNlo = Fout * Tn * N, Tn * N, N, 0, 1
    d.nlo, d.of_mul, d.of_add = 1 << 30, of_mul, of_add
    d.compute, d.in_dtype, d.out_dtype = _lib.F32X3, _lib.F32, _lib.F32
    d.wlayout = _lib.WLAYOUT_NK
    d.ntaps, d.ctot = len(taps), sum(segc)
    for i, c in enumerate(segc):
        d.seg_c[i] = c
    for i, (dF, dT) in enumerate(taps):
        d.tap_df[i], d.tap_dt[i] = dF, dT
    d.accumulate = accumulate
    return d


def _plan(d):
    info = _lib.HaloSplitInfo()
    rc = _lib.load(require_gpu=False).clskd_conv_halo_split_plan(C.byref(d), C.byref(info))
    assert rc == 0, _lib.load(require_gpu=False).clskd_last_error()
    return info


def _check(info, B, segc, Fi, Tn):
    assert 0 < info.lds_bytes <= 160 * 1024, info.lds_bytes
    assert info.ntiles >= 32 and 1 <= info.grid <= info.ntiles * info.col_halves
    assert info.tile_f * info.tile_t == 256
    for s, c in enumerate(segc):
        extent = B * Fi * Tn * c
        lo, hi = info.seg_min_off[s], info.seg_max_off[s]
        # every element of the segment is inside some tile's halo: the walk reaches both ends
        assert lo == 0 and hi == extent - 1, (s, lo, hi, extent)


@pytest.mark.parametrize("case", sorted(CASES))
def test_plan_test_shapes(case):
    B, segc, N, taps, sf, Fi, Fo, of_mul, of_add, halves = CASES[case]
    info = _plan(_desc(B, segc, N, taps, sf, Fi, Fo, of_mul, of_add, T))
    assert info.launches == 1 and info.col_halves == halves, (case, info.launches, info.col_halves)
    _check(info, B, segc, Fi, T)


@pytest.mark.parametrize("case", sorted(STUDENT))
def test_plan_student_shapes(case):
    """Every student layer of the benchmarked step is taken and its plan is in bounds."""
    B, segc, N, taps, sf, Fi, Fo, of_mul, of_add = STUDENT[case]
    info = _plan(_desc(B, segc, N, taps, sf, Fi, Fo, of_mul, of_add, STUDENT_T))
    assert info.launches == 1, case
    _check(info, B, segc, Fi, STUDENT_T)


def test_plan_refuses_what_the_kernel_does_not_take():
    B, segc, N, taps, sf, Fi, Fo, of_mul, of_add, _ = CASES["enc_n64"]
    assert _plan(_desc(B, segc, N, taps, sf, Fi, Fo, of_mul, of_add, T, accumulate=1)).launches == 0
    # fewer than 32 tiles (the shapes of test_gpu_split.py: 6-18 tiles)
    assert _plan(_desc(3, (64,), 64, taps, 2, 16, 8, 1, 0, 61)).launches == 0
    assert _plan(_desc(3, (16,), 32, taps, 2, 33, 17, 1, 0, 61)).launches == 0
