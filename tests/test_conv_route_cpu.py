"""The engine a conv descriptor dispatches to (clskd_conv_route: the dispatch table of
csrc/conv_igemm.hip, walked without launching) and clskd_conv_fold_capable, which is the same
walk followed by the row's fold column.  Pure host calls on descriptors with placeholder pointers
that are never dereferenced: no GPU is used and nothing is launched.

The expected engines are read off the cascade this table replaced (clskd_conv2d_fwd and
launch_conv_bf16 before it), for B = 3, Fo = 20, T = 101, K padded to 64:
  direct     DIRECT weight layout: nothing else is asked.
  halo       16-bit, N <= 64, a built tap count (10), the plan fits: the first 16-bit engine.
  gemm8      16-bit N = 128: the halo kernel plans N <= 64 only; conv_gemm8 takes N > 64, K % 64.
  lds_dma    16-bit 3 taps: no halo instance (4, 6, 9, 10 are built), conv_gemm8 needs N > 64;
             and every accumulating 16-bit launch, before any other engine is asked.
  pointwise  fp32 1x1, one 16-channel segment, N = 32, stride 1.
  halo_split CLSKD_F32X3, built tap count, >= 32 tiles (the plan of test_halo_split_plan.py).
  split3     CLSKD_F32X3 with 3 taps: conv_halo_split3_kernel has no such instance.
  halo_f32   plain fp32 (not split3's without CLSKD_F32_SPLIT=1), N = 64, 10 taps, Fo >= 8.
  igemm_f32  plain fp32 3 taps: no conv_halo_f32_kernel instance."""
import ctypes as C
import os
import subprocess
import sys

import pytest

from clskd import _lib
from halo_split_cases import ABF, DEC1, ENC, T
from test_halo_split_plan import _desc

# whether the engine's epilogue folds the BatchNorm finalize (gemm8: one N-tile, N <= 256)
FOLDS = {"direct": False, "halo": True, "halow": True, "gemm8": True, "lds_dma": False,
         "pointwise": False, "halo_split": True, "split3": True, "halo_f32": True,
         "igemm_f32": False}
_PROBE_FOLD = _lib.BnFold()  # zero record: only its presence is inspected


def _d(segc, N, taps, sf, Fi, Fo, of_mul, of_add, compute, accumulate=0, wlayout=_lib.WLAYOUT_NK):
    d = _desc(3, segc, N, taps, sf, Fi, Fo, of_mul, of_add, T, accumulate=accumulate)
    lowp = compute in (_lib.BF16, _lib.F16)
    d.compute = compute
    d.in_dtype = compute if lowp else _lib.F32
    d.out_dtype = _lib.F32 if accumulate else d.in_dtype
    d.K = -(-d.K // 64) * 64
    d.kvec = 8 if lowp else 4
    d.ktab, d.kseg = 0x3000000, 0x4000000
    d.wlayout = wlayout
    return d


# name: (descriptor arguments, the engine it reaches with every knob at its default)
CASES = {
    "direct": (((8, 8), 4, DEC1, 1, 20, 20, 2, 1, _lib.F32, 0, _lib.WLAYOUT_DIRECT), "direct"),
    "bf16_n64_10tap": (((32,), 64, ENC, 2, 40, 20, 1, 0, _lib.BF16), "halo"),
    "bf16_n32_4tap": (((32, 32), 32, DEC1, 1, 20, 20, 2, 1, _lib.BF16), "halo"),
    "bf16_n128_10tap": (((32,), 128, ENC, 2, 40, 20, 1, 0, _lib.BF16), "gemm8"),
    "bf16_n64_3tap": (((32,), 64, ABF[:3], 2, 40, 20, 1, 0, _lib.BF16), "lds_dma"),
    "bf16_n64_10tap_accumulate": (((32,), 64, ENC, 2, 40, 20, 1, 0, _lib.BF16, 1), "lds_dma"),
    "f32_1x1_c16_n32": (((16,), 32, [(0, 0)], 1, 20, 20, 1, 0, _lib.F32), "pointwise"),
    "f32x3_n64_10tap": (((16,), 64, ENC, 2, 40, 20, 1, 0, _lib.F32X3), "halo_split"),
    "f32x3_n64_3tap": (((16,), 64, ABF[:3], 2, 40, 20, 1, 0, _lib.F32X3), "split3"),
    "f32_n64_10tap": (((16,), 64, ENC, 2, 40, 20, 1, 0, _lib.F32), "halo_f32"),
    "f32_n32_4tap": (((8, 8), 32, DEC1, 1, 20, 20, 2, 1, _lib.F32), "halo_f32"),
    "f32_n64_3tap": (((16,), 64, ABF[:3], 2, 40, 20, 1, 0, _lib.F32), "igemm_f32"),
}
# the product knobs that switch a route, each at its non-default value
KNOBS = [("CLSKD_NO_HALO32", 1), ("CLSKD_F32_SPLIT", 1), ("CLSKD_HALO_SPLIT", 0),
         ("CLSKD_HALO32_SPLIT", 1)]


def _route(d):
    L = _lib.load(require_gpu=False)
    r = L.clskd_conv_route(C.byref(d))
    assert r is not None, L.clskd_last_error()
    return r.decode()


def _folds(d):
    d.bn_fold = C.addressof(_PROBE_FOLD)
    try:
        return _lib.load(require_gpu=False).clskd_conv_fold_capable(C.byref(d))
    finally:
        d.bn_fold = None


@pytest.mark.parametrize("case", sorted(CASES))
def test_route_of_each_engine(case):
    args, engine = CASES[case]
    assert _route(_d(*args)) == engine


@pytest.mark.parametrize("knob,value", [(None, 0)] + KNOBS, ids=lambda v: str(v))
@pytest.mark.parametrize("case", sorted(CASES))
def test_fold_capable_is_the_routed_engines_fold_column(case, knob, value):
    d = _d(*CASES[case][0])
    prev = _lib.set_knob(knob, value) if knob else None
    try:
        engine, folds = _route(d), _folds(d)
    finally:
        if knob:
            _lib.set_knob(knob, prev)
    print(case, knob, engine, folds)
    assert folds == int(FOLDS[engine])


def test_knobs_move_the_route():
    """Each product knob changes the engine of the descriptor it is meant for (so the test above
    does compare fold_capable against more than the default routes)."""
    moved = {("CLSKD_NO_HALO32", "f32_n64_10tap"): "igemm_f32",
             ("CLSKD_F32_SPLIT", "f32_n64_10tap"): "split3",
             ("CLSKD_HALO_SPLIT", "f32x3_n64_10tap"): "split3"}
    for (knob, case), engine in moved.items():
        prev = _lib.set_knob(knob, dict(KNOBS)[knob])
        try:
            assert _route(_d(*CASES[case][0])) == engine, (knob, case)
        finally:
            _lib.set_knob(knob, prev)


def test_route_refuses_what_the_dispatcher_refuses():
    L = _lib.load(require_gpu=False)
    d = _d(*CASES["f32_n64_10tap"][0])
    d.K += 8  # not padded
    assert L.clskd_conv_route(C.byref(d)) is None and b"padded" in L.clskd_last_error()
    d = _d(*CASES["direct"][0])
    d.N = 64  # outside the direct kernel's policy
    assert L.clskd_conv_route(C.byref(d)) is None and b"direct" in L.clskd_last_error()
    assert L.clskd_conv_route(None) is None


_CHILD = """
import sys
sys.path[:0] = sys.argv[1:3]
import ctypes as C
from clskd import _lib
import test_conv_route_cpu as R
assert _lib.experiments()
d = R._d(*R.CASES["bf16_n64_10tap"][0])
print("ROUTE", R._route(d), R._folds(d))
"""


@pytest.mark.skipif(not os.path.exists(os.path.join(os.path.dirname(_lib.LIB_PATH),
                                                    "libclskd_hip_exp.so")),
                    reason="the experiments library is not built")
def test_experiments_no_halo_routes_and_folds_alike():
    """CLSKD_NO_HALO=1 (experiments library): the narrow bf16 layer runs on the LDS-DMA engine,
    which has no fold epilogue, and clskd_conv_fold_capable says so."""
    here = os.path.dirname(os.path.abspath(__file__))
    pkg = os.path.dirname(os.path.dirname(_lib.LIB_PATH))
    env = dict(os.environ, CLSKD_LIB="exp", CLSKD_NO_HALO="1")
    out = subprocess.run([sys.executable, "-c", _CHILD, here, pkg], env=env, capture_output=True,
                         text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    assert "ROUTE lds_dma 0" in out.stdout, out.stdout
