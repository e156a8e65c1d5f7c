"""clskd_conv_fold_capable answers what the dispatcher does (csrc/conv_halo.hip, conv_halo32.hip:
conv_*_takes and launch_conv_* share one *_decide).  Pure host calls on descriptors with
placeholder pointers that are never dereferenced: no GPU is used and nothing is launched."""
import ctypes as C

import pytest

from clskd import _lib
from halo_split_cases import ABF, DEC0, DEC1, ENC, T
from test_halo_split_plan import _desc

BUILT = {4: DEC1, 6: DEC0, 9: ABF, 10: ENC}
# tap counts no halo kernel instance is built for (3: one column of the 3x3; 5: one of the 5x2)
UNBUILT = {3: ABF[:3], 5: ENC[::2]}

# B = 3, Fo = 20, T = 101: 3 x 4 = 36 tiles of 8 x 32 (>= 32).  Channels per segment: one 32-
# channel chunk (bf16) / two 8-channel chunks (fp32), so the [64][K] weights of the 10-tap layers
# stay resident beside the halo buffers without the column split.
# shape: (segment channels bf16, segment channels fp32, stride_f, Fi, Fo, of_mul, of_add)
SHAPES = {
    "enc": ((32,), (16,), 2, 40, 20, 1, 0),
    "dec_p1": ((32, 32), (8, 8), 1, 20, 20, 2, 1),
}
_PROBE_FOLD = _lib.BnFold()  # zero record: only its presence is inspected


def _capable(shape, N, taps, dtype):
    segc16, segc32, sf, Fi, Fo, of_mul, of_add = SHAPES[shape]
    lowp = dtype != _lib.F32
    d = _desc(3, segc16 if lowp else segc32, N, taps, sf, Fi, Fo, of_mul, of_add, T)
    d.compute = d.in_dtype = d.out_dtype = dtype
    d.K = -(-d.K // 64) * 64
    d.bn_fold = C.addressof(_PROBE_FOLD)
    return _lib.load(require_gpu=False).clskd_conv_fold_capable(C.byref(d))


@pytest.mark.parametrize("dtype", [_lib.BF16, _lib.F32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("N", [32, 64])
@pytest.mark.parametrize("shape", sorted(SHAPES))
@pytest.mark.parametrize("ntaps", sorted(BUILT))
def test_built_tap_counts_fold(ntaps, shape, N, dtype):
    assert _capable(shape, N, BUILT[ntaps], dtype) == 1


@pytest.mark.parametrize("dtype", [_lib.BF16, _lib.F32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("N", [32, 64])
@pytest.mark.parametrize("shape", sorted(SHAPES))
@pytest.mark.parametrize("ntaps", sorted(UNBUILT))
def test_unbuilt_tap_counts_do_not_fold(ntaps, shape, N, dtype):
    """Expected 0.  The halo plans of these descriptors fit, but conv_halo_kernel and
    conv_halo_f32_kernel are built for 4, 6, 9 and 10 taps only, so the launch declines and the
    layer runs on the generic engine: conv_igemm_bf16_dma for bf16 (conv_gemm8 takes N > 64
    only) and conv_igemm_f32 for fp32 (plain fp32 is not conv_split3_kernel's).  Neither has the
    folded BatchNorm finalize, so a bn_fold descriptor must be refused."""
    assert _capable(shape, N, UNBUILT[ntaps], dtype) == 0
