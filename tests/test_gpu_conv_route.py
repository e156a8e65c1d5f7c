"""clskd_conv_route names the engine whose kernel a launch then runs: the small layers of
test_conv_route_cpu.py, launched through ops.conv, and the kernel clskd_conv_last_kernel()
reports.  Numeric parity of each engine stays with its own suite."""
import ctypes as C

import pytest
import torch

from halo_split_cases import T
from test_conv_route_cpu import CASES

pytestmark = pytest.mark.gpu
DEV = "cuda"

KERNEL = {"direct": "conv_direct_kernel", "halo": "conv_halo_kernel", "halow": "conv_halow_kernel",
          "gemm8": "conv_gemm8_kernel", "lds_dma": "conv_igemm_bf16_dma",
          "pointwise": "conv_pointwise_kernel", "halo_split": "conv_halo_split3_kernel",
          "split3": "conv_split3_kernel", "halo_f32": "conv_halo_f32_kernel",
          "igemm_f32": "conv_igemm_f32"}


@pytest.mark.parametrize("case", sorted(CASES))
def test_launch_runs_the_routed_engine(case, monkeypatch):
    from clskd import _lib, ops
    (segc, N, taps, sf, Fi, Fo, of_mul, of_add, compute, *rest), engine = CASES[case]
    accumulate = bool(rest[0]) if rest else False
    bf16 = compute == _lib.BF16
    dt = torch.bfloat16 if bf16 else torch.float32
    B, Cin = 3, sum(segc)
    K = len(taps) * Cin
    g = torch.Generator().manual_seed(N + K)
    segs = [torch.randn(B, Fi, T, c, generator=g).to(DEV, dt) for c in segc]
    wp = ops.pack_weight(torch.randn(N, len(taps), Cin, generator=g).to(DEV) / K ** 0.5, K,
                         "bf16" if bf16 else "fp32")
    bias = torch.randn(N, generator=g).to(DEV)
    Fout = Fo * of_mul
    out = torch.zeros(B, Fout, T, N, device=DEV, dtype=torch.float32 if accumulate else dt)
    monkeypatch.setattr(ops, "_CONV_PLANS", {})  # the one plan of this launch, whatever ran before
    with ops.split_products(compute == _lib.F32X3):
        ops.conv([ops.seg_bftc(s) for s in segs], taps, B, Fo, T, N, wp, bias, out,
                 ops.OutMap(Fout * T * N, T * N, N, of_mul=of_mul, of_add=of_add), stride_f=sf,
                 accumulate=accumulate, mfma_only=engine != "direct")  # (ops' own direct policy)
    kernel = ops.conv_kernel_of_last_launch()
    torch.cuda.synchronize()
    (plan,) = ops._CONV_PLANS.values()
    L = _lib.load()
    route = L.clskd_conv_route(C.byref(plan.desc))
    assert route is not None, L.clskd_last_error()
    print(case, route.decode(), kernel)
    assert route.decode() == engine
    assert kernel.split("<")[0] == KERNEL[engine]
