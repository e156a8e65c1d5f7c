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


def test_launch_plans_own_their_k_tables(monkeypatch):
    """A descriptor holds its K table by address, and ops._ktab's cache is bounded: a process that
    plans more than its 1024 signatures (a long suite, variable clip lengths) drops tables that
    cached plans still point at.  The plan keeps the tensors, so a launch after the cache has let
    go of them (and the freed memory has been handed out again) gives the first launch's bits —
    for the forward plan and the weight-gradient plan."""
    import gc

    from clskd import ops
    monkeypatch.setattr(ops, "_CONV_PLANS", {})
    monkeypatch.setattr(ops, "_WGRAD_PLANS", {})
    ops._ktab.cache_clear()
    B, F, Tn, Ci, N = 2, 8, 7, 24, 40
    taps = [(kf - 2, kt - 1) for kf in range(5) for kt in range(2)]
    g = torch.Generator().manual_seed(5)
    x = torch.randn(B, F, Tn, Ci, generator=g).to(DEV)
    dy = torch.randn(B, F, Tn, N, generator=g).to(DEV)
    K = len(taps) * Ci
    wp = ops.pack_weight(torch.randn(N, len(taps), Ci, generator=g).to(DEV) / K ** 0.5, K)
    omap = ops.OutMap(F * Tn * N, Tn * N, N)

    def launch():
        out = torch.zeros(B, F, Tn, N, device=DEV)
        ops.conv([ops.seg_bftc(x)], taps, B, F, Tn, N, wp, None, out, omap, mfma_only=True)
        dw = torch.zeros_like(wp)
        ops.conv_wgrad([ops.seg_bftc(x)], taps, B, F, Tn, N, dy, omap, dw)
        torch.cuda.synchronize()
        return out, dw

    first = launch()
    (plan,) = ops._CONV_PLANS.values()
    (wplan,) = ops._WGRAD_PLANS.values()
    for desc, (kt, ks) in ((plan.desc, plan.ktab), (wplan[0], wplan[3])):
        assert (desc.ktab, desc.kseg) == (kt.data_ptr(), ks.data_ptr())
    ops._ktab.cache_clear()  # what the 1025th signature does to the oldest table
    gc.collect()
    torch.cuda.empty_cache()
    junk = [torch.full((256,), -1, dtype=torch.int32, device=DEV) for _ in range(64)]
    again = launch()
    assert len(ops._CONV_PLANS) == 1 and len(ops._WGRAD_PLANS) == 1 and junk
    assert torch.equal(again[0], first[0]) and torch.equal(again[1], first[1])
