"""Halo-tiled split-product conv (csrc/conv_halo_split.hip, CLSKD_HALO_SPLIT=1) against torch
fp64 at the split engine's derived bound (tests/test_gpu_split.py: |out - ref| <= 2e-5 * sum |x w|
+ 1e-7, statistics 1e-5 / 5e-5), beside conv_split3_kernel (CLSKD_HALO_SPLIT=0) on the same
inputs.  B = 3, T = 101: three full 32-step T tiles and a ragged one; >= 32 tiles so the kernel
takes the layer (the 4-row layer needs B = 16 for that: halo_split_cases.py); CLSKD_SPLIT_GRID
caps the grid so every workgroup walks several tiles."""
import numpy as np
import pytest
import torch

from halo_split_cases import CASES, T

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def refs():
    """fp64 reference, magnitude and inputs per case, computed once and shared (read-only)."""
    cache = {}

    def get(case):
        if case not in cache:
            import test_gpu_split as S
            from clskd import ops
            B, segc, N, taps, sf, Fi, Fo, of_mul, of_add, _ = CASES[case]
            g = torch.Generator().manual_seed(len(case) * 13 + N)
            segs = [torch.randn(B, Fi, T, c, generator=g) * 1.7 + 0.2 for c in segc]
            Cin = sum(segc)
            K = len(taps) * Cin
            w = torch.randn(N, len(taps), Cin, generator=g) * (0.7 / K ** 0.5)
            bias = torch.randn(N, generator=g)
            wp = ops.pack_weight(w.to(DEV), K)
            wq = wp[:, :K].cpu().double().view(N, len(taps), Cin)
            ref = S._ref(segs, taps, sf, Fo, T, wq, bias)
            mag = S._ref([s.abs() for s in segs], taps, sf, Fo, T, wq.abs(), bias.abs())
            cache[case] = ([s.to(DEV) for s in segs], wp, bias.to(DEV), ref, mag)
        return cache[case]
    return get


def _launch(case, data, accumulate=False, stats_on=True):
    from clskd import ops
    B, segc, N, taps, sf, Fi, Fo, of_mul, of_add, _ = CASES[case]
    segs, wp, bias, _, _ = data
    Fout = Fo * of_mul
    prior = torch.full((B, Fout, T, N), 0.25, device=DEV)
    out = prior.clone()
    nblk = ops.conv_mblocks(B, Fo, T)
    st = torch.full((nblk * N * 2,), float("nan"), device=DEV, dtype=torch.float64) \
        if stats_on and not accumulate else None
    with ops.split_products(True):
        ops.conv([ops.seg_bftc(s) for s in segs], taps, B, Fo, T, N, wp, bias, out,
                 ops.OutMap(Fout * T * N, T * N, N, of_mul=of_mul, of_add=of_add), stride_f=sf,
                 stats=st, accumulate=accumulate, mfma_only=True)
    return out, prior, st, ops.conv_kernel_of_last_launch()


def _check(case, data, out, prior, st):
    B, segc, N, taps, sf, Fi, Fo, of_mul, of_add, _ = CASES[case]
    _, _, _, ref, mag = data
    o = out.double().cpu()[:, of_add::of_mul]
    err = (o - ref).abs()
    bound = 2e-5 * mag + 1e-7
    worst = float((err / bound).max())
    print(f"{case}: max err {float(err.max()):.2e}, worst err/bound {worst:.3f}")
    assert worst <= 1.0
    if of_mul > 1:
        other = slice((of_add + 1) % of_mul, None, of_mul)
        assert torch.equal(out.cpu()[:, other], prior.cpu()[:, other])
    nblk = st.numel() // (N * 2)
    stc = st.view(nblk, N, 2).cpu()
    assert torch.isfinite(stc).all(), "every statistics slot must be written"
    S, Q = stc[..., 0].sum(0), stc[..., 1].sum(0)
    np.testing.assert_allclose(S.numpy(), ref.sum((0, 1, 2)).numpy(), rtol=1e-5,
                               atol=1e-5 * float(mag.sum((0, 1, 2)).max()))
    np.testing.assert_allclose(Q.numpy(), (ref * ref).sum((0, 1, 2)).numpy(), rtol=5e-5)


@pytest.fixture
def knobs():
    from clskd import _lib
    prev = {}

    def set_(**kw):
        for k, v in kw.items():
            p = _lib.set_knob(k, v)
            prev.setdefault(k, p)
    yield set_
    for k, v in prev.items():
        _lib.set_knob(k, v)


@pytest.mark.parametrize("grid", [0, 5])
@pytest.mark.parametrize("case", sorted(CASES))
def test_halo_split_against_torch(case, grid, refs, knobs):
    """Both routes against fp64; grid 5: 32-36 tiles on five workgroups (two per column half for
    the column-split shapes), seven to eighteen tiles each: the chunk prefetch crosses tile,
    F-block and batch boundaries."""
    data = refs(case)
    knobs(CLSKD_HALO_SPLIT=1, CLSKD_SPLIT_GRID=grid)
    out, prior, st, kname = _launch(case, data)
    assert kname.startswith("conv_halo_split3_kernel"), kname
    _check(case, data, out, prior, st)
    knobs(CLSKD_HALO_SPLIT=0)
    out0, prior0, st0, kname0 = _launch(case, data)
    assert kname0.startswith("conv_split3_kernel"), kname0
    _check(case, data, out0, prior0, st0)


@pytest.mark.parametrize("case", ["enc_n64", "dec_p0_n64_k768", "abf3x3_n64"])
def test_halo_split_bitwise_repeatable(case, refs, knobs):
    data = refs(case)
    knobs(CLSKD_HALO_SPLIT=1)
    out1, _, st1, kname = _launch(case, data)
    out2, _, st2, _ = _launch(case, data)
    assert kname.startswith("conv_halo_split3_kernel"), kname
    assert torch.equal(out1, out2) and torch.equal(st1, st2)


def test_halo_split_accumulate_stays_on_split3(refs, knobs):
    data = refs("enc_n64")
    knobs(CLSKD_HALO_SPLIT=1)
    _, _, _, kname = _launch("enc_n64", data, accumulate=True)
    assert kname.startswith("conv_split3_kernel"), kname


@pytest.mark.parametrize("case", ["enc_n64", "dec_p0_n64_k768"])
def test_halo_split_bn_fold_against_torch(case, refs, knobs):
    """Folded BatchNorm finalize (all columns per workgroup, and the column-split shape whose even
    / odd workgroups commit channels [0, 32) / [32, 64)) against the fp64 batch statistics."""
    from clskd import ops
    B, segc, N, taps, sf, Fi, Fo, of_mul, of_add, _ = CASES[case]
    segs, wp, bias, ref, _ = refs(case)
    knobs(CLSKD_HALO_SPLIT=1)
    g = torch.Generator().manual_seed(5)
    bn = torch.nn.BatchNorm2d(N).to(DEV)
    with torch.no_grad():
        bn.weight.copy_(torch.rand(N, generator=g) + 0.5)
        bn.bias.copy_(torch.randn(N, generator=g))
    mv = torch.empty(2, N, device=DEV)
    Fout = Fo * of_mul
    out = torch.zeros(B, Fout, T, N, device=DEV)
    stt = ops.BnStats(bn, N, B * Fo * T, 1, DEV, stats_out=(mv[0], mv[1]))
    with ops.split_products(True):
        ops.conv([ops.seg_bftc(s) for s in segs], taps, B, Fo, T, N, wp, bias, out,
                 ops.OutMap(Fout * T * N, T * N, N, of_mul=of_mul, of_add=of_add), stride_f=sf,
                 bn_stats=(stt, True), mfma_only=True)
    coef = stt.coefficients().clone()
    torch.cuda.synchronize()
    assert stt.mode == "fold"
    assert ops.conv_kernel_of_last_launch().startswith("conv_halo_split3_kernel")
    mean = ref.mean((0, 1, 2))
    var = ref.var((0, 1, 2), unbiased=False)
    np.testing.assert_allclose(mv[0].cpu().numpy(), mean.numpy(), rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(mv[1].cpu().numpy(), var.numpy(), rtol=1e-4, atol=1e-6)
    scale = bn.weight.detach().cpu().double() / torch.sqrt(var + bn.eps)
    np.testing.assert_allclose(coef[:N].cpu().numpy(), scale.numpy(), rtol=1e-4)
    acc, ticket = ops.bn_fold_state(bn, N, torch.device(DEV))
    assert int(acc.abs().sum()) == 0 and int(ticket.abs().sum()) == 0
