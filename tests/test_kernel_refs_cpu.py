"""The references of tests/kernel_refs.py against independent forms, at the shapes and inputs of
tests/test_gpu_kernel_refs.py (no GPU): a reference that is wrong would make the GPU tests
meaningless, so each autograd / torch-builtin form here meets a second derivation — explicit index
maps, the closed-form gradients in the kernels' comments, finite differences."""
import math

import pytest
import torch
import torch.nn.functional as F

import kernel_refs as R

f64 = torch.float64


def _nearest_f32(n_in, n_out):
    """ATen's nearest source index with the scale held in float32 (UpSample.h nearest_idx)."""
    scale = torch.tensor(n_in, dtype=torch.float32) / torch.tensor(n_out, dtype=torch.float32)
    s = torch.floor(torch.arange(n_out, dtype=torch.float32) * scale).long()
    return s.clamp(max=n_in - 1)


def _grid_pairs():
    pairs = set(R.NEAREST_PAIRS)
    for B, Fn, T, Fr, Tr, F2, T2 in R.ABF_CASES.values():
        pairs |= {(Fr, Fn), (Tr, T)} | ({(Fn, F2), (T, T2)} if F2 else set())
    for Fn, T, Fr, Tr in R.DOWN_CASES:
        pairs |= {(Fr, Fn), (Tr, T)}
    pairs |= {(64, 128), (128, 256), (131, 131)}  # the large ABF case
    return sorted(pairs)


@pytest.mark.parametrize("n_in,n_out", _grid_pairs())
@pytest.mark.parametrize("dtype", [torch.float32, f64])
def test_nearest_index_is_the_float32_scale_map(n_in, n_out, dtype):
    """F.interpolate(mode='nearest') picks the float32-scale index in float32 AND in float64, so
    the float64 references upsample on the same map as the kernels' nearest_src."""
    src = torch.arange(n_in, dtype=dtype).reshape(1, 1, n_in, 1)
    got = F.interpolate(src, size=(n_out, 1), mode="nearest").reshape(-1).long()
    assert torch.equal(got, _nearest_f32(n_in, n_out))


@pytest.mark.parametrize("Fn,T,Fr,Tr", R.DOWN_CASES + [(5, 7, 3, 4)])
def test_down_sum_is_an_index_add(Fn, T, Fr, Tr):
    g = torch.randn(2, Fn, T, 4, dtype=f64, generator=torch.Generator().manual_seed(1))
    prior = torch.randn(2, Fr, Tr, 4, dtype=f64, generator=torch.Generator().manual_seed(2))
    ref = torch.zeros(2, Fr, Tr, 4, dtype=f64)
    tmp = torch.zeros(2, Fr, T, 4, dtype=f64).index_add_(1, _nearest_f32(Fr, Fn), g)
    ref.index_add_(2, _nearest_f32(Tr, T), tmp)
    torch.testing.assert_close(R.nearest_down_sum(g, (Fr, Tr)), ref, rtol=1e-14, atol=1e-14)
    torch.testing.assert_close(R.nearest_down_sum(g, (Fr, Tr), prior), prior + ref, rtol=1e-14,
                               atol=1e-14)


@pytest.mark.parametrize("name", sorted(R.ABF_CASES))
def test_abf_backward_matches_the_closed_form(name):
    """Autograd of the fusion against csrc/norm_bwd.hip's comment: dx = g z0 + a0 w0x + a1 w1x,
    dy = g z1 + a0 w0y + a1 w1y, a_k = (sum_c g_c {x, y}_c) z_k (1 - z_k), with g = dout + the
    next level's gradient summed over each pixel's children."""
    case = R.ABF_CASES[name]
    d = {k: (v.double() if v is not None else None) for k, v in R.abf_inputs(case).items()}
    coef = None if name == "bare" else d["coef"]
    mv1 = None if name == "bare" else d["mv1"]
    dx, dyup, part, mag = R.abf_fuse_bwd(d["x1"], d["res"], d["w"], d["b"], coef, d["dout"],
                                         d["dnext"], mv1)
    B, Fn, T = case[:3]
    C = 64
    x = R.abf_affine(d["x1"], coef)
    yu = d["res"][:, _nearest_f32(case[3], Fn)][:, :, _nearest_f32(case[4], T)]
    g = d["dout"].clone()
    if d["dnext"] is not None:
        tmp = torch.zeros(B, Fn, case[6], C, dtype=f64).index_add_(1, _nearest_f32(Fn, case[5]),
                                                                 d["dnext"])
        g.index_add_(2, _nearest_f32(T, case[6]), tmp)
    w0x, w0y, w1x, w1y = d["w"][0, :C], d["w"][0, C:], d["w"][1, :C], d["w"][1, C:]
    z0 = torch.sigmoid(x @ w0x + yu @ w0y + d["b"][0])[..., None]
    z1 = torch.sigmoid(x @ w1x + yu @ w1y + d["b"][1])[..., None]
    a0 = (g * x).sum(-1, keepdim=True) * z0 * (1 - z0)
    a1 = (g * yu).sum(-1, keepdim=True) * z1 * (1 - z1)
    torch.testing.assert_close(dx, g * z0 + a0 * w0x + a1 * w1x, rtol=1e-12, atol=1e-13)
    torch.testing.assert_close(dyup, g * z1 + a0 * w0y + a1 * w1y, rtol=1e-12, atol=1e-13)
    torch.testing.assert_close(R.abf_fuse(d["x1"], d["res"], d["w"], d["b"], coef),
                               x * z0 + yu * z1, rtol=1e-13, atol=1e-14)
    if mv1 is not None:
        xhat = (d["x1"] - mv1[0]) / torch.sqrt(mv1[1] + 1e-5)
        torch.testing.assert_close(part[1], (dx * xhat).reshape(-1, C).sum(0), rtol=1e-11, atol=1e-12)
        assert (mag >= part.abs()).all()


@pytest.mark.parametrize("name", sorted(R.PAD_CASES))
def test_frame_pad_and_its_adjoint(name):
    """F.pad against the explicit mirror map (torch.stft center=True), the gradient against a
    scatter over that map; the limit case's middle samples collect three contributions."""
    L, pad, Lp, mode = R.PAD_CASES[name]
    x = torch.randn(3, L, dtype=f64, generator=torch.Generator().manual_seed(3))
    dxp = torch.randn(3, Lp, dtype=f64, generator=torch.Generator().manual_seed(4))
    ref = torch.zeros(3, Lp, dtype=f64)
    dref = torch.zeros(3, L, dtype=f64)
    hits = [0] * L
    for i in range(Lp):
        s = i - pad
        if mode == 1:
            s = -s if s < 0 else (2 * (L - 1) - s if s >= L else s)
        if 0 <= s < L:
            ref[:, i] = x[:, s]
            dref[:, s] += dxp[:, i]
            hits[s] += 1
    assert torch.equal(R.frame_pad(x, pad, Lp, mode), ref)
    torch.testing.assert_close(R.frame_pad_bwd(dxp, L, pad, mode), dref, rtol=1e-14, atol=1e-14)
    if name == "limit":
        assert hits == [2, 3, 3, 3, 2]


@pytest.mark.parametrize("name", sorted(R.OLA_CASES))
@pytest.mark.parametrize("clamp", [0, 1])
def test_ola_against_fold_and_its_gradient(name, clamp):
    """The loop overlap-add against F.fold; the gradient against dwav * [|pre| <= 1] / (window
    energy + 1e-8) read back per frame entry, exactly 0 outside [trim, trim + out_len); and the
    share of samples within the clamp gate's margin stays under 1 % for these inputs."""
    case = R.OLA_CASES[name]
    B, T, win, hop, trim, out_len = case
    frames, window, dwav = [t.double() for t in R.ola_inputs(case)]
    wav, pre = R.ola(frames, window, hop, out_len, trim, clamp)
    n = (T - 1) * hop + win
    fold = lambda c: F.fold(c, (1, n), (1, win), stride=(1, hop)).reshape(-1, n)
    acc = fold(frames.permute(0, 2, 1))
    den = fold((window * window)[None, :, None].expand(1, win, T)) + 1e-8
    full = acc / den
    torch.testing.assert_close(pre, full[:, trim:trim + out_len], rtol=1e-13, atol=1e-14)
    d, pre2 = R.ola_bwd(frames, window, dwav, hop, out_len, trim, clamp)
    assert torch.equal(pre2, pre)
    gate = torch.ones_like(pre) if not clamp else (pre.abs() <= 1).double()
    per_sample = dwav * gate / den[:, trim:trim + out_len]
    expect, inside = R.frames_of_samples(per_sample, T, win, hop, trim, 0.0)
    torch.testing.assert_close(d, expect, rtol=1e-13, atol=1e-14)
    assert (d[:, ~inside] == 0).all()
    near = ((pre.abs() - 1).abs() < R.OLA_GATE_MARGIN).double().mean().item()
    assert near <= 0.01, near
    if name == "model":
        assert 0.05 < (pre.abs() > 1).double().mean().item() < 0.6  # the gate is exercised


@pytest.mark.parametrize("name", sorted(R.STFT_CASES))
def test_stft_mag_loss_gradient_matches_the_closed_form(name):
    """csrc/norm_bwd.hip: dre = -scale * sign(log|Y| - log|X|) * re / |X|^2 where the power
    passes the 1e-7 floor, else 0; pad columns 0; the left-out share under 1 %."""
    case = R.STFT_CASES[name]
    nb, rows, ld, ldd = case
    X, Y = [t.double() for t in R.stft_inputs(case)]
    d = R.stft_mag_loss_bwd(X, Y, nb, 0.37, ldd)
    assert d.shape == (rows, ldd) and (d[:, 2 * nb:] == 0).all()
    re, im = X[:, :nb], X[:, nb:2 * nb]
    px = re * re + im * im
    sgn = torch.sign(R.stft_mags(Y, nb).log() - R.stft_mags(X, nb).log())
    k = torch.where(px >= 1e-7, -0.37 * sgn / px.clamp(min=1e-7), torch.zeros_like(px))
    torch.testing.assert_close(d[:, :nb], k * re, rtol=1e-12, atol=1e-14)
    torch.testing.assert_close(d[:, nb:2 * nb], k * im, rtol=1e-12, atol=1e-14)
    assert (d[:, 0:nb:7] == 0).all() and (d[:, 0:nb:5] == 0).all()
    assert (px[:, ::7] < 1e-9).all()
    assert R.stft_left_out(X, Y, nb).double().mean().item() <= 0.01
    out = R.stft_mag_loss(X, Y, nb, 0.1, 0.2)
    xm, ym = px.clamp(min=1e-7).sqrt(), R.stft_mags(Y, nb)
    assert abs(out[0].item() - 0.1 * math.sqrt(((ym - xm) ** 2).sum() / (ym ** 2).sum())) < 1e-13
    assert abs(out[1].item() - 0.2 * (ym / xm).log().abs().sum().item() / (rows * nb)) < 1e-13


@pytest.mark.parametrize("L", R.SISNR_LENGTHS)
def test_sisnr_rows_matches_the_projection_form(L):
    s1, s2 = [t.double()[:, :L] for t in R.sisnr_inputs(L)]
    got = R.sisnr_rows(s1, s2)
    for r in range(s1.shape[0]):
        a, b = s1[r], s2[r]
        st = torch.dot(a, b) / (torch.dot(b, b) + 1e-8) * b
        ref = 10 * math.log10(torch.dot(st, st).item() / (torch.dot(a - st, a - st).item() + 1e-8) + 1e-8)
        assert abs(got[r].item() - ref) < 1e-9
    if L >= 255:
        assert (got.abs() < 20).all(), got


def test_complex_combine_and_spec_bftc_layouts():
    g = torch.Generator().manual_seed(5)
    dre, dim = torch.randn(3, 37, generator=g), torch.randn(3, 37, generator=g)
    d = R.complex_combine_bwd(dre, dim)
    assert torch.equal(d, torch.stack([torch.cat([dre, dim]), torch.cat([dim, -dre])]))
    for B, T, ld, re0, im0, Fn in R.SPEC_CASES:
        spec = torch.randn(B, T, ld, generator=g)
        out = R.spec_bftc(spec, re0, im0, Fn)
        assert out.shape == (B, Fn, T, 2)
        assert out[B - 1, Fn - 1, T - 1, 0] == spec[B - 1, T - 1, re0 + Fn - 1]
        assert out[0, 2, 3, 1] == spec[0, 3, im0 + 2]


@pytest.mark.parametrize("B", R.SPKD_BATCHES)
@pytest.mark.parametrize("batchmean", [True, False])
def test_spkd_matrix_against_finite_differences(B, batchmean):
    """M = dG + dG^T: dz = M z is the autograd gradient, and dloss/dG matches central finite
    differences of the SPKD term over the Gram entries (float64); B = 1 gives exactly 0."""
    zs, zt = R.spkd_inputs(B)
    zs = zs[:, :, 8:16].double().reshape(B, -1)
    zt = zt.double().reshape(B, -1)
    M, dz, Gs, Gt = R.spkd_grad(zs, zt, batchmean, 0.37)
    torch.testing.assert_close(M @ zs, dz, rtol=1e-11, atol=1e-16)
    assert Gs.abs().min() >= 1e-3 * Gs.abs().max() and Gt.abs().min() >= 1e-3 * Gt.abs().max()
    if B == 1:
        assert (M == 0).all()
        return
    gen = torch.Generator().manual_seed(B)
    scale = float(Gs.abs().max())
    for _ in range(6):
        i, j = torch.randint(0, B, (2,), generator=gen).tolist()
        h = 1e-5 * scale
        E = torch.zeros_like(Gs)
        E[i, j] = h
        fd = (R.spkd_from_grams(Gs + E, Gt, batchmean, 0.37)
              - R.spkd_from_grams(Gs - E, Gt, batchmean, 0.37)).item() / (2 * h)
        # M_ij = dG_ij + dG_ji: recover dG from the same autograd leaf
        G = Gs.clone().requires_grad_()
        (dG,) = torch.autograd.grad(R.spkd_from_grams(G, Gt, batchmean, 0.37), G)
        assert abs(fd - dG[i, j].item()) <= 1e-6 * dG.abs().max().item() + 1e-18, (i, j)
        torch.testing.assert_close(M, dG + dG.t(), rtol=1e-12, atol=1e-20)


def test_batch_norm_references_against_torch():
    """kernel_refs.batch_norm_train / batch_norm_eval / bn_affine against F.batch_norm + F.prelu
    (float64), the two-slope PReLU against a per-channel loop, and the one-row statement."""
    import torch.nn.functional as F
    for rows, C in ((37, 24), (4864, 200)):
        d = {k: v.double() for k, v in R.bn_inputs(rows, C).items()}
        a = torch.tensor([0.25], dtype=torch.float64)
        r = R.batch_norm_train(d["x"], d["gamma"], d["beta"], d["rm"], d["rv"], 1e-5, 0.1, a)
        rm, rv = d["rm"].clone(), d["rv"].clone()
        y = F.prelu(F.batch_norm(d["x"], rm, rv, d["gamma"], d["beta"], True, 0.1, 1e-5), a)
        assert (r["y"] - y).abs().max() < 1e-12
        assert (r["rm"] - rm).abs().max() < 1e-12 and (r["rv"] - rv).abs().max() < 1e-12
        assert (r["var"] - d["x"].var(0, unbiased=False)).abs().max() < 1e-12
        e = R.batch_norm_eval(d["x"], d["gamma"], d["beta"], d["rm"], d["rv"], 1e-5, a)
        ye = F.prelu(F.batch_norm(d["x"], d["rm"], d["rv"], d["gamma"], d["beta"], False, 0.1, 1e-5), a)
        assert (e["y"] - ye).abs().max() < 1e-12
        two = R.bn_affine(d["x"], d["scale"], d["shift"], 0.25, 0.05)
        lin = d["x"] * d["scale"] + d["shift"]
        for c in range(C):
            slope = 0.25 if c < C // 2 else 0.05
            assert torch.equal(two[:, c], torch.where(lin[:, c] >= 0, lin[:, c], slope * lin[:, c]))
        assert (two < 0).any() and (two > 0).any()
    d = {k: v.double() for k, v in R.bn_inputs(1, 8).items()}
    r = R.batch_norm_train(d["x"], d["gamma"], d["beta"], d["rm"], d["rv"], 1e-5, 0.1)
    assert torch.equal(r["var"], torch.zeros(8, dtype=torch.float64))
    assert torch.equal(r["rv"], 0.9 * d["rv"]) and torch.isfinite(r["y"]).all()
    rows, C = R.BN_APPLY_LARGE
    assert rows * C // 8 > 4096 * 256 and (4096 * 256) % (C // 8)
