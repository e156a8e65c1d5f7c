"""GPU: the kernels of csrc/sup_loss.hip against the float64 restatement of tests/sup_loss_ref.py
under the suite's one tolerance rule (tests/kernel_refs.py:tolerance): every element within
8 * e32 + 4 * 2^-24 * max|ref64|, e32 the distance of the same torch expression in float32 from
float64; values at 5e-6 relative.  There is no gate in these losses, so no element is left out.
Each case prints `SUPK case e32 err tol`; profiles/sup_loss_margins.txt keeps one run's lines."""
import pytest
import torch

import kernel_refs as R
import sup_loss_ref as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
f32, f64 = torch.float32, torch.float64
VALUE_RTOL = 5e-6
SINGLE = [tuple(1.0 if i == k else 0.0 for i in range(5)) for k in range(5)]
MIXED = (0.3, 0.1, 0.2, 0.25, 0.15)


def _check(case, got, ref64, ref32, scale=None):
    e32, tol = R.tolerance(ref64, ref32, None, 8.0, scale)
    err = (got.detach().double().cpu() - ref64).abs()
    worst = float(err.max())
    print(f"SUPK {case} e32={e32:.3e} err={worst:.3e} tol={tol:.3e}")
    assert torch.isfinite(err).all(), case
    assert worst <= tol, (case, e32, worst, tol)


def _strided(t, ld, off, fill=777.0):
    """t [B, L] as a view of a [B, ld] device buffer `off` elements in (misaligned rows)."""
    B, L = t.shape
    buf = torch.full((B * ld + off,), fill, device=DEV)
    v = buf[off:].view(B, ld)[:, :L]
    v.copy_(t)
    return v


# (row stride - L, offsets of s / y / d from an aligned base): contiguous; misaligned rows that
# share their offset (16-byte accesses with a scalar head and tail); rows at different offsets
# (the scalar path)
LAYOUTS = ((0, (0, 0, 0)), (3, (1, 1, 1)), (3, (1, 2, 3)))


def _wave_case(tag, s, y, weights, layouts=LAYOUTS):
    from clskd import ops
    B, L = s.shape
    up = 0.625
    terms64 = S.wave_terms(s.double(), y.double())
    for wi, w in enumerate(weights):
        acc = bool(wi & 1)
        for pad, offs in layouts:
            ld = L + pad
            sd = s.to(DEV) if pad == 0 else _strided(s, ld, offs[0])
            yd = y.to(DEV) if pad == 0 else _strided(y, ld, offs[1])
            outs = []
            g = torch.Generator().manual_seed(9)
            d0 = torch.randn(B, L, generator=g)
            for rep in range(2):
                out, coef = ops.wave_loss(sd, yd, w, up)
                d = d0.clone().to(DEV) if pad == 0 else _strided(d0, ld, offs[2])
                ops.wave_loss_grad(sd, yd, coef, d, accumulate=acc)
                outs.append((out.clone(), coef.clone(), d.clone()))
                dview = d
            torch.cuda.synchronize()
            for a, b in zip(outs[0], outs[1]):
                assert torch.equal(a, b), "two runs differ"
            out, coef, d = outs[0]
            name = f"{tag}/B{B}L{L}ld{ld}o{offs[0]}{offs[1]}{offs[2]}w{wi}a{int(acc)}"
            # values: the components the weights select and their weighted total, 5e-6 relative
            # (the total against the sum of the terms' magnitudes: a mix may cancel)
            got = out.double().cpu()
            sel = [k for k in range(5) if w[k] != 0]
            for k in sel:
                assert abs(got[1 + k] - terms64[k]) <= VALUE_RTOL * abs(terms64[k]), (name, k, got, terms64)
            tot = sum(w[k] * terms64[k] for k in sel)
            mag = sum(abs(w[k] * terms64[k]) for k in sel)
            print(f"SUPK {name}/value got={float(got[0]):.9g} ref={float(tot):.9g}")
            assert abs(got[0] - tot) <= VALUE_RTOL * mag, (name, got, tot)
            # the table against the closed form (float64 restatement; p and p + q)
            c64 = S.coefficients(w, s.double(), y.double(), up)
            c32 = S.coefficients(w, s, y, up)
            pr64 = torch.stack([c64[:, 0], c64[:, 0] + c64[:, 1]], -1)
            pr32 = torch.stack([c32[:, 0], c32[:, 0] + c32[:, 1]], -1).double()
            _check(name + "/coef", coef, pr64, pr32)
            # the gradient against float64 autograd
            g64 = S.wave_grad_autograd(w, s.double(), y.double(), up)
            g32 = S.wave_grad_autograd(w, s, y, up)
            base = d0.double() if acc else 0.0
            _check(name + "/grad", d, g64 + base, (g32.double() + base) if acc else g32)
            if pad:  # nothing outside the rows was written
                assert (dview._base[:offs[2]] == 777.0).all()
                assert (dview._base[offs[2]:].view(B, ld)[:, L:] == 777.0).all()


@pytest.mark.parametrize("B", [1, 3, 16])
@pytest.mark.parametrize("L", [1, 7, 1600, 70001])
def test_wave_kernels_against_fp64(B, L):
    """L = 1, 7 (head / tail only), 1600, 70001 (a scalar tail, 18 blocks per row); contiguous
    rows and ld = L + 3 (misaligned rows, every row another offset: LAYOUTS); each single weight
    and one mix; upstream 0.625; accumulate on odd weight indices (onto a seeded buffer).

    L = 1 takes the MSE and SDR weights only: a one-sample estimate is always an exact multiple
    of its label, so the scale-invariant residual is zero and the reference's own SI-SNR / SI-SDR
    are log(x / 0) there — there is no value to hold the kernel to."""
    s, y = S.seeded_pair(B, L, seed=100 * B + L % 97)
    weights = SINGLE + [MIXED] if L > 1 else SINGLE[:2] + [(0.7, 0.3, 0, 0, 0)]
    _wave_case("wave", s, y, weights)


def test_wave_sums_do_not_cancel_when_the_estimate_is_nearly_the_label():
    """s = y + 1e-4-relative noise: sum (s - y)^2 is 1e-8 of sum s^2, which A - 2C + Y would hold
    to ~1e-8 relative in fp64 sums of fp32 products only by luck and a float32 pass not at all; the
    MSE and SDR values are held to 5e-6 and their gradients (p (s - y), r = 0) to the rule."""
    g = torch.Generator().manual_seed(77)
    y = 0.3 * torch.randn(3, 4099, generator=g)
    s = y + 3e-5 * torch.randn(3, 4099, generator=g)
    _wave_case("tiny", s.float(), y.float(), SINGLE[:2] + [(0.7, 0.3, 0, 0, 0)], LAYOUTS[:1])
    from clskd import ops
    out, coef = ops.wave_loss(s.to(DEV), y.to(DEV), (1, 1, 1, 1, 1))
    torch.cuda.synchronize()
    assert (coef[:, 1] != 0).any()
    t64 = S.wave_terms(s.double(), y.double())
    got = out.double().cpu()
    for k in range(5):  # the scale-invariant values too: the residuals are rebuilt around D
        print(f"SUPK tiny/term{k} got={float(got[1 + k]):.9g} ref={float(t64[k]):.9g}")
        assert abs(got[1 + k] - t64[k]) <= VALUE_RTOL * abs(t64[k]), (k, got, t64)


def _mel_case(B, T, ld):
    from clskd import ops
    clean, est = S.seeded_spec(B, T, ld, seed=10 * T + B)
    up = 1.75
    l64 = S.mel_from_specs(clean.double(), est.double())
    g64 = S.mel_grad_autograd(clean.double(), est.double(), up)
    g32 = S.mel_grad_autograd(clean, est, up)
    g64[:, :, 514:] = 0
    cd, ed = clean.to(DEV), est.to(DEV)
    name = f"mel/B{B}T{T}ld{ld}"
    vals = []
    for rep in range(2):
        out2 = torch.tensor([2.0, -1.0], device=DEV)
        ops.mel_loss(cd, ed, out2, scale=0.5, accumulate=True)
        vals.append(out2.clone())
    torch.cuda.synchronize()
    assert torch.equal(vals[0], vals[1])
    got = vals[0].double().cpu()
    print(f"SUPK {name}/value got={float(got[1]):.9g} ref={float(l64):.9g}")
    assert abs(got[1] - l64) <= VALUE_RTOL * abs(l64), (name, got, l64)
    assert abs(got[0] - (2.0 + 0.5 * l64)) <= VALUE_RTOL * (2.0 + 0.5 * abs(l64))
    w = ops.mel_loss(cd, ed)  # write mode
    assert torch.equal(w[1], vals[0][1]) and torch.equal(w[0], w[1])
    g = torch.Generator().manual_seed(3)
    d0 = torch.randn(B, T, ld, generator=g)
    for acc in (False, True):
        ds = []
        for rep in range(2):
            d = d0.clone().to(DEV)
            ops.mel_loss_bwd(cd, ed, d, up, accumulate=acc)
            ds.append(d)
        torch.cuda.synchronize()
        assert torch.equal(ds[0], ds[1])
        d = ds[0].cpu()
        assert torch.equal(d[:, :, 514:], d0[:, :, 514:])  # the pad columns are untouched
        base = d0.double() if acc else 0.0
        _check(f"{name}/a{int(acc)}/grad", d[:, :, :514], (g64 + base)[:, :, :514],
               ((g32.double() + base) if acc else g32)[:, :, :514])


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("T", [1, 2, 19, 163, 257, 300])
@pytest.mark.parametrize("ld", [514, 516])
def test_mel_kernels_against_fp64(B, T, ld):
    """T = 1 (one row spanning every frequency of the one frame), 2, 19, 163 (6 workgroups per
    clip, a ragged last one), 257 (rows of exactly one frequency: 257 consecutive frames), 300
    (T > 257: a row inside one frequency or across two); ld 514 and 516; value with scale and
    accumulate, and in write mode; gradient in write and accumulate mode onto a seeded buffer whose
    pad columns must survive; two runs bitwise equal."""
    _mel_case(B, T, ld)


def test_dccrn_loss_si_snr_is_bitwise_the_parents():
    """DCCRN.loss(..., 'SI-SNR') is still -si_snr of clskd_sisnr_rows + clskd_sum_f32, and the
    other waveform modes and one LMS mode return the restatement's values through the public
    method, with real / imag as forward returns them (views of one buffer) and as copies."""
    from clskd import config as cfg
    from clskd import ops
    from clskd.model import DCCRN
    from clskd.weights import STUDENT_SEED, apply_recipe
    m = apply_recipe(DCCRN(masking_mode="E", use_clstm=True, **cfg.STUDENT), STUDENT_SEED).to(DEV).train()
    x, y = S.seeded_batch(2, 1600, seed=7)
    X, Y = x.to(DEV), y.to(DEV)
    with torch.no_grad():
        _, _, real, imag, wav = m(X)
        rows = ops.sisnr_rows(wav, Y, 1e-8)
        parent = -ops.sum_f32(rows, torch.empty((), device=DEV), 1.0 / rows.numel())
        got = m.loss(wav, Y, real, imag, "SI-SNR")
        assert torch.equal(got, parent)
        assert torch.equal(m.loss(wav, Y), parent)  # the default mode, no spectra
        with S.oracle_dtype(f64) as O:
            cs = O.conv_stft(y.double())
        w64, r64, i64 = wav.double().cpu(), real.double().cpu(), imag.double().cpu()
        for mode in S.MODES:
            ref = float(S.dccrn_loss(mode, w64, y.double(), r64, i64, cs[:, :257], cs[:, 257:]))
            a = float(m.loss(wav, Y, real, imag, mode))
            b = float(m.loss(wav, Y, real.contiguous(), imag.contiguous(), mode))
            print(f"SUPK loss/{mode} got={a:.9g} copy={b:.9g} ref={ref:.9g}")
            # 2e-5: the clean spectrum is the device's float32 ConvSTFT of the labels here (the
            # kernels themselves are held to 5e-6 on identical inputs above)
            tol = (2e-5 if "LMS" in mode else VALUE_RTOL) * abs(ref)
            assert abs(a - ref) <= tol and abs(b - ref) <= tol, (mode, a, b, ref)
        for mode in S.PMSQE_MODES:
            with pytest.raises(NotImplementedError):
                m.loss(wav, Y, real, imag, mode)


def test_dccrn_backward_without_est_spec_is_bitwise_unchanged():
    """One KnowledgeDistillation step: the student gradients with g lacking 'est_spec' (today's
    call) equal those with g['est_spec'] = None, and a zero g['est_spec'] adds exactly nothing."""
    import clskd.backward as BW
    from clskd import config as cfg
    from clskd.data import synthetic_pairs
    from clskd.distill import KnowledgeDistillation
    from clskd.model import DCCRN
    from clskd.weights import ABF_SEED, STUDENT_SEED, TEACHER_SEED, apply_recipe
    t = apply_recipe(DCCRN(masking_mode="E", use_clstm=True, **cfg.TEACHER), TEACHER_SEED)
    s = apply_recipe(DCCRN(masking_mode="E", use_clstm=True, **cfg.STUDENT), STUDENT_SEED)
    kd = KnowledgeDistillation(t.train(), s.train(), abf_reinit="once").to(DEV)
    apply_recipe(kd.review_encoder, ABF_SEED, "encoder.")
    apply_recipe(kd.review_decoder, ABF_SEED, "decoder.")
    noisy, clean = synthetic_pairs(2, 1600, seed=5)
    X, Y = torch.from_numpy(noisy).to(DEV), torch.from_numpy(clean).to(DEV)
    res = []
    orig = BW.dccrn_backward
    for variant in ("absent", "none", "zeros"):
        def patched(m, tape, enc, dec, dec_in, lstm_io, g, pg, acc_params=False, join=None):
            assert "est_spec" not in g
            if variant == "none":
                g["est_spec"] = None
            elif variant == "zeros":
                g["est_spec"] = torch.zeros(tape["B"], tape["T"], 516, device=DEV)
            return orig(m, tape, enc, dec, dec_in, lstm_io, g, pg, acc_params, join)
        BW.dccrn_backward = patched
        try:
            grads = {p: torch.full_like(p, 3.0) for p in kd.student.parameters()}
            # a fresh taped forward per backward, as tests/test_gpu_backward.py repeats the step
            kd.backward_into(kd.forward_with_tape(X, Y), grads)
            torch.cuda.synchronize()
        finally:
            BW.dccrn_backward = orig
        res.append([grads[p].clone() for p in kd.student.parameters()])
    for a, b, c in zip(*res):
        assert torch.equal(a, b) and torch.equal(a, c)
        assert torch.isfinite(a).all()


def test_tools_for_loss_drop_ins():
    """sdr, si_sdr (each in both argument orders), l2_norm and get_array_mel_loss of
    clskd.tools_for_loss against the restatement; si_snr is the parent's function."""
    from clskd import tools_for_loss as TL
    a, b = S.seeded_pair(3, 1601, seed=21)
    A, B_ = a.to(DEV), b.to(DEV)
    a64, b64 = a.double(), b.double()
    for name, got, ref in (("sdr(a,b)", TL.sdr(A, B_), S.sdr(a64, b64)),
                           ("sdr(b,a)", TL.sdr(B_, A), S.sdr(b64, a64)),
                           ("si_sdr(a,b)", TL.si_sdr(A, B_), S.si_sdr(a64, b64)),
                           ("si_sdr(b,a)", TL.si_sdr(B_, A), S.si_sdr(b64, a64))):
        print(f"SUPK tools/{name} got={float(got):.9g} ref={float(ref):.9g}")
        assert got.dim() == 0 and abs(float(got) - float(ref)) <= VALUE_RTOL * abs(float(ref)), name
    assert torch.equal(TL.l2_norm(A, B_), torch.sum(A * B_, -1, keepdim=True))
    clean, est = S.seeded_spec(2, 19, 516, seed=4)
    got = TL.get_array_mel_loss(clean.to(DEV), est.to(DEV))
    ref = S.mel_from_specs(clean.double(), est.double())
    assert abs(float(got) - float(ref)) <= VALUE_RTOL * abs(float(ref))
    with pytest.raises(NotImplementedError):
        TL.sdr(A, B_, eps=1e-6)
