"""CPU references of the supervised losses (test infrastructure): a dtype-generic torch restatement
of the nine DCCRN.loss modes that need no PMSQE table (DCCRN.py:259-411, tools_for_loss.py:22-252),
the closed-form gradient coefficients of the waveform terms, and the end-to-end step references
(autograd through oracle.ref_cpu.dccrn_forward / oracle.asteroid_cpu.forward).

Every function computes in the dtype of its tensor arguments.  The mel rows are the reference's:
``perceptual_transform`` views the contiguous [257][T] magnitudes of one clip as (-1, 257), so row
r is the flat run [257 r, 257 r + 257) of the frequency-major array and filter position j is the
offset inside that run — restated here with the same ``reshape`` on the same layout, not with
index arithmetic."""
import contextlib
import math
import os

import numpy as np
import torch
import torch.nn.functional as F

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MODES = ("MSE", "SDR", "SI-SNR", "SI-SDR", "MSE+LMS", "MSE+SI-SNR", "SI-SNR+SI-SDR", "SDR+LMS",
         "SI-SNR+LMS")
WAVE_MODES = tuple(m for m in MODES if "LMS" not in m)
LMS_MODES = tuple(m for m in MODES if "LMS" in m)
PMSQE_MODES = ("MSE+PMSQE", "SDR+PMSQE", "SI-SNR+PMSQE")
SCALES = (16, 32, 64)
EPS = 1e-8


def fixture():
    return np.load(os.path.join(GOLDEN, "sup_loss.npz"))


# ------------------------------------------------------------------------------------------
# tools_for_loss.py
# ------------------------------------------------------------------------------------------
def dot(a, b):
    return torch.sum(a * b, -1, keepdim=True)


def sdr(s1, s2, eps=EPS):
    sn, d = dot(s1, s1), dot(s1 - s2, s1 - s2)
    return torch.mean(10 * torch.log10(sn ** 2 / (d ** 2 + eps)))


def si_snr(s1, s2, eps=EPS):
    target = dot(s1, s2) / (dot(s2, s2) + eps) * s2
    noise = s1 - target
    return torch.mean(10 * torch.log10(dot(target, target) / (dot(noise, noise) + eps) + eps))


def si_sdr(reference, estimation, eps=EPS):
    energy = torch.sum(reference ** 2, -1, keepdim=True)
    scaling = torch.sum(reference * estimation, -1, keepdim=True) / energy + eps
    proj = scaling * reference
    noise = estimation - proj
    ratio = torch.sum(proj ** 2, -1) / torch.sum(noise ** 2, -1) + eps
    return 10 * torch.log10(torch.mean(ratio) + eps)


def mel_filterbank(n, fft_size=512, fs=16000):
    """melFilterBank(n, fft_size) (tools_for_loss.py:133-177), float64 [n][fft_size / 2 + 1]: the
    n + 2 mel-spaced points are held in a float32 array while they are turned into bin edges."""
    bins = int(fft_size / 2) + 1
    nyq = fs / 2
    to_mel = lambda f: 1127.01048 * math.log(1 + f / 700.0)  # noqa: E731
    to_hz = lambda m: 700 * (math.exp(m / 1127.01048) - 1)  # noqa: E731
    pts = np.arange(n + 2).astype(np.float32) * (to_mel(nyq) - to_mel(0)) / (n + 1) + to_mel(0)
    for i in range(n + 2):
        pts[i] = to_hz(pts[i])
        pts[i] = math.floor(bins * pts[i] / nyq)
    e = [int(v) for v in pts]
    bank = np.zeros((n, bins))
    for i in range(1, n + 1):
        for j in range(e[i - 1], e[i]):
            bank[i - 1, j] = (float(j) - e[i - 1]) / (e[i] - e[i - 1])
        for j in range(e[i], e[i + 1]):
            bank[i - 1, j] = 1 - ((float(j) - e[i]) / (e[i + 1] - e[i]))
    return bank


_BANKS = {}


def banks(dtype):
    """The three filterbanks as the reference uses them: float32 values, transposed [257][S]."""
    if dtype not in _BANKS:
        _BANKS[dtype] = [torch.from_numpy(mel_filterbank(s).T.copy()).float().to(dtype) for s in SCALES]
    return _BANKS[dtype]


def mel_loss(clean_mags, est_mags):
    """get_array_mel_loss (tools_for_loss.py:195-252) of magnitudes [B][257][T] (frequency-major,
    as DCCRN.loss builds them)."""
    total = 0
    for c, e in zip(clean_mags, est_mags):
        rows_c = c.contiguous().reshape(-1, 257) / 512.0
        rows_e = e.contiguous().reshape(-1, 257) / 512.0
        dist = []
        for fb in banks(c.dtype):
            pc = torch.log(rows_c @ fb + 1e-7)
            pe = torch.log(rows_e @ fb + 1e-7)
            dist.append(torch.mean(torch.sqrt(torch.mean((pe - pc) ** 2, -1) + 1e-7)))
        total = total + torch.mean(torch.stack(dist))
    return total / len(clean_mags)


def mags(real, imag):
    return torch.sqrt(real ** 2 + imag ** 2 + 1e-7)


def lms(clean_real, clean_imag, real_spec, img_spec):
    return mel_loss(mags(clean_real, clean_imag), mags(real_spec, img_spec))


def dccrn_loss(mode, inputs, labels, real_spec=None, img_spec=None, clean_real=None, clean_imag=None):
    """DCCRN.loss (DCCRN.py:259-411).  clean_real / clean_imag [B][257][T]: self.stft(labels)."""
    if mode == "MSE":
        return F.mse_loss(inputs, labels)
    if mode == "SDR":
        return -sdr(labels, inputs)
    if mode == "SI-SNR":
        return -si_snr(inputs, labels)
    if mode == "SI-SDR":
        return -si_sdr(labels, inputs)
    if mode == "MSE+LMS":
        return (1e3 * F.mse_loss(inputs, labels) + lms(clean_real, clean_imag, real_spec, img_spec)) / 1001.0
    if mode == "MSE+SI-SNR":
        return (-si_snr(inputs, labels) + 100 * F.mse_loss(inputs, labels)) / 101
    if mode == "SI-SNR+SI-SDR":
        return (-si_snr(inputs, labels) - si_sdr(inputs, labels)) / 2
    if mode == "SDR+LMS":
        return (-sdr(labels, inputs) + 2 * lms(clean_real, clean_imag, real_spec, img_spec)) / 3
    if mode == "SI-SNR+LMS":
        return (-si_snr(inputs, labels) + 2 * lms(clean_real, clean_imag, real_spec, img_spec)) / 3
    raise ValueError(mode)


TERMS = (lambda s, y: F.mse_loss(s, y), lambda s, y: -sdr(y, s), lambda s, y: -si_snr(s, y),
         lambda s, y: -si_sdr(y, s), lambda s, y: -si_sdr(s, y))


def wave_terms(s, y):
    """The five components of clskd_wave_loss in order."""
    return torch.stack([t(s, y) for t in TERMS])


def weighted(w, s, y):
    """sum_k w_k l_k over the non-zero weights only (an unselected term that is not finite, as the
    scale-invariant ones are at L = 1, must not reach the sum or its gradient)."""
    return sum(float(wk) * TERMS[k](s, y) for k, wk in enumerate(w) if wk != 0)


# ------------------------------------------------------------------------------------------
# closed-form coefficients: d (sum_k w_k l_k) / d s_b = p_b s_b + q_b y_b
# ------------------------------------------------------------------------------------------
def coefficients(w, s, y, upstream=1.0, eps=EPS):
    """[B][2] in the dtype of s, from the per-row sums A = sum s^2, Y = sum y^2, C = sum s y,
    D = sum (s - y)^2 (the kernel's finalize states the same algebra in fp64)."""
    B, L = s.shape
    A, Y, C, D = (s * s).sum(-1), (y * y).sum(-1), (s * y).sum(-1), ((s - y) ** 2).sum(-1)
    K = 10.0 / math.log(10.0)
    p = torch.zeros_like(A)
    q = torch.zeros_like(A)

    def resid(X, Er, a):  # sum (e - a r)^2 with Er = sum r^2, X = sum r e
        u = 1 - a
        return D + 2 * u * (X - Er) + u * u * Er

    if w[0]:
        p = p + w[0] * 2.0 / (B * L)
        q = q - w[0] * 2.0 / (B * L)
    if w[1]:
        k1 = w[1] * 4 * K * D / (D * D + eps) / B
        p, q = p + k1, q - k1
    if w[2]:
        Ye = Y + eps
        a = C / Ye
        Tn = a * a * Y
        Ne = resid(C, Y, a) + eps
        r = Tn / Ne + eps
        K2 = w[2] * K / B / r
        p = p + K2 * 2 * Tn / Ne ** 2
        q = q - K2 * (2 * a * Y / (Ye * Ne) + Tn / Ne ** 2 * (2 * a + 2 * (C - a * Y) / Ye))
    if w[3]:
        a = C / Y + eps
        P = a * a * Y
        Nz = resid(C, Y, a)
        K3 = K / ((torch.mean(P / Nz + eps) + eps) * B)
        p = p + w[3] * K3 * 2 * P / Nz ** 2
        q = q - w[3] * K3 * (2 * a / Nz + P / Nz ** 2 * (2 * a - 2 * eps))
    if w[4]:
        c1 = C / A
        a = c1 + eps
        P = a * a * A
        Nz = resid(C, A, a)
        g = C - a * A
        K4 = K / ((torch.mean(P / Nz + eps) + eps) * B)
        ps = (-4 * a * c1 + 2 * a * a) / Nz - P / Nz ** 2 * (2 * a * a + 4 * g * c1 / A)
        qs = 2 * a / Nz + P / Nz ** 2 * (2 * a + 2 * g / A)
        p = p - w[4] * K4 * ps
        q = q - w[4] * K4 * qs
    return upstream * torch.stack([p, q], -1)


def wave_grad_autograd(w, s, y, upstream=1.0):
    ss = s.detach().clone().requires_grad_()
    (g,) = torch.autograd.grad(upstream * weighted(w, ss, y), ss)
    return g


# ------------------------------------------------------------------------------------------
# mel distance on frame-major spectra (the kernels' layout)
# ------------------------------------------------------------------------------------------
def spec_to_reim(spec):
    """[B][T][ld >= 514] (re at f, im at 257 + f) -> real, imag [B][257][T]."""
    return spec[:, :, :257].transpose(1, 2), spec[:, :, 257:514].transpose(1, 2)


def mel_from_specs(clean, est):
    cr, ci = spec_to_reim(clean)
    er, ei = spec_to_reim(est)
    return lms(cr, ci, er, ei)


def mel_grad_autograd(clean, est, upstream=1.0):
    e = est.detach().clone().requires_grad_()
    (g,) = torch.autograd.grad(upstream * mel_from_specs(clean, e), e)
    return g


# ------------------------------------------------------------------------------------------
# inputs
# ------------------------------------------------------------------------------------------
def seeded_batch(B, L, seed=0, peak=0.3):
    """(mixture, clean) [B, L] float32: broadband seeded noise (mini_train_ref.seeded_batch says
    why), the clean target correlated with the mixture (clean = 0.6 mixture + independent noise)
    so the SI-SDR of a network's estimate stays inside [-35, +20] dB, everything well inside the
    iSTFT's clamp(-1, 1)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, L, generator=g)
    x = x * (peak / x.abs().max())
    n = torch.randn(B, L, generator=g)
    y = 0.6 * x + 0.4 * n * (peak / n.abs().max())
    return x.float(), y.float()


def seeded_pair(B, L, seed=0, snr_scale=0.5, ld=None):
    """(estimate, labels) [B, L] float32 for the kernel tests, optionally as views of [B, ld]."""
    g = torch.Generator().manual_seed(seed)
    y = 0.3 * torch.randn(B, L, generator=g)
    s = (0.4 + 0.9 * torch.rand(B, 1, generator=g)) * y + snr_scale * 0.3 * torch.randn(B, L, generator=g)
    return s.float(), y.float()


def seeded_spec(B, T, ld, seed=0):
    """(clean, est) [B][T][ld] float32 spectra with STFT-like magnitudes spread over decades."""
    g = torch.Generator().manual_seed(seed)
    shape = 10.0 ** (-2.0 * torch.rand(1, 1, 257, generator=g))
    clean = torch.randn(B, T, ld, generator=g)
    est = clean + 0.5 * torch.randn(B, T, ld, generator=g)
    for t in (clean, est):
        t[:, :, :257] *= 20.0 * shape
        t[:, :, 257:514] *= 20.0 * shape
    return clean.float(), est.float()


# ------------------------------------------------------------------------------------------
# end-to-end step references
# ------------------------------------------------------------------------------------------
@contextlib.contextmanager
def oracle_dtype(dtype):
    """oracle.ref_cpu in `dtype`: its float32 STFT kernels (the values the device holds) cast to
    dtype, and torch's default dtype for the tensors it creates on the way."""
    from oracle import ref_cpu as R
    R._kernels()
    keep, was = R._KCACHE["k"], torch.get_default_dtype()
    R._KCACHE["k"] = tuple(k.to(dtype) for k in keep)
    torch.set_default_dtype(dtype)
    try:
        yield R
    finally:
        torch.set_default_dtype(was)
        R._KCACHE["k"] = keep


def dccrn_params(dtype, which="student"):
    """The recipe weights of the student (or teacher) configuration in `dtype`, requires_grad on
    every parameter."""
    from clskd import config as cfg
    from clskd.weights import STUDENT_SEED, TEACHER_SEED, recipe_state_dict
    from oracle import ref_cpu as R
    kw, seed = (cfg.STUDENT, STUDENT_SEED) if which == "student" else (cfg.TEACHER, TEACHER_SEED)
    ps = R.to_torch_params(recipe_state_dict(cfg.dccrn_param_shapes(**kw), seed))
    out = {}
    for k, v in ps.items():
        if v.is_floating_point():
            v = v.to(dtype).clone()
            if not k.endswith(("running_mean", "running_var")):
                v.requires_grad_()
        out[k] = v
    return out


def mrstft_mag(x, y):
    import mini_train_ref as M
    return M.mrstft_mag(x, y)


def dccrn_steps(modes, x, y, dtype=torch.float64, which="student"):
    """{mode: dict(loss, grads {name: tensor})} of the student (or teacher) DCCRN (recipe weights,
    train mode) for every mode in `modes` ('MRSTFT' included) from one forward in `dtype`."""
    with oracle_dtype(dtype) as R:
        ps = dccrn_params(dtype, which)
        x, y = x.to(dtype), y.to(dtype)
        fw = R.dccrn_forward(ps, x, train=True, lstm_fn=R.lstm)
        cs = R.conv_stft(y)
        cr, ci = cs[:, :257], cs[:, 257:]
        names = [k for k, v in ps.items() if v.requires_grad]
        out = {}
        for mode in modes:
            if mode == "MRSTFT":
                loss = mrstft_mag(fw["out_wav"], y)
            else:
                loss = dccrn_loss(mode, fw["out_wav"], y, fw["real"], fw["imag"], cr, ci)
            grads = torch.autograd.grad(loss, [ps[n] for n in names], retain_graph=True, allow_unused=True)
            out[mode] = dict(loss=loss.detach(), grads=dict(zip(names, grads)), wav=fw["out_wav"].detach())
    return out


def mini_steps(modes, x, y, dtype=torch.float64):
    """The same for the fixture DCCRNet_mini (waveform modes and 'MRSTFT')."""
    import mini_train_ref as M
    from oracle import asteroid_cpu as A
    sd = M.trainable_state(dtype)
    x, y = x.to(dtype), y.to(dtype)
    wav = A.forward(sd, x, train=True)
    names = M.trainable_keys(sd)
    out = {}
    for mode in modes:
        loss = mrstft_mag(wav, y) if mode == "MRSTFT" else dccrn_loss(mode, wav, y)
        grads = torch.autograd.grad(loss, [sd[n] for n in names], retain_graph=True)
        out[mode] = dict(loss=loss.detach(), grads=dict(zip(names, grads)), wav=wav.detach())
    return out


def is_pre_bn_bias(name, n_layers=6):
    """Conv biases in front of a train-mode normalisation: analytically zero gradient (the
    project's existing rule, tests/test_gpu_backward.py:_compare).  A normalisation follows every
    conv but the last decoder layer's (decoder.{n_layers - 1}, DCCRN.py:111-145)."""
    return name.endswith("_conv.bias") and not name.startswith(f"decoder.{n_layers - 1}.")


def grad_errors(got, ref, n_layers=6):
    """{name: (error, kind)}: relative L2, or for a pre-BN conv bias max(|got|, |ref|) / |dW ref|
    (gate 1e-3, as tests/test_gpu_backward.py).  n_layers: the model's encoder / decoder depth."""
    out = {}
    for n, r in ref.items():
        if r is None:
            continue
        g, r = got[n].double(), r.double()
        if is_pre_bn_bias(n, n_layers):
            wref = ref[n.replace(".bias", ".weight")].double().norm()
            out[n] = (float(max(g.norm(), r.norm()) / wref), "zero")
        else:
            out[n] = (float((g - r).norm() / r.norm()), "rel")
    return out
