"""Plain torch references of the small backward / loss kernels, one function per operation.

Test infrastructure for tests/test_gpu_kernel_refs.py (the kernels against these references on
the GPU) and tests/test_kernel_refs_cpu.py (these references against independent forms, no GPU).

Every function is dtype-generic: it computes in the dtype of its tensor arguments.  The tests call
each one twice — in float64 (the reference) and in float32 (the "same expression in float32" whose
distance to the float64 result scales the tolerance, see ``tolerance``).  The references are
written the plain way: ``F.interpolate(mode="nearest")``, ``F.pad(mode="reflect")``, a loop-based
overlap-add, the formulas in the comments of csrc/norm.hip, csrc/norm_bwd.hip and csrc/loss.hip,
and autograd with explicit leaves for every gradient.  None of them restates a kernel's index
arithmetic.

Layouts follow the kernels: feature maps are BFTC ([B][F][T][C], channels last), spectra are
rows of [re(0..nbins) | im(0..nbins) | pad].
"""
import torch
import torch.nn.functional as F

# (B, F, T, Fr, Tr, F2, T2): this level's grid, the residual's grid, the next level's grid (0: none)
ABF_CASES = {
    "model": (2, 8, 13, 4, 13, 16, 13),    # the model's path: F doubles, T equal
    "mix": (2, 6, 7, 6, 7, 6, 14),         # identity residual, 1x / 2x mix
    "general": (2, 5, 7, 3, 4, 7, 9),      # non-integer ratios on both axes
    "double": (2, 4, 5, 2, 3, 8, 10),      # 2x on both axes: all four children of the fast path
    "bare": (1, 3, 5, 3, 5, 0, 0),         # no next level, no BN partials, no folded affine
}
DOWN_CASES = [(7, 9, 3, 4), (8, 13, 4, 13), (5, 5, 5, 5)]  # (F, T, Fr, Tr)
NEAREST_PAIRS = [(3, 8), (5, 7), (4, 9), (7, 13), (1, 6)]  # (in, out)
# (L, pad, Lp, mode): reflect, reflect truncated, reflect at its limit, zero mode
PAD_CASES = {
    "reflect": (401, 256, 401 + 2 * 256, 1),
    "truncated": (401, 256, 401 + 256 + 3, 1),
    "limit": (5, 4, 5 + 2 * 4, 1),
    "zero": (250, 300, 250 + 2 * 300, 0),
}
# (B, T, win, hop, trim, out_len)
OLA_CASES = {
    "model": (2, 9, 400, 100, 300, 600),
    "small": (1, 5, 10, 3, 2, 14),
    "one": (1, 1, 8, 4, 0, 8),
    "ragged": (2, 9, 400, 100, 300, 570),
}
# (nbins, rows, ld, ldd)
STFT_CASES = {"n17_ld34": (17, 33, 34, 36), "n17_ld36": (17, 33, 36, 36), "n257": (257, 5, 514, 516)}
SISNR_LENGTHS = [1, 255, 257, 1000]
SPEC_CASES = [(2, 65, 40, 1, 21, 19), (1, 64, 70, 0, 35, 33)]  # (B, T, ld, re0, im0, F)
SPKD_BATCHES = [1, 5, 16, 29, 32]

OLA_GATE_MARGIN = 1e-4    # | |pre-clamp sample| - 1 |
STFT_SIGN_MARGIN = 1e-5   # | log|Y| - log|X| |
STFT_FLOOR_MARGIN = 1e-8  # | re^2 + im^2 - 1e-7 |


def tolerance(ref64, ref32, keep=None, factor=8.0, scale=None):
    """(e32, tol) of the suite's one rule: e32 = max|ref32 - ref64| over the compared elements,
    tol = factor * e32 + 4 * 2^-24 * scale with scale = max|ref64| unless given (a tensor
    broadcastable to ref64 for sums: the sum of the terms' magnitudes).  Never looks at a kernel's
    output."""
    d = (ref32.double() - ref64).abs()
    a = ref64.abs()
    if keep is not None:
        d, a = d[keep], a[keep]
    e32 = float(d.max()) if d.numel() else 0.0
    if scale is None:
        scale = float(a.max()) if a.numel() else 0.0
    return e32, factor * e32 + 4.0 * 2.0 ** -24 * scale


def cast(dtype, *ts):
    return [None if t is None else t.to(dtype) for t in ts]


# ------------------------------------------------------------------------------------------
# ReviewKD attention fusion (framework.py:209-219)
# ------------------------------------------------------------------------------------------
def upsample(t, size):
    """Nearest upsampling of a BFTC map to the grid `size` = (F, T)."""
    return F.interpolate(t.permute(0, 3, 1, 2), size=tuple(size), mode="nearest").permute(0, 2, 3, 1)


def abf_mix(x, yu, w, b):
    """z = sigmoid(w . [x; yu] + b) (w [2][2C], b [2]); out = x z0 + yu z1."""
    z = torch.sigmoid(torch.cat([x, yu], -1) @ w.t() + b)
    return x * z[..., 0:1] + yu * z[..., 1:2]


def abf_affine(x1, coef):
    """x = x1 * scale + shift with coef = [scale | shift] (the folded conv1 BatchNorm), or x1."""
    if coef is None:
        return x1
    C = x1.shape[-1]
    return x1 * coef[:C] + coef[C:]


def abf_fuse(x1, res, w, b, coef=None):
    return abf_mix(abf_affine(x1, coef), upsample(res, x1.shape[1:3]), w, b)


def abf_fuse_bwd(x1, res, w, b, coef, dout, dnext=None, mv1=None, eps=1e-5):
    """loss = sum(out * dout) + sum(upsample(out, next grid) * dnext); returns dloss/dx (x = the
    BN1 output), dloss/dyu (yu = the upsampled residual, a leaf) and, with mv1 = [mean1; var1],
    the conv1-BatchNorm backward sums per channel: part[0] = sum dx, part[1] = sum dx * xhat1 and
    mag[k] = the sum of the magnitudes of part[k]'s terms."""
    x = abf_affine(x1, coef).detach().requires_grad_()
    yu = upsample(res, x1.shape[1:3]).detach().requires_grad_()
    out = abf_mix(x, yu, w, b)
    loss = (out * dout).sum()
    if dnext is not None:
        loss = loss + (upsample(out, dnext.shape[1:3]) * dnext).sum()
    dx, dyup = torch.autograd.grad(loss, [x, yu])
    part = mag = None
    if mv1 is not None:
        xhat = (x1 - mv1[0]) * torch.rsqrt(mv1[1] + eps)
        terms = (dx, dx * xhat)
        part = torch.stack([t.sum((0, 1, 2)) for t in terms])
        mag = torch.stack([t.abs().sum((0, 1, 2)) for t in terms])
    return dx, dyup, part, mag


def nearest_down_sum(g, size, prior=None):
    """Adjoint of the nearest upsampling `size` -> g's grid applied to g (+ prior)."""
    B, _, _, C = g.shape
    u = torch.zeros(B, size[0], size[1], C, dtype=g.dtype, requires_grad=True)
    (d,) = torch.autograd.grad((upsample(u, g.shape[1:3]) * g).sum(), u)
    return d if prior is None else prior + d


# ------------------------------------------------------------------------------------------
# waveform tail: framing pad, overlap-add, log-magnitude loss, SI-SNR, complex combine
# ------------------------------------------------------------------------------------------
def frame_pad(x, pad, Lp, mode):
    """x [B][L] padded by `pad` on both ends (mode 1: reflect, 0: zeros), cut to Lp columns."""
    xp = F.pad(x.unsqueeze(0), (pad, pad), mode="reflect" if mode == 1 else "constant").squeeze(0)
    if Lp > xp.shape[1]:
        xp = F.pad(xp, (0, Lp - xp.shape[1]))
    return xp[:, :Lp]


def frame_pad_bwd(dxp, L, pad, mode, prior=None):
    x = torch.zeros(dxp.shape[0], L, dtype=dxp.dtype, requires_grad=True)
    (d,) = torch.autograd.grad((frame_pad(x, pad, dxp.shape[1], mode) * dxp).sum(), x)
    return d if prior is None else prior + d


def ola(frames, window, hop, out_len, trim, clamp):
    """ConviSTFT tail (tools_for_model.py:95-107, DCCRN.py:237): overlap-add of the frames
    [B][T][win], divided by the overlap-added window energy + 1e-8, samples [trim, trim + out_len),
    optionally clamped to [-1, 1].  Returns (wav, the pre-clamp samples)."""
    B, T, win = frames.shape
    n = (T - 1) * hop + win
    acc = frames.new_zeros(B, n)
    coff = frames.new_zeros(n)
    for t in range(T):
        acc = acc + F.pad(frames[:, t], (t * hop, n - t * hop - win))
        coff = coff + F.pad(window * window, (t * hop, n - t * hop - win))
    pre = (acc / (coff + 1e-8))[:, trim:trim + out_len]
    return (pre.clamp(-1.0, 1.0) if clamp else pre), pre


def ola_bwd(frames, window, dwav, hop, out_len, trim, clamp):
    """d sum(wav * dwav) / d frames; also the pre-clamp samples (the clamp gate's decision value)."""
    fr = frames.detach().clone().requires_grad_()
    wav, pre = ola(fr, window, hop, out_len, trim, clamp)
    (d,) = torch.autograd.grad((wav * dwav).sum(), fr)
    return d, pre.detach()


def frames_of_samples(s, T, win, hop, trim, fill):
    """The per-sample tensor s [B][out_len] seen from every frame entry: [B][T][win] holding
    s[b][t*hop + o - trim], `fill` where that sample lies outside [0, out_len)."""
    out_len = s.shape[1]
    idx = torch.arange(T)[:, None] * hop + torch.arange(win)[None, :] - trim
    ok = (idx >= 0) & (idx < out_len)
    v = s[:, idx.clamp(0, out_len - 1)]
    return torch.where(ok, v, torch.full_like(v, fill)), ok


def stft_mags(X, nbins):
    re, im = X[..., :nbins], X[..., nbins:2 * nbins]
    return torch.sqrt((re * re + im * im).clamp(min=1e-7))


def stft_mag_loss(X, Y, nbins, factor_sc, factor_mag, prior=None):
    """[spectral convergence, log-magnitude L1] of the estimate's spectrum X against Y
    (framework.py:16-101), each times its factor (+ prior)."""
    xm, ym = stft_mags(X, nbins), stft_mags(Y, nbins)
    sc = factor_sc * torch.linalg.norm(ym - xm) / torch.linalg.norm(ym)
    mag = factor_mag * (ym.log() - xm.log()).abs().mean()
    out = torch.stack([sc, mag])
    return out if prior is None else prior + out


def stft_mag_loss_bwd(X, Y, nbins, scale, ldd):
    """d (scale * sum|log|Y| - log|X||) / dX as rows of ldd columns (zero pad columns)."""
    Xl = X.detach().clone().requires_grad_()
    loss = scale * (stft_mags(Y, nbins).log() - stft_mags(Xl, nbins).log()).abs().sum()
    (d,) = torch.autograd.grad(loss, Xl)
    return F.pad(d[..., :2 * nbins], (0, ldd - 2 * nbins))


def sisnr_rows(s1, s2, eps=1e-8):
    """tools_for_loss.py:37-47, no DC removal: 10 log10(|s_t|^2 / (|e|^2 + eps) + eps) per row."""
    alpha = (s1 * s2).sum(-1, keepdim=True) / ((s2 * s2).sum(-1, keepdim=True) + eps)
    st = alpha * s2
    e = s1 - st
    return 10.0 * torch.log10((st * st).sum(-1) / ((e * e).sum(-1) + eps) + eps)


def complex_combine(rr, ii, ir, ri):
    """tools_for_model.py:168-169."""
    return rr - ii, ir + ri


def complex_combine_bwd(dre, dim):
    """Gradient w.r.t. the two LSTMs' outputs h [ws][2B][n] of real = h[0][:B] - h[1][B:],
    imag = h[0][B:] + h[1][:B]."""
    B = dre.shape[0]
    h = torch.zeros((2, 2 * B) + tuple(dre.shape[1:]), dtype=dre.dtype, requires_grad=True)
    real, imag = complex_combine(h[0, :B], h[1, B:], h[0, B:], h[1, :B])
    (d,) = torch.autograd.grad((real * dre).sum() + (imag * dim).sum(), h)
    return d


def spec_bftc(spec, re0, im0, Fn):
    """Frame-major spectrum [B][T][ld] -> BFTC encoder input [B][F][T][2] (re | im)."""
    return torch.stack([spec[:, :, re0:re0 + Fn], spec[:, :, im0:im0 + Fn]], -1).permute(0, 2, 1, 3)


# ------------------------------------------------------------------------------------------
# BatchNorm + PReLU over rows of C channels (csrc/norm.hip, csrc/common.h:bn_channel_coeffs)
# ------------------------------------------------------------------------------------------
BN_CHANNELS = (8, 24, 40, 72, 200)   # C/8 = 1, 3, 5, 9, 25 and C/4 = 2, 6, 10, 18, 50
BN_ROWS = (1, 37, 4864)              # one row; fewer rows than row lanes; several blocks
# C/8 = 3 does not divide the apply kernel's largest grid stride (4096 x 256 items), and only
# above that many items does a lane visit a second item and so another channel group
BN_APPLY_LARGE = (349589, 24)        # rows x 3 items = 4096 x 256 + 191


def bn_affine(x, scale, shift, alpha=None, alpha_im=None):
    """y = x scale + shift per channel, then PReLU with one slope — or, with alpha_im, alpha on
    the first half of the channels (real) and alpha_im on the second (imaginary)."""
    y = x * scale + shift
    if alpha is None:
        return y
    if alpha_im is None:
        return torch.where(y >= 0, y, alpha * y)
    h = x.shape[-1] // 2
    return torch.cat([torch.where(y[..., :h] >= 0, y[..., :h], alpha * y[..., :h]),
                      torch.where(y[..., h:] >= 0, y[..., h:], alpha_im * y[..., h:])], -1)


def bn_coeffs(mean, var, gamma, beta, eps):
    scale = gamma * torch.rsqrt(var + eps)
    return scale, beta - mean * scale


def batch_norm_train(x, gamma, beta, rm, rv, eps, momentum, alpha=None):
    """nn.BatchNorm2d train forward over x [rows][C]: batch mean and biased variance, the
    [scale | shift] coefficients, y (+ PReLU) and one running update (the unbiased variance; for
    one row, where that is undefined, the biased one — 0 — takes its place, as the kernel does)."""
    n = x.shape[0]
    mean = x.mean(0)
    var = ((x - mean) ** 2).mean(0)
    scale, shift = bn_coeffs(mean, var, gamma, beta, eps)
    unb = var * n / (n - 1) if n > 1 else var
    return dict(mean=mean, var=var, scale=scale, shift=shift, y=bn_affine(x, scale, shift, alpha),
                rm=(1 - momentum) * rm + momentum * mean, rv=(1 - momentum) * rv + momentum * unb)


def batch_norm_eval(x, gamma, beta, rm, rv, eps, alpha=None):
    scale, shift = bn_coeffs(rm, rv, gamma, beta, eps)
    return dict(scale=scale, shift=shift, y=bn_affine(x, scale, shift, alpha))


def bn_inputs(rows, C, seed=0):
    """fp32 CPU tensors: x [rows][C] with a per-channel level and spread, the affine parameters,
    non-trivial running statistics and [scale | shift] coefficients of mixed sign."""
    g = _gen(6000 + seed + 7 * C + rows % 1000)
    rn = lambda *s: torch.randn(*s, generator=g)
    x = rn(rows, C) * (0.5 + torch.rand(C, generator=g)) + 0.5 * rn(C)
    return dict(x=x.contiguous(), gamma=1.0 + 0.3 * rn(C), beta=0.2 * rn(C), rm=0.3 * rn(C),
                rv=0.5 + torch.rand(C, generator=g), scale=(0.5 + rn(C).abs()) * torch.sign(rn(C)),
                shift=0.5 * rn(C))


# ------------------------------------------------------------------------------------------
# SPKD (framework.py:150-172)
# ------------------------------------------------------------------------------------------
def spkd_from_grams(Gs, Gt, batchmean, scale):
    ns, nt = F.normalize(Gs, p=1, dim=1), F.normalize(Gt, p=1, dim=1)  # row L1, floor 1e-12
    loss = ((nt - ns) ** 2).sum()
    if batchmean:
        loss = loss / Gs.shape[0] ** 2
    return scale * loss


def spkd_grad(zs, zt, batchmean, scale):
    """Gradient of the SPKD term of student rows zs [B][Ns] against teacher rows zt [B][Nt]:
    returns M = dG + dG^T (dG = dloss / dGs), dz = dloss / dzs, and the two Grams."""
    z = zs.detach().clone().requires_grad_()
    Gs = z @ z.t()
    Gs.retain_grad()
    Gt = zt @ zt.t()
    spkd_from_grams(Gs, Gt, batchmean, scale).backward()
    return Gs.grad + Gs.grad.t(), z.grad, Gs.detach(), Gt


# ------------------------------------------------------------------------------------------
# inputs of the test cases (fixed seeds), shared by the GPU tests and the CPU self-checks
# ------------------------------------------------------------------------------------------
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def abf_inputs(case, seed=0, C=64):
    """fp32 CPU tensors of one ABF case (w [2][2C]; coef / mv1 as the ReviewKD backward's)."""
    B, Fn, T, Fr, Tr, F2, T2 = case
    g = _gen(1000 + seed)
    rn = lambda *s: torch.randn(*s, generator=g)
    d = dict(x1=rn(B, Fn, T, C), res=rn(B, Fr, Tr, C), w=(rn(2, 2 * C) * 0.2).contiguous(),
             b=rn(2) * 0.1, coef=torch.cat([rn(C).abs() + 0.5, rn(C) * 0.1]).contiguous(),
             mv1=torch.stack([rn(C) * 0.1, rn(C).abs() + 0.5]).contiguous(), dout=rn(B, Fn, T, C),
             dnext=rn(B, F2, T2, C) if F2 else None)
    return d


def hamming(win):
    return torch.hamming_window(win, periodic=True, dtype=torch.float64).float()


def ola_inputs(case, seed=0):
    """Frames = N(0, 1) times the window (what a windowed inverse transform hands the kernel)."""
    B, T, win, hop, trim, out_len = case
    g = _gen(2000 + seed)
    window = hamming(win)
    frames = (torch.randn(B, T, win, generator=g) * window).contiguous()
    dwav = torch.randn(B, out_len, generator=g)
    return frames, window, dwav


def stft_inputs(case, seed=0):
    """Gaussian spectra X, Y [rows][ld]; every 7th bin of X scaled to magnitude 1e-5 (below the
    1e-7 power floor), every 5th bin of Y equal to X; pad columns of both hold 7.0."""
    nb, rows, ld, _ = case
    g = _gen(3000 + seed)
    X = torch.randn(rows, ld, generator=g)
    Y = torch.randn(rows, ld, generator=g)
    mag = torch.sqrt(X[:, :nb] ** 2 + X[:, nb:2 * nb] ** 2)
    s = torch.ones(rows, nb)
    s[:, ::7] = 1e-5 / mag[:, ::7]
    X[:, :nb] *= s
    X[:, nb:2 * nb] *= s
    Y[:, 0:nb:5] = X[:, 0:nb:5]
    Y[:, nb:2 * nb:5] = X[:, nb:2 * nb:5]
    X[:, 2 * nb:] = 7.0
    Y[:, 2 * nb:] = 7.0
    return X.contiguous(), Y.contiguous()


def stft_left_out(X64, Y64, nbins):
    """Bins [rows][nbins] too close to a gate of the backward for a float32 kernel to be held to
    the float64 decision: the sign of log|Y| - log|X| (bins where Y equals X exactly are not
    close calls: both sides compute the same number, their gradient is exactly 0 and is checked
    as such) and the 1e-7 power floor."""
    px = X64[:, :nbins] ** 2 + X64[:, nbins:2 * nbins] ** 2
    dlog = stft_mags(Y64, nbins).log() - stft_mags(X64, nbins).log()
    same = (Y64[:, :2 * nbins] == X64[:, :2 * nbins])
    same = same[:, :nbins] & same[:, nbins:]
    return ((dlog.abs() < STFT_SIGN_MARGIN) & ~same) | ((px - 1e-7).abs() < STFT_FLOOR_MARGIN)


def sisnr_inputs(L, rows=3, seed=0):
    """Target rows and estimates = gain * target + independent noise, as [rows][L + 5] buffers
    the tests view with a row stride."""
    g = _gen(4000 + seed + L)
    s2 = torch.randn(rows, L + 5, generator=g)
    noise = torch.randn(rows, L + 5, generator=g)
    gain = torch.tensor([1.0, 0.5, 2.0])[:rows, None]
    lvl = torch.tensor([0.3, 1.0, 3.0])[:rows, None]
    return (gain * s2 + lvl * noise).contiguous(), s2.contiguous()


def spkd_inputs(B, seed=0, P=37, Ctot=24, Cs=8):
    """|N(0,1)| + 0.1 features (every Gram entry positive): the student's tensor [B][P][Ctot]
    fp32 (its view: channels [8, 16)), the teacher's [B][P][Cs] bf16."""
    g = _gen(5000 + seed + B)
    zs = torch.randn(B, P, Ctot, generator=g).abs() + 0.1
    zt = (torch.randn(B, P, Cs, generator=g).abs() + 0.1).to(torch.bfloat16)
    return zs.contiguous(), zt.contiguous()
