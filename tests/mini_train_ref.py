"""CPU references of the asteroid DCCRNet_mini training step (test infrastructure).

The step reference is autograd through ``oracle.asteroid_cpu.forward`` (plain differentiable
torch) on a copy of the fixture checkpoint's state dict, with the three output-level KD losses of
the reference's scripts written with ``oracle.ref_cpu``'s MRSTFT / SPKD functions:

  base = mrstft log-magnitude(student, clean)            (fft 512 / win 400 / hop 100)
  kd   = spkd_loss(student, teacher, 'batchmean')        distill_SPKD.py:69-87
       | F.mse_loss(student, teacher)                    distill_MSE.py:70-90
       | mrstft log-magnitude(student, teacher)          distill_STFT.py:67-84

and closed forms of the three kernels of csrc/mini_bwd.hip through autograd of the oracle's own
expressions.  Every function computes in the dtype of its tensor arguments; none restates a
kernel's index arithmetic.
"""
import os

import numpy as np
import torch
import torch.nn.functional as F

from oracle import asteroid_cpu as A
from oracle import ref_cpu as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NOT_TRAINED = ("running_mean", "running_var", "num_batches_tracked", "_filters", "torch_window")
KD_KINDS = ("spkd", "mse", "stft")


def fixture():
    return np.load(os.path.join(GOLDEN, "asteroid_mini.npz"))


def trainable_state(dtype=torch.float64):
    """The fixture's state dict in `dtype`, requires_grad on every float entry that is a
    parameter (not a running statistic, not a filterbank buffer)."""
    sd = {}
    for k, v in A.state_dict_from_fixture(fixture()).items():
        if v.is_floating_point():
            v = v.to(dtype).clone()
            if not k.endswith(NOT_TRAINED):
                v.requires_grad_()
        sd[k] = v
    return sd


def trainable_keys(sd):
    return [k for k, v in sd.items() if v.requires_grad]


def seeded_batch(B, L, seed=0, peak=0.3):
    """(mixture, clean, teacher waveform) [B, L] float32: three independent seeded Gaussian
    noises, the mixture at a peak of 0.3 (the fixture mixtures' range), the clean target at
    0.8 and the teacher's waveform at 0.7 of it.

    Broadband targets on purpose.  The losses are L1 of log magnitudes floored at 1e-7, whose
    gradient per bin is sign / |X|: a target made of a few pure tones (clskd.data.synthetic_pairs)
    leaves 40 % of its bins on the floor, the gradients of the one-element tensors (PReLU slopes,
    output biases) then nearly cancel, and a float32 evaluation of this very reference on the
    CPU misses the 2e-3 gradient gate on them (3.0e-3) — a gate no float32 step can be held to.
    With noise every bin is filled and the reference's own float32 evaluation passes the gate on
    all 112 tensors (tests/test_mini_train_ref_cpu.py asserts it), so the gate measures the
    device step and not the conditioning of the inputs.  The choice rests on the reference
    alone, never on a device result."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, L, generator=g)
    x = x * (peak / x.abs().max())
    y = torch.randn(B, L, generator=g)
    y = y * (0.8 * peak / y.abs().max())
    t = torch.randn(B, L, generator=g)
    t = t * (0.7 * peak / t.abs().max())
    return x.float(), y.float(), t.float()


def mrstft_mag(x, y):
    """stft_loss(x, y)[1] of the distillation scripts: 0.1 * L1 of the log magnitudes."""
    w = torch.hann_window(400, dtype=x.dtype)
    xm = R.stft_mag(x, 512, 100, 400, w)
    ym = R.stft_mag(y, 512, 100, 400, w)
    return 0.1 * F.l1_loss(torch.log(ym), torch.log(xm))


def kd_loss(kd, s, t):
    if kd == "spkd":
        return R.spkd_loss(s, t, "batchmean")
    if kd == "mse":
        return F.mse_loss(s, t)
    if kd == "stft":
        return mrstft_mag(s, t)
    raise ValueError(kd)


def reference_step(kd, x, y, t, dtype=torch.float64):
    """One step in `dtype`: dict(loss, base, kd, wav, grads {state-dict key: gradient})."""
    sd = trainable_state(dtype)
    x, y, t = x.to(dtype), y.to(dtype), t.to(dtype)
    wav = A.forward(sd, x, train=True)
    base = mrstft_mag(wav, y)
    k = kd_loss(kd, wav, t)
    loss = base + k
    keys = trainable_keys(sd)
    grads = torch.autograd.grad(loss, [sd[n] for n in keys])
    return dict(loss=loss.detach(), base=base.detach(), kd=k.detach(), wav=wav.detach(),
                grads=dict(zip(keys, grads)), sd=sd)


# ------------------------------------------------------------------------------------------
# closed forms of the kernels
# ------------------------------------------------------------------------------------------
def bound_mask_apply(mr, mi, sr, si):
    """oracle/asteroid_cpu.py:127-131: BoundComplexMask('tanh') then mask * spectrum."""
    mag = torch.tanh(torch.sqrt(mr ** 2 + mi ** 2))
    ph = torch.atan2(mi, mr)
    br, bi = mag * torch.cos(ph), mag * torch.sin(ph)
    return br * sr - bi * si, br * si + bi * sr


def mask_bdt_bwd(spec, mask, T, dest):
    """d sum(est * dest) / d mask for spec [B][T][>=514] (re at f, im at 257 + f), mask
    [B][256][Tm][2] read at t < T, dest [B][T][>=514].  Elements with |M| = 0 get
    g = conj(X) dest, the limit of the Jacobian (autograd gives NaN there)."""
    m = mask.detach().clone().requires_grad_()
    mr, mi = m[:, :, :T, 0], m[:, :, :T, 1]
    sr, si = spec[:, :, 0:256].transpose(1, 2), spec[:, :, 257:513].transpose(1, 2)
    dre, dim = dest[:, :, 0:256].transpose(1, 2), dest[:, :, 257:513].transpose(1, 2)
    er, ei = bound_mask_apply(mr, mi, sr, si)
    (dm,) = torch.autograd.grad((er * dre).sum() + (ei * dim).sum(), m)
    zero = (mask[:, :, :T, 0] == 0) & (mask[:, :, :T, 1] == 0)
    g = torch.stack([sr * dre + si * dim, sr * dim - si * dre], -1)
    dm = dm.clone()
    dm[:, :, :T][zero] = g[zero]
    return dm


def bn_reim_forward(x, gamma, beta, alpha, eps=1e-5):
    """OnReIm(BatchNorm2d, train) + OnReIm(PReLU) over BFTC rows x [rows][C]: the re module on
    channels [0, C/2), the im module on [C/2, C).  Returns (y, y_bn)."""
    h = x.shape[1] // 2
    ys, yb = [], []
    for k, sl in enumerate((slice(0, h), slice(h, 2 * h))):
        b = F.batch_norm(x[:, sl], None, None, gamma[sl], beta[sl], True, 0.1, eps)
        yb.append(b)
        ys.append(F.prelu(b, alpha[k:k + 1]))
    return torch.cat(ys, 1), torch.cat(yb, 1)


def bn_reim_bwd(x, dy, gamma, beta, alpha, eps=1e-5):
    """(dx, dgamma, dbeta, dalpha [2], y_bn) of sum(y * dy)."""
    xs, g, b, a = [t.detach().clone().requires_grad_() for t in (x, gamma, beta, alpha)]
    y, yb = bn_reim_forward(xs, g, b, a, eps)
    dx, dg, db, da = torch.autograd.grad((y * dy).sum(), [xs, g, b, a])
    return dx, dg, db, da, yb.detach()


def bn_coefficients(x, gamma, beta, eps=1e-5):
    """(scale, shift, mean, biased var) per channel, as the forward's finalize hands them on."""
    mean = x.mean(0)
    var = x.var(0, unbiased=False)
    scale = gamma * torch.rsqrt(var + eps)
    return scale, beta - mean * scale, mean, var


def mse_loss_grad(a, b, scale=1.0):
    """(scale * F.mse_loss(a, b), its gradient w.r.t. a)."""
    aa = a.detach().clone().requires_grad_()
    loss = scale * F.mse_loss(aa, b)
    (da,) = torch.autograd.grad(loss, aa)
    return loss.detach(), da
