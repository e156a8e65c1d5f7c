"""tools_for_loss.py drop-in: l2_norm-based SI-SNR (tools_for_loss.py:22-47) for the CLSKD hot
path, and the supervised menu of DCCRN.loss — sdr, si_sdr (tools_for_loss.py:30-97) and the mel
log-spectral distance get_array_mel_loss (tools_for_loss.py:124-252) — evaluated by the kernels of
csrc/sup_loss.hip.  The PMSQE losses need asteroid's tables and are not provided."""
import math

import numpy as np
import torch

from . import config as cfg
from . import ops


def si_snr(s1, s2, eps=1e-8):
    """Mean over rows of 10*log10(||s_t||^2 / (||e||^2 + eps) + eps), no DC removal
    (tools_for_loss.py:37-47).  Computed by clskd_sisnr_rows + clskd_sum_f32 on the device."""
    rows = ops.sisnr_rows(s1, s2, eps)
    out = torch.empty((), dtype=torch.float32, device=rows.device)
    return ops.sum_f32(rows, out, 1.0 / rows.numel())


def si_snr_rows(s1, s2, eps=1e-8):
    return ops.sisnr_rows(s1, s2, eps)


def _eps_is_default(eps):
    if eps != 1e-8:
        raise NotImplementedError("the supervised loss kernels carry the reference's eps = 1e-8")


def l2_norm(s1, s2):
    """sum(s1 * s2, -1, keepdim=True) (tools_for_loss.py:22-27); for s1 is s2 or s1 - s2 against
    itself callers want sdr / si_snr, which never materialise it."""
    return torch.sum(s1 * s2, -1, keepdim=True)


def sdr(s1, s2, eps=1e-8):
    """mean_b 10 log10(sn^2 / (sn_m_shn^2 + eps)), sn = sum s1^2, sn_m_shn = sum (s1 - s2)^2
    (tools_for_loss.py:30-34: both energies squared once more, as there)."""
    _eps_is_default(eps)
    out, _ = ops.wave_loss(s2, s1, (0, 1, 0, 0, 0), want_coef=False)
    return -out[2]


def si_sdr(reference, estimation, eps=1e-8):
    """10 log10(mean_b(|a r|^2 / |e - a r|^2 + eps) + eps), a = <r, e> / |r|^2 + eps
    (tools_for_loss.py:50-97: eps on the scaling, the ratio averaged before the log)."""
    _eps_is_default(eps)
    out, _ = ops.wave_loss(estimation, reference, (0, 0, 0, 1, 0), want_coef=False)
    return -out[4]


def freqToMel(freq):
    return 1127.01048 * math.log(1 + freq / 700.0)


def melToFreq(mel):
    return 700 * (math.exp(mel / 1127.01048) - 1)


def melFilterBank(numCoeffs, fftSize=None):
    """[numCoeffs][bins] triangular filters with the reference's edge arithmetic
    (tools_for_loss.py:133-177): numCoeffs + 2 mel-spaced points held in float32, mapped to
    floor(bins * hz / nyquist); filter i rises over [edge i-1, edge i) and falls over
    [edge i, edge i+1)."""
    nyquist = cfg.fs / 2
    bins = cfg.win_len if fftSize is None else int(fftSize / 2) + 1
    top, bottom = freqToMel(nyquist), freqToMel(0)
    pts = np.arange(numCoeffs + 2).astype(np.float32) * (top - bottom) / (numCoeffs + 1) + bottom
    for i in range(numCoeffs + 2):
        pts[i] = melToFreq(pts[i])
        pts[i] = math.floor(bins * pts[i] / nyquist)
    edges = [int(p) for p in pts]
    bank = np.zeros((numCoeffs, bins))
    for i in range(1, numCoeffs + 1):
        lo, mid, hi = edges[i - 1], edges[i], edges[i + 1]
        for j in range(lo, mid):
            bank[i - 1, j] = (float(j) - lo) / (mid - lo)
        for j in range(mid, hi):
            bank[i - 1, j] = 1 - ((float(j) - mid) / (hi - mid))
    return bank


def spectrum_pair(real_spec, img_spec):
    """The frame-major [B][T][ld] buffer behind real / imag as DCCRN.forward returns them
    (permuted views of one buffer: re at column f, im at 257 + f); any other pair is copied into
    a fresh [B][T][514] buffer."""
    B, Fq, T = real_spec.shape
    assert Fq == 257 and img_spec.shape == real_spec.shape
    ld = real_spec.stride(0) // T if T else 0
    if (real_spec.dtype == torch.float32 and img_spec.dtype == torch.float32 and ld >= 514
            and real_spec.stride() == (T * ld, 1, ld) and img_spec.stride() == (T * ld, 1, ld)
            and img_spec.data_ptr() - real_spec.data_ptr() == 257 * 4
            and real_spec.storage_offset() + B * T * ld <= real_spec.untyped_storage().nbytes() // 4):
        return torch.as_strided(real_spec, (B, T, ld), (T * ld, ld, 1))
    buf = torch.empty(B, T, 514, dtype=torch.float32, device=real_spec.device)
    buf[:, :, :257] = real_spec.permute(0, 2, 1)
    buf[:, :, 257:] = img_spec.permute(0, 2, 1)
    return buf


def get_array_mel_loss(clean_array, est_array):
    """tools_for_loss.py:245-252 on two *spectra* [B][T][ld >= 514] (frame-major, re at f, im at
    257 + f): DCCRN.loss forms the magnitudes sqrt(re^2 + im^2 + 1e-7) first and the kernel does
    that on load.  Returns a 0-d device tensor."""
    return ops.mel_loss(clean_array, est_array)[1]
