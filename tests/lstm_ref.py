"""Plain torch reference of the LSTM recurrence (csrc/lstm.hip), its case tables and its tolerances.

Test infrastructure for tests/test_gpu_lstm_edges.py (the kernels against this reference on the
GPU) and tests/test_lstm_ref_cpu.py (this reference against torch.nn.LSTM, and the tolerances it
yields against the project's earlier bounds; no GPU).

``lstm_ref`` is dtype-generic in the style of tests/kernel_refs.py: it computes in the dtype of
its arguments, is called in float64 (the reference) and in float32 (the "same expression in
float32" whose distance to the float64 result scales the tolerance, kernel_refs.tolerance), and
restates no index arithmetic of a kernel.  The activations are written in the forms csrc/common.h
documents (sigm_fast, tanh_fast, tanh_gate); in float64 they are sigmoid and tanh.  In float32 an
optional perturbation multiplies each exp2 result and each reciprocal by 1 + s * 2^-23, s drawn
from {-1, 0, 1}: the "~1 ulp each" common.h states for v_exp_f32 and v_rcp_f32.
"""
import functools
import math

import torch

import kernel_refs

LOG2E = 1.4426950408889634

# The sequence lengths sit on the boundaries of csrc/lstm.hip.  A change of CH, of the history
# ring's depth, of the forward's unroll or of the backward's operand ring must update these lists
# (DESIGN.md §25):
#   - lstm_recurrent_kernel flushes its history every CH = 32 steps and once more, partially, at
#     T - 1: T % 32 in {31, 0, 1};
#   - the history ring holds 2 * CH = 64 rows, h(-1) in row 63 and h(t-1) in row (t + 63) % 64:
#     T = 63, 64, 65 (the ring's first wrap) and 97 (a second full flush after the wrap, then a
#     partial one);
#   - both forward kernels unroll by two and prefetch two steps ahead, clamped at T - 1:
#     T = 1, 2, 3 and both parities;
#   - lstm_bwd_wave_kernel keeps four operand sets (fetch(T-1 .. T-4), early breaks): T < 4 and
#     every residue of T mod 4.
FWD_T = (1, 2, 3, 4, 5, 31, 32, 33, 63, 64, 65, 97)
PRE_T = (1, 2, 3, 4, 5, 33, 64, 65)
BWD_T = (1, 2, 3, 4, 5, 6, 7, 8, 9, 33, 64, 65)
PLANAR_T = 65      # the planar dense layout, once per variant
PRIO_T = 65        # CLSKD_LSTM_PRIO 0 / 1
CELL_STEPS = 70    # lstm_cell carried past the ring depth of the offline kernels
HIDDEN = (16, 32, 64, 128)
NWS, NSEQ = 2, 3
SINGLE = ((32, 65), (128, 65))  # (H, T) of the nws = nseq = 1 runs

# the project's earlier bounds: what the rule's tolerance may not exceed for any case
CEIL_H = 2e-5
CEIL_PRE = 1e-5
CEIL_C = (1e-5, 1e-6)   # rel * max|c| + abs
CEIL_DG = 1e-4          # * max|ref|: the elementwise reading of the relative L2 bound


def all_cases():
    """Every (H, T, nws, nseq) the GPU file runs."""
    out = []
    for H in HIDDEN:
        ts = set(FWD_T) | set(BWD_T) | {PLANAR_T, PRIO_T, CELL_STEPS}
        if H == 32:
            ts |= set(PRE_T)
        out += [(H, T, NWS, NSEQ) for T in sorted(ts)]
    out += [(H, T, 1, 1) for H, T in SINGLE]
    return out


def inputs(H, T, nws=NWS, nseq=NSEQ):
    """fp32 CPU tensors of one case, as in the earlier tests: gx, dh ~ N(0, 1), whh ~ N(0, 1) *
    0.2 sqrt(32 / H); one seed per case."""
    g = torch.Generator().manual_seed(7000 + 1000 * H + 10 * T + 3 * nws + nseq)
    gx = torch.randn(nws, nseq, T, 4 * H, generator=g)
    whh = torch.randn(nws, 4 * H, H, generator=g) * (0.2 * math.sqrt(32 / H))
    dh = torch.randn(nws, nseq, T, H, generator=g)
    return gx, whh, dh


class _Ulp:
    """x -> x * (1 + s * 2^-23), s drawn from {-1, 0, 1} per element (float32 only)."""

    def __init__(self, seed, dtype):
        self.g = None
        if seed is not None and dtype == torch.float32:
            self.g = torch.Generator().manual_seed(seed)

    def __call__(self, x):
        if self.g is None:
            return x
        s = torch.randint(-1, 2, x.shape, generator=self.g).to(x.dtype)
        return x * (1.0 + s * 2.0 ** -23)


def _sigmoid(x, ulp):
    return ulp(1.0 / (1.0 + ulp(torch.exp2(-x * LOG2E))))


def _tanh(x, ulp):
    return 1.0 - 2.0 * ulp(1.0 / (1.0 + ulp(torch.exp2(x * (2.0 * LOG2E)))))


def _tanh_gate(x, ulp):
    return 2.0 * _sigmoid(2.0 * x, ulp) - 1.0


def lstm_ref(gx, whh, dh=None, perturb=None):
    """Zero-state LSTM recurrence, gate order i, f, g, o, in the dtype of gx.
    gx [nws][nseq][T][4H] (gate inputs), whh [nws][4H][H], dh [nws][nseq][T][H].
    Returns dict(h, pre, c) [nws][nseq][T][.] and, given dh, dgx = d sum(h * dh) / d gx (autograd
    with gx as the leaf) — the gate gradients."""
    ulp = _Ulp(perturb, gx.dtype)
    H = whh.shape[2]
    gx = gx.detach().clone().requires_grad_(dh is not None)
    wt = whh.transpose(1, 2)
    h = gx.new_zeros(gx.shape[0], gx.shape[1], H)
    c = gx.new_zeros(gx.shape[0], gx.shape[1], H)
    hs, pres, cs = [], [], []
    for t in range(gx.shape[2]):
        z = gx[:, :, t] + torch.matmul(h, wt)
        i, f, g, o = z.split(H, -1)
        c = _sigmoid(f, ulp) * c + _sigmoid(i, ulp) * _tanh_gate(g, ulp)
        h = _sigmoid(o, ulp) * _tanh(c, ulp)
        hs.append(h)
        pres.append(z)
        cs.append(c)
    hs = torch.stack(hs, 2)
    out = dict(h=hs.detach(), pre=torch.stack(pres, 2).detach(), c=torch.stack(cs, 2).detach())
    if dh is not None:
        (out["dgx"],) = torch.autograd.grad((hs * dh).sum(), gx)
    return out


PERTURB_SEEDS = (None, 11, 23)   # the plain float32 run and two perturbed ones
KEYS = ("h", "pre", "c", "dgx")


@functools.lru_cache(maxsize=None)
def case(H, T, nws=NWS, nseq=NSEQ):
    """One case, computed once and shared (leave it unchanged): the fp32 inputs, the float64
    reference `ref` and, per compared tensor, `tol[key] = (e32, tol)` of the suite's rule with
    factor 8, e32 = the largest distance of the three float32 restatements to float64."""
    gx, whh, dh = inputs(H, T, nws, nseq)
    ref = lstm_ref(gx.double(), whh.double(), dh.double())
    runs = [lstm_ref(gx, whh, dh, perturb=s) for s in PERTURB_SEEDS]
    tol = {}
    for k in KEYS:
        ets = [kernel_refs.tolerance(ref[k], r[k], factor=8.0) for r in runs]
        tol[k] = (max(e for e, _ in ets), max(t for _, t in ets))
    return dict(gx=gx, whh=whh, dh=dh, ref=ref, tol=tol)


def ceilings(ref):
    """The earlier bounds per compared tensor, from the float64 reference alone."""
    return dict(h=CEIL_H, pre=CEIL_PRE, c=CEIL_C[0] * float(ref["c"].abs().max()) + CEIL_C[1],
                dgx=CEIL_DG * float(ref["dgx"].abs().max()))
