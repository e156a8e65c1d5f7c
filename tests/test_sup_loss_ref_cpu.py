"""CPU checks of the supervised-loss references (tests/sup_loss_ref.py): the restatement against
the fixture the reference itself wrote (tests/golden/gen_sup_loss.py), the filterbanks exactly,
the `view` row mapping, the closed-form gradient coefficients against float64 autograd and finite
differences, the host filter table, and the qualification of the end-to-end inputs: the
reference's own float32 evaluation passes the device gates (loss 5e-5 relative, every parameter
tensor 2e-3 relative L2; tests/test_gpu_supervised.py) on every tensor, mode and model."""
import numpy as np
import pytest
import torch

import kernel_refs as KR
import sup_loss_ref as S

f32, f64 = torch.float32, torch.float64
GRAD_GATE, ZERO_GATE, LOSS_GATE = 2e-3, 1e-3, 5e-5


def _fx():
    fx = S.fixture()
    t = lambda k: torch.from_numpy(fx[k])  # noqa: E731
    return fx, t


@pytest.mark.parametrize("mode", S.MODES)
def test_restatement_matches_the_reference_fixture(mode):
    """Values at 1e-6 relative (float64 restatement vs the reference's float32 value: 1e-6 is
    ~8 float32 ulps of the result); gradients under the suite's rule with e32 = the distance of
    the restatement's own float32 evaluation from its float64 one."""
    fx, t = _fx()
    res = {}
    for dt in (f64, f32):
        a, r, i = [t(k).to(dt).requires_grad_() for k in ("inputs", "real_spec", "img_spec")]
        loss = S.dccrn_loss(mode, a, t("labels").to(dt), r, i, t("clean_real").to(dt), t("clean_imag").to(dt))
        g = torch.autograd.grad(loss, [a, r, i], allow_unused=True)
        res[dt] = (loss.detach(), g)
    ref = float(fx[f"{mode}/loss"])
    assert abs(float(res[f64][0]) - ref) <= 1e-6 * abs(ref), (float(res[f64][0]), ref)
    names = ["d_inputs"] + (["d_real", "d_imag"] if "LMS" in mode else [])
    for k, name in enumerate(names):
        g64, g32 = res[f64][1][k], res[f32][1][k]
        e32, tol = KR.tolerance(g64, g32)
        err = float((t(f"{mode}/{name}").double() - g64).abs().max())
        print(f"SUPREF {mode} {name} e32={e32:.3e} err={err:.3e} tol={tol:.3e}")
        assert err <= tol, (mode, name, err, tol)
    if "LMS" not in mode:
        assert res[f64][1][1] is None and res[f64][1][2] is None


def test_filterbanks_are_the_references_exactly():
    from clskd.tools_for_loss import melFilterBank
    fx, _ = _fx()
    for n in S.SCALES:
        ref = fx[f"bank{n}"]
        assert ref.shape == (n, 257)
        assert np.array_equal(S.mel_filterbank(n), ref)
        assert np.array_equal(melFilterBank(n, 512), ref)
        assert ((ref != 0).sum(0) <= 2).all() and ((ref != 0).sum(1) >= 1).all()


def test_view_rows_are_flat_runs_of_the_frequency_major_array():
    """x.view(-1, 257) of a contiguous [257][T] array: row r, position j is flat element
    257 r + j = (f, t) with f T + t = 257 r + j — not the transpose (frame t, bin j)."""
    T = 19
    x = torch.arange(257 * T, dtype=f64).reshape(257, T)
    rows = x.view(-1, 257)
    assert rows.shape == (T, 257)
    for r, j in ((0, 0), (3, 100), (18, 256)):
        n = 257 * r + j
        assert rows[r, j] == x[n // T, n % T]
    assert not torch.equal(rows, x.t())
    # and the loss depends on it: the transposed reading gives another value
    _, t = _fx()
    cm = S.mags(t("clean_real").double(), t("clean_imag").double())
    em = S.mags(t("real_spec").double(), t("img_spec").double())
    a = S.mel_loss(cm, em)
    b = S.mel_loss(cm.transpose(1, 2).contiguous().transpose(1, 2), em.transpose(1, 2).contiguous().transpose(1, 2))
    assert float(a) == float(b)  # same logical array, any storage: reshape reads logical order
    wrong = S.mel_loss(cm.transpose(1, 2).contiguous(), em.transpose(1, 2).contiguous())
    assert abs(float(wrong) - float(a)) > 1e-3 * float(a)


WEIGHTS = [(1, 0, 0, 0, 0), (0, 1, 0, 0, 0), (0, 0, 1, 0, 0), (0, 0, 0, 1, 0), (0, 0, 0, 0, 1),
           (0.3, 0.1, 0.2, 0.25, 0.15)]


@pytest.mark.parametrize("w", WEIGHTS)
def test_closed_form_coefficients_against_autograd_and_finite_differences(w):
    s, y = [v.double() for v in S.seeded_pair(3, 257, seed=5)]
    up = 0.7
    co = S.coefficients(w, s, y, up)
    g = co[:, 0:1] * s + co[:, 1:2] * y
    ga = S.wave_grad_autograd(w, s, y, up)
    assert float((g - ga).abs().max()) <= 1e-11 * float(ga.abs().max())
    f = lambda v: up * S.weighted(w, v, y)  # noqa: E731
    for idx in ((0, 0), (1, 100), (2, 256)):
        sp, sm = s.clone(), s.clone()
        sp[idx] += 1e-6
        sm[idx] -= 1e-6
        fd = float((f(sp) - f(sm)) / 2e-6)
        assert abs(fd - float(g[idx])) <= 1e-6 * max(1.0, float(ga.abs().max())), (idx, fd, float(g[idx]))


def test_components_are_the_modes_mixes():
    """out[1..5] of the kernel and the mode table reproduce every waveform mode."""
    from clskd.supervised import LOSS_MODES
    s, y = [v.double() for v in S.seeded_pair(2, 400, seed=6)]
    for mode in S.WAVE_MODES:
        w, wm = LOSS_MODES[mode]
        assert wm == 0.0
        a, b = float(S.weighted(w, s, y)), float(S.dccrn_loss(mode, s, y))
        assert abs(a - b) <= 1e-12 * abs(b), mode
    assert sorted(LOSS_MODES) == sorted(S.MODES)


def test_host_filter_table_restates_the_banks():
    from clskd import ops
    fx, _ = _fx()
    tab = ops.mel_table_host([fx[f"bank{n}"] for n in S.SCALES])
    assert tab.dtype == np.int32 and tab.size == ops.MEL_TABLE_WORDS
    W = tab[:112 * 257].view(np.float32).reshape(112, 257)
    supp = tab[112 * 257:112 * 257 + 224].reshape(112, 2)
    pk = tab[112 * 257 + 224:112 * 257 + 224 + 1542].reshape(257, 6)
    pw = tab[112 * 257 + 224 + 1542:].view(np.float32).reshape(257, 6)
    full = np.concatenate([fx[f"bank{n}"] for n in S.SCALES], 0).astype(np.float32)
    assert np.array_equal(W, full)
    dense = np.zeros_like(full)
    for j in range(257):
        for i in range(6):
            if pw[j, i] != 0:
                dense[pk[j, i], j] += pw[j, i]
    assert np.array_equal(dense, full)
    for k in range(112):
        assert (full[k, :supp[k, 0]] == 0).all() and (full[k, supp[k, 1]:] == 0).all()
        assert 0 <= supp[k, 0] < supp[k, 1] <= 257
    assert pk.min() >= 0 and pk.max() < 112


# ------------------------------------------------------------------------------------------
# the end-to-end inputs qualify: float32 autograd of the reference passes the device gates
# ------------------------------------------------------------------------------------------
# Seed 7 of seeds 1..8: the one whose float32 reference evaluation has the widest margin under the
# 2e-3 gate on both models (1.4e-4 student DCCRN, 4.6e-4 DCCRNet_mini; seeds 1, 3 and 5 miss it on a
# one-element PReLU slope, whose gradient nearly cancels under the scale-invariant losses).  The
# choice rests on the reference alone.  tests/test_gpu_supervised.py uses the same.
E2E = dict(B=2, L=1600, seed=7)


def _qualify(tag, r64, r32):
    for mode in r64:
        l64, l32 = float(r64[mode]["loss"]), float(r32[mode]["loss"])
        dl = abs(l32 - l64) / abs(l64)
        errs = S.grad_errors(r32[mode]["grads"], r64[mode]["grads"])
        worst = max(((n, e) for n, (e, kind) in errs.items() if kind == "rel"), key=lambda v: v[1])
        wz = max([e for e, kind in errs.values() if kind == "zero"], default=0.0)
        print(f"SUPQUAL {tag} {mode:14s} loss={l64:.6f} dloss={dl:.2e} worst={worst[0]} {worst[1]:.2e} zero={wz:.2e}")
        for n, g in r64[mode]["grads"].items():
            assert g is not None and torch.isfinite(g).all(), (mode, n)
        assert dl <= LOSS_GATE, (mode, dl)
        assert worst[1] <= GRAD_GATE, (mode, worst)
        assert wz <= ZERO_GATE, (mode, wz)
        # SI-SDR of the estimate inside [-35, +20] dB: the one-pass noise energy keeps its digits
        sd = -float(S.dccrn_loss("SI-SDR", r64[mode]["wav"], S.seeded_batch(**E2E)[1].double()))
        assert -35.0 <= sd <= 20.0, sd
        assert float(r64[mode]["wav"].abs().max()) < 1.0  # inside the clamp


def test_student_dccrn_inputs_qualify():
    x, y = S.seeded_batch(**E2E)
    modes = S.MODES + ("MRSTFT",)
    r64, r32 = S.dccrn_steps(modes, x, y, f64), S.dccrn_steps(modes, x, y, f32)
    assert len(r64["MSE"]["grads"]) == len(r32["MSE"]["grads"]) > 50
    _qualify("dccrn", r64, r32)


def test_mini_inputs_qualify():
    x, y = S.seeded_batch(**E2E)
    modes = S.WAVE_MODES + ("MRSTFT",)
    r64, r32 = S.mini_steps(modes, x, y, f64), S.mini_steps(modes, x, y, f32)
    assert len(r64["MSE"]["grads"]) == 112
    _qualify("mini", r64, r32)
