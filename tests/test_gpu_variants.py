"""GPU: clskd.DCCRN with masking_mode 'C' / 'R' and with the real-LSTM bottleneck
(use_clstm=False), end to end at B = 2 x 1600 samples (T = 19).

Forward against what the reference's own models computed (tests/golden/variants_*.npz) under the
gates tests/test_gpu_cbn.py holds its out_wav records to (rms 1e-5, max 1e-4, absolute), on all
five returned tensors, train and eval mode; one use_cbn=True case per new option and a forward with
rnn_units=128 against the float64 restatement (tests/variants_ref.py) evaluated here on the CPU.
SupervisedTraining gradients against float64 autograd of the restatement under the gates of
tests/test_gpu_supervised.py, unchanged: loss 5e-5 relative, every parameter tensor 2e-3 relative
L2, the analytically-zero pre-normalisation conv biases 1e-3 of |dW|; no tensor is left out.  Each
variant runs at the seed tests/test_variants_ref_cpu.py qualifies for it.  Each case prints its
per-tensor table (`VARGRAD` lines).  StreamingDCCRN with mask 'R' against the offline eval
forward at the tolerance of tests/test_gpu_streaming.py (max 1e-4, rms 1e-5)."""
import numpy as np
import pytest
import torch

import sup_loss_ref as S
import variants_ref as V

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GRAD_GATE, ZERO_GATE, LOSS_GATE = 2e-3, 1e-3, 5e-5


def _model(variant, train=True, use_cbn=False, **kw):
    from clskd import config as cfg
    from clskd.model import DCCRN
    from clskd.weights import STUDENT_SEED, apply_recipe
    m = apply_recipe(DCCRN(masking_mode=variant[0], use_clstm=variant[1], use_cbn=use_cbn,
                           **{**cfg.STUDENT, **kw}), STUDENT_SEED).to(DEV)
    return m.train(train)


def _batch(variant):
    x, y = S.seeded_batch(**V.e2e(variant))
    return x.to(DEV), y.to(DEV)


def _held(tagline, got, ref):
    ref = np.asarray(ref, np.float64)
    d = got.double().cpu().numpy() - ref
    rms, mx = float(np.sqrt(np.mean(d * d))), float(np.abs(d).max())
    print(f"VARFWD {tagline} rms {rms:.2e} max {mx:.2e} (peak {np.abs(ref).max():.2f})")
    assert rms <= 1e-5 and mx <= 1e-4, (tagline, rms, mx)


@pytest.mark.parametrize("mode", ["train", "eval"])
@pytest.mark.parametrize("variant", V.FIXTURE_VARIANTS, ids=V.tag)
def test_forward_matches_the_reference_fixture(variant, mode):
    fx = V.fixture(variant)
    m = _model(variant, train=mode == "train")
    with torch.no_grad():
        outs = m(_batch(variant)[0])
    for k, got in zip(V.OUTPUTS, outs):
        assert tuple(got.shape) == fx[f"{mode}/{k}"].shape, k
        _held(f"{V.tag(variant)} {mode} {k}", got, fx[f"{mode}/{k}"])


@pytest.mark.parametrize("variant,kw", [(("R", True), {}), (("C", False), {}), (("E", False), {}),
                                        (("C", False), dict(rnn_units=128))],
                         ids=["Rc-cbn", "Cr-cbn", "Er-cbn", "Cr-H128"])
def test_forward_matches_the_fp64_restatement(variant, kw):
    """One use_cbn=True case per new option (train mode: batch statistics and running buffers) and
    the real LSTM at H = 128, against the float64 restatement evaluated on the CPU."""
    use_cbn = not kw
    m = _model(variant, use_cbn=use_cbn, **kw)
    X, _ = _batch(variant)
    with torch.no_grad():
        outs = m(X)
    with S.oracle_dtype(torch.float64) as R, torch.no_grad():
        ps = V.params(torch.float64, variant[1], use_cbn, grad=False, **kw)
        fw = V.dccrn_forward(ps, X.cpu().double(), *variant, train=True, update_stats=True,
                             lstm_fn=R.lstm, use_cbn=use_cbn)
    assert float(fw["pre_clamp"].abs().max()) < 0.99
    for k, got in zip(V.OUTPUTS, outs):
        _held(f"{V.tag(variant)} {'cbn' if use_cbn else kw} {k}", got, fw[k].numpy())
    if use_cbn:  # the running buffers moved once
        sd = m.state_dict()
        for k in ("encoder.0.1.RMr", "decoder.4.1.RVri"):
            assert V.rel(sd[k], ps[k]) <= 1e-5, k


def _grad_case(variant, mode):
    from clskd.supervised import SupervisedTraining
    X, Y = _batch(variant)
    ref = V.e2e_reference(variant)[mode]
    mod = SupervisedTraining(_model(variant), mode)
    out = mod.forward_with_tape(X, Y)
    grads = {p: torch.full_like(p, 7.0) for p in mod.student.parameters()}
    mod.backward_into(out, grads)
    torch.cuda.synchronize()
    names = dict(mod.student.named_parameters())
    assert sorted(names) == sorted(ref["grads"])
    errs = S.grad_errors({n: grads[p].cpu() for n, p in names.items()}, ref["grads"])
    assert sorted(errs) == sorted(names)  # no tensor is left out
    rows, bad = [], []
    for n, (e, k) in errs.items():
        rows.append(f"VARGRAD {V.tag(variant)} {mode} {n:45s} {e:.2e}"
                    + (" (|g| / |dW|, analytically 0)" if k == "zero" else ""))
        if not e <= (ZERO_GATE if k == "zero" else GRAD_GATE):
            bad.append((n, e))
    l, lr = out["loss"].item(), float(ref["loss"])
    dl = abs(l - lr) / abs(lr)
    worst = max(e for e, k in errs.values() if k == "rel")
    rows.append(f"VARGRAD {V.tag(variant)} {mode} loss hip={l:.7f} ref={lr:.7f} rel={dl:.2e} "
                f"worst={worst:.2e}")
    print("\n".join(rows))
    assert np.isfinite(l)
    assert dl <= LOSS_GATE, (variant, mode, l, lr, dl)
    assert not bad, bad


@pytest.mark.parametrize("variant,mode", [(v, lm) for v in V.VARIANTS for lm in V.STEP_MODES[v]],
                         ids=lambda v: V.tag(v) if isinstance(v, tuple) else v)
def test_supervised_gradients_against_fp64_reference(variant, mode):
    """The LMS cases drive g['est_spec'] into the new mask backward."""
    _grad_case(variant, mode)


@pytest.mark.parametrize("variant", [("R", True), ("C", False)], ids=V.tag)
def test_autograd_dropin_train_step_and_validation(variant):
    """loss.backward() through training_step gives backward_into's bits; two train_steps equal two
    manual (taped forward, backward_into, FlatAdam.step) steps bitwise and move every new
    parameter; validation_step runs; DCCRN.loss takes the model's own real / imag."""
    from clskd import config as cfg
    from clskd.supervised import SupervisedTraining
    from clskd.train import FlatAdam, FlatParams
    mode = "SI-SNR+LMS"
    X, Y = _batch(variant)
    mod = SupervisedTraining(_model(variant), mode)
    loss = mod.training_step((X, Y), 0)
    assert loss.requires_grad
    loss.backward()
    out = mod.forward_with_tape(X, Y)
    assert torch.equal(out["loss"], loss.detach())
    g1 = {p: torch.empty_like(p) for p in mod.student.parameters()}
    mod.backward_into(out, g1)
    for n, p in mod.student.named_parameters():
        assert torch.equal(p.grad, g1[p]), n
    a, b = SupervisedTraining(_model(variant), mode), SupervisedTraining(_model(variant), mode)
    before = {k: v.clone() for k, v in a.student.state_dict().items()}
    fa, fb = FlatParams(a.student), FlatParams(b.student)
    oa, ob = FlatAdam(fa, lr=cfg.learning_rate), FlatAdam(fb, lr=cfg.learning_rate)
    la, lb = [], []
    for _ in range(2):
        la.append(a.train_step((X, Y), fa, oa).clone())
        o = b.forward_with_tape(X, Y)
        b.backward_into(o, fb.grad_dict())
        ob.step()
        lb.append(o["loss"].clone())
    torch.cuda.synchronize()
    assert torch.equal(fa.data, fb.data) and torch.equal(fa.grad, fb.grad)
    assert torch.equal(la[0], lb[0]) and torch.equal(la[1], lb[1])
    assert torch.equal(la[0], out["loss"]) and la[1].item() != la[0].item()
    sa = a.student.state_dict()
    if not variant[1]:
        for k in V.REAL_LSTM_KEYS:
            assert not torch.equal(sa[k], before[k]), k
    xv, yv = S.seeded_batch(2, 16000, seed=5)  # STOI needs more than 0.1 s
    val = a.validation_step((xv.to(DEV), yv.to(DEV)))
    assert set(val) == {"si_sdr", "si_sdr_imp", "stoi", "stoi_imp"} and a.student.training
    a.student.eval()
    with torch.no_grad():
        _, _, re, im, wav = a.student(X)
        for lm in S.MODES:
            assert np.isfinite(a.student.loss(wav, Y, re, im, loss_mode=lm).item()), lm


@pytest.mark.parametrize("mask", ["R"])  # mask 'C' runs only on the real LSTM, which does not stream
def test_per_layer_streaming_equals_the_offline_eval_forward(mask):
    from clskd.streaming import StreamingDCCRN
    variant = (mask, True)
    x, _ = S.seeded_batch(2, 3200, seed=11)
    x = x.to(DEV)
    m = _model(variant)
    with torch.no_grad():
        m(x)  # one train-mode pass: non-trivial running statistics
        m.eval()
        ref = m(x)[-1]
    out = StreamingDCCRN(m, 2, graph=True).process(x)
    torch.cuda.synchronize()
    assert out.shape == ref.shape == (2, 3200)
    _held(f"stream mask {mask}", out, ref.double().cpu().numpy())
