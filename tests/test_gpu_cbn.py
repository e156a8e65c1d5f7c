"""GPU: clskd.DCCRN(use_cbn=True) end to end.

Forward against what the reference's own DCCRN(use_cbn=True) computed (tests/golden/cbn.npz) under
the forward gate tests/test_gpu_parity.py holds the BatchNorm model to (rms 1e-5, max 1e-4), the
running buffers after the train forward against the float64 restatement (tests/cbn_ref.py).
SupervisedTraining gradients for the nine DCCRN.loss modes against float64 autograd of the
restatement under the gates of tests/test_gpu_supervised.py: loss 5e-5 relative, every parameter
tensor 2e-3 relative L2, the analytically-zero pre-normalisation conv biases 1e-3 of |dW|.
'MRSTFT' does not qualify on these inputs (tests/test_cbn_ref_cpu.py: the float32 reference alone
is at 4.7e-3 on encoder.4.2.weight), so its loss is checked and its gradients are printed only.
Each case prints its per-tensor table (`CBNGRAD` lines); profiles/cbn_grad_parity.txt keeps one
run's tables."""
import numpy as np
import pytest
import torch

import cbn_ref as CR
import sup_loss_ref as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GRAD_GATE, ZERO_GATE, LOSS_GATE = 2e-3, 1e-3, 5e-5


def _model(use_cbn=True, train=True):
    from clskd import config as cfg
    from clskd.model import DCCRN
    from clskd.weights import STUDENT_SEED, apply_recipe
    m = apply_recipe(DCCRN(masking_mode="E", use_clstm=True, use_cbn=use_cbn, **cfg.STUDENT),
                     STUDENT_SEED).to(DEV)
    return m.train(train)


def _batch():
    x, y = S.seeded_batch(**CR.E2E)
    return x.to(DEV), y.to(DEV)


@pytest.mark.parametrize("mode", ["train", "eval"])
def test_forward_matches_the_reference_fixture(mode):
    from clskd.feature_extraction import DCCRN as Taps
    fx = CR.fixture()
    m = _model(train=mode == "train")
    X, _ = _batch()
    with torch.no_grad():
        outs = m(X)
        wav = outs[-1].cpu().numpy()
    ref = fx[f"model/out_wav_{mode}"]
    d = wav.astype(np.float64) - ref
    print(f"CBNFWD {mode} rms {np.sqrt(np.mean(d * d)):.2e} max {np.abs(d).max():.2e}")
    assert np.sqrt(np.mean(d * d)) <= 1e-5
    np.testing.assert_allclose(wav, ref, atol=1e-4)
    # the running buffers: lerped once in train mode, untouched in eval mode
    with S.oracle_dtype(torch.float64):
        ps = CR.cbn_params(torch.float64, grad=False)
        with torch.no_grad():
            fw = CR.dccrn_forward_cbn(ps, X.cpu().double(), train=mode == "train",
                                      update_stats=mode == "train")
    sd = m.state_dict()
    for k, v in ps.items():
        leaf = k.rsplit(".", 1)[-1]
        if leaf in CR.CBN_BUFFERS:
            e = float((sd[k].double().cpu() - v).norm() / v.norm())
            assert e <= 1e-5, (k, e)
        elif leaf == "num_batches_tracked":
            assert int(sd[k]) == (1 if mode == "train" else 0), k
    # feature_extraction taps of a CBN model, under the tap tolerances of tests/test_gpu_parity.py
    if mode == "eval":
        fe = Taps(m)
        with torch.no_grad():
            maps = fe.extract_feature_maps(X)
        fe.remove_hook()
        assert len(maps["encoder"]) == 6 and len(maps["decoder"]) == 6
        for got, want in zip(maps["encoder"] + maps["decoder"], fw["enc"] + fw["dec"]):
            np.testing.assert_allclose(got.cpu().numpy(), want.numpy(), rtol=2e-4, atol=2e-5)


def _grad_case(mode):
    from clskd.supervised import SupervisedTraining
    X, Y = _batch()
    ref = CR.e2e_reference()[mode]
    mod = SupervisedTraining(_model(), mode)
    out = mod.forward_with_tape(X, Y)
    grads = {p: torch.full_like(p, 7.0) for p in mod.student.parameters()}
    mod.backward_into(out, grads)
    torch.cuda.synchronize()
    names = dict(mod.student.named_parameters())
    assert sorted(names) == sorted(ref["grads"])
    errs = S.grad_errors({n: grads[p].cpu() for n, p in names.items()}, ref["grads"])
    assert sorted(errs) == sorted(names)
    gated = mode in CR.GRAD_MODES
    rows, bad = [], []
    for n, (e, k) in errs.items():
        rows.append(f"CBNGRAD {mode} {n:55s} {e:.2e}"
                    + (" (|g| / |dW|, analytically 0)" if k == "zero" else ""))
        if gated and not e <= (ZERO_GATE if k == "zero" else GRAD_GATE):
            bad.append((n, e))
    l, lr = out["loss"].item(), float(ref["loss"])
    dl = abs(l - lr) / abs(lr)
    worst = max(e for e, k in errs.values() if k == "rel")
    rows.append(f"CBNGRAD {mode} loss hip={l:.7f} ref={lr:.7f} rel={dl:.2e} worst={worst:.2e}"
                + ("" if gated else " (gradients not gated: inputs do not qualify)"))
    print("\n".join(rows))
    assert np.isfinite(l)
    assert dl <= LOSS_GATE, (mode, l, lr, dl)
    assert not bad, bad


@pytest.mark.parametrize("mode", CR.ALL_MODES)
def test_supervised_gradients_against_fp64_reference(mode):
    """The student DCCRN(use_cbn=True) (recipe weights), B = 2, L = 1600 (T = 19)."""
    _grad_case(mode)


def test_autograd_dropin_and_train_step():
    """loss.backward() through training_step gives backward_into's bits; two train_steps equal two
    manual (taped forward, backward_into, FlatAdam.step) steps bitwise; validation_step runs the
    eval-mode ComplexBatchNorm and leaves the model in train mode."""
    from clskd import config as cfg
    from clskd.supervised import SupervisedTraining
    from clskd.train import FlatAdam, FlatParams
    mode = "SI-SNR+LMS"
    X, Y = _batch()
    mod = SupervisedTraining(_model(), mode)
    loss = mod.training_step((X, Y), 0)
    assert loss.requires_grad
    loss.backward()
    # (a second forward of the same module has moved its running buffers, not its batch statistics)
    out = mod.forward_with_tape(X, Y)
    assert torch.equal(out["loss"], loss.detach())
    g1 = {p: torch.empty_like(p) for p in mod.student.parameters()}
    mod.backward_into(out, g1)
    for n, p in mod.student.named_parameters():
        assert torch.equal(p.grad, g1[p]), n
    a, b = SupervisedTraining(_model(), mode), SupervisedTraining(_model(), mode)
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
    sa, sb = a.student.state_dict(), b.student.state_dict()
    assert all(torch.equal(sa[k], sb[k]) for k in sa)
    assert int(sa["encoder.0.1.num_batches_tracked"]) == 2
    xv, yv = S.seeded_batch(2, 16000, seed=5)  # STOI needs more than 0.1 s
    val = a.validation_step((xv.to(DEV), yv.to(DEV)))
    assert set(val) == {"si_sdr", "si_sdr_imp", "stoi", "stoi_imp"}
    assert a.student.training and int(a.student.state_dict()["encoder.0.1.num_batches_tracked"]) == 2
    # DCCRN.loss on a CBN model's outputs
    a.student.eval()
    with torch.no_grad():
        _, _, re, im, wav = a.student(X)
        v = a.student.loss(wav, Y, re, im, loss_mode="SI-SNR+LMS")
    assert np.isfinite(v.item())


def test_unsupported_consumers_raise():
    from clskd.distill import KnowledgeDistillation, SPKDDistillation
    from clskd.distill_mini import OutputDistillation
    from clskd.graph import StepGraph
    from clskd.streaming import StreamingDCCRN
    cbn, bn = _model(), _model(use_cbn=False)
    X, Y = _batch()

    def refused(fn):
        with pytest.raises(NotImplementedError, match="use_cbn"):
            fn()

    for cls in (KnowledgeDistillation, SPKDDistillation):
        refused(lambda: cls(bn, cbn))
        refused(lambda: cls(cbn, bn))
    refused(lambda: OutputDistillation(cbn, bn))
    refused(lambda: StreamingDCCRN(_model(train=False), 1))
    refused(lambda: cbn.run(X, train=True, gram_taps=[]))
    kd = KnowledgeDistillation(_teacher(), bn, abf_reinit="once").to(DEV)
    kd.student = cbn  # a step object whose student was swapped afterwards
    refused(lambda: StepGraph(kd, X, Y))
    cbn.compute = "bf16"
    refused(lambda: cbn.run(X, train=False))


def _teacher():
    from clskd import config as cfg
    from clskd.model import DCCRN
    return DCCRN(masking_mode="E", use_clstm=True, **cfg.TEACHER)
