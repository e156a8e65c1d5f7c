"""GPU: clskd.supervised.SupervisedTraining end to end against float64 autograd of the restatement
(tests/sup_loss_ref.py) through the CPU oracles (oracle.ref_cpu.dccrn_forward for the student
DCCRN, oracle.asteroid_cpu.forward for the fixture DCCRNet_mini).

Gates — the project's existing ones (tests/test_gpu_backward.py, tests/test_gpu_mini_backward.py):
the loss within 5e-5 relative, every parameter tensor within 2e-3 relative L2; the conv biases in
front of a train-mode BatchNorm have an analytically zero gradient and are held, as
tests/test_gpu_backward.py:_compare holds them, to |g| <= 1e-3 |dW| of their layer.  The inputs are
qualified on the CPU (tests/test_sup_loss_ref_cpu.py: the reference's own float32 evaluation
passes both gates on every tensor).  Each case prints its per-tensor table (`SUPGRAD` lines);
profiles/sup_train_grad_parity.txt keeps one run's tables."""
import functools

import numpy as np
import pytest
import torch

import sup_loss_ref as S
from conftest import golden

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GRAD_GATE, ZERO_GATE, LOSS_GATE = 2e-3, 1e-3, 5e-5
E2E = dict(B=2, L=1600, seed=7)  # tests/test_sup_loss_ref_cpu.py qualifies these inputs
DCCRN_MODES = S.MODES + ("MRSTFT",)
MINI_MODES = S.WAVE_MODES + ("MRSTFT",)


def _dccrn():
    from clskd import config as cfg
    from clskd.model import DCCRN
    from clskd.weights import STUDENT_SEED, apply_recipe
    return apply_recipe(DCCRN(masking_mode="E", use_clstm=True, **cfg.STUDENT), STUDENT_SEED).to(DEV).train()


def _mini():
    from clskd.asteroid import DCCRNet_mini, load_conf
    return DCCRNet_mini.from_pretrained(load_conf(golden("asteroid_mini.npz"))).to(DEV).train()


@functools.lru_cache(maxsize=None)
def _reference(kind):
    """One float64 forward per model, every mode's loss and gradients from it; shared, read only."""
    x, y = S.seeded_batch(**E2E)
    return (S.dccrn_steps(DCCRN_MODES, x, y) if kind == "dccrn" else S.mini_steps(MINI_MODES, x, y))


def _grad_case(kind, mode):
    from clskd.supervised import SupervisedTraining
    x, y = S.seeded_batch(**E2E)
    ref = _reference(kind)[mode]
    mod = SupervisedTraining(_dccrn() if kind == "dccrn" else _mini(), mode)
    out = mod.forward_with_tape(x.to(DEV), y.to(DEV))
    grads = {p: torch.full_like(p, 7.0) for p in mod.student.parameters()}
    mod.backward_into(out, grads)
    torch.cuda.synchronize()
    names = dict(mod.student.named_parameters())
    assert sorted(names) == sorted(ref["grads"])
    errs = S.grad_errors({n: grads[p].cpu() for n, p in names.items()}, ref["grads"])
    assert sorted(errs) == sorted(names)
    rows, bad = [], []
    for n, (e, k) in errs.items():
        rows.append(f"SUPGRAD {kind} {mode} {n:55s} {e:.2e}" + (" (|g| / |dW|, analytically 0)" if k == "zero" else ""))
        if not e <= (ZERO_GATE if k == "zero" else GRAD_GATE):
            bad.append((n, e))
    l, lr = out["loss"].item(), float(ref["loss"])
    dl = abs(l - lr) / abs(lr)
    worst = max(e for e, k in errs.values() if k == "rel")
    rows.append(f"SUPGRAD {kind} {mode} loss hip={l:.7f} ref={lr:.7f} rel={dl:.2e} worst={worst:.2e}")
    print("\n".join(rows))
    assert np.isfinite(l)
    assert dl <= LOSS_GATE, (mode, l, lr, dl)
    assert not bad, bad


@pytest.mark.parametrize("mode", DCCRN_MODES)
def test_student_dccrn_gradients_against_fp64_reference(mode):
    """The student DCCRN (recipe weights), B = 2, L = 1600 (T = 19): every DCCRN.loss mode — the
    three LMS ones through g['est_spec'] — and 'MRSTFT'."""
    _grad_case("dccrn", mode)


@pytest.mark.parametrize("mode", MINI_MODES)
def test_mini_gradients_against_fp64_reference(mode):
    """The fixture DCCRNet_mini, same inputs: the waveform modes and 'MRSTFT', all 112 tensors."""
    _grad_case("mini", mode)


@pytest.mark.parametrize("kind,mode", [("dccrn", "SI-SNR+LMS"), ("mini", "MSE+SI-SNR")])
def test_autograd_dropin_and_train_step(kind, mode):
    """loss.backward() through training_step gives backward_into's bits; upstream scales the
    gradients; two train_steps equal two manual (taped forward, backward_into, FlatAdam.step)
    steps bitwise; validation_step returns the four metrics; configure_optimizers is Adam."""
    from clskd import config as cfg
    from clskd.supervised import SupervisedTraining
    from clskd.train import FlatAdam, FlatParams
    make = _dccrn if kind == "dccrn" else _mini
    x, y = S.seeded_batch(**E2E)
    X, Y = x.to(DEV), y.to(DEV)
    mod = SupervisedTraining(make(), mode)
    loss = mod.training_step((X, Y), 0)
    assert loss.requires_grad
    loss.backward()
    out = mod.forward_with_tape(X, Y)
    assert torch.equal(out["loss"], loss.detach())
    g1 = {p: torch.empty_like(p) for p in mod.student.parameters()}
    mod.backward_into(out, g1)
    gh = {p: torch.empty_like(p) for p in mod.student.parameters()}
    mod.backward_into(out, gh, upstream=0.5)
    for n, p in mod.student.named_parameters():
        assert torch.equal(p.grad, g1[p]), n
        if not S.is_pre_bn_bias(n):
            e = float((gh[p].double() - 0.5 * g1[p].double()).norm() / (0.5 * g1[p].double().norm()))
            assert e <= 1e-5, (n, e)
    assert torch.equal(mod.training_step((X, Y), 0, return_parts=True)["loss"], out["loss"])
    mod.student.zero_grad(set_to_none=True)
    a, b = SupervisedTraining(make(), mode), SupervisedTraining(make(), mode)
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
    xv, yv = S.seeded_batch(2, 16000, seed=5)  # STOI needs more than 0.1 s
    val = a.validation_step((xv.to(DEV), yv.to(DEV)))
    assert set(val) == {"si_sdr", "si_sdr_imp", "stoi", "stoi_imp"}
    assert isinstance(a.configure_optimizers(), torch.optim.Adam)


def test_second_backward_over_one_tape_repeats_lstm_gradients():
    """With CLSKD_LSTM_PRE=0 the taped forward leaves only the gate inputs in the tape and the
    backward rebuilds the pre-activations in place, once per tape: a second backward_into over
    the same forward_with_tape result gives the LSTM parameter gradients of the first, bitwise."""
    from clskd import _lib
    from clskd.supervised import SupervisedTraining
    x, y = S.seeded_batch(**E2E)
    prev = _lib.set_knob("CLSKD_LSTM_PRE", 0)
    try:
        mod = SupervisedTraining(_dccrn(), "MSE")
        out = mod.forward_with_tape(x.to(DEV), y.to(DEV))
        grads = []
        for _ in range(2):
            g = {p: torch.full_like(p, 7.0) for p in mod.student.parameters()}
            mod.backward_into(out, g)
            grads.append(g)
        torch.cuda.synchronize()
    finally:
        _lib.set_knob("CLSKD_LSTM_PRE", prev)
    lstm = [(n, p) for n, p in mod.student.named_parameters()
            if n.startswith("enhance.") and ("weight_ih" in n or "weight_hh" in n or "bias_ih" in n
                                             or "bias_hh" in n)]
    assert len(lstm) == 2 * 2 * 4  # two layers x (real, imag) x four tensors
    for n, p in lstm:
        assert torch.equal(grads[0][p], grads[1][p]), n


def test_unsupported_modes_raise():
    import clskd
    from clskd import config as cfg
    from clskd.model import DCCRN
    from clskd.supervised import SupervisedTraining
    assert clskd.SupervisedTraining is SupervisedTraining
    for mode in S.PMSQE_MODES:
        with pytest.raises(NotImplementedError):
            SupervisedTraining(_dccrn(), mode)
    mini = _mini()
    for mode in S.LMS_MODES:
        with pytest.raises(NotImplementedError):
            SupervisedTraining(mini, mode)
    with pytest.raises(NotImplementedError):  # the teacher configuration: not gradient-checked
        SupervisedTraining(DCCRN(masking_mode="E", use_clstm=True, **cfg.TEACHER), "MSE")
    with pytest.raises(TypeError):
        SupervisedTraining(torch.nn.Linear(2, 2), "MSE")
