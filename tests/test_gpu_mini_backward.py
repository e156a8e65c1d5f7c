"""GPU: the DCCRNet_mini training step (clskd.distill_mini.OutputDistillation, the taped
DCCRNet_mini.run and clskd.asteroid_backward.mini_backward) on the fixture checkpoint against the
float64 step reference of tests/mini_train_ref.py (autograd through oracle.asteroid_cpu.forward).

Gates: every one of the 112 trainable tensors within 2e-3 relative L2 of the float64 gradient
(the project's fp32 gradient gate, tests/test_gpu_backward.py), the loss within 5e-5 relative
(DESIGN §4).  The module tree has no conv bias in front of a BatchNorm (the encoder / decoder
convs have none; the output layer's bias has no BatchNorm behind it), so every tensor is held to
the relative gate.  Each gradient case prints its per-tensor table (`MINIGRAD` lines);
profiles/mini_train_grad_parity.txt keeps a run's tables."""
import numpy as np
import pytest
import torch
import torch.nn as nn

import mini_train_ref as M
from conftest import golden

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GRAD_GATE = 2e-3
LOSS_GATE = 5e-5


class _FixedTeacher(nn.Module):
    """A frozen teacher whose forward returns a given waveform [B, L]."""

    def __init__(self, wav):
        super().__init__()
        self.register_buffer("wav", wav)

    def forward(self, x):
        return self.wav


def _student():
    from clskd.asteroid import DCCRNet_mini, load_conf
    return DCCRNet_mini.from_pretrained(load_conf(golden("asteroid_mini.npz"))).to(DEV).train()


def _kd(kind, t):
    from clskd.distill_mini import OutputDistillation
    return OutputDistillation(_FixedTeacher(t.to(DEV)), _student(), kd=kind)


def _rel(a, b):
    return float(np.linalg.norm(a.astype(np.float64) - b) / np.linalg.norm(b))


def _grad_case(kind, B, L, seed):
    x, y, t = M.seeded_batch(B, L, seed=seed)
    ref = M.reference_step(kind, x, y, t, torch.float64)
    kd = _kd(kind, t)
    out = kd.forward_with_tape(x.to(DEV), y.to(DEV))
    grads = {p: torch.full_like(p, 7.0) for p in kd.student.parameters()}
    kd.backward_into(out, grads)
    torch.cuda.synchronize()
    names = dict(kd.student.named_parameters())
    assert sorted(names) == sorted(ref["grads"]) and len(names) == 112
    rows, bad = [], []
    for n, p in names.items():
        e = _rel(grads[p].cpu().numpy(), ref["grads"][n].numpy())
        rows.append(f"MINIGRAD {kind} B{B} L{L} {n:55s} {e:.2e}")
        if not e <= GRAD_GATE:
            bad.append((n, e))
    dl = abs(out["loss"].item() - float(ref["loss"])) / abs(float(ref["loss"]))
    wav = _rel(out["student_wav"].cpu().numpy(), ref["wav"].numpy())
    rows.append(f"MINIGRAD {kind} B{B} L{L} loss hip={out['loss'].item():.7f} ref={float(ref['loss']):.7f} "
                f"rel={dl:.2e} wav rel={wav:.2e} worst={max(float(r.split()[-1]) for r in rows):.2e}")
    print("\n".join(rows))
    return kd, names, grads, ref, dl, bad


@pytest.mark.parametrize("kind", M.KD_KINDS)
def test_gradients_against_fp64_reference(kind):
    """B = 3, L = 1600 (T = 13): all 112 tensors and the loss, for each KD term.

    The inputs are broadband seeded noise (mini_train_ref.seeded_batch says why): on them the
    reference's own float32 evaluation on the CPU passes both gates on all 112 tensors
    (tests/test_mini_train_ref_cpu.py), so the gates measure the device step.  Measured on
    MI355X (profiles/mini_train_grad_parity.txt): loss within 1.2e-8; the worst tensor, always a
    one-element one (a PReLU slope or an output bias: a sum over a whole map with
    cancellation), at 4.4e-4 (spkd), 8.4e-4 (mse) and 1.35e-3 (stft)."""
    _, _, _, _, dl, bad = _grad_case(kind, 3, 1600, seed=1)
    assert dl <= LOSS_GATE, dl
    assert not bad, bad


def test_ragged_tail_carries_no_gradient():
    """B = 2, L = 1250 (T = 9): the samples at or past 100 (T + 3) = 1200 are pad_x_to_y zeros of
    the forward; L % 4 = 2 also takes the SPKD Gram's padded view."""
    _, _, _, _, dl, bad = _grad_case("spkd", 2, 1250, seed=2)
    assert dl <= LOSS_GATE, dl
    assert not bad, bad


def test_one_frame_at_the_lstm_gives_zero_recurrent_weight_gradients():
    """B = 2, L = 1000 (T = 7, one frame at the last encoder): h_{t-1} is the zero initial state,
    so the four weight_hh_l0 gradients are exactly zero on the device too."""
    x, y, t = M.seeded_batch(2, 1000, seed=2)
    kd = _kd("mse", t)
    out = kd.forward_with_tape(x.to(DEV), y.to(DEV))
    grads = {p: torch.full_like(p, 7.0) for p in kd.student.parameters()}
    kd.backward_into(out, grads)
    torch.cuda.synchronize()
    hh = [(n, p) for n, p in kd.student.named_parameters() if n.endswith("weight_hh_l0")]
    assert len(hh) == 4
    for n, p in hh:
        assert (grads[p] == 0).all(), n
    assert all(torch.isfinite(g).all() for g in grads.values())
    ref = M.reference_step("mse", x, y, t, torch.float64)
    for n, p in kd.student.named_parameters():
        if ".rnns.0." in n and n.endswith("weight_ih_l0"):
            assert _rel(grads[p].cpu().numpy(), ref["grads"][n].numpy()) <= GRAD_GATE, n


def test_taped_forward_is_bitwise_the_untaped_one():
    """Waveform, mask and every buffer (running statistics, batch counters) after a taped run
    equal those after an untaped run of the same checkpoint."""
    x, _, _ = M.seeded_batch(3, 1600, seed=3)
    a, b = _student(), _student()
    with torch.no_grad():
        ra = a.run(x.to(DEV), True)
        tape = {}
        rb = b.run(x.to(DEV), True, tape=tape)
    torch.cuda.synchronize()
    assert torch.equal(ra["wav"], rb["wav"]) and torch.equal(ra["mask"], rb["mask"])
    for (n, u), (_, v) in zip(a.named_buffers(), b.named_buffers()):
        assert torch.equal(u, v), n
    assert len(tape["enc_bn"]) == 6 and len(tape["dec_bn"]) == 5 and len(tape["lstm"]) == 2
    for raw, coef, mv, *_ in tape["enc_bn"] + tape["dec_bn"]:
        assert torch.isfinite(raw).all() and torch.isfinite(coef).all() and (mv[1] >= 0).all()


def test_bitwise_repeatable_autograd_dropin_and_train_step():
    """Two backward passes give the same bits; loss.backward() through training_step gives
    backward_into's bits; train_step equals forward_with_tape + backward_into + opt.step()
    bitwise; one FlatAdam step with weight decay 5e-4 matches torch.optim.Adam(weight_decay=5e-4)
    on the same gradients; the forward after the step sees the new weights."""
    from clskd import config as cfg
    from clskd.train import FlatAdam, FlatParams
    x, y, t = M.seeded_batch(3, 1600, seed=4)
    X, Y = x.to(DEV), y.to(DEV)
    kd = _kd("spkd", t)
    loss = kd.training_step((X, Y), 0)
    assert loss.requires_grad
    loss.backward()
    g_auto = {n: p.grad.clone() for n, p in kd.student.named_parameters()}
    out = kd.forward_with_tape(X, Y)
    assert torch.equal(out["loss"], loss.detach())
    g1 = {p: torch.empty_like(p) for p in kd.student.parameters()}
    g2 = {p: torch.empty_like(p) for p in kd.student.parameters()}
    kd.backward_into(out, g1)
    kd.backward_into(out, g2)  # the same tape again
    g3 = {p: torch.empty_like(p) for p in kd.student.parameters()}
    kd.backward_into(kd.forward_with_tape(X, Y), g3)
    for n, p in kd.student.named_parameters():
        assert torch.equal(g1[p], g2[p]) and torch.equal(g1[p], g3[p]), n
        assert torch.equal(g_auto[n], g1[p]), n
    # upstream scales the gradients
    gs = {p: torch.empty_like(p) for p in kd.student.parameters()}
    kd.backward_into(out, gs, upstream=0.5)
    ga = {p: g1[p].clone() for p in kd.student.parameters()}
    kd.backward_into(out, ga, accumulate=True)  # accumulate adds
    for n, p in kd.student.named_parameters():
        assert _rel(gs[p].cpu().numpy(), 0.5 * g1[p].double().cpu().numpy()) <= 1e-5, n
        assert _rel(ga[p].cpu().numpy(), 2.0 * g1[p].double().cpu().numpy()) <= 1e-6, n
    # one Adam step through the flat buffers vs torch.optim.Adam on the same gradients
    ref_params = {n: p.detach().clone().requires_grad_() for n, p in kd.student.named_parameters()}
    for n, p in kd.student.named_parameters():
        ref_params[n].grad = g1[p].clone()
    torch.optim.Adam(list(ref_params.values()), lr=cfg.learning_rate, weight_decay=5e-4).step()
    kd.student.zero_grad(set_to_none=True)
    # a second module on the same checkpoint takes the step through train_step
    kd2 = _kd("spkd", t)
    flat, flat2 = FlatParams(kd.student), FlatParams(kd2.student)
    opt = FlatAdam(flat, lr=cfg.learning_rate, weight_decay=5e-4)
    opt2 = FlatAdam(flat2, lr=cfg.learning_rate, weight_decay=5e-4)
    kd.backward_into(kd.forward_with_tape(X, Y), flat.grad_dict())
    for p in flat.params:
        assert torch.equal(flat.gviews[p], g1[p])
    opt.step()
    l2 = kd2.train_step((X, Y), flat2, opt2)
    torch.cuda.synchronize()
    assert torch.equal(l2, out["loss"])
    assert torch.equal(flat.data, flat2.data) and torch.equal(flat.grad, flat2.grad)
    for n, p in kd.student.named_parameters():
        np.testing.assert_allclose(p.detach().cpu().numpy(), ref_params[n].detach().cpu().numpy(),
                                   rtol=1e-6, atol=1e-7, err_msg=n)
    # the packed-weight caches see the update: the next forward uses the new weights
    l3 = kd.training_step((X, Y), 0, return_parts=True)["loss"].item()
    assert l3 != loss.item()
    # configure_optimizers: Adam, the reference's weight decay
    o = kd.configure_optimizers()
    assert isinstance(o, torch.optim.Adam) and o.defaults["weight_decay"] == 5e-4


def test_dccrn_teacher_and_validation_step():
    """A small clskd.DCCRN as the frozen teacher (the stand-in of DESIGN §7) for each KD term:
    finite loss and gradients; validation_step returns the four metrics."""
    from clskd import config as cfg
    from clskd.distill_mini import OutputDistillation
    from clskd.model import DCCRN
    from clskd.weights import STUDENT_SEED, apply_recipe
    x, y, _ = M.seeded_batch(2, 16000, seed=5)
    X, Y = x.to(DEV), y.to(DEV)
    teacher = apply_recipe(DCCRN(masking_mode="E", use_clstm=True, **cfg.STUDENT), STUDENT_SEED).to(DEV)
    for kind in M.KD_KINDS:
        kd = OutputDistillation(teacher, _student(), kd=kind)
        assert not any(p.requires_grad for p in kd.teacher.parameters())
        loss = kd.training_step((X, Y), 0)
        loss.backward()
        assert torch.isfinite(loss)
        assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in kd.student.parameters())
    val = kd.validation_step((X, Y))
    assert set(val) == {"si_sdr", "si_sdr_imp", "stoi", "stoi_imp"}
    assert all(np.isfinite(v) for v in val.values())
