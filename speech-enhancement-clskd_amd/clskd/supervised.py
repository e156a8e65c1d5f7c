"""Supervised training: a DCCRN (or the asteroid ``DCCRNet_mini``) on labels alone, with the
reference's ``DCCRN.loss`` menu (DCCRN.py:259-411) as the objective — the no-teacher baseline of
every distillation result, and the way the teacher the distillation scripts load was produced
(``config.loss_mode``).

The step is HIP kernels end to end: the taped forward, the loss kernels of csrc/sup_loss.hip
(waveform terms from one pass of per-row sums, the mel log-spectral distance "LMS" over the masked
spectrum), their gradients (``wave_loss_grad`` at the waveform, ``mel_loss_bwd`` at the masked
spectrum: ``dccrn_backward``'s ``g['est_spec']``) and the existing backward, fp32 on the exact
engines.  One extra mode, 'MRSTFT', is the distillation scripts' base loss alone (the MRSTFT
log-magnitude term of ``distill*.py`` with the KD term removed).

The PMSQE modes need asteroid's SingleSrcPMSQE tables and raise NotImplementedError."""
import torch
import torch.nn as nn

from . import config as cfg
from . import ops
from .asteroid import DCCRNet_mini
from .asteroid_backward import mini_backward
from .backward import _zeros, dccrn_backward, mrstft_backward
from .distill import _validation_step
from .framework import MultiResolutionSTFTLoss
from .model import DCCRN

# mode -> (weights of (mse, -sdr(y, s), -si_snr(s, y), -si_sdr(y, s), -si_sdr(s, y)), weight of
# LMS): the reference's r1 : r2 / (r1 + r2) mixes (DCCRN.py:285-301, 324-328, 344-348, 384-388)
LOSS_MODES = {
    "MSE": ((1.0, 0, 0, 0, 0), 0.0),
    "SDR": ((0, 1.0, 0, 0, 0), 0.0),
    "SI-SNR": ((0, 0, 1.0, 0, 0), 0.0),
    "SI-SDR": ((0, 0, 0, 1.0, 0), 0.0),
    "MSE+SI-SNR": ((100.0 / 101.0, 0, 1.0 / 101.0, 0, 0), 0.0),
    "SI-SNR+SI-SDR": ((0, 0, 0.5, 0, 0.5), 0.0),
    "MSE+LMS": ((1000.0 / 1001.0, 0, 0, 0, 0), 1.0 / 1001.0),
    "SDR+LMS": ((0, 1.0 / 3.0, 0, 0, 0), 2.0 / 3.0),
    "SI-SNR+LMS": ((0, 0, 1.0 / 3.0, 0, 0), 2.0 / 3.0),
}
PMSQE_MODES = ("MSE+PMSQE", "SDR+PMSQE", "SI-SNR+PMSQE", "PMSQE")
EXTRA_MODES = ("MRSTFT",)


def check_mode(loss_mode, extra=False):
    if loss_mode in LOSS_MODES or (extra and loss_mode in EXTRA_MODES):
        return
    if "PMSQE" in str(loss_mode):
        raise NotImplementedError(
            f"loss_mode {loss_mode!r}: the PMSQE losses need asteroid's SingleSrcPMSQE tables")
    raise NotImplementedError(f"loss_mode {loss_mode!r} is not one of {sorted(LOSS_MODES)}")


def menu_loss(loss_mode, s, y, clean_spec=None, est_spec=None, upstream=1.0, want_coef=False):
    """One DCCRN.loss mode on the device: s / y [B, L]; for the LMS modes clean_spec / est_spec
    are the frame-major spectra [B][T][ld >= 514].  Returns (loss 0-d, coef or None): coef [B, 2]
    is the waveform gradient's table for ops.wave_loss_grad, scaled by upstream."""
    check_mode(loss_mode)
    w, wm = LOSS_MODES[loss_mode]
    out, coef = ops.wave_loss(s, y, w, upstream, want_coef)
    if wm == 0.0:
        return out[0], coef
    tot = torch.empty(2, dtype=torch.float32, device=out.device)
    ops.sum_f32(out[0:1], tot[0:1])
    ops.mel_loss(clean_spec, est_spec, tot, scale=wm, accumulate=True)
    return tot[0], coef


class SupervisedTraining(nn.Module):
    """A model trained on (noisy, clean) pairs with one DCCRN.loss mode: the step signatures of
    ``KnowledgeDistillation`` / ``OutputDistillation`` without a teacher.

    model: a ``clskd.DCCRN`` — the student configuration (config.kernel_num_student,
    rnn_units_student) on either LSTM stack, or on the complex stack any other one that constructs
    (tests/test_gpu_configs.py holds the gradients of other widths, depths and LSTM layer counts
    to the same gates) except the teacher configuration.  The teacher configuration (DESIGN.md
    §18) and the reference's default widths on the real LSTM (§24) each missed that gate in
    their trial and raise NotImplementedError; ``use_cbn`` False or True:
    the taped forward and ``dccrn_backward`` route a ComplexBatchNorm model through csrc/cbn.hip —
    or a ``DCCRNet_mini``.
    loss_mode: a DCCRN.loss mode (LOSS_MODES) or 'MRSTFT'.  For a DCCRNet_mini the LMS modes raise
    NotImplementedError (mini_backward has no entry point at the masked spectrum)."""

    def __init__(self, model, loss_mode="SI-SNR", sftf_loss=MultiResolutionSTFTLoss, cfg=cfg):
        super().__init__()
        check_mode(loss_mode, extra=True)
        self.is_mini = isinstance(model, DCCRNet_mini)
        if not self.is_mini and not isinstance(model, DCCRN):
            raise TypeError("SupervisedTraining trains a clskd.DCCRN or a clskd.asteroid.DCCRNet_mini")
        self.uses_lms = loss_mode in LOSS_MODES and LOSS_MODES[loss_mode][1] != 0.0
        if self.is_mini and self.uses_lms:
            raise NotImplementedError(
                f"loss_mode {loss_mode!r}: DCCRNet_mini's backward has no masked-spectrum entry point")
        if not self.is_mini and (list(model.kernel_num[1:]) == list(cfg.kernel_num)
                                 and model.rnn_units == cfg.rnn_units and model.use_clstm):
            raise NotImplementedError(
                "SupervisedTraining: the teacher DCCRN configuration (kernel_num "
                f"{list(cfg.kernel_num)}, rnn_units {cfg.rnn_units}) is not supported: it missed "
                "the end-to-end gradient gate in its one trial (DESIGN.md §18)")
        if not self.is_mini and not model.use_clstm and (
                list(model.kernel_num[1:]) != list(cfg.kernel_num_student)
                or model.rnn_units != cfg.rnn_units_student):
            raise NotImplementedError(
                f"SupervisedTraining: use_clstm=False with kernel_num {list(model.kernel_num[1:])}, "
                f"rnn_units {model.rnn_units} is not supported: on the real-LSTM stack only the "
                f"student configuration (kernel_num {list(cfg.kernel_num_student)}, rnn_units "
                f"{cfg.rnn_units_student}) is held to the end-to-end gradient gate; the reference's "
                "default widths missed it in their trial (DESIGN.md §24)")
        self.automatic_optimization = True
        self.student = model  # the trained model, under the name the shared helpers use
        self.student.compute = "fp32"
        self.loss_mode = loss_mode
        self.stft_loss = (sftf_loss(fft_sizes=[512], win_lengths=[400], hop_sizes=[100])
                          if loss_mode == "MRSTFT" else None)
        self.cfg = cfg
        self.last = None

    @property
    def model(self):
        return self.student

    def forward(self, x):
        return self.student(x)

    def configure_optimizers(self):
        return torch.optim.Adam(self.student.parameters(), lr=self.cfg.learning_rate)

    def validation_step(self, batch, batch_idx=0):
        return _validation_step(self, batch)

    def _wants_grad(self):
        return torch.is_grad_enabled() and any(p.requires_grad for p in self.student.parameters())

    # ------------------------------------------------------------------ forward + loss
    @torch.no_grad()
    def _step(self, X, y, tape):
        X = X.float().reshape(X.shape[0], -1).contiguous()
        y = y.float().reshape(X.shape[0], -1).contiguous()
        m = self.student
        st = {} if tape else None
        if self.is_mini:
            fwd = m.run(X, m.training, tape=st)
            s = fwd["wav"]
        else:
            fwd = m.run(X, train=m.training, bn_updates=1 if m.training else 0, want_masks=False,
                        tape=st)
            s = fwd["out_wav"]
        tapes = dict(s=st, ms=None, clean=None) if tape else None
        if self.loss_mode == "MRSTFT":
            buf = torch.empty(2, dtype=torch.float32, device=X.device)
            ms = [] if tape else None
            self.stft_loss(s, y, out2=buf, tape=ms)
            loss = buf[1]
            if tape:
                tapes["ms"] = ms
        else:
            clean = m.spectrum(y) if self.uses_lms else None
            loss, coef = menu_loss(self.loss_mode, s, y, clean, fwd["est"] if self.uses_lms else None,
                                   want_coef=bool(tape))
            if tape:
                tapes["clean"], tapes["coef"] = clean, coef
        return dict(loss=loss, wav=s, labels=y, fwd=fwd, tape=tapes)

    def training_step(self, batch, batch_idx=0, return_parts=False):
        """Under autograd (grad enabled, trainable model) the returned loss is connected to the
        model's parameters: loss.backward() runs the HIP backward and accumulates into .grad."""
        X, y = batch
        if self._wants_grad() and not return_parts:
            params = [p for p in self.student.parameters() if p.requires_grad]
            return _SupervisedLoss.apply(self, X, y, *params)
        out = self._step(X, y, tape=False)
        self.last = out
        return out if return_parts else out["loss"]

    def forward_with_tape(self, X, y):
        out = self._step(X, y, tape=True)
        self.last = out
        return out

    # ------------------------------------------------------------------ backward
    @torch.no_grad()
    def backward_into(self, out, grads, accumulate=False, upstream=1.0):
        """Gradients of upstream * out['loss'] (a forward_with_tape result) into `grads`
        (parameter -> fp32 tensor)."""
        tp = out["tape"]
        if tp is None:
            raise ValueError("backward_into needs a forward_with_tape result")
        s, y, fwd = out["wav"], out["labels"], out["fwd"]
        B, L = s.shape
        dev = s.device
        d_wav = torch.empty(B, L, dtype=torch.float32, device=dev)
        d_est = None
        if self.loss_mode == "MRSTFT":
            ops.fill(d_wav, 0.0)
            mrstft_backward(tp["ms"], d_wav, upstream)
        else:
            # the forward's finalize already wrote the table for upstream = 1; any other
            # upstream is folded in by one more sums pass + finalize
            w, wm = LOSS_MODES[self.loss_mode]
            coef = tp["coef"]
            if upstream != 1.0:
                _, coef = ops.wave_loss(s, y, w, upstream, want_coef=True)
            ops.wave_loss_grad(s, y, coef, d_wav)
            if wm != 0.0:
                est = fwd["est"]
                d_est = _zeros(est.shape, dev)  # [B][T][516]: the tail columns stay zero
                ops.mel_loss_bwd(tp["clean"], est, d_est, upstream * wm)
        if self.is_mini:
            mini_backward(self.student, tp["s"], d_wav, grads, acc_params=accumulate)
            return
        enc, dec, dec_in = fwd["enc"], fwd["dec"], fwd["dec_in"]
        # (every decoder output but the last: the mask's gradient comes from the waveform tail)
        g = dict(enc=[_zeros(t.shape, dev) for t in enc], dec=[_zeros(t.shape, dev) for t in dec[:-1]],
                 dec_in=_zeros(dec_in.shape, dev), wav=d_wav, est_spec=d_est)
        dccrn_backward(self.student, tp["s"], enc, dec, dec_in, fwd["lstm_io"], g, grads,
                       acc_params=accumulate)

    def train_step(self, batch, flat, opt):
        """One training step without autograd bookkeeping: taped fwd + loss -> HIP backward into
        the flat gradient buffer -> (multi-rank) one all-reduce -> one Adam launch.
        flat: train.FlatParams(self.student); opt: train.FlatAdam(flat, ...)."""
        from .train import allreduce_grads
        X, y = batch
        out = self.forward_with_tape(X, y)
        self.backward_into(out, flat.grad_dict())
        scale = allreduce_grads(flat)
        opt.step(grad_scale=scale)
        return out["loss"]


class _SupervisedLoss(torch.autograd.Function):
    """Connects the HIP step to autograd like distill._CLSKDLoss: forward = forward_with_tape,
    backward = backward_into, one gradient per parameter."""

    @staticmethod
    def forward(ctx, mod, X, y, *params):
        out = mod.forward_with_tape(X, y)
        ctx.mod, ctx.out, ctx.params = mod, out, params
        return out["loss"].clone()

    @staticmethod
    def backward(ctx, gout):
        mod, out, params = ctx.mod, ctx.out, ctx.params
        up = float(gout.reshape(()).item()) if gout is not None else 1.0
        grads = {p: torch.empty_like(p, dtype=torch.float32) for p in params}
        mod.backward_into(out, grads, accumulate=False, upstream=up)
        ctx.out = None
        return (None, None, None) + tuple(grads[p] for p in params)
