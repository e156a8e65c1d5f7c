"""Output-level knowledge distillation of the asteroid ``DCCRNet_mini`` student: the training
modules of the reference's three simpler scripts (distill_SPKD.py:37-87, distill_MSE.py:37-90,
distill_STFT.py:37-84) as one class.  They need no feature taps: loss = MRSTFT log-magnitude
base loss of the student's estimate against the clean target (fft 512 / win 400 / hop 100) + one
KD term between the student's and the frozen teacher's waveforms:

  kd="spkd"  SPKDLoss(student_wav, teacher_wav, 'batchmean') on the [B, L] rows
  kd="mse"   F.mse_loss(student, teacher)
  kd="stft"  stft_loss(student, teacher)[1]

The step is HIP kernels end to end: the taped ``DCCRNet_mini.run``, the loss kernels, the loss
gradients w.r.t. the estimate (``mrstft_backward``, ``spkd_grad`` + ``gram_bwd``,
``mse_loss_grad``) and ``asteroid_backward.mini_backward``, fp32 on the exact engines.
"""
import torch
import torch.nn as nn

from . import config as cfg
from . import ops
from .asteroid import DCCRNet_mini
from .asteroid_backward import mini_backward
from .backward import mrstft_backward
from .distill import _validation_step
from .framework import MultiResolutionSTFTLoss, SPKDLoss
from .model import DCCRN, refuse_cbn, refuse_mask_mode, refuse_real_lstm

KD_KINDS = ("spkd", "mse", "stft")


def _wave(model, x):
    """[B, L] estimate of a model whose forward returns [B, 1, L] or [B, L] (a local DCCRN is
    asked for its waveform alone)."""
    out = model(x, is_feat=True) if isinstance(model, DCCRN) else model(x)
    out = out.reshape(x.shape[0], -1)
    if out.shape != x.shape:
        raise ValueError(f"OutputDistillation: estimate {tuple(out.shape)} for input {tuple(x.shape)}")
    return out.float().contiguous()


class OutputDistillation(nn.Module):
    """distill_SPKD.py / distill_MSE.py / distill_STFT.py without Lightning, for a DCCRNet_mini
    student: the constructor and step signatures of ``KnowledgeDistillation``.  The teacher is
    frozen: a ``clskd.DCCRN`` or a ``DCCRNet_mini`` (anything whose forward returns [B, 1, L] or
    [B, L])."""

    def __init__(self, teacher, student, kd="spkd", sftf_loss=MultiResolutionSTFTLoss,
                 spkd_loss=SPKDLoss, cfg=cfg):
        super().__init__()
        refuse_cbn(teacher, "OutputDistillation")
        refuse_mask_mode(teacher, "OutputDistillation")
        refuse_real_lstm(teacher, "OutputDistillation")
        if kd not in KD_KINDS:
            raise ValueError(f"kd must be one of {KD_KINDS}, got {kd!r}")
        if not isinstance(student, DCCRNet_mini):
            raise TypeError("OutputDistillation trains a clskd.asteroid.DCCRNet_mini student")
        self.automatic_optimization = True
        self.teacher = teacher
        for p in self.teacher.parameters():
            p.requires_grad = False
        self.student = student
        self.student.compute = "fp32"
        self.kd = kd
        self.spkd_loss = spkd_loss
        self.stft_loss = sftf_loss(fft_sizes=[512], win_lengths=[400], hop_sizes=[100])
        self.cfg = cfg
        self.last = None

    def forward(self, x):
        return self.student(x)

    def configure_optimizers(self):
        """Adam with weight decay 5e-4, as the three reference scripts configure it."""
        return torch.optim.Adam(self.student.parameters(), lr=self.cfg.learning_rate,
                                weight_decay=5e-4)

    def validation_step(self, batch, batch_idx=0):
        return _validation_step(self, batch)

    def _wants_grad(self):
        return torch.is_grad_enabled() and any(p.requires_grad for p in self.student.parameters())

    # ------------------------------------------------------------------ forward + loss
    @torch.no_grad()
    def _step(self, X, y, tape):
        X = X.float().reshape(X.shape[0], -1).contiguous()
        y = y.float().reshape(X.shape[0], -1).contiguous()
        B = X.shape[0]
        dev = X.device
        t = _wave(self.teacher, X)
        st = {} if tape else None
        s = self.student.run(X, self.student.training, tape=st)["wav"]
        buf = torch.empty(3, dtype=torch.float32, device=dev)  # [sc, base, kd]
        tapes = dict(s=st, ms=[], kd=None) if tape else None
        self.stft_loss(s, y, out2=buf[0:2], tape=tapes["ms"] if tape else None)
        if self.kd == "spkd":
            # the reference's SPKDLoss(student, teacher, 'batchmean')(): one Gram launch over
            # both waveforms, one finalize; the slabs stay for the gradient
            slabs = ops.GramSlabs([ops.gram_view(s), ops.gram_view(t)], B)
            ops.spkd_finalize(slabs.refs[0:1], slabs.refs[1:2], B, True, out=buf[2:3])
            if tape:
                tapes["kd"] = slabs
        elif self.kd == "mse":
            ops.mse_loss_grad(s, t, buf[2:3])
        else:
            k2 = torch.empty(2, dtype=torch.float32, device=dev)
            kt = [] if tape else None
            self.stft_loss(s, t, out2=k2, tape=kt)
            ops.sum_f32(k2[1:2], buf[2:3])
            if tape:
                tapes["kd"] = kt
        total = torch.empty((), dtype=torch.float32, device=dev)
        ops.sum_f32(buf[1:], total)
        return dict(loss=total, base=buf[1], kd=buf[2], student_wav=s, teacher_wav=t, tape=tapes)

    def training_step(self, batch, batch_idx=0, return_parts=False):
        """Under autograd (grad enabled, trainable student) the returned loss is connected to the
        student's parameters: loss.backward() runs the HIP backward and accumulates into .grad."""
        X, y = batch
        if self._wants_grad() and not return_parts:
            params = [p for p in self.student.parameters() if p.requires_grad]
            return _OutputKDLoss.apply(self, X, y, *params)
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
        """Student gradients of upstream * out['loss'] (a forward_with_tape result) into `grads`
        (parameter -> fp32 tensor)."""
        tp = out["tape"]
        if tp is None:
            raise ValueError("backward_into needs a forward_with_tape result")
        s, t = out["student_wav"], out["teacher_wav"]
        B, L = s.shape
        dev = s.device
        d_wav = torch.empty(B, L, dtype=torch.float32, device=dev)
        if self.kd == "mse":  # the first writer of d_wav
            ops.mse_loss_grad(s, t, torch.empty(1, dtype=torch.float32, device=dev), d_wav,
                              scale=upstream)
        elif self.kd == "spkd":
            slabs = tp["kd"]
            M = ops.spkd_grad(slabs.refs[0:1], slabs.refs[1:2], B, True, upstream, device=dev)
            v = ops.gram_view(s)
            if v.tensor is s:
                ops.gram_bwd([(v, M[0], d_wav, L, v.Ctot, 0, False)], B)
            else:  # L % 4 != 0: the Gram read a zero-padded copy; fold its gradient back
                Lp = v.sB
                dz = torch.empty(B, Lp, dtype=torch.float32, device=dev)
                ops.gram_bwd([(v, M[0], dz, Lp, v.Ctot, 0, False)], B)
                ops.frame_pad_bwd(dz, L, 0, 0, d_wav)
        else:
            ops.fill(d_wav, 0.0)
            mrstft_backward(tp["kd"], d_wav, upstream)
        mrstft_backward(tp["ms"], d_wav, upstream)
        mini_backward(self.student, tp["s"], d_wav, grads, acc_params=accumulate)

    def train_step(self, batch, flat, opt):
        """One training step without autograd bookkeeping: taped fwd + loss -> HIP backward into
        the flat gradient buffer -> (multi-rank) one all-reduce -> one Adam launch.
        flat: train.FlatParams(self.student); opt: train.FlatAdam(flat, weight_decay=5e-4, ...)."""
        from .train import allreduce_grads
        X, y = batch
        out = self.forward_with_tape(X, y)
        self.backward_into(out, flat.grad_dict())
        scale = allreduce_grads(flat)
        opt.step(grad_scale=scale)
        return out["loss"]


class _OutputKDLoss(torch.autograd.Function):
    """Connects the HIP step to autograd like distill._CLSKDLoss: forward = forward_with_tape,
    backward = backward_into, one gradient per student parameter."""

    @staticmethod
    def forward(ctx, kd, X, y, *params):
        out = kd.forward_with_tape(X, y)
        ctx.kd, ctx.out, ctx.params = kd, out, params
        return out["loss"].clone()

    @staticmethod
    def backward(ctx, gout):
        kd, out, params = ctx.kd, ctx.out, ctx.params
        up = float(gout.reshape(()).item()) if gout is not None else 1.0
        grads = {p: torch.empty_like(p, dtype=torch.float32) for p in params}
        kd.backward_into(out, grads, accumulate=False, upstream=up)
        ctx.out = None
        return (None, None, None) + tuple(grads[p] for p in params)
