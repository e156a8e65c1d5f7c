"""DCCRN configurations beside the two shipped ones (cfg.STUDENT, cfg.TEACHER): channel counts that
are no power of two, five and seven encoder / decoder layers, one and three complex-LSTM layers,
and the reference's default widths on the real LSTM.  The case table, the recipe weights and model
of a case, and its float64 reference (tests/variants_ref.dccrn_forward, which is generic in depth
and rnn_layers) in the shape of variants_ref.steps.  tests/test_config_ref_cpu.py qualifies the
inputs on the CPU (float32 against float64 evaluation of the reference alone);
tests/test_gpu_configs.py holds clskd.DCCRN to it.  Test infrastructure, imported like
variants_ref; the table of margins is kept as profiles/config_margins.txt (python
tests/config_cases.py prints it)."""
import functools

import torch

import cbn_ref as CR
import sup_loss_ref as S
import variants_ref as V

# name -> the constructor arguments that differ from DCCRN(masking_mode="E", use_cbn=False)
CASES = {
    # C/8 = 1,3,5,9,9,6 and C/4 = 2,6,10,18,18,12 (the BatchNorm lane mappings), N and K tails in
    # every conv, LSTM input 4 x 24 per half
    "odd6": dict(kernel_num=[8, 24, 40, 72, 72, 48], rnn_units=64, rnn_layers=2, use_clstm=True),
    # seven layers, D4 = 256 / 2^7 = 2, one complex-LSTM layer that also projects (H = 16)
    "deep7": dict(kernel_num=[8, 8, 16, 16, 32, 32, 64], rnn_units=32, rnn_layers=1,
                  use_clstm=True),
    # five layers, D4 = 8, three LSTM layers, the projection on layer 2 (H = 64)
    "five3": dict(kernel_num=[8, 16, 24, 48, 48], rnn_units=128, rnn_layers=3, use_clstm=True),
    # the reference's default widths on the real LSTM: C6 = 256, LSTM input and `tranform` 1024
    "default_real": dict(kernel_num=[16, 32, 64, 128, 256, 256], rnn_units=128, rnn_layers=2,
                         use_clstm=False),
}
NAMES = tuple(CASES)
# the SupervisedTraining cases of tests/test_gpu_configs.py (default_real: refused by
# SupervisedTraining by name; the test asserts the refusal)
GRAD_MODES = {"odd6": ("SI-SNR+LMS", "MSE"), "deep7": ("SI-SNR",), "five3": ("SI-SNR",),
              "default_real": ("SI-SNR",)}
# the mode the CPU qualification table is stated for
QUALIFY_MODE = "SI-SNR"
E2E = dict(B=2, L=1600, seed=7)  # T = 19
RAGGED = dict(B=3, L=401, seed=7)
# gates of the GPU tests (tests/test_gpu_variants.py, tests/test_gpu_supervised.py); the CPU
# qualification holds the reference's own float32 evaluation to a tenth of each
WAV_RMS, WAV_MAX, LOSS_GATE, GRAD_GATE, ZERO_GATE = 1e-5, 1e-4, 5e-5, 2e-3, 1e-3


def case(c):
    return CASES[c] if isinstance(c, str) else c


def n_layers(c):
    return len(case(c)["kernel_num"])


def ctor(c, use_cbn=False):
    """Keyword arguments of clskd.DCCRN for a case."""
    return dict(masking_mode="E", use_cbn=use_cbn, **case(c))


def shapes(c, use_cbn=False):
    from clskd import config as cfg
    k = case(c)
    return cfg.dccrn_param_shapes(k["rnn_units"], k["kernel_num"], rnn_layers=k["rnn_layers"],
                                  use_cbn=use_cbn, use_clstm=k["use_clstm"])


def params(c, dtype=torch.float64, grad=True, use_cbn=False):
    """Recipe weights (STUDENT_SEED) of a case in dtype, requires_grad on every parameter: shaped
    like variants_ref.params."""
    from clskd.weights import STUDENT_SEED, recipe_state_dict
    from oracle import ref_cpu as R
    ps = R.to_torch_params(recipe_state_dict(shapes(c, use_cbn), STUDENT_SEED))
    out = {}
    for k, v in ps.items():
        if v.is_floating_point():
            v = v.to(dtype).clone()
            leaf = k.rsplit(".", 1)[-1]
            if grad and leaf not in CR.CBN_BUFFERS + ("running_mean", "running_var"):
                v.requires_grad_()
        out[k] = v
    return out


def model(c, train=True, use_cbn=False):
    from clskd.model import DCCRN
    from clskd.weights import STUDENT_SEED, apply_recipe
    return apply_recipe(DCCRN(**ctor(c, use_cbn)), STUDENT_SEED).train(train)


def batch(**kw):
    return S.seeded_batch(**{**E2E, **kw})


def forward(c, ps, x, R, train=True, update_stats=False, use_cbn=False):
    """variants_ref.dccrn_forward of a case (inside S.oracle_dtype(dtype) as R)."""
    k = case(c)
    return V.dccrn_forward(ps, x, "E", k["use_clstm"], train=train, update_stats=update_stats,
                           lstm_fn=R.lstm, use_cbn=use_cbn, n_layers=n_layers(c),
                           rnn_layers=k["rnn_layers"])


def reference(c, loss_modes, dtype=torch.float64, use_cbn=False, x=None, y=None):
    """{loss_mode: dict(loss, grads {name: tensor}, wav, pre_clamp, acts)} of DCCRN(**ctor(case))
    on recipe weights in train mode at the E2E inputs, from one forward in dtype (acts: the PReLU
    outputs, encoder then decoder)."""
    if x is None:
        x, y = batch()
    with S.oracle_dtype(dtype) as R:
        ps = params(c, dtype, use_cbn=use_cbn)
        x, y = x.to(dtype), y.to(dtype)
        fw = forward(c, ps, x, R, train=True, use_cbn=use_cbn)
        cs = R.conv_stft(y)
        cr, ci = cs[:, :257], cs[:, 257:]
        names = [k for k, v in ps.items() if v.requires_grad]
        out = {}
        for lm in loss_modes:
            loss = S.dccrn_loss(lm, fw["out_wav"], y, fw["real"], fw["imag"], cr, ci)
            grads = torch.autograd.grad(loss, [ps[n] for n in names], retain_graph=True,
                                        allow_unused=True)
            out[lm] = dict(loss=loss.detach(), grads=dict(zip(names, grads)),
                           wav=fw["out_wav"].detach(), pre_clamp=fw["pre_clamp"].detach(),
                           acts=[t.detach() for t in fw["enc"] + fw["dec"][:-1]])
    return out


@functools.lru_cache(maxsize=None)
def grad_reference(name, dtype=torch.float64):
    """reference() of a named case over its GRAD_MODES (and QUALIFY_MODE); shared, read only."""
    modes = tuple(dict.fromkeys(GRAD_MODES[name] + (QUALIFY_MODE,)))
    return reference(name, modes, dtype)


@functools.lru_cache(maxsize=None)
def forward_reference(name, use_cbn=False, B=E2E["B"], L=E2E["L"]):
    """The float64 forwards a GPU forward test compares with, detached; shared, read only:
    train (first train-mode pass, running statistics updated once), eval (eval-mode pass on those
    statistics), stats1 / stats2 (the normalisation buffers after one and two updates)."""
    x, _ = S.seeded_batch(B, L, seed=E2E["seed"])
    buffers = ("running_mean", "running_var") + tuple(CR.CBN_BUFFERS)
    with S.oracle_dtype(torch.float64) as R, torch.no_grad():
        ps = params(name, torch.float64, grad=False, use_cbn=use_cbn)
        snap = lambda: {k: v.clone() for k, v in ps.items() if k.rsplit(".", 1)[-1] in buffers}  # noqa: E731
        x = x.double()
        train = forward(name, ps, x, R, train=True, update_stats=True, use_cbn=use_cbn)
        stats1 = snap()
        ev = forward(name, ps, x, R, train=False, use_cbn=use_cbn)
        forward(name, ps, x, R, train=True, update_stats=True, use_cbn=use_cbn)
        stats2 = snap()
    return dict(train=train, eval=ev, stats1=stats1, stats2=stats2)


def margins(name):
    """The float32 evaluation of the reference against its float64 one for a named case at
    QUALIFY_MODE: dict(peak, wav_rms, wav_max, loss, grad, grad_name, zero, kink) — kink: the
    smallest |PReLU output| of the float64 forward, for the record: a device forward whose
    rounding puts such an element on the other branch differentiates another function there."""
    r64, r32 = grad_reference(name)[QUALIFY_MODE], grad_reference(name, torch.float32)[QUALIFY_MODE]
    d = r32["wav"].double() - r64["wav"]
    l64, l32 = float(r64["loss"]), float(r32["loss"])
    errs = S.grad_errors(r32["grads"], r64["grads"], n_layers(name))
    rel = {n: e for n, (e, k) in errs.items() if k == "rel"}
    worst = max(rel, key=rel.get)
    return dict(peak=float(r64["pre_clamp"].abs().max()), wav_rms=float(d.pow(2).mean().sqrt()),
                wav_max=float(d.abs().max()), loss=abs(l32 - l64) / abs(l64), grad=rel[worst],
                grad_name=worst, zero=max(e for e, k in errs.values() if k == "zero"),
                kink=min(float(a.abs().min()) for a in r64["acts"]))


def margin_line(name, m):
    return (f"CFGREF {name:13s} peak {m['peak']:.3f} wav rms {m['wav_rms']:.1e} max "
            f"{m['wav_max']:.1e} loss {m['loss']:.1e} grad {m['grad']:.1e} ({m['grad_name']}) "
            f"zero {m['zero']:.1e} | smallest |activation| at a PReLU {m['kink']:.1e}")


if __name__ == "__main__":  # the CPU table of profiles/config_margins.txt
    for nm in NAMES:
        print(margin_line(nm, margins(nm)))
