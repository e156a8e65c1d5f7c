"""CPU: the inputs of tests/test_gpu_configs.py are qualified on the reference alone, and the
constructor says what is not built.

For every case of tests/config_cases.py the float32 evaluation of the float64 restatement stays
within ONE TENTH of each gate the HIP model is held to on the GPU (waveform rms 1e-5 / max 1e-4,
loss 5e-5, every gradient tensor 2e-3 relative L2, analytically-zero biases 1e-3 of |dW|), and the
pre-clamp peak stays below 0.99 (no clamp decision depends on rounding).  The generalised
machinery (depth-aware zero-bias classifier, config_cases.reference) returns at the nominal
student what sup_loss_ref returns today, bit for bit.  Each case prints its `CFGREF` line
(profiles/config_margins.txt keeps the table)."""
import pytest
import torch

import config_cases as C
import sup_loss_ref as S


@pytest.mark.parametrize("name", C.NAMES)
def test_float32_evaluation_of_the_reference_is_a_tenth_inside_every_gate(name):
    m = C.margins(name)
    print(C.margin_line(name, m))
    assert m["peak"] < 0.99
    assert m["wav_rms"] <= C.WAV_RMS / 10 and m["wav_max"] <= C.WAV_MAX / 10, m
    assert m["loss"] <= C.LOSS_GATE / 10, m
    assert m["grad"] <= C.GRAD_GATE / 10, m
    assert m["zero"] <= C.ZERO_GATE / 10, m


@pytest.mark.parametrize("name", C.NAMES)
def test_every_parameter_has_a_gradient_entry_and_vice_versa(name):
    from clskd.model import DCCRN
    m = DCCRN(**C.ctor(name))
    names = sorted(n for n, _ in m.named_parameters())
    ref = C.grad_reference(name)
    for mode in C.GRAD_MODES[name]:
        assert sorted(ref[mode]["grads"]) == names, mode
        assert all(g is not None for g in ref[mode]["grads"].values())
    sd = {k: v for k, v in m.state_dict().items() if not k.startswith(("stft.", "istft."))}
    assert list(sd) == list(C.shapes(name))
    assert all(tuple(v.shape) == tuple(C.shapes(name)[k]) for k, v in sd.items())
    k = C.CASES[name]
    nl = len(k["kernel_num"])
    assert len(m.encoder) == len(m.decoder) == nl and m.hidden_dim == 256 // 2 ** nl
    if k["use_clstm"]:
        assert len(m.enhance) == k["rnn_layers"]
        assert [e.projection_dim is not None for e in m.enhance] == \
            [i == k["rnn_layers"] - 1 for i in range(k["rnn_layers"])]


def test_use_cbn_odd6_has_every_parameter_in_the_shape_table():
    from clskd.model import DCCRN
    m = DCCRN(**C.ctor("odd6", use_cbn=True))
    sd = [k for k in m.state_dict() if not k.startswith(("stft.", "istft."))]
    assert sd == list(C.shapes("odd6", use_cbn=True))


def test_the_classifier_puts_todays_names_in_zero_at_six_layers():
    """For a six-layer model: the conv biases of encoder 0..5 and decoder 0..4, as before."""
    from clskd import config as cfg
    names = list(cfg.dccrn_param_shapes(**cfg.STUDENT))
    today = {n for n in names if n.endswith("_conv.bias") and not n.startswith("decoder.5.")}
    assert {n for n in names if S.is_pre_bn_bias(n)} == today
    assert {n for n in names if S.is_pre_bn_bias(n, 6)} == today
    assert len(today) == 2 * 11
    # at seven layers decoder.5's bias sits before a BatchNorm, decoder.6's does not; at five
    # decoder.4's is the mask layer's
    assert S.is_pre_bn_bias("decoder.5.0.real_conv.bias", 7)
    assert not S.is_pre_bn_bias("decoder.6.0.imag_conv.bias", 7)
    assert not S.is_pre_bn_bias("decoder.4.0.real_conv.bias", 5)
    assert S.is_pre_bn_bias("decoder.3.0.real_conv.bias", 5)
    for name in C.NAMES:  # the rule, from the shape table: zero exactly when a norm follows
        sh, nl = C.shapes(name), C.n_layers(name)
        for n in sh:
            if n.endswith("_conv.bias"):
                follows = n.rsplit(".0.", 1)[0] + ".1.weight" in sh
                assert S.is_pre_bn_bias(n, nl) == follows, (name, n)


def test_the_generalised_reference_returns_todays_bits_for_the_student():
    """config_cases.reference at the student's configuration against variants_ref.steps (the same
    restatement: every bit) and sup_loss_ref.dccrn_steps (oracle.ref_cpu's own forward: the same
    loss and waveform bits; its autograd graph sums the gradients in another order, so those to
    1e-12)."""
    import variants_ref as V
    from clskd import config as cfg
    x, y = S.seeded_batch(2, 1600, seed=3)
    student = dict(rnn_layers=2, use_clstm=True, **cfg.STUDENT)
    modes = ("SI-SNR", "MSE+LMS")
    new = C.reference(student, modes, torch.float64, x=x, y=y)
    var = V.steps(("E", True), modes, x, y, torch.float64)
    old = S.dccrn_steps(modes, x, y, torch.float64)
    for lm in modes:
        for other in (var, old):
            assert torch.equal(new[lm]["loss"], other[lm]["loss"]), lm
            assert torch.equal(new[lm]["wav"], other[lm]["wav"]), lm
            assert sorted(new[lm]["grads"]) == sorted(other[lm]["grads"])
        for n, g in var[lm]["grads"].items():
            assert torch.equal(new[lm]["grads"][n], g), (lm, n)
        assert S.grad_errors(new[lm]["grads"], var[lm]["grads"], 6) == \
            S.grad_errors(new[lm]["grads"], var[lm]["grads"])
        errs = S.grad_errors(new[lm]["grads"], old[lm]["grads"], 6)
        assert max(e for e, k in errs.values() if k == "rel") <= 1e-12


def test_what_is_not_built_is_refused_at_construction_by_name():
    from clskd import config as cfg
    from clskd.model import DCCRN
    ok = dict(masking_mode="E", use_clstm=True, rnn_units=64)
    with pytest.raises(NotImplementedError, match="kernel_num.*multiple of 8"):
        DCCRN(kernel_num=[8, 12, 32, 64, 64, 64], **ok)
    with pytest.raises(NotImplementedError, match="kernel_num.*multiple of 8"):
        DCCRN(kernel_num=[8, 16, 32, 64, 64, 4], **ok)
    with pytest.raises(NotImplementedError, match="rnn_units=96"):
        DCCRN(kernel_num=cfg.kernel_num_student, masking_mode="E", use_clstm=True, rnn_units=96)
    with pytest.raises(NotImplementedError, match="rnn_units=512"):
        DCCRN(kernel_num=cfg.kernel_num_student, masking_mode="E", use_clstm=True, rnn_units=512)
    with pytest.raises(NotImplementedError, match="kernel_num has 9 entries"):
        DCCRN(kernel_num=[8] * 9, **ok)
    with pytest.raises(NotImplementedError, match="kernel_num has 0 entries"):
        DCCRN(kernel_num=[], **ok)
    with pytest.raises(NotImplementedError, match="rnn_layers=0"):
        DCCRN(kernel_num=cfg.kernel_num_student, rnn_layers=0, **ok)
    # what constructed before still constructs: the shipped pair, the eight-layer limit, the
    # reference's default widths, every built hidden size on either stack
    for kw in (cfg.STUDENT, cfg.TEACHER):
        DCCRN(masking_mode="E", use_clstm=True, **kw)
    assert DCCRN(kernel_num=[8] * 8, **ok).hidden_dim == 1
    for ru in (32, 64, 128, 256):
        DCCRN(kernel_num=cfg.kernel_num_student, masking_mode="E", use_clstm=True, rnn_units=ru)
    for name in C.NAMES:
        DCCRN(**C.ctor(name))


def test_supervised_training_names_the_real_lstm_configuration_it_refuses():
    """default_real missed the gradient gate on the GPU: SupervisedTraining
    refuses it by name and keeps the student widths on the real LSTM and the other cases."""
    from clskd import config as cfg
    from clskd.model import DCCRN
    from clskd.supervised import SupervisedTraining
    with pytest.raises(NotImplementedError, match=r"use_clstm=False.*kernel_num \[16, 32, 64, 128, 256, 256\]"):
        SupervisedTraining(C.model("default_real"), "SI-SNR")
    with pytest.raises(NotImplementedError, match="rnn_units 128"):
        SupervisedTraining(DCCRN(masking_mode="E", use_clstm=False, kernel_num=cfg.kernel_num_student,
                                 rnn_units=128), "MSE")
    with pytest.raises(NotImplementedError, match="teacher"):
        SupervisedTraining(DCCRN(masking_mode="E", use_clstm=True, **cfg.TEACHER), "MSE")
    SupervisedTraining(DCCRN(masking_mode="C", use_clstm=False, **cfg.STUDENT), "SI-SNR+LMS")
    for name in ("odd6", "deep7", "five3"):
        SupervisedTraining(C.model(name), C.GRAD_MODES[name][0])
