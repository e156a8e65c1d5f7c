"""CPU checks of the DCCRN variants (masking modes 'C' / 'R', use_clstm=False): the float64
restatement (tests/variants_ref.py) against what the reference's own models wrote
(tests/golden/gen_variants.py), the parameter tables, construction and recipe loading of the four
(masking_mode, use_clstm) combinations, the choice of the end-to-end seeds, and every refusal.

Bounds.  The reference's loss value: 1e-6 relative (~8 float32 ulps of the result).  Its tensors
and gradients: the suite's rule (kernel_refs.tolerance) with e32 = the distance of
the restatement's own float32 evaluation from its float64 one — the reference's values are float32
evaluations of the same formulas in another summation order."""
import numpy as np
import pytest
import torch

import kernel_refs as KR
import sup_loss_ref as S
import variants_ref as V

f32, f64 = torch.float32, torch.float64
GRAD_GATE, ZERO_GATE, LOSS_GATE = 2e-3, 1e-3, 5e-5


def _model(variant, use_cbn=False, **kw):
    from clskd import config as cfg
    from clskd.model import DCCRN
    return DCCRN(masking_mode=variant[0], use_clstm=variant[1], use_cbn=use_cbn,
                 **{**cfg.STUDENT, **kw})


@pytest.mark.parametrize("variant", V.FIXTURE_VARIANTS, ids=V.tag)
def test_restatement_matches_the_reference_fixture(variant):
    fx = V.fixture(variant)
    x, y = S.seeded_batch(**V.e2e(variant))
    for tm in ("train", "eval"):
        res = {}
        for dt in (f64, f32):
            with S.oracle_dtype(dt) as R, torch.no_grad():
                res[dt] = V.dccrn_forward(V.params(dt, variant[1], grad=False), x.to(dt), *variant,
                                          train=tm == "train", lstm_fn=R.lstm)
        assert float(res[f64]["pre_clamp"].abs().max()) < 0.99  # nothing clamps
        for k in V.OUTPUTS:
            ref = torch.from_numpy(fx[f"{tm}/{k}"]).double()
            e32, tol = KR.tolerance(res[f64][k], res[f32][k])
            err = float((ref - res[f64][k]).abs().max())
            print(f"VARREF {V.tag(variant)} {tm} {k:9s} rel-L2 {V.rel(ref, res[f64][k]):.2e} "
                  f"e32={e32:.2e} err={err:.2e} tol={tol:.2e}")
            assert err <= tol, (variant, tm, k, err, tol)
    # the reference's loss and its float32 autograd gradients
    lm = V.FIXTURE_LOSS[variant]
    r64, r32 = V.steps(variant, (lm,), x, y, f64)[lm], V.steps(variant, (lm,), x, y, f32)[lm]
    ref = float(fx["loss"])
    assert abs(float(r64["loss"]) - ref) <= 1e-6 * abs(ref), (float(r64["loss"]), ref)
    for n in V.fixture_grads(variant):
        g64, g32 = r64["grads"][n], r32["grads"][n]
        e32, tol = KR.tolerance(g64, g32)
        err = float((torch.from_numpy(fx[f"grad/{n}"]).double() - g64).abs().max())
        print(f"VARREF {V.tag(variant)} {lm} d {n} e32={e32:.2e} err={err:.2e} tol={tol:.2e}")
        assert err <= tol, (variant, n, err, tol)


@pytest.mark.parametrize("variant", V.FIXTURE_VARIANTS, ids=V.tag)
def test_variants_construct_with_the_references_keys_and_load_the_recipe(variant):
    from clskd import config as cfg
    from clskd.weights import STUDENT_SEED, apply_recipe, recipe_state_dict
    fx = V.fixture(variant)
    m = _model(variant)
    assert m.masking_mode == variant[0] and m.use_clstm is variant[1]
    keys = [k for k in m.state_dict() if not k.startswith(("stft.", "istft."))]
    shapes = cfg.dccrn_param_shapes(use_clstm=variant[1], **cfg.STUDENT)
    assert keys == list(shapes) == [str(k) for k in fx["keys"]]
    assert all(tuple(m.state_dict()[k].shape) == tuple(shapes[k]) for k in keys)
    apply_recipe(m, STUDENT_SEED)
    sd = recipe_state_dict(shapes, STUDENT_SEED)
    for k in keys:
        assert np.array_equal(m.state_dict()[k].numpy(), sd[k]), k
    if not variant[1]:
        assert isinstance(m.enhance, torch.nn.LSTM) and m.enhance.num_layers == 2
        assert isinstance(m.tranform, torch.nn.Linear)
        assert set(V.REAL_LSTM_KEYS) <= set(keys)
        assert tuple(shapes["enhance.weight_ih_l0"]) == (256, 256)
        assert tuple(shapes["tranform.weight"]) == (256, 64)
        for k in V.REAL_LSTM_KEYS:  # U(+-1/sqrt(H)) with H = 64 = in_features of `tranform`
            assert 0.1 < float(np.abs(sd[k]).max()) <= 0.125, k
        assert _model(variant, rnn_layers=3).enhance.num_layers == 2  # DCCRN.py:101-108


def test_the_references_default_constructor_arguments_are_accepted_or_named():
    """DCCRN() as the reference's callers write it (use_clstm=False, masking_mode='E') builds for
    the hidden sizes of the recurrence and names rnn_units otherwise (256: its own default)."""
    from clskd.model import DCCRN
    from clskd import config as cfg
    for H in (16, 32, 64, 128):
        assert DCCRN(rnn_units=H, kernel_num=cfg.kernel_num_student).enhance.hidden_size == H
    for H in (256, 48):
        with pytest.raises(NotImplementedError, match="rnn_units") as e:
            DCCRN(rnn_units=H, use_clstm=False, kernel_num=cfg.kernel_num_student)
        assert "16, 32, 64, 128" in str(e.value)
    with pytest.raises(NotImplementedError, match="rnn_units"):
        DCCRN()
    with pytest.raises(NotImplementedError, match="masking_mode"):
        DCCRN(masking_mode="X", use_clstm=True)
    # the pairing that stays refused (tests/test_abi.py holds it): mask 'C' on the complex stack
    with pytest.raises(NotImplementedError, match="masking_mode='C'"):
        DCCRN(masking_mode="C", use_clstm=True, kernel_num=cfg.kernel_num_student, rnn_units=64)
    with pytest.raises(NotImplementedError, match="kernel_size"):
        DCCRN(kernel_size=3, use_clstm=True)
    with pytest.raises(NotImplementedError):
        DCCRN(use_clstm=True, win_len=320)


@pytest.mark.parametrize("variant", V.VARIANTS, ids=V.tag)
def test_the_end_to_end_seed_is_the_widest_margin_and_qualifies(variant):
    """The float32 evaluation of the reference passes the device gates at the chosen seed, and no
    seed of 1..8 has a margin more than twice as wide (the margins of the best seeds are a few
    float32 roundings apart, so their order may differ between CPUs; profiles/
    variants_grad_parity.txt keeps one run's table)."""
    table = V.seed_margins(variant)
    for s, (w, n, dl, wz) in table.items():
        print(f"VARSEED {V.tag(variant)} seed {s} worst {w:.2e} ({n}) dloss {dl:.2e} zero {wz:.2e}")
    w, n, dl, wz = table[V.SEEDS[variant]]
    assert w <= 0.1 * GRAD_GATE and dl <= 0.1 * LOSS_GATE and wz <= 0.01 * ZERO_GATE, (w, n, dl, wz)
    assert w <= 2 * min(v[0] for v in table.values())
    r64 = V.e2e_reference(variant)
    y = S.seeded_batch(**V.e2e(variant))[1].double()
    for lm, r in r64.items():
        assert all(g is not None and torch.isfinite(g).all() for g in r["grads"].values()), lm
        assert float(r["pre_clamp"].abs().max()) < 0.99
        assert -35.0 <= -float(S.dccrn_loss("SI-SDR", r["wav"], y)) <= 20.0
    if not variant[1]:
        assert set(V.REAL_LSTM_KEYS) <= set(r64[V.STEP_MODES[variant][0]]["grads"])


def _refused(match, fn):
    with pytest.raises(NotImplementedError, match=match):
        fn()


@pytest.mark.parametrize("variant", [("R", True), ("E", False)], ids=V.tag)
def test_unsupported_consumers_name_the_option(variant):
    from clskd import config as cfg
    from clskd.distill import KnowledgeDistillation, SPKDDistillation
    from clskd.distill_mini import OutputDistillation
    from clskd.feature_extraction import DCCRN as Taps
    from clskd.graph import StepGraph
    from clskd.model import DCCRN
    from clskd.streaming import FusedStreamingDCCRN, StreamingDCCRN
    name = "use_clstm" if not variant[1] else "masking_mode"
    new, old = _model(variant).eval(), DCCRN(masking_mode="E", use_clstm=True, **cfg.STUDENT)
    for cls in (KnowledgeDistillation, SPKDDistillation):
        _refused(name, lambda: cls(old, new))
        _refused(name, lambda: cls(new, old))
    _refused(name, lambda: OutputDistillation(new, None))
    _refused(name, lambda: FusedStreamingDCCRN(new, 1))
    kd = KnowledgeDistillation(DCCRN(masking_mode="E", use_clstm=True, **cfg.TEACHER), old)
    kd.student = new  # a step object whose student was swapped afterwards
    _refused(name, lambda: StepGraph(kd, torch.zeros(1, 1600), torch.zeros(1, 1600)))
    if not variant[1]:
        _refused(name, lambda: StreamingDCCRN(new, 1))
        _refused(name, lambda: Taps(new))
        _refused(name, lambda: new.run(torch.zeros(1, 1600), train=False, gram_taps=[]))
    new.compute = "bf16"  # a 16-bit compute mode (refused before the device is touched)
    _refused(name, lambda: new.run(torch.zeros(1, 1600), train=False))
