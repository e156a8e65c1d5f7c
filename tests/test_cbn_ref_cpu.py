"""CPU checks for ComplexBatchNorm: the restatement (tests/cbn_ref.py) against what the
reference's own layer and model computed (tests/golden/cbn.npz, written by
tests/golden/gen_cbn.py), the module tree / key order / recipe of clskd.DCCRN(use_cbn=True), the
new ABI symbols, and the qualification of the GPU tests' inputs: the restatement's own float32
evaluation stays inside the device gates (tests/test_gpu_cbn.py, tests/test_gpu_cbn_kernels.py)
with margin, so a device miss is the device's.

Bounds.  The layer record is float64 on both sides: 1e-12 absolute on values of order 1 is ~4,500
float64 ulps, room for the two sides' different summation orders over 42 rows and nothing else.
The model's out_wav is the reference's float32; the float64 restatement is held to it by the
forward gate tests/test_gpu_parity.py holds the BatchNorm model to (rms 1e-5, max 1e-4)."""
import numpy as np
import pytest
import torch

import cbn_ref as CR
import sup_loss_ref as S

f32, f64 = torch.float32, torch.float64
GRAD_GATE, ZERO_GATE, LOSS_GATE = 2e-3, 1e-3, 5e-5  # tests/test_gpu_supervised.py
KERNEL_GATE = 1e-5  # tests/test_gpu_backward.py: bn_bwd


def test_layer_restatement_matches_the_reference_fixture():
    fx = CR.fixture()
    x = torch.from_numpy(fx["layer/x"])
    assert torch.equal(x, CR.layer_input().double())
    p = CR.layer_params(x.shape[1] // 2)
    y = CR.complex_batch_norm(x, p, "layer.", train=True, update_stats=True)
    e = float((y - torch.from_numpy(fx["layer/y_train"])).abs().max())
    print(f"CBNREF layer train max abs {e:.2e}")
    assert e <= 1e-12
    for k in CR.CBN_BUFFERS:
        eb = float((p["layer." + k] - torch.from_numpy(fx[f"layer/{k}"])).abs().max())
        print(f"CBNREF layer {k} max abs {eb:.2e}")
        assert eb <= 1e-12, k
    ye = CR.complex_batch_norm(x, p, "layer.", train=False)
    ee = float((ye - torch.from_numpy(fx["layer/y_eval"])).abs().max())
    print(f"CBNREF layer eval max abs {ee:.2e}")
    assert ee <= 1e-12


@pytest.mark.parametrize("mode", ["train", "eval"])
def test_model_restatement_matches_the_reference_fixture(mode):
    fx = CR.fixture()
    x, _ = S.seeded_batch(**CR.E2E)
    with S.oracle_dtype(f64):
        with torch.no_grad():
            wav = CR.dccrn_forward_cbn(CR.cbn_params(f64, grad=False), x.double(),
                                       train=mode == "train")["out_wav"]
    ref = fx[f"model/out_wav_{mode}"].astype(np.float64)
    d = wav.numpy() - ref
    print(f"CBNREF model {mode} rms {np.sqrt(np.mean(d * d)):.2e} max {np.abs(d).max():.2e}")
    assert np.sqrt(np.mean(d * d)) <= 1e-5 and np.abs(d).max() <= 1e-4
    assert np.abs(ref).max() < 0.99  # nothing clamps


def test_module_tree_keys_and_recipe():
    from clskd import config as cfg
    from clskd.model import DCCRN, ComplexBatchNorm
    from clskd.weights import STUDENT_SEED, apply_recipe, recipe_state_dict
    fx = CR.fixture()
    torch.manual_seed(0)
    m = DCCRN(masking_mode="E", use_clstm=True, use_cbn=True, **cfg.STUDENT)
    keys = [k for k in m.state_dict() if not k.startswith(("stft.", "istft."))]
    shapes = cfg.dccrn_param_shapes(use_cbn=True, **cfg.STUDENT)
    assert keys == list(shapes) == [str(k) for k in fx["model/keys"]]
    assert all(tuple(m.state_dict()[k].shape) == tuple(shapes[k]) for k in keys)
    layer = m.encoder[0][1]
    assert isinstance(layer, ComplexBatchNorm) and layer.num_features == 4
    # the reference's init (tools_for_model.py:385-392)
    assert torch.all(layer.Wrr == 1) and torch.all(layer.Wii == 1) and torch.all(layer.Br == 0)
    assert 0 < float(layer.Wri.detach().abs().max()) <= 0.9
    assert torch.all(layer.RVrr == 1) and torch.all(layer.RVri == 0) and torch.all(layer.RMr == 0)
    assert not any(isinstance(x, torch.nn.BatchNorm2d) for x in m.modules())
    apply_recipe(m, STUDENT_SEED)
    sd = recipe_state_dict(shapes, STUDENT_SEED)
    for k in keys:
        assert np.array_equal(m.state_dict()[k].numpy(), sd[k]), k
    # the running V of the recipe is positive definite, Wri inside the reference's range
    for k in keys:
        if k.endswith("RVri"):
            pre = k[:-4]
            assert np.all(sd[pre + "RVrr"] * sd[pre + "RVii"] - sd[k] ** 2 > 0.5)
        if k.endswith("Wri"):
            assert np.abs(sd[k]).max() <= 0.9
    # everything else the constructor refuses stays refused
    for kw in (dict(masking_mode="C"), dict(use_clstm=False), dict(kernel_size=3)):
        with pytest.raises(NotImplementedError):
            DCCRN(**{**dict(masking_mode="E", use_clstm=True, use_cbn=True), **kw})


# sha256 over (key, raw bytes) in key order of the recipe, taken from the commit before the
# ComplexBatchNorm rules were added to clskd.weights
RECIPE_SHA256 = {
    "student": "0eaa43c2eecdc59cad34ca65b8b4a82e1a4f0f4a6b54ddc041266338b8f22965",
    "teacher": "df7358fb5b96f2b6d262abf02c6970f723121bc1585acea5956d7e20114a8326",
    "abf": "9022c7bb3133f162c27a93ec3e9bbf98208a736afcbea4f282098cef730a095f",
}


def test_recipe_of_the_batchnorm_models_is_unchanged():
    """Existing keys keep their exact values."""
    import hashlib

    from clskd import config as cfg
    from clskd.weights import ABF_SEED, STUDENT_SEED, TEACHER_SEED, recipe_state_dict
    cases = {
        "student": (cfg.dccrn_param_shapes(**cfg.STUDENT), STUDENT_SEED),
        "teacher": (cfg.dccrn_param_shapes(**cfg.TEACHER), TEACHER_SEED),
        "abf": ({**cfg.review_param_shapes("encoder"), **cfg.review_param_shapes("decoder")},
                ABF_SEED),
    }
    for name, (shapes, seed) in cases.items():
        assert not any(k.rsplit(".", 1)[-1] in CR.CBN_PARAMS + CR.CBN_BUFFERS for k in shapes)
        h = hashlib.sha256()
        for k, v in recipe_state_dict(shapes, seed).items():
            h.update(k.encode())
            h.update(np.ascontiguousarray(v).tobytes())
        assert h.hexdigest() == RECIPE_SHA256[name], name


def test_abi_symbols_present():
    from clskd import _lib
    lib = _lib.load(require_gpu=False)
    for name in ("clskd_cbn_stats_blocks", "clskd_cbn_stats_partial", "clskd_cbn_finalize",
                 "clskd_cbn_eval_coeffs", "clskd_cbn_apply", "clskd_cbn_bwd_blocks",
                 "clskd_cbn_bwd_workspace", "clskd_cbn_bwd"):
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    assert lib.clskd_cbn_bwd_workspace(3, 8) == 3 * 4 * 7 + 4 + 18
    assert lib.clskd_cbn_stats_blocks(42, 8) == 1 and lib.clskd_cbn_bwd_blocks(4864, 8) == 5
    # argument validation happens before any launch (no GPU needed): C must be a multiple of 8
    assert lib.clskd_cbn_apply(16, 16, 4, 12, 16, None, None) != 0
    assert b"cbn_apply" in lib.clskd_last_error()


# ------------------------------------------------------------------------------------------
# qualification of the GPU tests' inputs
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", CR.KERNEL_SHAPES)
def test_kernel_inputs_qualify(shape):
    """float32 against float64 evaluation of the restatement on the kernel tests' inputs: every
    gated tensor at most 1e-6, a tenth of the 1e-5 gate.  The scalar dalpha is a cancelling sum
    (|sum| is 0.1 - 5 % of the sum of |terms| with dy = N) where torch's float32 summation alone
    sits at up to 7e-6: it is held to the gate itself here; the device accumulates it in
    float64."""
    worst = 0.0
    for i, rho in enumerate(CR.RHOS):
        x, dy, p = CR.kernel_case(shape, rho, seed=i)
        r64 = CR.kernel_reference(x, dy, p, 0.25)
        r32 = CR.kernel_reference(x, dy, p, 0.25, dtype=f32)
        for k, v in r64.items():
            e = CR.rel(r32[k], v)
            worst = max(worst, e)
            assert e <= (KERNEL_GATE if k == "dalpha" else 0.1 * KERNEL_GATE), (shape, rho, k, e)
        # the inputs exercise both PReLU branches and a correlated V
        assert 0.2 < float((r64["y"] < 0).double().mean()) < 0.8
        if rho:
            assert float((r64["Vri"] / (r64["Vrr"] * r64["Vii"]).sqrt()).abs().min()) > 0.3
    print(f"CBNQUAL kernel {shape} worst float32-vs-float64 {worst:.2e}")


def test_e2e_inputs_qualify():
    """The restatement's float32 evaluation at the end-to-end inputs against its float64 one, all
    nine DCCRN.loss modes: inside the device gates with at least a factor 10 on the parameter
    tensors; the analytically-zero pre-normalisation conv biases far inside theirs; nothing
    clamps.  'MRSTFT' is recorded only: it does not qualify for the gradient gate."""
    r64, r32 = CR.e2e_reference(f64), CR.e2e_reference(f32)
    assert float(r64["MSE"]["wav"].abs().max()) < 0.99
    for mode in CR.ALL_MODES:
        errs = S.grad_errors(r32[mode]["grads"], r64[mode]["grads"])
        worst = max(errs.items(), key=lambda kv: kv[1][0] if kv[1][1] == "rel" else 0)
        zero = max((e for e, k in errs.values() if k == "zero"), default=0.0)
        dl = abs(float(r32[mode]["loss"]) - float(r64[mode]["loss"])) / abs(float(r64[mode]["loss"]))
        print(f"CBNQUAL e2e {mode:14s} loss {dl:.2e} worst {worst[0]} {worst[1][0]:.2e} "
              f"zero-bias {zero:.2e}")
        assert dl <= 0.1 * LOSS_GATE
        if mode in CR.GRAD_MODES:
            assert worst[1][0] <= 0.1 * GRAD_GATE, (mode, worst)
            assert zero <= 0.01 * ZERO_GATE, (mode, zero)
    names = set(r64["MSE"]["grads"])
    assert {"encoder.0.1.Wri", "decoder.4.1.Bi", "encoder.5.2.weight"} <= names
    assert not any(k.rsplit(".", 1)[-1] in CR.CBN_BUFFERS for k in names)
