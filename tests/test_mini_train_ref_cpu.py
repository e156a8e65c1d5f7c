"""CPU checks of the DCCRNet_mini training-step references (tests/mini_train_ref.py): the step
reference is complete and finite, its float32 evaluation passes the device gates
(2e-3 relative L2 per gradient tensor, tests/test_gpu_backward.py; 5e-5 relative on the loss,
DESIGN §4), and the closed forms of the three kernels agree with finite differences."""
import pytest
import torch

import mini_train_ref as M

f64 = torch.float64


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


# (kd, B, L, seed): the shapes and seeds of the device gradient cases (tests/test_gpu_mini_backward.py)
CASES = [("spkd", 3, 1600, 1), ("mse", 3, 1600, 1), ("stft", 3, 1600, 1), ("spkd", 2, 1250, 2)]


@pytest.mark.parametrize("kd,B,L,seed", CASES)
def test_step_reference_is_complete_and_float32_passes_the_gates(kd, B, L, seed):
    """The device step is another float32 evaluation of this reference, so the gates are
    attainable on these inputs only if torch's float32 evaluation of the reference itself
    passes them on every one of the 112 tensors — the one-element ones (22 PReLU slopes, two
    output biases: sums over a whole map with cancellation) included.  This is what qualifies
    M.seeded_batch as the input of the device test."""
    x, y, t = M.seeded_batch(B, L, seed=seed)
    r64, r32 = M.reference_step(kd, x, y, t, f64), M.reference_step(kd, x, y, t, torch.float32)
    assert len(r64["grads"]) == 112
    worst = ("", 0.0)
    for k, g in r64["grads"].items():
        assert torch.isfinite(g).all() and g.abs().max() > 0, k
        worst = max(worst, (k, _rel(r32["grads"][k], g)), key=lambda v: v[1])
    dl = abs(float(r32["loss"]) - float(r64["loss"])) / abs(float(r64["loss"]))
    print(f"MINIREF {kd} B{B} L{L} loss={float(r64['loss']):.6f} dloss={dl:.2e} worst={worst[0]} {worst[1]:.2e}")
    assert worst[1] <= 2e-3, worst
    assert dl <= 5e-5


def test_one_frame_at_the_lstm_gives_exactly_zero_recurrent_weight_gradients():
    """L = 1000: T = 7, one frame at the last encoder, so h_{t-1} is the zero initial state."""
    x, y, t = M.seeded_batch(2, 1000, seed=2)
    r = M.reference_step("mse", x, y, t, f64)
    hh = [k for k in r["grads"] if k.endswith("weight_hh_l0")]
    assert len(hh) == 4
    for k in hh:
        assert (r["grads"][k] == 0).all(), k
    ih = [k for k in r["grads"] if k.endswith("weight_ih_l0") and ".rnns.0." in k]
    assert all(r["grads"][k].abs().max() > 0 for k in ih)


def _fd(fn, x, idx, h=1e-6):
    xp, xm = x.clone(), x.clone()
    xp[idx] += h
    xm[idx] -= h
    return (fn(xp) - fn(xm)) / (2 * h)


def _mask_case(B=2, T=5, Tm=7, seed=3):
    g = torch.Generator().manual_seed(seed)
    spec = torch.randn(B, T, 514, generator=g, dtype=f64)
    dest = torch.randn(B, T, 516, generator=g, dtype=f64)
    r = 0.05 + 2.95 * torch.rand(B, 256, Tm, generator=g, dtype=f64)
    th = 6.283185307179586 * torch.rand(B, 256, Tm, generator=g, dtype=f64)
    mask = torch.stack([r * torch.cos(th), r * torch.sin(th)], -1)
    return spec, mask, T, dest


def test_mask_reference_against_finite_differences_and_its_limit_at_zero():
    spec, mask, T, dest = _mask_case()
    dm = M.mask_bdt_bwd(spec, mask, T, dest)
    assert (dm[:, :, T:] == 0).all()

    def loss(m):
        sr, si = spec[:, :, 0:256].transpose(1, 2), spec[:, :, 257:513].transpose(1, 2)
        er, ei = M.bound_mask_apply(m[:, :, :T, 0], m[:, :, :T, 1], sr, si)
        return ((er * dest[:, :, 0:256].transpose(1, 2)).sum()
                + (ei * dest[:, :, 257:513].transpose(1, 2)).sum())

    for idx in [(0, 0, 0, 0), (1, 255, 4, 1), (0, 17, 2, 1), (1, 100, 3, 0)]:
        fd = _fd(loss, mask, idx)
        assert abs(float(fd) - float(dm[idx])) <= 1e-7 * max(1.0, abs(float(dm[idx]))), idx
    # r -> 0: the Jacobian tends to the identity, so the gradient tends to g = conj(X) dest —
    # the value the reference (and the kernel) write at r = 0 exactly
    m0 = mask.clone()
    m0[0, 5, 1] = 0.0
    g = M.mask_bdt_bwd(spec, m0, T, dest)[0, 5, 1]
    assert torch.isfinite(g).all()
    prev = None
    for eps in (1e-2, 1e-3, 1e-4):
        me = mask.clone()
        me[0, 5, 1, 0], me[0, 5, 1, 1] = 0.6 * eps, -0.8 * eps
        d = (M.mask_bdt_bwd(spec, me, T, dest)[0, 5, 1] - g).abs().max()
        assert d <= 2.0 * eps * eps * g.abs().max()  # tanh(r) / r = 1 - r^2 / 3 + ...
        assert prev is None or d < prev
        prev = d


def test_bn_reim_reference_against_finite_differences():
    g = torch.Generator().manual_seed(4)
    rows, C = 37, 8
    x = torch.randn(rows, C, generator=g, dtype=f64) * 1.5 + 0.3
    dy = torch.randn(rows, C, generator=g, dtype=f64)
    gamma = 0.5 + torch.rand(C, generator=g, dtype=f64)
    beta = 0.2 * torch.randn(C, generator=g, dtype=f64)
    alpha = torch.tensor([0.25, 0.05], dtype=f64)
    dx, dg, db, da, yb = M.bn_reim_bwd(x, dy, gamma, beta, alpha)
    assert yb.abs().min() > 1e-4  # no element at the PReLU gate: the differences are smooth
    f = lambda **kw: (M.bn_reim_forward(kw.get("x", x), kw.get("gamma", gamma),  # noqa: E731
                                        kw.get("beta", beta), kw.get("alpha", alpha))[0] * dy).sum()
    for idx in [(0, 0), (36, 7), (11, 4)]:
        assert abs(float(_fd(lambda v: f(x=v), x, idx)) - float(dx[idx])) <= 1e-7
    for c in (0, 3, 4, 7):
        assert abs(float(_fd(lambda v: f(gamma=v), gamma, c)) - float(dg[c])) <= 1e-7
        assert abs(float(_fd(lambda v: f(beta=v), beta, c)) - float(db[c])) <= 1e-7
    for k in (0, 1):
        assert abs(float(_fd(lambda v: f(alpha=v), alpha, k)) - float(da[k])) <= 1e-7
    # one slope for both halves is a different function
    dx1 = M.bn_reim_bwd(x, dy, gamma, beta, torch.tensor([0.25, 0.25], dtype=f64))[0]
    assert (dx1[:, :C // 2] == dx[:, :C // 2]).all() and (dx1 - dx).abs().max() > 1e-3
    sc, sh, mean, var = M.bn_coefficients(x, gamma, beta)
    assert torch.allclose(x * sc + sh, yb, rtol=0, atol=1e-12)


def test_mse_reference_against_finite_differences():
    g = torch.Generator().manual_seed(5)
    a = torch.randn(1027, generator=g, dtype=f64)
    b = torch.randn(1027, generator=g, dtype=f64)
    loss, da = M.mse_loss_grad(a, b, scale=0.7)
    assert abs(float(loss) - 0.7 * float(((a - b) ** 2).mean())) <= 1e-14
    for i in (0, 513, 1026):
        fd = _fd(lambda v: M.mse_loss_grad(v, b, 0.7)[0], a, i)
        assert abs(float(fd) - float(da[i])) <= 1e-9
