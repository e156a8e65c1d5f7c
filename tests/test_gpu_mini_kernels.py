"""GPU: the three kernels of the DCCRNet_mini backward (csrc/mini_bwd.hip; the OnReIm BatchNorm
pair is clskd_bn_bwd_reim in csrc/norm_bwd.hip) against the float64 closed forms of
tests/mini_train_ref.py, under the suite's one tolerance rule (tests/kernel_refs.py:tolerance):
every element within 8 * e32 + 4 * 2^-24 * max|ref64|, e32 the distance of the same torch
expression in float32 from float64; sums of float32 terms with the sum of the terms' magnitudes
as the scale.  Each case prints `MINIK case e32 err tol`."""
import pytest
import torch

import kernel_refs as R
import mini_train_ref as M

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
f32, f64 = torch.float32, torch.float64


def _check(case, got, ref64, ref32, keep=None, scale=None):
    e32, tol = R.tolerance(ref64, ref32, keep, 8.0, scale)
    err = (got.detach().double().cpu() - ref64).abs()
    tol_t = torch.broadcast_to(torch.as_tensor(tol, dtype=f64), err.shape)
    if keep is not None:
        err, tol_t = err[keep], tol_t[keep]
    err, tol_t = err.reshape(-1), tol_t.reshape(-1)
    i = int(torch.argmax(err / tol_t))
    print(f"MINIK {case} e32={e32:.3e} err={err[i].item():.3e} tol={tol_t[i].item():.3e}")
    assert torch.isfinite(err).all(), case
    assert (err <= tol_t).all(), (case, e32, err[i].item(), tol_t[i].item())


# ------------------------------------------------------------------------------------------
# mask_bdt_bwd
# ------------------------------------------------------------------------------------------
SENTINEL = 1.0e6


@pytest.mark.parametrize("B,T", [(1, 1), (2, 5), (2, 16), (3, 19)])
@pytest.mark.parametrize("extra", [0, 2])
def test_mask_bdt_bwd_against_fp64(B, T, extra):
    """(1, 1); (2, 5); one full 16-frame tile; a tile plus a ragged one.  Tm = T and T + 2 (the
    extra columns get zero); ldest = 516 with the Nyquist columns (256, 513) and the tail holding
    a sentinel that must not reach dmask; one element at r = 0 must equal g = conj(X) dest."""
    from clskd import ops
    Tm = T + extra
    g = torch.Generator().manual_seed(100 * B + T + extra)
    spec = torch.randn(B, T, 514, generator=g)
    dest = torch.randn(B, T, 516, generator=g)
    dest[:, :, 256] = SENTINEL
    dest[:, :, 513:] = SENTINEL
    r = 0.05 + 2.95 * torch.rand(B, 256, Tm, generator=g)
    th = 6.2831853 * torch.rand(B, 256, Tm, generator=g)
    mask = torch.stack([r * torch.cos(th), r * torch.sin(th)], -1).contiguous()
    b0, f0, t0 = B - 1, 37, T - 1
    mask[b0, f0, t0] = 0.0
    ref64 = M.mask_bdt_bwd(spec.double(), mask.double(), T, dest.double())
    ref32 = M.mask_bdt_bwd(spec, mask, T, dest)
    dmask = torch.full(mask.shape, 9.0, device=DEV)
    ops.mask_bdt_bwd(spec.to(DEV), mask.to(DEV), T, dest.to(DEV), dmask)
    torch.cuda.synchronize()
    _check(f"mask_bdt_bwd/B{B}T{T}Tm{Tm}", dmask, ref64, ref32)
    if extra:
        assert (dmask[:, :, T:] == 0).all()
    # r = 0: g, to float32 rounding of its two products
    xr, xi = spec[b0, t0, f0].double(), spec[b0, t0, 257 + f0].double()
    dr, di = dest[b0, t0, f0].double(), dest[b0, t0, 257 + f0].double()
    gz = torch.stack([xr * dr + xi * di, xr * di - xi * dr])
    got = dmask[b0, f0, t0].double().cpu()
    assert torch.equal(ref64[b0, f0, t0], gz)
    assert (got - gz).abs().max() <= 4 * 2.0 ** -24 * (abs(xr * dr) + abs(xi * di) + abs(xr * di) + abs(xi * dr))
    assert dmask.abs().max() < 1e3  # no sentinel


# ------------------------------------------------------------------------------------------
# bn_bwd_reim
# ------------------------------------------------------------------------------------------
GATE_MARGIN = 1e-5  # |y_bn|: the float32 distance of the PReLU gate's decision value from 0


def _bn_case(rows, C, seed):
    """Inputs whose float64 reference alone decides the gate: dy is zero on the elements with
    |y_bn| inside the margin (they then contribute nothing on either side of the gate)."""
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(rows, C, generator=g) * (0.5 + torch.rand(C, generator=g)) + 0.3 * torch.randn(C, generator=g))
    dy = torch.randn(rows, C, generator=g)
    gamma = 0.5 + torch.rand(C, generator=g)
    beta = 0.3 * torch.randn(C, generator=g)
    alpha = torch.tensor([0.25, 0.05])
    yb = M.bn_reim_forward(x.double(), gamma.double(), beta.double(), alpha.double())[1]
    keep = yb.abs() >= GATE_MARGIN
    assert (~keep).double().mean() < 0.01
    dy = dy * keep
    return x, dy, gamma, beta, alpha, keep


BN_SHAPES = [(7, 8), (1030, 16), (4099, 64), (9, 4), (1030, 24), (515, 40)]


@pytest.mark.parametrize("rows,C", BN_SHAPES)
@pytest.mark.parametrize("acc_dx,acc_p", [(False, False), (True, False), (False, True), (True, True)])
def test_bn_bwd_reim_against_fp64(rows, C, acc_dx, acc_p):
    """Slopes 0.25 (re half) and 0.05 (im half): one slope for both halves fails.  One block, a
    ragged pair of blocks and nine blocks of the reduce; C = 4 (one quad per row, a quad that
    spans both halves), C = 24 and C = 40 (256 is no multiple of the quads per row: idle threads
    behind the reduce's row-lane guard); accumulate_dx / accumulate_params each on and off (onto
    seeded buffers)."""
    from clskd import ops
    x, dy, gamma, beta, alpha, keep = _bn_case(rows, C, 7 * rows + C)
    sc, sh, mean, var = M.bn_coefficients(x.double(), gamma.double(), beta.double())
    # the kernel receives float32 coefficients: the references run on exactly those inputs
    r64 = M.bn_reim_bwd(x.double(), dy.double(), gamma.double(), beta.double(), alpha.double())
    r32 = M.bn_reim_bwd(x, dy, gamma, beta, alpha)
    g = torch.Generator().manual_seed(5)
    dx0 = torch.randn(rows, C, generator=g)
    p0 = [torch.randn(C, generator=g), torch.randn(C, generator=g), torch.randn(2, generator=g)]
    dx = dx0.clone().to(DEV)
    dgam, dbet, dalp = [t.clone().to(DEV) for t in p0]
    dv = lambda t: t.float().to(DEV).contiguous()  # noqa: E731
    ops.bn_bwd_reim(dv(x), dv(dy), dv(sc), dv(sh), dv(mean), dv(var), 1e-5, dv(gamma), dv(alpha), dx,
                    dgam, dbet, dalp, accumulate_dx=acc_dx, accumulate_params=acc_p)
    torch.cuda.synchronize()
    tag = f"bn_bwd_reim/r{rows}C{C}a{int(acc_dx)}{int(acc_p)}"
    base = dx0.double() if acc_dx else 0.0
    _check(tag + "/dx", dx, r64[0] + base, r32[0].double() + base if acc_dx else r32[0], keep)
    # sums of float32 terms: scale = the sum of the terms' magnitudes, per channel / per half
    xh = (x.double() - mean) * torch.rsqrt(var + 1e-5)
    yb = r64[4]
    slope = torch.where(yb > 0, torch.ones_like(yb), torch.cat(
        [alpha[0].double().expand(rows, C // 2), alpha[1].double().expand(rows, C // 2)], 1))
    dz = dy.double() * slope
    mags = [(dz * xh).abs().sum(0), dz.abs().sum(0),
            torch.stack([t.sum() for t in ((yb * dy.double()).abs() * (yb <= 0)).split(C // 2, 1)])]
    for name, got, k, mag, p in (("dgamma", dgam, 1, mags[0], p0[0]), ("dbeta", dbet, 2, mags[1], p0[1]),
                                 ("dalpha", dalp, 3, mags[2], p0[2])):
        b = p.double() if acc_p else 0.0
        _check(f"{tag}/{name}", got, r64[k] + b, (r32[k].double() + b) if acc_p else r32[k],
               scale=mag + (p.double().abs() if acc_p else 0.0))


@pytest.mark.parametrize("rows,C", BN_SHAPES)
@pytest.mark.parametrize("acc", [False, True])
def test_bn_bwd_reim_equal_slopes_is_bn_bwd(rows, C, acc):
    """With one slope for both halves the OnReIm entry is clskd_bn_bwd: dx, dgamma and dbeta
    bit for bit (accumulating onto seeded buffers or not), and dalpha_re + dalpha_im = dalpha to
    three float32 roundings (the two halves' and their sum's, each <= 2^-24 relative: within
    2 * 2^-24 * (|dalpha_re| + |dalpha_im|); the bound carries a factor 2 of margin).  The slope
    gradients start from zero in both modes, so an accumulating call adds nothing to that count."""
    from clskd import ops
    x, dy, gamma, beta, _, _ = _bn_case(rows, C, 7 * rows + C)
    sc, sh, mean, var = M.bn_coefficients(x.double(), gamma.double(), beta.double())
    dv = lambda t: t.float().to(DEV).contiguous()  # noqa: E731
    args = [dv(t) for t in (x, dy, sc, sh, mean, var)]
    g = torch.Generator().manual_seed(5)
    dx0, dg0, db0 = torch.randn(rows, C, generator=g), torch.randn(C, generator=g), torch.randn(C, generator=g)
    outs = []
    for fn, alpha in ((ops.bn_bwd_reim, [0.25, 0.25]), (ops.bn_bwd, [0.25])):
        dx, dgam, dbet = dx0.clone().to(DEV), dg0.clone().to(DEV), db0.clone().to(DEV)
        dalp = torch.zeros(len(alpha), device=DEV)
        fn(*args, 1e-5, dv(gamma), torch.tensor(alpha, device=DEV), dx, dgam, dbet, dalp,
           accumulate_dx=acc, accumulate_params=acc)
        outs.append((dx, dgam, dbet, dalp))
    torch.cuda.synchronize()
    (dx2, dg2, db2, da2), (dx1, dg1, db1, da1) = outs
    assert torch.equal(dx2, dx1) and torch.equal(dg2, dg1) and torch.equal(db2, db1)
    da2, da1 = da2.double().cpu(), da1.double().cpu()
    err, tol = float((da2.sum() - da1[0]).abs()), float(4 * 2.0 ** -24 * da2.abs().sum())
    print(f"MINIK bn_bwd_reim=bn_bwd/r{rows}C{C}a{int(acc)}/dalpha err={err:.3e} tol={tol:.3e}")
    assert err <= tol, (err, tol)


# ------------------------------------------------------------------------------------------
# mse_loss_grad
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 3, 1027, 48000])
@pytest.mark.parametrize("acc", [False, True])
def test_mse_loss_grad_against_fp64(n, acc):
    """n = 1, 3 (tail only), 1027 (quads + a tail of 3), 48000 (several blocks); accumulate on
    and off; two calls give the same bits; an unaligned view takes the scalar path."""
    from clskd import ops
    g = torch.Generator().manual_seed(n)
    a, b = torch.randn(n, generator=g), torch.randn(n, generator=g)
    da0, l0 = torch.randn(n, generator=g), torch.randn(1, generator=g)
    scale = 0.7
    s32 = float(torch.tensor(scale, dtype=f32))
    l64, d64 = M.mse_loss_grad(a.double(), b.double(), s32)
    l32, d32 = M.mse_loss_grad(a, b, s32)
    outs = []
    for rep in range(2):
        da, loss = da0.clone().to(DEV), l0.clone().to(DEV)
        ops.mse_loss_grad(a.to(DEV), b.to(DEV), loss, da, scale=scale, accumulate=acc)
        outs.append((loss.clone(), da.clone()))
    torch.cuda.synchronize()
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    loss, da = outs[0]
    bl, bd = (l0.double(), da0.double()) if acc else (0.0, 0.0)
    _check(f"mse/n{n}a{int(acc)}/da", da, d64 + bd, (d32.double() + bd) if acc else d32)
    _check(f"mse/n{n}a{int(acc)}/loss", loss, (l64 + bl).reshape(1), ((l32.double() + bl) if acc else l32).reshape(1),
           scale=float(l64.abs() + (l0.double().abs() if acc else 0.0)))
    # unaligned pointers (views one element in): the scalar path, same values
    if n > 4:
        au, bu = torch.zeros(n + 1, device=DEV), torch.zeros(n + 1, device=DEV)
        au[1:], bu[1:] = a.to(DEV), b.to(DEV)
        dau, lu = torch.empty(n + 1, device=DEV), torch.empty(1, device=DEV)
        ops.mse_loss_grad(au[1:], bu[1:], lu, dau[1:], scale=scale)
        torch.cuda.synchronize()
        _check(f"mse/n{n}/unaligned/da", dau[1:], d64, d32)
        _check(f"mse/n{n}/unaligned/loss", lu, l64.reshape(1), l32.reshape(1), scale=float(l64.abs()))
