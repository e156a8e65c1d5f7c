"""GPU: the masking mode 'C' / 'R' kernels (clskd_mask_cr, clskd_mask_cr_bwd) against float64
autograd of the two-line formula (DCCRN.py:227-230), at the shapes and gates of
tests/test_gpu_backward.py::test_mask_e_tiles_against_fp64: ragged last tile and mask columns past
T, exactly one tile, one frame; forward 1e-5 and backward 1e-4 relative L2; row pitches 520 / 600;
sentinel-filled outputs.  Each case prints a `MASKCR` line (profiles/variants_margins.txt)."""
import pytest
import torch

import variants_ref as V

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _rel(got, ref):
    return float((got - ref).norm() / ref.norm())


@pytest.mark.parametrize("mode", V.MODES)
@pytest.mark.parametrize("B,T,extra", [(3, 37, 2), (2, 16, 0), (1, 1, 0)])
def test_mask_cr_tiles_against_fp64(mode, B, T, extra):
    from clskd import ops
    g = torch.Generator().manual_seed(B * 100 + T)
    Tm = T + 1 + extra
    spec = torch.randn(B, T, 520, generator=g, dtype=torch.float64)
    mask = torch.randn(B, 256, Tm, 2, generator=g, dtype=torch.float64)
    dest = torch.randn(B, T, 600, generator=g, dtype=torch.float64)
    mr_ = mask[:, :, 1:T + 1, 0].transpose(1, 2).clone().requires_grad_(True)
    mi_ = mask[:, :, 1:T + 1, 1].transpose(1, 2).clone().requires_grad_(True)
    z = torch.zeros(B, T, 1, dtype=torch.float64)
    mr = torch.cat([z, mr_], -1)  # F.pad(..., [0, 0, 1, 0]): the DC bin sees a zero mask
    mi = torch.cat([z, mi_], -1)
    e_re, e_im = V.apply_mask(mode, spec[..., :257], spec[..., 257:514], mr, mi)
    (e_re * dest[..., :257] + e_im * dest[..., 257:514]).sum().backward()
    f32 = lambda t: t.to(DEV, torch.float32).contiguous()  # noqa: E731
    est = torch.full((B, T, 600), 7.0, device=DEV)
    out_r = torch.full((B, T, 257), 7.0, device=DEV)
    out_i = torch.full((B, T, 257), 7.0, device=DEV)
    ops.mask(mode, f32(spec), f32(mask), T, est, out_r, out_i)
    est2 = torch.full((B, T, 600), 7.0, device=DEV)
    ops.mask(mode, f32(spec), f32(mask), T, est2)  # without the optional mask outputs
    dmask = torch.full((B, 256, Tm, 2), 7.0, device=DEV)
    ops.mask_bwd(mode, f32(spec), f32(mask), T, f32(dest), dmask)
    torch.cuda.synchronize()
    assert torch.equal(est, est2)
    est, dmask = est.cpu().double(), dmask.cpu().double()
    errs = (_rel(est[..., :257], e_re.detach()), _rel(est[..., 257:514], e_im.detach()),
            _rel(dmask[:, :, 1:T + 1, 0], mr_.grad.transpose(1, 2)),
            _rel(dmask[:, :, 1:T + 1, 1], mi_.grad.transpose(1, 2)))
    print(f"MASKCR {mode} B={B} T={T} Tm={Tm} fwd re {errs[0]:.2e} im {errs[1]:.2e} (gate 1e-5) "
          f"bwd mr {errs[2]:.2e} mi {errs[3]:.2e} (gate 1e-4)")
    assert errs[0] < 1e-5 and errs[1] < 1e-5
    assert torch.all(est[..., 514:600] == 0)
    assert errs[2] < 1e-4 and errs[3] < 1e-4
    assert torch.all(dmask[:, :, 0] == 0) and torch.all(dmask[:, :, T + 1:] == 0)
    # mask_r / mask_i: the padded mask, bitwise
    assert torch.equal(out_r.cpu(), mr.detach().float()) and torch.equal(out_i.cpu(), mi.detach().float())


def test_mask_routes_e_to_its_own_entries():
    """ops.mask('E') / ops.mask_bwd('E') are ops.mask_e / ops.mask_e_bwd, bit for bit."""
    from clskd import ops
    g = torch.Generator().manual_seed(5)
    B, T, Tm = 2, 19, 20
    spec = torch.randn(B, T, 514, generator=g).to(DEV)
    mask = torch.randn(B, 256, Tm, 2, generator=g).to(DEV)
    dest = torch.randn(B, T, 516, generator=g).to(DEV)
    a, b = torch.empty(B, T, 516, device=DEV), torch.empty(B, T, 516, device=DEV)
    da, db = torch.empty_like(mask), torch.empty_like(mask)
    ops.mask("E", spec, mask, T, a)
    ops.mask_e(spec, mask, T, b)
    ops.mask_bwd("E", spec, mask, T, dest, da)
    ops.mask_e_bwd(spec, mask, T, dest, db)
    assert torch.equal(a, b) and torch.equal(da, db)
    with pytest.raises(ValueError, match="masking_mode"):
        ops.mask("X", spec, mask, T, a)
