"""GPU: the LSTM recurrence entries with ONE weight set (the real-LSTM bottleneck of
DCCRN(use_clstm=False): 1 set x B sequences, where the complex stack runs 2 x 2B and every other
test launches two sets): the grid's set dimension is 1 and no set stride is ever applied.
lstm_recurrent, lstm_recurrent_pre (where capable), lstm_cell and lstm_bwd at B = 3, T = 37 for
every built hidden size against a float64 LSTM, at the tolerances of the two-set tests
(tests/test_gpu_parity.py: 2e-5 on h; tests/test_gpu_backward.py: 1e-5 / 1e-6 on pre-activations
and cell states, 1e-4 relative L2 on the gate gradients)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B, T = 3, 37


def _case(H):
    g = torch.Generator().manual_seed(100 + H)
    gx = torch.randn(B, T, 4 * H, generator=g)
    whh = torch.randn(1, 4 * H, H, generator=g) * (0.2 * (32 / H) ** 0.5)
    dh = torch.randn(B, T, H, generator=g)
    return gx, whh, dh


def _ref(gx, whh, dh, H):
    """float64 recurrence from zero state with autograd: h, pre, c [B][T][.], d loss / d gx."""
    gx = gx.double().requires_grad_()
    W = whh[0].double()
    h = torch.zeros(B, H, dtype=torch.float64)
    c = torch.zeros(B, H, dtype=torch.float64)
    hs, pres, cs = [], [], []
    for t in range(T):
        z = gx[:, t] + h @ W.t()
        i, f, gg, o = z.split(H, 1)
        c = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(gg)
        h = torch.sigmoid(o) * torch.tanh(c)
        hs.append(h)
        pres.append(z.detach())
        cs.append(c.detach())
    hs = torch.stack(hs, 1)
    (hs * dh.double()).sum().backward()
    return hs.detach(), torch.stack(pres, 1), torch.stack(cs, 1), gx.grad


@pytest.mark.parametrize("H", [16, 32, 64, 128])
def test_one_weight_set_against_fp64(H):
    from clskd import ops
    gx, whh, dh = _case(H)
    h64, pre64, c64, dg64 = _ref(gx, whh, dh, H)
    whh_d, dh_d = whh.to(DEV), dh.to(DEV)
    st = (4 * H, T * 4 * H, 4 * H)
    # forward
    out = torch.full((1, B, T, H), float("nan"), device=DEV)
    ops.lstm_recurrent(gx.to(DEV), *st, whh_d, 1, B, T, H, out, B * T * H, T * H, H)
    np.testing.assert_allclose(out[0].double().cpu().numpy(), h64.numpy(), rtol=2e-5, atol=2e-5)
    # forward that leaves the pre-activations and the cell states
    cells = None
    if ops.lstm_pre_capable(H):
        g2 = gx.to(DEV).clone()
        out2 = torch.full((1, B, T, H), float("nan"), device=DEV)
        cells = torch.full((B * T * H,), float("nan"), device=DEV)
        ops.lstm_recurrent_pre(g2, *st, whh_d, 1, B, T, H, out2, B * T * H, T * H, H, cbuf=cells)
        np.testing.assert_allclose(out2[0].double().cpu().numpy(), h64.numpy(), rtol=2e-5, atol=2e-5)
        np.testing.assert_allclose(g2.double().cpu().numpy(), pre64.numpy(), rtol=1e-5, atol=1e-5)
        np.testing.assert_allclose(cells.view(B, T, H).double().cpu().numpy(), c64.numpy(),
                                   rtol=1e-5, atol=1e-6)
    # one step at a time with carried state
    h = torch.zeros(1, B, H, device=DEV)
    c = torch.zeros(1, B, H, device=DEV)
    gxd = gx.to(DEV)
    for t in range(5):
        o = torch.full((1, B, H), float("nan"), device=DEV)
        ops.lstm_cell(gxd[:, t].contiguous(), 4 * H, 4 * H, whh_d, 1, B, H, h, c, B * H, H, o, B * H, H)
        assert torch.equal(h, o), t
        np.testing.assert_allclose(o[0].double().cpu().numpy(), h64[:, t].numpy(), rtol=2e-5, atol=2e-5)
    # backward from the float64 pre-activations, with its own cell-state scan and with the forward's
    pre_d = pre64.float().to(DEV)
    for cb in ([None] if cells is None else [None, cells]):
        dg = torch.full((1, B, T, 4 * H), float("nan"), device=DEV)
        ops.lstm_bwd(pre_d, st, dh_d, (B * T * H, T * H, H), whh_d, 1, B, T, H, dg, st, cells=cb)
        e = float((dg[0].double().cpu() - dg64).norm() / dg64.norm())
        print(f"LSTM1SET H={H} cells={'fwd' if cb is not None else 'scan'} dgates rel {e:.2e}")
        assert e < 1e-4
