"""tests/lstm_ref.py against independent forms, no GPU: the float64 reference against
torch.nn.LSTM (forward and its own autograd), and the tolerance the suite's rule yields for every
case of the GPU file against the project's earlier bounds (the ceiling condition)."""
import pytest
import torch

import lstm_ref as L


@pytest.mark.parametrize("T", [1, 5, 65])
@pytest.mark.parametrize("H", [16, 128])
def test_reference_matches_nn_lstm_in_float64(H, T):
    """lstm_ref's activation forms (1 / (1 + exp2(-x log2 e)), 1 - 2 / (1 + exp2(2c log2 e)),
    2 sigmoid(2x) - 1) are sigmoid and tanh in float64: h, the final c and the gradient w.r.t. the
    gate inputs agree with nn.LSTM (weights copied in, both biases folded into gx) to 1e-12."""
    nseq, D = 3, 7
    g = torch.Generator().manual_seed(H + T)
    lstm = torch.nn.LSTM(D, H, batch_first=True).double()
    with torch.no_grad():
        for p in lstm.parameters():
            p.copy_(torch.randn(p.shape, generator=g, dtype=torch.float64) * 0.3)
    x = torch.randn(nseq, T, D, generator=g, dtype=torch.float64)
    dh = torch.randn(nseq, T, H, generator=g, dtype=torch.float64)
    gx = (x @ lstm.weight_ih_l0.t() + lstm.bias_ih_l0 + lstm.bias_hh_l0).detach().requires_grad_()
    # nn.LSTM's own autograd with gx as the leaf: gx is the input of an LSTM whose W_ih is the
    # identity and whose biases are zero
    ident = torch.nn.LSTM(4 * H, H, batch_first=True).double()
    with torch.no_grad():
        ident.weight_ih_l0.copy_(torch.eye(4 * H, dtype=torch.float64))
        ident.weight_hh_l0.copy_(lstm.weight_hh_l0)
        ident.bias_ih_l0.zero_()
        ident.bias_hh_l0.zero_()
    out, (_, cn) = ident(gx)
    (out * dh).sum().backward()
    direct, (_, cn_direct) = lstm(x)   # the biased LSTM on x: the fold itself
    out_d, cn_d = out.detach(), cn.detach()
    assert float((out_d - direct.detach()).abs().max()) < 1e-12
    assert float((cn_d - cn_direct.detach()).abs().max()) < 1e-12
    r = L.lstm_ref(gx.detach()[None], lstm.weight_hh_l0.detach()[None], dh[None])
    assert r["h"].dtype == torch.float64
    assert float((r["h"][0] - out.detach()).abs().max()) < 1e-12
    assert float((r["c"][0, :, -1] - cn.detach()[0]).abs().max()) < 1e-12
    assert float((r["dgx"][0] - gx.grad).abs().max()) < 1e-12


def test_perturbation_is_float32_only_and_one_ulp():
    gx, whh, dh = L.inputs(16, 5)
    a = L.lstm_ref(gx.double(), whh.double(), dh.double())
    b = L.lstm_ref(gx.double(), whh.double(), dh.double(), perturb=11)
    assert all(torch.equal(a[k], b[k]) for k in L.KEYS)
    p, q = L.lstm_ref(gx, whh, dh), L.lstm_ref(gx, whh, dh, perturb=11)
    assert p["h"].dtype == torch.float32 and not torch.equal(p["h"], q["h"])
    # first step, o gate closed form: h differs by a few ulp of activations of magnitude <= 1
    assert float((p["h"][:, :, 0] - q["h"][:, :, 0]).abs().max()) < 16 * 2.0 ** -23
    x = torch.linspace(1.0, 1.99, 1000)   # one binade: 2^-23 relative is one to two ulp
    d = (L._Ulp(3, torch.float32)(x).double() - x.double()) * 2.0 ** 23
    assert set(d.sign().int().tolist()) == {-1, 0, 1} and float(d.abs().max()) <= 2.0


@pytest.mark.parametrize("H", L.HIDDEN)
def test_rule_tolerance_stays_under_the_earlier_bounds(H):
    """The ceiling condition, from the reference alone: for every case of the GPU file the
    tolerance of kernel_refs.tolerance (factor 8, e32 over the plain and two perturbed float32
    restatements) does not exceed 2e-5 on h, 1e-5 on the pre-activations, 1e-5 max|c| + 1e-6 on
    the cell states and 1e-4 max|ref| on the gate gradients.  A case that breaks it is a badly
    chosen input."""
    bad = []
    for (h, T, nws, nseq) in [c for c in L.all_cases() if c[0] == H]:
        cs = L.case(h, T, nws, nseq)
        ceil = L.ceilings(cs["ref"])
        for k in L.KEYS:
            e32, tol = cs["tol"][k]
            print(f"LSTMREF H={h} T={T} nws={nws} nseq={nseq} {k}: e32 {e32:.2e} tol {tol:.2e} "
                  f"ceiling {ceil[k]:.2e}")
            if not tol <= ceil[k]:
                bad.append((h, T, nws, nseq, k, tol, ceil[k]))
    assert not bad, bad
