"""GPU: the ComplexBatchNorm kernels (csrc/cbn.hip through ops.cbn_forward / cbn_apply / cbn_bwd)
against float64 autograd of the restatement (tests/cbn_ref.py).

Gate: relative L2 <= 1e-5 — the project's bn_bwd gate (tests/test_gpu_backward.py) — on y, dx,
dalpha, the five parameter gradients, the batch statistics (means, V + eps, V^-1/2) and the
updated running buffers, n_updates = 2 and eval mode included.  tests/test_cbn_ref_cpu.py
qualifies the inputs: the restatement's own float32 evaluation is at <= 1e-6 on every tensor.
Shapes (B, Cc, F, T): 42 rows with C = 8 (one quad per part), C = 64, C = 256 (the teacher's
width), and 4864 rows (several blocks with a tail in every pass)."""
import types

import pytest
import torch

import cbn_ref as CR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GATE = 1e-5
CASES = [(s, i) for s in CR.KERNEL_SHAPES for i in range(len(CR.RHOS))]


def _layer(p):
    """The leaves as a parameter holder on the device (what ops.cbn_* read from a module)."""
    return types.SimpleNamespace(eps=1e-5, momentum=0.1,
                                 **{k: v.clone().to(DEV) for k, v in p.items()})


def _run(x, dy, p, alpha, n_updates=1, train=True):
    from clskd import ops
    L = _layer(p)
    xd, dyd = x.to(DEV), dy.to(DEV)
    al = None if alpha is None else torch.tensor([alpha], device=DEV)
    y, coef, stats = ops.cbn_forward(xd, torch.empty_like(xd), L, train, n_updates, alpha=al,
                                     return_coef=True)
    got = dict(y=y, coef=coef, stats=stats, layer=L)
    if train:
        Cc = x.shape[-1] // 2
        g = {k: torch.full((Cc,), 7.0, device=DEV) for k in CR.CBN_PARAMS}
        da = torch.full((1,), 7.0, device=DEV) if al is not None else None
        dx = torch.full_like(xd, 7.0)
        ops.cbn_bwd(xd, dyd, coef, stats, L, al, dx, g["Wrr"], g["Wri"], g["Wii"], g["Br"],
                    g["Bi"], da)
        got.update(dx=dx, dalpha=da, **{"d" + k: v for k, v in g.items()})
    torch.cuda.synchronize()
    return got


def _check(got, ref, keys, tag):
    rows, bad = [], []
    for k in keys:
        e = CR.rel(got[k], ref[k])
        rows.append(f"CBNKERN {tag} {k:6s} {e:.2e}")
        if not e <= GATE:
            bad.append((k, e))
    print("\n".join(rows))
    assert not bad, (tag, bad)


def _stats_ref(ref):
    """The stats table [8][Cc] of the reference: M, V + eps, V^-1/2."""
    U = CR.coefficients(ref["Vrr"], ref["Vri"], ref["Vii"])
    return torch.stack([ref["Mr"], ref["Mi"], ref["Vrr"] + 1e-5, ref["Vri"], ref["Vii"] + 1e-5,
                        U[0], U[1], U[2]])


@pytest.mark.parametrize("shape,irho", CASES)
def test_forward_and_backward_against_fp64(shape, irho):
    rho = CR.RHOS[irho]
    x, dy, p = CR.kernel_case(shape, rho, seed=irho)
    ref = CR.kernel_reference(x, dy, p, 0.25)
    got = _run(x, dy, p, 0.25)
    got.update({k: getattr(got["layer"], k) for k in CR.CBN_BUFFERS})
    ref["stats"] = _stats_ref(ref)
    _check(got, ref, ["y", "dx", "dalpha", "stats"] + ["d" + k for k in CR.CBN_PARAMS]
           + list(CR.CBN_BUFFERS), f"{shape} rho={rho}")


def test_without_prelu_two_updates_and_eval():
    shape, rho = CR.KERNEL_SHAPES[1], 0.7
    x, dy, p = CR.kernel_case(shape, rho, seed=1)
    # no PReLU
    ref = CR.kernel_reference(x, dy, p, None)
    got = _run(x, dy, p, None)
    assert got["dalpha"] is None
    _check(got, ref, ["y", "dx"] + ["d" + k for k in CR.CBN_PARAMS], "no-prelu")
    # n_updates = 2: the running buffers lerped twice, everything else as with one
    ref2 = CR.kernel_reference(x, dy, p, 0.25, n_updates=2)
    got2 = _run(x, dy, p, 0.25, n_updates=2)
    got2.update({k: getattr(got2["layer"], k) for k in CR.CBN_BUFFERS})
    _check(got2, ref2, ["y"] + list(CR.CBN_BUFFERS), "n_updates=2")
    ref1 = CR.kernel_reference(x, dy, p, 0.25, n_updates=1)
    assert CR.rel(ref2["RVri"], ref1["RVri"]) > 1e-3  # the second lerp is visible
    # n_updates = 0 leaves the buffers alone
    got0 = _run(x, dy, p, 0.25, n_updates=0)
    for k in CR.CBN_BUFFERS:
        assert torch.equal(getattr(got0["layer"], k).cpu(), p[k]), k
    # eval: the running buffers normalise, and stay
    refe = CR.kernel_reference(x, dy, p, 0.25, train=False)
    gote = _run(x, dy, p, 0.25, train=False)
    _check(gote, refe, ["y"], "eval")
    for k in CR.CBN_BUFFERS:
        assert torch.equal(getattr(gote["layer"], k).cpu(), p[k]), k


def test_inplace_accumulate_and_determinism():
    from clskd import ops
    shape = CR.KERNEL_SHAPES[3]
    x, dy, p = CR.kernel_case(shape, 0.7, seed=1)
    a = _run(x, dy, p, 0.25)
    b = _run(x, dy, p, 0.25)
    for k in ["y", "dx", "dalpha", "coef", "stats"] + ["d" + k for k in CR.CBN_PARAMS]:
        assert torch.equal(a[k], b[k]), k  # two runs: the same bits
    L, al = a["layer"], torch.tensor([0.25], device=DEV)
    xd, dyd = x.to(DEV), dy.to(DEV)
    xin = xd.clone()
    assert ops.cbn_apply(xin, xin, a["coef"], al) is xin
    assert torch.equal(xin, a["y"])  # in place = out of place
    # accumulate_* adds onto pre-filled buffers
    Cc = shape[1]
    g = {k: torch.full((Cc,), 3.0, device=DEV) for k in CR.CBN_PARAMS}
    da = torch.full((1,), 3.0, device=DEV)
    dx = torch.full_like(xd, 3.0)
    ops.cbn_bwd(xd, dyd, a["coef"], a["stats"], L, al, dx, g["Wrr"], g["Wri"], g["Wii"], g["Br"],
                g["Bi"], da, accumulate_dx=True, accumulate_params=True)
    torch.cuda.synchronize()
    assert torch.equal(dx, a["dx"] + 3.0)
    assert torch.equal(da, a["dalpha"] + 3.0)
    for k in CR.CBN_PARAMS:
        assert torch.equal(g[k], a["d" + k] + 3.0), k
    # parameters only (dx = None) gives the same parameter gradients
    g2 = {k: torch.empty(Cc, device=DEV) for k in CR.CBN_PARAMS}
    ops.cbn_bwd(xd, dyd, a["coef"], a["stats"], L, al, None, g2["Wrr"], g2["Wri"], g2["Wii"],
                g2["Br"], g2["Bi"], None)
    for k in CR.CBN_PARAMS:
        assert torch.equal(g2[k], a["d" + k]), k


def test_rejects_what_it_does_not_support():
    from clskd import ops
    x, _, p = CR.kernel_case(CR.KERNEL_SHAPES[0], 0.0)
    L = _layer(p)
    with pytest.raises(RuntimeError):
        ops.cbn_forward(x.to(DEV).bfloat16(), None, L, True)
    with pytest.raises(RuntimeError):
        ops.cbn_forward(torch.zeros(2, 3, 12, device=DEV), None, L, True)
