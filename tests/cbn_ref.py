"""ComplexBatchNorm reference: a dtype-generic (float64-capable) restatement of the layer
(tools_for_model.py:398-508), the DCCRN forward with it (oracle.ref_cpu's own functions, only
the normalisation replaced) and the end-to-end step references in the shape of
sup_loss_ref.dccrn_steps.  tests/golden/cbn.npz holds what the reference's own layer and model
computed (tests/golden/gen_cbn.py); tests/test_cbn_ref_cpu.py holds this file to it."""
import contextlib
import functools
import os

import numpy as np
import torch

import sup_loss_ref as S

CBN_PARAMS = ("Wrr", "Wri", "Wii", "Br", "Bi")
CBN_BUFFERS = ("RMr", "RMi", "RVrr", "RVri", "RVii")
LAYER_SEED = 77
LAYER_SHAPE = (2, 8, 3, 7)  # NCHW of the fixture's layer record: Cc = 4, 42 rows


def fixture():
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cbn.npz"))


def coefficients(Vrr, Vri, Vii, eps=1e-5):
    """(Urr, Uri, Uii) = (V + eps I)^-1/2 by the closed form of the 2x2 square root."""
    Vrr, Vii = Vrr + eps, Vii + eps
    s = (Vrr * Vii - Vri * Vri).sqrt()
    t = (Vrr + Vii + 2 * s).sqrt()
    rst = 1.0 / (s * t)
    return (s + Vii) * rst, -Vri * rst, (s + Vrr) * rst


def complex_batch_norm(x, p, pre="", train=True, momentum=0.1, eps=1e-5, update_stats=False,
                       n_updates=1, stats=None):
    """x [B, 2 Cc, F, T] (NCHW, real channels first).  p[pre + leaf]: the layer's leaves.
    train: batch statistics (update_stats: the running buffers are lerped in place n_updates times,
    V before eps); else the running buffers.  stats: a dict that receives Mr Mi Vrr Vri Vii (V
    before eps)."""
    xr, xi = torch.chunk(x, 2, 1)
    v = lambda t: t.reshape(1, -1, 1, 1)  # noqa: E731
    if train:
        Mr, Mi = xr.mean((0, 2, 3), keepdim=True), xi.mean((0, 2, 3), keepdim=True)
    else:
        Mr, Mi = v(p[pre + "RMr"]), v(p[pre + "RMi"])
    xr, xi = xr - Mr, xi - Mi
    if train:
        Vrr = (xr * xr).mean((0, 2, 3), keepdim=True)
        Vri = (xr * xi).mean((0, 2, 3), keepdim=True)
        Vii = (xi * xi).mean((0, 2, 3), keepdim=True)
        if update_stats:
            with torch.no_grad():
                for _ in range(n_updates):
                    for k, b in zip(CBN_BUFFERS, (Mr, Mi, Vrr, Vri, Vii)):
                        p[pre + k].lerp_(b.reshape(-1).to(p[pre + k].dtype), momentum)
    else:
        Vrr, Vri, Vii = v(p[pre + "RVrr"]), v(p[pre + "RVri"]), v(p[pre + "RVii"])
    if stats is not None:
        stats.update(Mr=Mr.reshape(-1), Mi=Mi.reshape(-1), Vrr=Vrr.reshape(-1),
                     Vri=Vri.reshape(-1), Vii=Vii.reshape(-1))
    Urr, Uri, Uii = coefficients(Vrr, Vri, Vii, eps)
    Wrr, Wri, Wii = v(p[pre + "Wrr"]), v(p[pre + "Wri"]), v(p[pre + "Wii"])
    Zrr, Zri = Wrr * Urr + Wri * Uri, Wrr * Uri + Wri * Uii
    Zir, Zii = Wri * Urr + Wii * Uri, Wri * Uri + Wii * Uii
    yr = Zrr * xr + Zri * xi + v(p[pre + "Br"])
    yi = Zir * xr + Zii * xi + v(p[pre + "Bi"])
    return torch.cat([yr, yi], 1)


def layer_params(Cc, seed=LAYER_SEED, dtype=torch.float64, pre="layer."):
    """Recipe values of one layer's ten leaves (clskd.weights), keys pre + leaf."""
    from clskd.weights import recipe_state_dict
    sd = recipe_state_dict({pre + k: (Cc,) for k in CBN_PARAMS + CBN_BUFFERS}, seed)
    return {k: torch.from_numpy(v).to(dtype) for k, v in sd.items()}


def layer_input(shape=LAYER_SHAPE, seed=LAYER_SEED, rho=0.7):
    """[B, 2 Cc, F, T] float32: xr = 2N + 0.5, xi = rho xr + sqrt(1 - rho^2) (2N - 0.3)."""
    B, C, F, T = shape
    g = torch.Generator().manual_seed(seed)
    xr = 2 * torch.randn(B, C // 2, F, T, generator=g) + 0.5
    xi = rho * xr + (1 - rho * rho) ** 0.5 * (2 * torch.randn(B, C // 2, F, T, generator=g) - 0.3)
    return torch.cat([xr, xi], 1).float()


# ------------------------------------------------------------------------------------------
# the model
# ------------------------------------------------------------------------------------------
@contextlib.contextmanager
def _cbn_oracle(R):
    """oracle.ref_cpu with its batch_norm replaced by complex_batch_norm (same call signature)."""
    keep = R.batch_norm
    R.batch_norm = lambda x, p, pre, train, momentum=0.1, eps=1e-5, update_stats=False: \
        complex_batch_norm(x, p, pre, train, momentum, eps, update_stats)
    try:
        yield R
    finally:
        R.batch_norm = keep


def dccrn_forward_cbn(p, inputs, train=True, update_stats=False, lstm_fn=None):
    """oracle.ref_cpu.dccrn_forward of a use_cbn=True parameter dict."""
    from oracle import ref_cpu as R
    with _cbn_oracle(R):
        return R.dccrn_forward(p, inputs, train=train, lstm_fn=lstm_fn or R.lstm_torch,
                               update_stats=update_stats)


def cbn_params(dtype=torch.float64, grad=True):
    """Recipe weights of the student DCCRN(use_cbn=True) in dtype; requires_grad on parameters."""
    from clskd import config as cfg
    from clskd.weights import STUDENT_SEED, recipe_state_dict
    from oracle import ref_cpu as R
    ps = R.to_torch_params(recipe_state_dict(cfg.dccrn_param_shapes(use_cbn=True, **cfg.STUDENT),
                                             STUDENT_SEED))
    out = {}
    for k, v in ps.items():
        if v.is_floating_point():
            v = v.to(dtype).clone()
            if grad and k.rsplit(".", 1)[-1] not in CBN_BUFFERS:
                v.requires_grad_()
        out[k] = v
    return out


def cbn_steps(modes, x, y, dtype=torch.float64):
    """{mode: dict(loss, grads {name: tensor}, wav)} of the student DCCRN(use_cbn=True) (recipe
    weights, train mode) for every mode in `modes` ('MRSTFT' included) from one forward in dtype."""
    with S.oracle_dtype(dtype) as R:
        ps = cbn_params(dtype)
        x, y = x.to(dtype), y.to(dtype)
        fw = dccrn_forward_cbn(ps, x, train=True, lstm_fn=R.lstm)
        cs = R.conv_stft(y)
        cr, ci = cs[:, :257], cs[:, 257:]
        names = [k for k, v in ps.items() if v.requires_grad]
        out = {}
        for mode in modes:
            if mode == "MRSTFT":
                loss = S.mrstft_mag(fw["out_wav"], y)
            else:
                loss = S.dccrn_loss(mode, fw["out_wav"], y, fw["real"], fw["imag"], cr, ci)
            grads = torch.autograd.grad(loss, [ps[n] for n in names], retain_graph=True,
                                        allow_unused=True)
            out[mode] = dict(loss=loss.detach(), grads=dict(zip(names, grads)),
                             wav=fw["out_wav"].detach())
    return out


E2E = dict(B=2, L=1600, seed=7)
GRAD_MODES = S.MODES  # 'MRSTFT' does not qualify on these inputs: its loss only (ALL_MODES)
ALL_MODES = S.MODES + ("MRSTFT",)


@functools.lru_cache(maxsize=None)
def e2e_reference(dtype=torch.float64):
    """One forward in dtype at the E2E inputs, every mode's loss and gradients; shared, read only."""
    x, y = S.seeded_batch(**E2E)
    return cbn_steps(ALL_MODES, x, y, dtype)


# ------------------------------------------------------------------------------------------
# kernel-level reference (BFTC in, autograd in dtype)
# ------------------------------------------------------------------------------------------
KERNEL_SHAPES = [(2, 4, 3, 7), (2, 32, 16, 19), (1, 128, 5, 9), (2, 4, 128, 19)]  # (B, Cc, F, T)
RHOS = (0.0, 0.7, 0.95)


def kernel_case(shape, rho, seed=0):
    """(x BFTC [B, F, T, 2 Cc] float32, dy like x, params {leaf: float32 [Cc]})."""
    B, Cc, F, T = shape
    x = layer_input((B, 2 * Cc, F, T), seed=1000 + seed, rho=rho).permute(0, 2, 3, 1).contiguous()
    g = torch.Generator().manual_seed(2000 + seed)
    dy = torch.randn(B, F, T, 2 * Cc, generator=g)
    p = {k: v.float() for k, v in layer_params(Cc, seed=LAYER_SEED + seed, pre="").items()}
    return x, dy, p


def kernel_reference(x, dy, p, alpha, train=True, n_updates=1, dtype=torch.float64):
    """The layer (+ PReLU when alpha is not None) on BFTC x in dtype with autograd: dict of y,
    dx, dalpha, the five parameter gradients, the batch statistics and the updated buffers."""
    q = {k: v.to(dtype).clone() for k, v in p.items()}
    for k in CBN_PARAMS:
        q[k].requires_grad_()
    xn = x.to(dtype).permute(0, 3, 1, 2).clone().requires_grad_()
    a = None if alpha is None else torch.tensor([alpha], dtype=dtype, requires_grad=True)
    st = {}
    y = complex_batch_norm(xn, q, "", train, update_stats=train and n_updates > 0,
                           n_updates=n_updates, stats=st)
    if a is not None:
        y = torch.nn.functional.prelu(y, a)
    y.backward(dy.to(dtype).permute(0, 3, 1, 2))
    out = dict(y=y.detach().permute(0, 2, 3, 1), dx=xn.grad.permute(0, 2, 3, 1),
               dalpha=None if a is None else a.grad)
    out.update({"d" + k: q[k].grad for k in CBN_PARAMS})
    out.update({k: q[k].detach() for k in CBN_BUFFERS})
    out.update({k: v.detach() for k, v in st.items()})
    return out


def rel(got, ref):
    got, ref = got.double().cpu(), ref.double()
    return float((got - ref).norm() / ref.norm())
