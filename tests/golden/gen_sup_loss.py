"""Fixture generator for the supervised losses: runs the reference's own ``DCCRN.loss``
(DCCRN.py:259-411) and ``melFilterBank`` (tools_for_loss.py:133-177) on the CPU and writes
tests/golden/sup_loss.npz.  Needs the reference checkout (see _ref_shims.REFERENCE); never runs
on the GPU box.  Only the .npz is committed.

Contents: the three filterbank matrices; seeded inputs at B = 2, L = 1600 (T = 19): the estimate
`inputs`, the `labels`, and a masked spectrum `real_spec` / `img_spec` [2][257][19]; per mode the
loss value and the reference's float32 autograd gradients w.r.t. inputs (and, for the LMS modes,
real_spec and img_spec).

    python tests/golden/gen_sup_loss.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(REPO, "speech-enhancement-clskd_amd"))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)

import _ref_shims  # noqa: E402

_ref_shims.install()

import torch  # noqa: E402

import DCCRN as ref_dccrn  # noqa: E402  (reference module)
import tools_for_loss as ref_loss  # noqa: E402

ref_loss.DEVICE = torch.device("cpu")

import sup_loss_ref as S  # noqa: E402
from clskd import config as ccfg  # noqa: E402


def main():
    out = {}
    for n in S.SCALES:
        out[f"bank{n}"] = ref_loss.melFilterBank(n, 512)
    B, L, T = 2, 1600, 19
    s, y = S.seeded_pair(B, L, seed=11)
    _, est = S.seeded_spec(B, T, 514, seed=12)
    real, imag = [t.contiguous() for t in S.spec_to_reim(est)]
    out.update(inputs=s.numpy(), labels=y.numpy(), real_spec=real.numpy(), img_spec=imag.numpy())
    model = ref_dccrn.DCCRN(rnn_units=ccfg.rnn_units_student, masking_mode="E", use_clstm=True,
                            kernel_num=ccfg.kernel_num_student)
    with torch.no_grad():
        cs = model.stft(y)
    out["clean_real"], out["clean_imag"] = cs[:, :257].numpy(), cs[:, 257:].numpy()
    for mode in S.MODES:
        a = s.clone().requires_grad_()
        r = real.clone().requires_grad_()
        i = imag.clone().requires_grad_()
        loss = model.loss(a, y, r, i, loss_mode=mode)
        loss.backward()
        out[f"{mode}/loss"] = np.float32(loss.item())
        out[f"{mode}/d_inputs"] = a.grad.numpy()
        if "LMS" in mode:
            out[f"{mode}/d_real"] = r.grad.numpy()
            out[f"{mode}/d_imag"] = i.grad.numpy()
        print(mode, loss.item())
    path = os.path.join(HERE, "sup_loss.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
