"""Fixture generator for the DCCRN variants (masking modes 'C' and 'R', use_clstm=False): runs the
reference's own ``DCCRN(masking_mode, use_clstm)`` in the student configuration on the CPU and
writes one tests/golden/variants_<tag>.npz per variant of variants_ref.FIXTURE_VARIANTS.  Needs the reference checkout (see _ref_shims.REFERENCE) and
runs on the CPU only.  Only the .npz files are committed.

Contents, per variant, on recipe weights (STUDENT_SEED) and variants_ref.e2e(variant): the five
tensors forward returns (mask_real, mask_imag, real, imag, out_wav) in train and eval mode (each
from freshly loaded weights), the state-dict key list, and for variants_ref.FIXTURE_LOSS[variant]
the reference's train-mode loss value and its float32 autograd gradients of
variants_ref.fixture_grads(variant) (for use_clstm=False: the ten parameters it adds).

    python tests/golden/gen_variants.py
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
import variants_ref as V  # noqa: E402
from clskd import config as ccfg  # noqa: E402
from clskd.weights import STUDENT_SEED, apply_recipe  # noqa: E402


def _model(variant, train):
    model = ref_dccrn.DCCRN(rnn_units=ccfg.rnn_units_student, masking_mode=variant[0],
                            use_clstm=variant[1], kernel_num=list(ccfg.kernel_num_student))
    apply_recipe(model, STUDENT_SEED)
    return model.train(train)


def main():
    for var in V.FIXTURE_VARIANTS:
        out = {}
        xb, yb = S.seeded_batch(**V.e2e(var))
        for tm in ("train", "eval"):
            model = _model(var, tm == "train")
            with torch.no_grad():
                res = model(xb)
            for k, v in zip(V.OUTPUTS, res):
                out[f"{tm}/{k}"] = v.numpy()
            pre = torch.squeeze(model.istft(torch.cat([res[2], res[3]], 1)), 1)
            assert float(pre.abs().max()) < 1.0, "an output sample was clamped"
        out["keys"] = np.array([k for k in model.state_dict()
                                if not k.startswith(("stft.", "istft."))])
        model = _model(var, True)
        _, _, real, imag, wav = model(xb)
        loss = model.loss(wav, yb, real, imag, loss_mode=V.FIXTURE_LOSS[var])
        loss.backward()
        out["loss"] = np.float32(loss.item())
        named = dict(model.named_parameters())
        for n in V.fixture_grads(var):
            out[f"grad/{n}"] = named[n].grad.numpy()
        path = os.path.join(HERE, f"variants_{V.tag(var)}.npz")
        np.savez_compressed(path, **out)
        print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
