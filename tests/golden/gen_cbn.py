"""Fixture generator for ComplexBatchNorm: runs the reference's own layer
(tools_for_model.py:335-508) and its ``DCCRN(use_cbn=True, use_clstm=True)`` in the student
configuration on the CPU and writes tests/golden/cbn.npz.  Needs the reference checkout (see
_ref_shims.REFERENCE); never runs on the GPU box.  Only the .npz is committed.

Contents: a float64 layer record (cbn_ref.layer_input / layer_params: the input, the train-mode output,
the five running buffers after that one train forward, the eval-mode output with those buffers)
and the model's out_wav on recipe weights and seeded_batch(2, 1600, seed=7), train and eval mode
(each from freshly loaded weights).

    python tests/golden/gen_cbn.py
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
import tools_for_model as ref_tools  # noqa: E402

import cbn_ref as CR  # noqa: E402
import sup_loss_ref as S  # noqa: E402
from clskd import config as ccfg  # noqa: E402
from clskd.weights import STUDENT_SEED, apply_recipe  # noqa: E402


def main():
    out = {}
    x = CR.layer_input().double()  # the layer record in float64: the restatement is held to 1e-12
    layer = ref_tools.ComplexBatchNorm(x.shape[1]).double()
    layer.load_state_dict({k[len("layer."):]: v for k, v in
                           CR.layer_params(x.shape[1] // 2).items()}, strict=False)
    with torch.no_grad():
        layer.train()
        out["layer/x"] = x.numpy()
        out["layer/y_train"] = layer(x).numpy()
        for k in CR.CBN_BUFFERS:
            out[f"layer/{k}"] = getattr(layer, k).numpy().copy()
        assert int(layer.num_batches_tracked) == 1
        layer.eval()
        out["layer/y_eval"] = layer(x).numpy()

    xb, _ = S.seeded_batch(**CR.E2E)
    for mode in ("train", "eval"):
        model = ref_dccrn.DCCRN(rnn_units=ccfg.rnn_units_student, masking_mode="E", use_clstm=True,
                                use_cbn=True, kernel_num=list(ccfg.kernel_num_student))
        apply_recipe(model, STUDENT_SEED)
        model.train(mode == "train")
        with torch.no_grad():
            out[f"model/out_wav_{mode}"] = model(xb)[-1].numpy()
    out["model/keys"] = np.array([k for k in model.state_dict()
                                  if not k.startswith(("stft.", "istft."))])
    path = os.path.join(HERE, "cbn.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
