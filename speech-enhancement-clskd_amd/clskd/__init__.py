"""clskd — MI355X-native DCCRN + CLSKD (cross-layer similarity KD) hot path.

Drop-in counterparts of the reference modules (KhanhNguyen4999/Speech-Enhancement-CLSKD):
  DCCRN.py                -> clskd.model.DCCRN
  framework.py            -> clskd.framework (MultiResolutionSTFTLoss, SPKDLoss, ABF, ReviewKD,
                             build_review_kd)
  feature_extraction.py   -> clskd.feature_extraction.DCCRN
  tools_for_loss.py       -> clskd.tools_for_loss (si_snr, sdr, si_sdr, melFilterBank,
                             get_array_mel_loss)
  DCCRN.loss              -> clskd.model.DCCRN.loss; a training module around it:
                             clskd.supervised.SupervisedTraining
  distill.py              -> clskd.distill.KnowledgeDistillation (training_step)
  distill_SPKD.py         -> clskd.distill.SPKDDistillation
  distill_SPKD.py / distill_MSE.py / distill_STFT.py with the asteroid DCCRNet_mini student
                          -> clskd.distill_mini.OutputDistillation (kd="spkd" | "mse" | "stft")
  config.py               -> clskd.config
A whole step can be captured and replayed as one hipGraph (clskd.graph.StepGraph).
All arithmetic runs in libclskd_hip.so (gfx950); there is no CPU fallback.
"""
from . import config  # noqa: F401
from .weights import recipe_state_dict  # noqa: F401


def __getattr__(name):
    # heavy modules (torch + the HIP library) load lazily
    if name in ("DCCRN",):
        from .model import DCCRN
        return DCCRN
    if name in ("KnowledgeDistillation", "SPKDDistillation", "clskd_step"):
        from . import distill
        return getattr(distill, name)
    if name == "OutputDistillation":
        from .distill_mini import OutputDistillation
        return OutputDistillation
    if name == "SupervisedTraining":
        from .supervised import SupervisedTraining
        return SupervisedTraining
    if name == "DCCRNet_mini":
        from .asteroid import DCCRNet_mini
        return DCCRNet_mini
    if name in ("MultiResolutionSTFTLoss", "SPKDLoss", "build_review_kd", "ReviewKD", "ABF"):
        from . import framework
        return getattr(framework, name)
    if name == "StepGraph":
        from .graph import StepGraph
        return StepGraph
    raise AttributeError(name)
