"""The OpenShape flavour of ViT-Lens (reference tree VitLens-OpenShape/src): a point-cloud Lens + ViT tower
trained against PRECOMPUTED unit-norm image / text features.  `CLIPBindWrap` (models/clip_bind.py), the tri-modal loss with
its retrieval accuracies (loss.py:80-185), `LogitScaleNetwork` (models/LogitScaleNetwork.py) and the step body of
`Trainer.train_one_epoch_openclip` (train.py:784-843) on the drop-in modules; every FLOP runs in the HIP kernels.  The
evaluation of every epoch (`calculate_metrics`, train.py:716-782, and its three callers) counts on the device; the recipe
as a fused step with micro-batches and the recipe's optimizer groups is `vitlens_hip.step.OpenShapeStep`."""
from .clip_bind import CLIPBindWrap, LogitScaleNetwork
from .eval import Metrics, calculate_metrics, test_modelnet40, test_objaverse_lvis, test_scanobjectnn
from .loss import TriClipLoss
from .train import openclip_step

__all__ = ["CLIPBindWrap", "LogitScaleNetwork", "TriClipLoss", "openclip_step", "Metrics", "calculate_metrics", "test_modelnet40",
           "test_objaverse_lvis", "test_scanobjectnn"]
