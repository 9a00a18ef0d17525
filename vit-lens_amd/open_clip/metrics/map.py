"""Mean average precision accumulator (protocol and result keys of the reference's open_clip/metrics/map.py:12-53, the
AudioSet-style multi-label evaluation): scores and multi-hot targets of every batch are collected, gathered across ranks,
and each class is scored on the host by scikit-learn's `average_precision_score` over sigmoid(score) - or, with
`initialize(on_device=True)`, on the device by `vitlens_hip.ops.average_precision` over the raw scores."""
import numpy as np
import torch

from .base_metric import BaseMetric


class MAP(BaseMetric):
    def initialize(self, on_device=False):
        """on_device=False: the reference's path, bit for bit (sigmoid, copy to the host, scikit-learn).  on_device=True: the
        per-class average precision is computed by the HIP kernel on the gathered device tensors and `C` doubles are read once.
        The kernel ranks the RAW scores (sigmoid is strictly monotone, so the ranking is the same); the one difference from the
        host path: two distinct scores that float32 sigmoid collapses into one value are a tie there and stay distinct here.  A
        class without positives scores 0.0 on both paths (scikit-learn 1.7; older releases gave NaN)."""
        self.on_device = bool(on_device)
        self._reset()

    def compute(self, ids, logits, targets):
        self._push(ids=ids, score=logits.float(), target=targets.float())

    def merge_results(self, output_predict=False):
        from sklearn.metrics import average_precision_score
        ids, score, target = self._collected("ids"), self._collected("score"), self._collected("target")
        if getattr(self, "on_device", False):
            return self._merge_on_device(ids, score, target, output_predict)
        prob = torch.sigmoid(score).cpu().numpy()
        while target.dim() > prob.ndim:            # a stray singleton axis from the collate function
            target = target.squeeze(0) if target.size(0) == 1 else target.squeeze(1)
        truth = target.cpu().numpy()
        per_class = average_precision_score(truth, prob, average=None)
        return {"map": np.mean(per_class), "map_cnt": len(truth),
                "predict_results": self._prediction_table(ids, prob.tolist(), output_predict)}

    def _merge_on_device(self, ids, score, target, output_predict):
        from vitlens_hip import ops
        while target.dim() > score.dim():
            target = target.squeeze(0) if target.size(0) == 1 else target.squeeze(1)
        dev = score.device if score.is_cuda else torch.device("cuda", torch.cuda.current_device())
        score, target = score.to(dev).contiguous(), target.to(dev).contiguous()
        per_class = ops.average_precision(score, target).cpu().numpy()          # the one read: C doubles
        table = self._prediction_table(ids, torch.sigmoid(score).cpu().numpy().tolist(), True) if output_predict else {}
        return {"map": np.mean(per_class), "map_cnt": int(target.shape[0]), "predict_results": table}
