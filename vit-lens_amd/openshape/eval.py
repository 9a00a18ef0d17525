"""The evaluation the OpenShape loop runs after every epoch (reference: VitLens-OpenShape/src/train.py:716-782
`Trainer.calculate_metrics`, and its callers `test_modelnet40` :608-648, `test_objaverse_lvis`, `test_scanobjectnn`): an
eval-mode tower over batches of {features_dense, xyz_dense, category}, logits = normalize(pred) @ normalize(clip_text_feat).T,
top-1 / 3 / 5, overall and per-class accuracy.

Counting is on the device (vl_eval_hits; its calls ACCUMULATE, and one call counts two values of k, so top-3 is a second call
on the same logits), the host reads the counters once, at the end.  In a multi-rank run the integer counters are all-reduced -
the reference gathers every rank's logits and labels and counts again; the counts are the same."""
from collections import namedtuple

import torch

Metrics = namedtuple("Metrics", "topk_acc overall_acc per_cat_acc per_cat_correct per_cat_count samples")
Metrics.__doc__ = """topk_acc: [top-1, top-3, top-5] in percent (train.py:556-570); overall_acc = per_cat_correct.sum() /
per_cat_count.sum(), a fraction; per_cat_acc: float64 [num_class], NaN for a class without samples (the reference's 0 / 0);
per_cat_correct / per_cat_count: int64 [num_class]; samples: the labelled samples seen (all ranks)."""


def _logits(pred, cls_unit_b):
    """normalize(pred) @ cls^T on the device: f32 [B, num_class] (cls_unit_b: the column operand, made once per evaluation)."""
    from vitlens_hip import ops
    return ops.logits_gemm(ops.split_bf16x3(ops.l2_normalize(pred.float().contiguous()), 0), cls_unit_b, 1.0)


def _classifier(clip_text_feat, device):
    from vitlens_hip import ops
    return ops.split_bf16x3(ops.l2_normalize(torch.as_tensor(clip_text_feat).to(device=device, dtype=torch.float32).contiguous()), 1)


def _reduce(t):
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        dist.all_reduce(t, op=dist.ReduceOp.SUM)
    return t


def calculate_metrics(model, dataloader, clip_text_feat, num_class: int, device="cuda") -> Metrics:
    from vitlens_hip import ops
    device = torch.device(device)
    cls = _classifier(clip_text_feat, device)
    # [top-1, top-3], [top-1, top-5], and per class: samples, hits at 1, hits at 3 - one int32 buffer, one read
    counters = torch.zeros(4 + 3 * num_class, device=device, dtype=torch.int32)
    h13, h15, per_class = counters[0:2], counters[2:4], counters[4:].view(3, num_class)
    with torch.no_grad():
        for data in dataloader:
            pred = model(data["features_dense"].to(device), xyz=data["xyz_dense"].to(device))
            logits = _logits(pred, cls)
            target = torch.as_tensor(data["category"]).to(device).long().contiguous()
            ops.eval_hits(logits, target, (1, 3), hits=h13, per_class=per_class)
            ops.eval_hits(logits, target, (1, 5), hits=h15)
    v = _reduce(counters.to(torch.int64)).tolist()          # the one host read
    count = torch.tensor(v[4:4 + num_class], dtype=torch.int64)
    correct = torch.tensor(v[4 + num_class:4 + 2 * num_class], dtype=torch.int64)
    n = int(count.sum())
    pct = lambda h: 100.0 * h / n if n else float("nan")
    overall = float(correct.sum()) / n if n else float("nan")
    return Metrics([pct(v[0]), pct(v[1]), pct(v[3])], overall, correct.double() / count.double(), correct, count, n)


def _test(model, loader, num_class, clip_text_feat, device):
    was_training = getattr(model, "training", False)
    if hasattr(model, "eval"):
        model.eval()
    try:
        feat = loader.dataset.clip_cat_feat if clip_text_feat is None else clip_text_feat
        return calculate_metrics(model, loader, feat, num_class, device)
    finally:
        if was_training:
            model.train()


def test_modelnet40(model, loader, clip_text_feat=None, device="cuda") -> Metrics:
    """train.py:608-648.  clip_text_feat: default `loader.dataset.clip_cat_feat`, as there."""
    return _test(model, loader, 40, clip_text_feat, device)


def test_objaverse_lvis(model, loader, clip_text_feat=None, device="cuda") -> Metrics:
    return _test(model, loader, 1156, clip_text_feat, device)


def test_scanobjectnn(model, loader, clip_text_feat=None, device="cuda") -> Metrics:
    return _test(model, loader, 15, clip_text_feat, device)


for _f in (test_modelnet40, test_objaverse_lvis, test_scanobjectnn):
    _f.__test__ = False          # (drivers named after the reference's methods, not tests)
