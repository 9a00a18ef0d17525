"""Zero-shot classification loop (reference: training/zero_shot.py:84-110 `run`, :36-81 accuracy helpers):
for every batch of an iterable `(inputs, target)` encode through the model, score against the template-averaged text
classifier (`open_clip.build_zero_shot_classifier`) on the HIP GEMM and count top-1 / top-5 hits.  The data loaders and
the per-dataset wrappers of the reference (`test_zeroshot_3d_core`, `test_rgbd_cls_single`, ...) are dataset plumbing and
stay out; they reduce to this loop with a different `feature_key` / input keyword."""
import torch

from open_clip import accuracy, zero_shot_logits


def run(model, classifier, dataloader, args, input_key="image", feature_key="image_features", logit_scale=100.0):
    """-> (top1, top5) as fractions of the samples seen.  `input_key` / `feature_key`: ("image", "image_features") is the
    reference's `run`; ("visual_x", "visual_features") scores the modality tower."""
    device = getattr(args, "device", None) or "cuda"
    top1 = top5 = n = 0.0
    with torch.no_grad():
        for inputs, target in dataloader:
            inputs, target = inputs.to(device), target.to(device)
            output = model(**{input_key: inputs})
            feats = output[feature_key] if isinstance(output, dict) else output[0]
            logits = zero_shot_logits(feats, classifier, logit_scale=logit_scale)
            a1, a5 = accuracy(logits, target, topk=(1, 5))
            top1 += a1; top5 += a5; n += inputs.size(0)
    return top1 / n, top5 / n


def test_linprob_single(test_loader, model, tokenizer, dataset_name="Linear Probe CLS", args=None):
    """The linear probe's evaluation (training/zero_shot.py:1025-1091): eval mode, logits = model(x) per batch, top-1 and - with
    at least five classes - top-5 accuracy in percent over the samples seen -> {"acc1": ..., "acc5": ...} or {"acc1": ...}.
    The hits are counted on the device (vl_topk_hits, the two counters accumulate over the batches) and read once at the end."""
    import logging
    from open_clip.utils import get_model
    from vitlens_hip import ops
    dataset = test_loader.dataset
    acc5 = len(dataset.idx2label) >= 5
    net = get_model(model)
    net.eval()
    device = torch.device(getattr(args, "device", None) or "cuda")
    hits, n = None, 0
    with torch.no_grad():
        for batch in test_loader:
            x, target = batch[args.v_key], batch["label"]
            if isinstance(target, list):
                target = torch.LongTensor(target)
            x, target = x.to(device, non_blocking=True), target.to(device, non_blocking=True)
            logits = net(x)
            hits, _ = ops.topk_hits(logits.float(), target, (1, 5) if acc5 else (1, 2), hits=hits)
            n += x.size(0)
    if getattr(args, "distributed", False):
        torch.distributed.barrier()
    h1, h5 = (int(v) for v in hits.tolist())
    out = {"acc1": 100.0 * h1 / n, "acc5": 100.0 * h5 / n} if acc5 else {"acc1": 100.0 * h1 / n}
    logging.info(f"[{dataset_name}] : Linear Probe * " + " ".join(f"Acc@{k[3:]} {v:.3f}" for k, v in out.items()))
    return out


test_linprob_single.__test__ = False          # (a product function whose name the reference chose; not a pytest case)
