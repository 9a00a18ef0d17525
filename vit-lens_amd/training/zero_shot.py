"""Zero-shot evaluation (reference: training/zero_shot.py): the step every `*_main.py` runs after an epoch,
whose `acc1` field `--save-best` reads.

  run, test_linprob_single                                        the ImageNet-style loop and the linear probe's evaluation
  test_zeroshot_3d_core                                           ModelNet40 / Objaverse-LVIS, with per-class top-1 / top-5 rates
  test_rgbd_cls_single / _core                                    SUN-RGBD, NYUv2: classes folded into "others" (cond_acc)
  test_audio_single_map / _cls / _ret, test_audiotasks_core       AudioSet mAP, ESC-50 / VGGSound accuracy, Clotho / AudioCaps recall
  test_tactle_cls_single, test_tactiletasks_core                  Touch-and-Go
  test_eeg_cls_single, test_eegtasks_core                         ImageNet-EEG

Names, positional signatures, batch keys, result keys and log lines are the reference's.  Every driver builds the template-averaged
classifier with `open_clip.build_zero_shot_classifier`, scores with `zero_shot_logits` (the HIP GEMM) and counts with
`ops.eval_hits` into device counters (mAP: `ops.average_precision` through `MAP(on_device=True)`); nothing is read on the host
inside the batch loop, the counters are read once at the end, and a multi-rank run adds them with one all-reduce of integers.
An accuracy is 100 * sum(hits) / sum(N).  The reference averages per-batch float32 percentages weighted by the batch size and
calls `scaled_all_reduce` per batch (the mean over ranks of each batch's percentage); the two agree in a single process (up to
the float32 rounding of each batch's percentage) and whenever all ranks see batches of equal size, and differ when the ranks'
batch sizes differ - there the reference weights samples unequally and this module does not.

Prompt templates: the reference keeps them as code (a scene-classification and a sound template list, lambdas inside the
tactile and EEG functions).  Here every single-dataset driver takes `templates=None` after the reference's parameters and falls
back to `test_loader.dataset.templates`; the 3D driver reads templates.json / labels.json under `args.pc_meta_data_dir` (or
`open_clip.constants.PC_META_DATA_DIR`), keyed by `args.val_data_prompt` / `args.val_data` as in the reference.

Out of scope: `test_vidret_single` / `test_vidret_core` (the video path is dead in the reference), `test_imgret_single`,
`zero_shot_eval` (ImageNet) and the datasets themselves."""
import json
import logging
import os

import torch

from open_clip import accuracy, build_zero_shot_classifier, zero_shot_logits


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


# ---- the per-dataset drivers ----------------------------------------------------------------------------------------------
MAP_ON_DEVICE = True          # profiles/eval_metrics.json: 5.3 ms on the device, 784 ms for sigmoid + copy + scikit-learn


def _device(args):
    return torch.device(getattr(args, "device", None) or "cuda")


def _eval_model(model):
    from open_clip.utils import get_model
    net = get_model(model)
    net.eval()
    return net


def _templates(templates, dataset, driver):
    if templates is None:
        templates = getattr(dataset, "templates", None)
    if templates is None or len(templates) == 0:
        raise ValueError(f"{driver}: no prompt templates - pass templates=[...] (format strings with one {{}} or callables "
                         "label -> text) or give the dataset a `templates` attribute")
    return list(templates)


def _classifier(net, tokenizer, labels, templates, device):
    """[E, C]: per class the unit mean of its templates' unit text embeddings (the loop every reference driver spells out)."""
    return build_zero_shot_classifier(net, tokenizer, [labels[i] for i in range(len(labels))], templates, num_classes_per_batch=10,
                                      device=device)


def _features(net, x, n_clip=1):
    """Unit features of a batch from the modality tower: encode_visual (encode_image for a plain CLIP), F.normalize on the device;
    with n_clip > 1 the rows are a sample's clips and their mean is normalised."""
    from vitlens_hip import ops
    f = net.encode_visual(x) if hasattr(net, "encode_visual") else net.encode_image(x)
    f = f.float()
    if f.dim() != 2 or f.stride(1) != 1:
        f = f.reshape(f.shape[0], -1).contiguous()
    return ops.clip_mean_normalize(f, n_clip) if n_clip > 1 else ops.l2_normalize(f.contiguous())


def _audio_features(net, audio, device):
    """[B, n_clip, T, F] -> the normalised mean of the clips' features; [B, T, F] -> the normalised features."""
    audio = audio.to(device, non_blocking=True)
    if audio.ndim == 4:
        return _features(net, audio.reshape(-1, *audio.shape[2:]), n_clip=audio.size(1))
    if audio.ndim == 3:
        return _features(net, audio)
    raise ValueError(f"audio batch of shape {tuple(audio.shape)}: [B, n_clip, T, F] or [B, T, F] expected")


def _target(target, device):
    if isinstance(target, (list, tuple)):
        target = torch.LongTensor(target)
    return target.to(device, non_blocking=True).long().contiguous()


def _totals(counters, n):
    """The device counters (int32, any shape) and the sample count as Python ints: one all-reduce of integers in a multi-rank
    run, one read."""
    import torch.distributed as dist
    from open_clip.metrics.base_metric import BaseMetric
    t = torch.cat([counters.reshape(-1).to(torch.int64), torch.tensor([n], dtype=torch.int64).to(counters.device)])
    if BaseMetric.multi_rank():
        t = t.to(BaseMetric.comm_device())
        dist.all_reduce(t, op=dist.ReduceOp.SUM)
    v = t.tolist()
    return v[:-1], v[-1]


def _barrier(args):
    if getattr(args, "distributed", False):
        torch.distributed.barrier()


def _count_topk(test_loader, net, classifier, input_key, ks, device, class_map=None, per_class=None, on_batch=None):
    """The batch loop of the accuracy drivers -> (hits int32 [2] on the device, samples seen)."""
    from vitlens_hip import ops
    hits, n = torch.zeros(2, device=device, dtype=torch.int32), 0
    for batch in test_loader:
        x, target = batch[input_key].to(device, non_blocking=True), _target(batch["label"], device)
        logits = zero_shot_logits(_features(net, x), classifier, logit_scale=1.0)
        ops.eval_hits(logits, target, ks, class_map=class_map, hits=hits, per_class=per_class)
        n += x.size(0)
        if on_batch is not None:
            on_batch(batch, target)
    return hits, n


def test_zeroshot_3d_core(test_loader, model, tokenizer, args=None, return_per_class=False):
    """ModelNet40 / Objaverse-LVIS (training/zero_shot.py:155-257) -> dict(modelnet40={"acc1", "acc5"}) in percent; prints the
    reference's three per-class lines (names in first-seen order, top-1 rates, top-5 rates) from the device counters.
    return_per_class: -> (that dict, {"names", "count", "top1", "top5"}).  In a multi-rank run the counters are the sum over the
    ranks (the reference prints each rank's own) and the names are those this rank's loader produced."""
    from open_clip import constants
    device = _device(args)
    net = _eval_model(model)
    print("=> encoding captions")
    meta = getattr(args, "pc_meta_data_dir", None) or constants.PC_META_DATA_DIR
    if not os.path.isdir(meta):
        raise ValueError(f"test_zeroshot_3d_core: no directory {meta!r} - set args.pc_meta_data_dir (or open_clip.constants."
                         "PC_META_DATA_DIR) to the folder that holds templates.json and labels.json")
    with open(os.path.join(meta, "templates.json")) as f:
        templates = json.load(f)[args.val_data_prompt]
    with open(os.path.join(meta, "labels.json")) as f:
        labels = json.load(f)[args.val_data]
    seen_names, seen_targets = [], []

    def remember(batch, target):
        seen_names.append(list(batch["class_name"]))
        seen_targets.append(target)
    with torch.no_grad():
        classifier = _classifier(net, tokenizer, labels, templates, device)
        per_class = torch.zeros(3, len(labels), device=device, dtype=torch.int32)
        hits, n = _count_topk(test_loader, net, classifier, "pc", (1, 5), device, per_class=per_class, on_batch=remember)
    vals, n = _totals(torch.cat([hits, per_class.reshape(-1)]), n)
    (h1, h5), table = vals[:2], [vals[2 + i * len(labels):2 + (i + 1) * len(labels)] for i in range(3)]
    # the names are the loader's strings, the counters are indexed by label: one more read pairs them up
    labels_of = {}
    flat_t = torch.cat(seen_targets).tolist() if seen_targets else []
    for name, t in zip((nm for names in seen_names for nm in names), flat_t):
        labels_of.setdefault(name, set()).add(t)
    count, top1, top5 = {}, {}, {}
    for name, idx in labels_of.items():
        idx = [i for i in idx if 0 <= i < len(labels)]
        count[name] = sum(table[0][i] for i in idx)
        top1[name] = sum(table[1][i] for i in idx) / count[name] if count[name] else 0.0
        top5[name] = sum(table[2][i] for i in idx) / count[name] if count[name] else 0.0
    print(",".join(top1.keys()))
    print(",".join(str(v) for v in top1.values()))
    print(",".join(str(v) for v in top5.values()))
    acc1, acc5 = 100.0 * h1 / n, 100.0 * h5 / n
    logging.info(f"0-shot * Acc@1 {acc1:.3f} Acc@5 {acc5:.3f}")
    out = dict(modelnet40={"acc1": acc1, "acc5": acc5})
    return (out, {"names": list(top1), "count": count, "top1": top1, "top5": top5}) if return_per_class else out


def _cls_single(driver, test_loader, model, tokenizer, dataset_name, args, templates, input_key, with_acc5=True, class_map=False):
    from vitlens_hip import ops
    device = _device(args)
    net = _eval_model(model)
    dataset = test_loader.dataset
    print("=> encoding captions w/ templates")
    labels = dataset.idx2label
    with torch.no_grad():
        classifier = _classifier(net, tokenizer, labels, _templates(templates, dataset, driver), device)
        cmap = None
        if class_map and hasattr(dataset, "other_idx"):
            cmap = ops.class_map_from_merge(len(labels), dataset.map_to_others_idx, dataset.other_idx, device)
        hits, n = _count_topk(test_loader, net, classifier, input_key, (1, 5) if with_acc5 else (1, 2), device, class_map=cmap)
    _barrier(args)
    (h1, h5), n = _totals(hits, n)
    out = {"acc1": 100.0 * h1 / n, "acc5": 100.0 * h5 / n} if with_acc5 else {"acc1": 100.0 * h1 / n}
    logging.info(f"[{dataset_name}] : 0-shot * " + " ".join(f"Acc@{k[3:]} {v:.3f}" for k, v in out.items()))
    return out


def test_rgbd_cls_single(test_loader, model, tokenizer, dataset_name, args=None, templates=None):
    """SUN-RGBD / NYUv2 scene classification from depth (training/zero_shot.py:260-348) -> {"acc1", "acc5"} in percent.  A
    dataset with `other_idx` / `map_to_others_idx` is scored by cond_acc: those classes count as one, in the predictions and
    in the targets (the class map of ops.eval_hits)."""
    return _cls_single("test_rgbd_cls_single", test_loader, model, tokenizer, dataset_name, args, templates, "depth", class_map=True)


def _core(single, testloaders, model, tokenizer, args, single_name):
    if isinstance(testloaders, dict):
        return {dname: single(dloader, model, tokenizer, dname, args) for dname, dloader in testloaders.items()}
    return {"Single Eval": single(testloaders, model, tokenizer, single_name, args)}


def test_rgbd_cls_core(testloaders, model, tokenizer, args=None):
    return _core(test_rgbd_cls_single, testloaders, model, tokenizer, args, "Eval RGBD-CLS Dataset")


def _ids(ids, device):
    return (ids if torch.is_tensor(ids) else torch.tensor(ids)).to(device)


def test_audio_single_map(testloader, model, tokenizer, dataset_name="Eval Audio mAP", args=None, templates=None):
    """AudioSet-style multi-label evaluation (training/zero_shot.py:572-638): batch keys id / audio / target (multi-hot) ->
    MAP's result {"map", "map_cnt", "predict_results"} plus "acc1" = map.  The per-class average precision runs on the device
    (MAP(on_device=True)) while MAP_ON_DEVICE holds."""
    from open_clip.metrics import MAP
    device = _device(args)
    net = _eval_model(model)
    metric = MAP()
    metric.initialize(on_device=MAP_ON_DEVICE)
    dataset = testloader.dataset
    with torch.no_grad():
        classifier = _classifier(net, tokenizer, dataset.idx2label, _templates(templates, dataset, "test_audio_single_map"), device)
        for batch in testloader:
            feats = _audio_features(net, batch["audio"], device)
            logits = zero_shot_logits(feats, classifier, logit_scale=1.0)
            metric.compute(_ids(batch["id"], device), logits, batch["target"].to(device, non_blocking=True))
    _barrier(args)
    stats = metric.merge_results()
    stats["acc1"] = stats["map"]
    logging.info(f'[{dataset_name}] : 0-shot * mAP {stats["map"]}')
    return stats


def test_audio_single_cls(testloader, model, tokenizer, dataset_name="Eval Audio Cls", args=None, templates=None):
    """Single-label audio classification (training/zero_shot.py:641-706): batch keys id / audio / label -> Accuracy's result
    {"accuracy" (a fraction), "score_sum", "score_cnt", "predict_results"} plus "acc1" = accuracy.  Multi-hot [B, C] labels
    take the Accuracy accumulator (the value at the arg-max counts)."""
    from vitlens_hip import ops
    device = _device(args)
    net = _eval_model(model)
    print("=> encoding captions w/ templates")
    dataset = testloader.dataset
    hits, n, metric = torch.zeros(2, device=device, dtype=torch.int32), 0, None
    with torch.no_grad():
        classifier = _classifier(net, tokenizer, dataset.idx2label, _templates(templates, dataset, "test_audio_single_cls"), device)
        for batch in testloader:
            feats = _audio_features(net, batch["audio"], device)
            logits = zero_shot_logits(feats, classifier, logit_scale=1.0)
            target = batch["label"]
            if torch.is_tensor(target) and target.dim() == 2:
                if metric is None:
                    from open_clip.metrics import Accuracy
                    metric = Accuracy()
                    metric.initialize()
                metric.compute(_ids(batch["id"], device), logits, target.to(device, non_blocking=True))
            else:
                ops.eval_hits(logits, _target(target, device), (1, 2), hits=hits)
                n += feats.size(0)
    if metric is not None:
        stats = metric.merge_results()
    else:
        (h1, _), n = _totals(hits, n)
        stats = {"accuracy": h1 / n, "score_sum": float(h1), "score_cnt": n, "predict_results": {}}
    stats["acc1"] = stats["accuracy"]
    logging.info(f'[{dataset_name}] : Classification * Acc@1 {stats["accuracy"]}')
    return stats


def _rank_block(count, rank, world):
    """Rank `rank`'s contiguous block of range(count) when every rank r takes len(range(r, count, world)) items."""
    sizes = [len(range(r, count, world)) for r in range(world)]
    start = sum(sizes[:rank])
    return start, start + sizes[rank]


def test_audio_single_ret(testloader, model, tokenizer, dataset_name="Eval Audio Ret", args=None):
    """Audio-text retrieval (training/zero_shot.py:709-788): the dataset's `texts` / `text_ids` are encoded in chunks of 50 (each
    rank its block, gathered), the audio features are collected by `Recall`; -> Recall's result with img_* renamed to audio_*
    and "acc1" = the mean of the six recalls as a fraction."""
    import torch.distributed as dist
    from open_clip.metrics import Recall
    from open_clip.utils import all_gather, is_dist_avail_and_initialized
    device = _device(args)
    net = _eval_model(model)
    metric = Recall()
    dataset = testloader.dataset
    texts = dataset.texts
    with torch.no_grad():
        text_ids = torch.tensor(dataset.text_ids).to(device)
        multi = is_dist_avail_and_initialized()
        start, end = _rank_block(len(text_ids), dist.get_rank() if multi else 0, dist.get_world_size() if multi else 1)
        parts = [net.encode_text(tokenizer(list(texts[i:min(i + 50, end)])).to(device, non_blocking=True))
                 for i in range(start, end, 50)]
        text_logits = torch.cat(parts, dim=0)
        if multi:
            text_logits = all_gather(text_logits)
        metric.initialize(text_ids=text_ids, text_logits=text_logits)
        for batch in testloader:
            metric.compute(_ids(batch["uniq_id"], device), _audio_features(net, batch["audio"], device))
        stats = metric.merge_results()
    for key in list(stats.keys()):
        if key.startswith("img"):
            stats[key.replace("img", "audio")] = stats.pop(key)
    stats["acc1"] = (stats["txt_r1"] + stats["txt_r5"] + stats["txt_r10"] + stats["audio_r1"] + stats["audio_r5"]
                     + stats["audio_r10"]) / (6 * 100.0)
    logging.info("**  %s ** Eval result = %s" % (dataset_name, json.dumps(stats)))
    return stats


def test_audiotasks_core(testloaders, model, tokenizer, args=None):
    """Each loader by its dataset's `eval_metric`: "map", "acc" or "recall"."""
    fns = {"map": test_audio_single_map, "acc": test_audio_single_cls, "recall": test_audio_single_ret}
    if isinstance(testloaders, dict):
        return {dname: fns[dloader.dataset.eval_metric.lower()](dloader, model, tokenizer, dname, args)
                for dname, dloader in testloaders.items()}
    return {"Single Eval": fns[testloaders.dataset.eval_metric.lower()](testloaders, model, tokenizer, "Eval Audio Dataset", args)}


def test_tactle_cls_single(test_loader, model, tokenizer, dataset_name="Eval tag cls", args=None, templates=None):
    """Touch-and-Go material / hard-soft / rough-smooth classification (training/zero_shot.py:813-912) -> {"acc1", "acc5"} in
    percent, or {"acc1"} alone when the dataset has fewer than five classes."""
    print(test_loader.dataset.label2idx)
    return _cls_single("test_tactle_cls_single", test_loader, model, tokenizer, dataset_name, args, templates, "tactile",
                       with_acc5=len(test_loader.dataset.idx2label) >= 5)


def test_tactiletasks_core(testloaders, model, tokenizer, args=None):
    return _core(test_tactle_cls_single, testloaders, model, tokenizer, args, "Eval Tac-CLS")


def test_eeg_cls_single(test_loader, model, tokenizer, dataset_name="Eval EEG cls", args=None, templates=None):
    """ImageNet-EEG classification (training/zero_shot.py:927-1010) -> {"acc1", "acc5"} in percent."""
    return _cls_single("test_eeg_cls_single", test_loader, model, tokenizer, dataset_name, args, templates, "eeg")


def test_eegtasks_core(testloaders, model, tokenizer, args=None):
    return _core(test_eeg_cls_single, testloaders, model, tokenizer, args, "Eval EEG-CLS")


for _f in (test_zeroshot_3d_core, test_rgbd_cls_single, test_rgbd_cls_core, test_audio_single_map, test_audio_single_cls,
           test_audio_single_ret, test_audiotasks_core, test_tactle_cls_single, test_tactiletasks_core, test_eeg_cls_single,
           test_eegtasks_core):
    _f.__test__ = False          # (product functions whose names the reference chose; not pytest cases)
