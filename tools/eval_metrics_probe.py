"""Time the per-class average precision of the AudioSet-style evaluation on the device against the host path it replaces:
    python tools/eval_metrics_probe.py [--out profiles/eval_metrics.json] [--rounds 5]

At N = 20 000 samples, C = 527 classes, 0.5 % positives plus one class at 40 %:
  device   `ops.average_precision` on the raw scores, device events around `iters` consecutive calls, then the read of C doubles
  host     what `open_clip.metrics.MAP.merge_results` did before: sigmoid on the device, copy of scores and targets to the host,
           scikit-learn's average_precision_score(average=None); a host clock around the whole (it ends in host work)
The two are alternated over `rounds` rounds after a warm-up of each; the median round is reported with the extremes.  Also timed:
the device path with EVERY column 50 % positive, its O(N^2) worst case.  The two paths' results are compared on the way."""
import argparse
import json
import os
import statistics
import sys
import time
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "vit-lens_amd"))


def device_ms(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters, out


def host_path(scores, targets):
    from sklearn.metrics import average_precision_score
    t0 = time.perf_counter()
    prob = torch.sigmoid(scores).cpu().numpy()
    truth = targets.cpu().numpy()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ap = average_precision_score(truth, prob, average=None)
    return (time.perf_counter() - t0) * 1e3, ap


def summary(v):
    return {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "rounds": len(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--n", type=int, default=20000)
    ap.add_argument("--classes", type=int, default=527)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("eval_metrics_probe needs a GPU")
    from vitlens_hip import ops
    N, C = a.n, a.classes
    rng = np.random.default_rng(0)
    scores = torch.from_numpy((rng.standard_normal((N, C)) * 0.1).astype(np.float32)).cuda()
    pos = rng.random((N, C)) < 0.005
    pos[:, 0] = rng.random(N) < 0.4
    targets = torch.from_numpy(pos.astype(np.float32)).cuda()
    dense = torch.from_numpy((rng.random((N, C)) < 0.5).astype(np.float32)).cuda()

    def device_path():
        return ops.average_precision(scores, targets)
    for _ in range(2):
        device_path()
    host_path(scores, targets)
    torch.cuda.synchronize()
    dev_t, host_t = [], []
    for _ in range(a.rounds):
        ms, out = device_ms(device_path, a.iters)
        t0 = time.perf_counter()
        dev_ap = out.cpu().numpy()
        read_ms = (time.perf_counter() - t0) * 1e3
        dev_t.append(ms + read_ms)
        ms, host_ap = host_path(scores, targets)
        host_t.append(ms)
    same_ties = ops.average_precision(torch.sigmoid(scores), targets).cpu().numpy()        # the host path's tie groups
    ops.average_precision(scores, dense)
    torch.cuda.synchronize()
    dense_t = [device_ms(lambda: ops.average_precision(scores, dense), 2)[0] for _ in range(3)]
    res = {"device": torch.cuda.get_device_name(0), "N": N, "C": C, "positives": int(pos.sum()), "iters_per_round": a.iters,
           "device_path": dict(summary(dev_t), what="ops.average_precision + read of C doubles"),
           "host_path": dict(summary(host_t), what="sigmoid + copy to the host + scikit-learn average_precision_score"),
           "device_path_all_columns_half_positive": dict(summary(dense_t), what="the O(N^2) worst case, device path only"),
           "max_abs_difference_of_ap": {
               "raw scores on the device, sigmoid on the host (float32 sigmoid merges distinct scores into ties)":
                   float(np.abs(dev_ap - host_ap).max()),
               "the same float32 sigmoid values on both paths": float(np.abs(same_ties - host_ap).max())},
           "map": {"device": float(dev_ap.mean()), "host": float(host_ap.mean())}}
    print(json.dumps(res, indent=1))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
