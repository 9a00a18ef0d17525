"""NumPy restatements of the evaluation kernels (csrc/vl_eval.hip), in fp64 and integers:
  eval_hits          hits, per-class counts and the arg-max from an explicit stable sort of every row
  cond_acc_hits      the reference's cond_acc by its own route: top-k of the raw logits, map predictions and target, any-equal
  average_precision  scikit-learn's average_precision_score(average=None) by the threshold-group formula
  clip_mean_normalize  the mean over a sample's clips, then F.normalize"""
import numpy as np


def _order(row):
    """Class indices from the best to the worst logit: descending value, the lower index first among equals; a NaN orders as
    -inf (it is never "greater")."""
    key = np.where(np.isnan(row), -np.inf, row.astype(np.float64))
    return np.argsort(-key, kind="stable")


def eval_hits(logits, target, ks, class_map=None):
    """-> hits [2], per_class [3, C] (samples, hits at ks[0], hits at ks[1], by target), pred [B].  A sample hits at k when the
    best-placed member of its target's group stands among the first k of the sorted row; with a NaN at that member's place the
    comparisons of the kernel (nothing is greater than a NaN, nothing equals it) give rank 0."""
    logits = np.asarray(logits)
    B, C = logits.shape
    cmap = np.arange(C) if class_map is None else np.asarray(class_map)
    hits, per_class, pred = np.zeros(2, np.int64), np.zeros((3, C), np.int64), np.zeros(B, np.int64)
    for b in range(B):
        order = _order(logits[b])
        pred[b] = order[0]
        t = int(target[b])
        if t < 0 or t >= C:
            continue
        m = int(order[cmap[order] == cmap[t]][0])                       # the first member of the target's group in the sorted row
        numbers = order[~np.isnan(logits[b, order])]                    # its place among the row's numbers
        rank = 0 if np.isnan(logits[b, m]) else int(np.nonzero(numbers == m)[0][0])
        per_class[0, t] += 1
        for i, k in enumerate(ks):
            if rank < k:
                hits[i] += 1
                per_class[1 + i, t] += 1
    return hits, per_class, pred


def cond_acc_hits(logits, target, idx_mapping, merge_idx, ks):
    """Hit counts of the reference's cond_acc (training/zero_shot.py:62-81) on rows without ties among their first max(ks)
    logits: the first k classes of the sorted row and the target are mapped; a hit if any mapped prediction equals the target."""
    logits = np.asarray(logits, np.float64)
    fold = lambda c: merge_idx if c in set(idx_mapping) else c
    out = []
    for k in ks:
        n = 0
        for b in range(logits.shape[0]):
            top = np.argsort(-logits[b], kind="stable")[:k]
            n += any(fold(int(c)) == fold(int(target[b])) for c in top)
        out.append(n)
    return out


def average_precision(scores, targets):
    """Per class: the scores' distinct values in descending order are the thresholds; at threshold n, with tp_n positives and
    cnt_n samples at or above it, precision_n = tp_n / cnt_n and recall_n = tp_n / P;  AP = sum_n (recall_n - recall_{n-1})
    precision_n.  No positives: 0.0 (scikit-learn 1.7)."""
    scores, pos = np.asarray(scores, np.float64), np.asarray(targets) > 0
    out = np.zeros(scores.shape[1], np.float64)
    for c in range(scores.shape[1]):
        s, y = scores[:, c], pos[:, c]
        P = int(y.sum())
        if P == 0:
            continue
        order = np.argsort(-s, kind="stable")
        s, y = s[order], y[order]
        last = np.r_[np.nonzero(s[1:] != s[:-1])[0], len(s) - 1]            # the last sample of every group of equal scores
        tp, cnt = np.cumsum(y)[last], last + 1
        ap, prev = 0.0, 0
        for tp_n, cnt_n in zip(tp.tolist(), cnt.tolist()):
            ap += (tp_n - prev) / P * (tp_n / cnt_n)
            prev = tp_n
        out[c] = ap
    return out


def clip_mean_normalize(x, n_clip, eps=1e-12):
    x = np.asarray(x, np.float64)
    m = x.reshape(x.shape[0] // n_clip, n_clip, -1).mean(axis=1)
    return m / np.maximum(np.sqrt((m * m).sum(axis=1, keepdims=True)), eps)


def gridded_columns(N, C, seed):
    """The five kinds of class columns of the average-precision tests, cycled over the C classes: all positive, one positive,
    none, 17-level heavy ties, no ties (while N <= 2049).  Scores lie on a 2^-10 grid in [-1, 1]: all 2049 grid values stay
    distinct under float32 sigmoid, so a path that ranks sigmoid(score) sees the same tie groups."""
    rng = np.random.default_rng(seed)
    scores, targets = np.zeros((N, C), np.float32), np.zeros((N, C), np.float32)
    for c in range(C):
        kind = c % 5
        if kind == 3:
            scores[:, c] = rng.integers(-8, 9, N) / 8.0
        elif kind == 4 and N <= 2049:
            scores[:, c] = (rng.permutation(2049)[:N] - 1024) / 1024.0
        else:
            scores[:, c] = rng.integers(-1024, 1025, N) / 1024.0
        if kind == 0:
            targets[:, c] = 1.0
        elif kind == 1:
            targets[rng.integers(0, N), c] = 1.0
        elif kind >= 3:
            targets[:, c] = rng.random(N) < 0.3
    return scores, targets
