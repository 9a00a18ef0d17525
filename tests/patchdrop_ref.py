"""Patch dropout on the host (helper, no tests): the reference's PatchDropout (open_clip/transformer.py:53-90) restated on top
of the oracle, and the device key rule of vl_patch_keep / vitlens_hip.step restated in numpy on top of tests/philox_ref.py.

    keep_count(T, p)                 the kept-token count, the reference's expression in Python floats
    keep_indices(keys, K)            rand.topk(K).indices
    vit_trunk_keep(...)              O.vit_trunk with the kept rows gathered after the positional add, before ln_pre
    philox_keys / philox_keep        vl_patch_keep's own keys (keys == NULL) and the selection it makes of them
    sample0(step, rank, tower, o)    the fused steps' sample number (vitlens_hip.step.drop_sample0), restated
"""
import numpy as np
import torch

import vitlens_oracle as O
from philox_ref import philox4x32_10


def keep_count(T: int, p: float) -> int:
    keep_prob = 1 - p
    return max(1, int(T * keep_prob))


def keep_indices(keys: torch.Tensor, K: int) -> torch.Tensor:
    return keys.topk(K, dim=-1).indices


def inverse(keep: torch.Tensor, T: int) -> torch.Tensor:
    """inv[b, t] = j + 1 where keep[b, j] == t, else 0."""
    B, K = keep.shape
    inv = torch.zeros(B, T, dtype=torch.int64)
    inv.scatter_(1, keep.long(), torch.arange(1, K + 1).expand(B, K))
    return inv


def vit_trunk_keep(sd, p, tokens, spec, keep, use_orig_pos=True, pos2=None):
    """tokens [B,T,D] (pos2 [T,D]: the adapter's positional table, added to the tokens first) -> features [B,E]; keep int
    [B,K].  [cls; tokens] + positional_embedding -> x[arange(B)[:,None], keep] on the rows behind the class token -> ln_pre
    -> blocks -> ln_post(x[:,0]) @ proj."""
    N = tokens.shape[0]
    if pos2 is not None:
        tokens = tokens + pos2
    cls = sd[p + "class_embedding"].view(1, 1, -1).expand(N, 1, -1)
    x = torch.cat([cls, tokens], dim=1)
    if use_orig_pos:
        x = x + sd[p + "positional_embedding"]
    c, x = x[:, :1], x[:, 1:]
    x = x[torch.arange(N)[:, None], keep.long()]
    x = torch.cat([c, x], dim=1)
    x = O.layer_norm(x, sd[p + "ln_pre.weight"], sd[p + "ln_pre.bias"])
    x = O.transformer(sd, p + "transformer.", x, spec.layers, spec.heads)
    pooled = O.layer_norm(x[:, 0], sd[p + "ln_post.weight"], sd[p + "ln_post.bias"])
    return pooled @ sd[p + "proj"]


# ---- the device key rule ---------------------------------------------------------------------------------------------------
def philox_keys(seed: int, sample0: int, B: int, T: int) -> np.ndarray:
    """uint32 [B,T]: the key of (b, t) = word t & 3 of Philox4x32-10, counter (t >> 2, lo32(s), hi32(s), 0) with s = sample0 + b
    (64-bit, wrapping), key words (lo32(seed), hi32(seed))."""
    groups = (T + 3) // 4
    g = np.arange(groups, dtype=np.uint64)
    out = np.empty((B, T), dtype=np.uint32)
    for b in range(B):
        s = (int(sample0) + b) & 0xFFFFFFFFFFFFFFFF
        lo, hi = np.full(groups, s & 0xFFFFFFFF, dtype=np.uint64), np.full(groups, s >> 32, dtype=np.uint64)
        w = np.stack(philox4x32_10(g, lo, hi, np.zeros(groups, dtype=np.uint64), seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF), axis=1)
        out[b] = w.reshape(-1)[:T].astype(np.uint32)
    return out


def select_desc(keys: np.ndarray, K: int) -> np.ndarray:
    """The K largest per row, largest first, ties to the lower index (a stable sort of the negated keys)."""
    order = np.argsort(-keys.astype(np.int64), axis=1, kind="stable")
    return order[:, :K].astype(np.int32)


def philox_keep(seed: int, sample0: int, B: int, T: int, K: int) -> np.ndarray:
    return select_desc(philox_keys(seed, sample0, B, T), K)


def sample0(step: int, rank: int, tower: int, offset: int) -> int:
    """((step mod 2^27) << 36) | (rank << 22) | (tower << 20) | offset   (tower: 0 = visual, 1 = image)."""
    assert 0 <= rank < 1 << 14 and 0 <= tower < 4 and 0 <= offset < 1 << 20
    return ((step % (1 << 27)) << 36) | (rank << 22) | (tower << 20) | offset
