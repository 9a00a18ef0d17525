"""Perceiver dropout on the host (helper, no tests): the mask rule of csrc/vl_lens_drop.hip restated in numpy on top of
tests/philox_ref.py, and the reference's arithmetic under GIVEN masks restated in fp64 torch on top of the oracle.

The mask (include/vitlens_hip.h).  Element e is kept iff its Philox4x32-10 word is >= round(p * 2^32) as a uint32; a kept value
is multiplied by 1 / (1 - p) computed in fp32.  Key = (lo32(seed), hi32(seed)); counter =
(group, lo32(sample0 + b), hi32(sample0 + b), sublayer):

    attention probability (h, i, j):   group = (h * Lq + i) * ceil(Lk / 4) + j // 4,   word j % 4
    FeedForward output (row i, col c): group = i * (D // 4) + c // 4,                  word c % 4

    sample0(step, rank, offset)      vitlens_hip.step.drop_sample0 with the Lens's tower id 2, restated
    sublayer(selfs, li, sj, ff)      the sub-layer's position in the Perceiver's forward (engine.lens_sublayer, restated)
    attn_keep / ff_keep              bool masks [B,H,Lq,Lk] / [B*n, D]
    attention / feed_forward         one sub-layer's branch under a given mask (perceiver.py:91-102, 105-154)
    perceiver                        Perceiver.forward(return_embeddings=True) under a list of masks in call order
    perceiver_masks                  that list, for a draw (seed, sample0, pa, pf)
"""
import numpy as np
import torch

import vitlens_oracle as O
from philox_ref import philox4x32_10

DROP_TOWER_LENS = 2


def sample0(step: int, rank: int, offset: int) -> int:
    """((step mod 2^27) << 36) | (rank << 22) | (2 << 20) | offset."""
    assert 0 <= rank < 1 << 14 and 0 <= offset < 1 << 20
    return ((step % (1 << 27)) << 36) | (rank << 22) | (DROP_TOWER_LENS << 20) | offset


def sublayer(self_per_cross: int, li: int, sj: int = -1, ff: bool = False) -> int:
    """Layer li: cross attention, its FeedForward, then self_per_cross x (self-attention, FeedForward), counted from 0."""
    return li * (2 + 2 * self_per_cross) + 2 * (sj + 1) + (1 if ff else 0)


def threshold(p: float) -> int:
    return int(np.rint(float(p) * 4294967296.0))


def scale32(p: float) -> np.float32:
    return np.float32(1.0) / (np.float32(1.0) - np.float32(p))


def group_words(seed: int, sample: int, sub: int, groups: np.ndarray) -> np.ndarray:
    """uint32 [len(groups), 4]: the four words of every group of one sample."""
    g = np.asarray(groups, dtype=np.uint64)
    s = int(sample) & 0xFFFFFFFFFFFFFFFF
    full = lambda v: np.full(g.shape, v, dtype=np.uint64)
    w = philox4x32_10(g, full(s & 0xFFFFFFFF), full(s >> 32), full(sub), seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    return np.stack(w, axis=-1).astype(np.uint32)


def attn_keep(seed: int, sample0_: int, sub: int, p: float, B: int, H: int, Lq: int, Lk: int) -> np.ndarray:
    kg = (Lk + 3) // 4
    out = np.empty((B, H, Lq, Lk), dtype=bool)
    groups = np.arange(H * Lq * kg, dtype=np.uint64)
    for b in range(B):
        w = group_words(seed, sample0_ + b, sub, groups).reshape(H, Lq, kg * 4)
        out[b] = w[:, :, :Lk] >= np.uint32(threshold(p))
    return out


def ff_keep(seed: int, sample0_: int, sub: int, p: float, B: int, n: int, D: int) -> np.ndarray:
    assert D % 4 == 0
    out = np.empty((B, n, D), dtype=bool)
    groups = np.arange(n * (D // 4), dtype=np.uint64)
    for b in range(B):
        out[b] = group_words(seed, sample0_ + b, sub, groups).reshape(n, D) >= np.uint32(threshold(p))
    return out.reshape(B * n, D)


# ---- the arithmetic under given masks, fp64 ------------------------------------------------------------------------------------
def _mult(keep, p, like):
    """M / (1 - p) with the kernels' fp32 scale, as a tensor of `like`'s dtype."""
    return torch.as_tensor(np.asarray(keep), dtype=like.dtype) * float(scale32(p))


def attention(q, k, v, scale: float, keep=None, p: float = 0.0):
    """q [B,H,Lq,dh], k, v [B,H,Lk,dh] -> (out [B,H,Lq,dh], lse [B,H,Lq]): P = softmax(scale q k^T) over ALL keys,
    out = (P * M / (1 - p)) v.  lse does not know about the mask."""
    s = (q @ k.transpose(-1, -2)) * scale
    lse = torch.logsumexp(s, dim=-1)
    P = torch.exp(s - lse.unsqueeze(-1))
    if keep is not None:
        P = P * _mult(keep, p, P)
    return P @ v, lse


def feed_forward(x0, y, keep=None, p: float = 0.0):
    """x1 = x0 + y * M / (1 - p): y = the second Linear's output WITH its bias, the residual is not dropped."""
    return x0 + (y if keep is None else y * _mult(keep, p, y))


def perceiver_masks(seed, sample0_, pa, pf, B, Tc, lens):
    """The masks of one forward in call order (None where a probability is 0): attention masks [B,H,n,Lk], FF masks [B*n, D]."""
    out, n, D = [], lens.num_latents, lens.latent_dim
    for li in range(lens.depth):
        k = sublayer(lens.self_per_cross, li)
        out.append(attn_keep(seed, sample0_, k, pa, B, lens.cross_heads, n, Tc) if pa > 0 else None)
        out.append(ff_keep(seed, sample0_, k + 1, pf, B, n, D) if pf > 0 else None)
        for sj in range(lens.self_per_cross):
            k = sublayer(lens.self_per_cross, li, sj)
            out.append(attn_keep(seed, sample0_, k, pa, B, lens.latent_heads, n, n) if pa > 0 else None)
            out.append(ff_keep(seed, sample0_, k + 1, pf, B, n, D) if pf > 0 else None)
    return out


def perceiver(sd, p, data, lens, masks=None, pa: float = 0.0, pf: float = 0.0):
    """oracle.perceiver with dropout under `masks` (perceiver_masks' order).  data [B,Tc,C] -> latents [B,n,D]; the dtype is
    the operands' (fp64 for a reference)."""
    B = data.shape[0]
    nsub = lens.depth * (2 + 2 * lens.self_per_cross)
    it = iter(masks if masks is not None else [None] * nsub)

    def attn(q, x, ctx, heads, dh):
        n, m = x.shape[1], ctx.shape[1]
        hf = lambda t, L: t.reshape(B, L, heads, dh).permute(0, 2, 1, 3)
        qq = O.linear(x, sd[q + "to_q.weight"])
        kk, vv = O.linear(ctx, sd[q + "to_kv.weight"]).chunk(2, dim=-1)
        o, _ = attention(hf(qq, n), hf(kk, m), hf(vv, m), dh ** -0.5, next(it), pa)
        o = o.permute(0, 2, 1, 3).reshape(B, n, heads * dh)
        return O.linear(o, sd[q + "to_out.weight"], sd[q + "to_out.bias"])

    def ff(q, x0, h):
        keep = next(it)
        y = O.lens_ff(sd, q, h)
        return feed_forward(x0, y, None if keep is None else np.asarray(keep).reshape(y.shape), pf)
    x = sd[p + "latents"].unsqueeze(0).expand(B, -1, -1)
    ln = lambda t, q: O.layer_norm(t, sd[q + ".weight"], sd[q + ".bias"])
    for i in range(lens.depth):
        q = f"{p}layers.{i}."
        x = attn(q + "0.fn.", ln(x, q + "0.norm"), ln(data, q + "0.norm_context"), lens.cross_heads, lens.cross_dim_head) + x
        x = ff(q + "1.fn.", x, ln(x, q + "1.norm"))
        for j in range(lens.self_per_cross):
            r = f"{q}2.{j}."
            h = ln(x, r + "0.norm")
            x = attn(r + "0.fn.", h, h, lens.latent_heads, lens.latent_dim_head) + x
            x = ff(r + "1.fn.", x, ln(x, r + "1.norm"))
    return x


# ---- the shapes of the GPU tests (tests/test_hip_perceiver_drop.py) and their seeds ----------------------------------------------
# name -> (B, H, Lq, Lk, dh, p, drop_seed).  tests/test_perceiver_drop_host.py checks on the host that with these seeds the kept
# fraction of every case is within 4 sigma of 1 - p.
ATTN_CASES = {
    "a": (2, 1, 64, 600, 64, 0.1, 101),      # cross attention, three key chunks, ragged last tile
    "b": (2, 4, 96, 96, 64, 0.1, 102),       # latent self-attention, one chunk
    "b50": (2, 4, 96, 96, 64, 0.5, 103),
    "c": (1, 2, 40, 77, 32, 0.1, 104),       # head dim 32, ragged queries and keys
    "d": (1, 2, 64, 64, 104, 0.1, 105),      # head dim padded to 128
}
# name -> (B, n, D, p, drop_seed): 70 rows x 128 (rows no multiple of a block), and D = 1664, the widest latent_dim of a recipe
FF_CASES = {"rows70": (2, 35, 128, 0.1, 201), "wide": (2, 5, 1664, 0.1, 202), "half": (3, 7, 64, 0.5, 203)}
ATTN_SAMPLE0 = sample0(3, 1, 5)              # a step, a rank and an offset that are not zero
ATTN_SUB = 6
TINY_SEED = 301                              # the whole tiny Perceiver (tiny_audio.npz) at pa = pf = 0.1
