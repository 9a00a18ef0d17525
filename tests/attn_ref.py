"""Attention forward: the float64 reference, the declared rounding contract as a model, and seeded score generators.

attn_fwd_ref    explicit softmax in float64 on the kernels' own 16-bit operands, q2 = dtype(q * qscale) being the rounding
                the kernels apply as they load q.  Scores are in the log2 domain (p = 2^s; the kernels' qscale carries
                log2(e)) unless log2=False (vl_attn_fwd_f32 takes a natural-log scale).  The causal mask is top-left aligned
                (key > query masked).  Chunked over the batch so that the bench geometry fits.
attn_fwd_model  what the kernels promise and no more: exact softmax, the unnormalised P (relative to the true row maximum)
                rounded to `dtype`, P.V and the row sum exact, the result rounded to `dtype`; lse from scores of a float32
                matmul.  dtype float32: float32 arithmetic throughout.  Its distance from attn_fwd_ref is what rounding
                alone costs - the yardstick of every tolerance in test_hip_attn_fwd.py (test_attn_ref_host.py pins it).
make_scores     seeded q, k, v as contiguous [B, H, L, dh] CPU tensors of `dtype` and the qscale to pass to the kernel.
"""
import math

import torch

LOG2E = 1.4426950408889634
LN2 = math.log(2.0)
KINDS = ("normal", "ramp", "descend", "negative", "sink_first", "sink_last", "straddle")
STRADDLE_STEPS = (7.5, 8.5)           # rise of the tile maximum of even query rows, alternating


def q_rounded(q, qscale, dtype):
    """q2 = dtype(q * qscale), the product taken in float32 as the kernels do."""
    return (q.float() * float(qscale)).to(dtype)


def ref_scores(q, k, qscale, causal, dtype):
    """float64 scores q2 . k^T [B, H, Lq, Lk] with the causal mask applied (small problems: not chunked)."""
    s = q_rounded(q, qscale, dtype).double() @ k.double().transpose(-1, -2)
    return _mask(s, causal)


def _mask(s, causal):
    if causal:
        Lq, Lk = s.shape[-2:]
        s = s.masked_fill(torch.ones(Lq, Lk, dtype=torch.bool, device=s.device).triu(1), float("-inf"))
    return s


def _batch_chunk(B, H, Lq, Lk, budget=1 << 28):
    return max(1, min(B, budget // max(1, H * Lq * Lk * 8)))


def _exp(x, log2):
    return torch.exp2(x) if log2 else torch.exp(x)


def _lse(m, l, log2):
    return (m + torch.log2(l)) * LN2 if log2 else m + torch.log(l)


def attn_fwd_ref(q, k, v, qscale, causal, dtype, log2=True):
    """out [B, H, Lq, dh] float64 and lse [B, H, Lq] float64 in natural-log units."""
    B, H, Lq, _ = q.shape
    step = _batch_chunk(B, H, Lq, k.shape[2])
    outs, lses = [], []
    for b0 in range(0, B, step):
        sl = slice(b0, b0 + step)
        s = _mask(q_rounded(q[sl], qscale, dtype).double() @ k[sl].double().transpose(-1, -2), causal)
        m = s.amax(-1, keepdim=True)
        p = _exp(s - m, log2)
        l = p.sum(-1, keepdim=True)
        outs.append((p @ v[sl].double()) / l)
        lses.append(_lse(m, l, log2).squeeze(-1))
    return torch.cat(outs), torch.cat(lses)


def attn_fwd_model(q, k, v, qscale, causal, dtype, log2=True):
    """(out_model [B, H, Lq, dh] in `dtype`, lse_model [B, H, Lq] float64): the rounding contract, see the module docstring."""
    B, H, Lq, _ = q.shape
    step = _batch_chunk(B, H, Lq, k.shape[2])
    outs, lses = [], []
    for b0 in range(0, B, step):
        sl = slice(b0, b0 + step)
        q2 = q_rounded(q[sl], qscale, dtype)
        s32 = _mask(q2.float() @ k[sl].float().transpose(-1, -2), causal)
        if dtype == torch.float32:
            m = s32.amax(-1, keepdim=True)
            p = _exp(s32 - m, log2)
            l = p.sum(-1, keepdim=True)
            outs.append((p @ v[sl]) / l)
            lses.append(_lse(m, l, log2).squeeze(-1).double())
            continue
        s = _mask(q2.double() @ k[sl].double().transpose(-1, -2), causal)
        m = s.amax(-1, keepdim=True)
        p = _exp(s - m, log2)
        outs.append(((p.to(dtype).double() @ v[sl].double()) / p.sum(-1, keepdim=True)).to(dtype))
        s32 = s32.double()
        m32 = s32.amax(-1, keepdim=True)
        lses.append(_lse(m32, _exp(s32 - m32, log2).sum(-1, keepdim=True), log2).squeeze(-1))
    return torch.cat(outs), torch.cat(lses)


def straddle_gain(Lk):
    """Gain of every key in the straddle kind: 16 (t // 2) + 7.5 (t % 2) for the keys of tile t, held in two channels so that
    both parts are exact in bf16 (the sum would need nine bits beyond tile 16)."""
    t = torch.arange(Lk) // 32
    return 16.0 * (t // 2), 7.5 * (t % 2)


def make_scores(kind, B, H, Lq, Lk, dh, seed, dtype=torch.bfloat16):
    """(q, k, v, qscale): contiguous [B, H, L, dh] CPU tensors of `dtype`.

    normal      standard normal q, k, v (drawn as the token-major matrices of the backward tests' inputs), q scaled by
                dh^-0.5 log2(e) inside the kernel.
    ramp        later keys score higher (the running maximum keeps growing), one very peaked query row, one dominant key;
                q pre-scaled (qscale = 1).            } as in the backward tests'
    negative    every score about -3 dh log2 units.   } _attn_bwd_inputs
    descend     ramp reversed: the maximum sits in the first tile, later tiles underflow to 0.
    sink_first  one key (the first / the last) scores 15 log2 units above a floor that is flat to about +-0.5; every floor
    sink_last   key shares ONE value row, distinct from the sink's, so the floor's mass ((Lk - 1) 2^-15: 0.8 % at 257 keys)
                moves the output coherently.  P of a floor key is 2^-15, a half subnormal, where the sink is seen first.
    straddle    key tile t adds 16 (t // 2) + 7.5 (t % 2) to the scores of even query rows (their tile maximum rises by 7.5,
                8.5, 7.5, ... - over the kernel's 2^8 threshold every second tile), nothing to those of odd rows, whose
                scores drift by +0.25 (rows 4i + 1) or -0.25 (rows 4i + 3) per tile: one wave holds lanes above the
                threshold, lanes at 0 < mx <= 8 and lanes at mx < 0 in the same rescale branch.  Everything else in the
                scores is a pattern that repeats every 32 keys (q = +-1, k multiples of 1/64), so the steps are exact.
    sink_* and straddle pass q doubled with qscale = 0.5 (exact), so that the kernels' scaling code runs."""
    if kind not in KINDS:
        raise ValueError(f"unknown score kind {kind!r}")
    g = torch.Generator().manual_seed(seed)
    inner = H * dh
    heads = lambda t, L, c0=0: t[:, c0:c0 + inner].reshape(B, L, H, dh).permute(0, 2, 1, 3).contiguous()
    if kind == "normal":
        q2 = torch.randn(B * Lq, inner, generator=g)
        kv2 = torch.randn(B * Lk, 2 * inner, generator=g)
        return heads(q2, Lq).to(dtype), heads(kv2, Lk).to(dtype), heads(kv2, Lk, inner).to(dtype), dh ** -0.5 * LOG2E
    if kind in ("ramp", "descend", "negative"):
        q = torch.randn(B, H, Lq, dh, generator=g)
        k = torch.randn(B, H, Lk, dh, generator=g)
        v = torch.randn(B, H, Lk, dh, generator=g)
        torch.randn(B, H, Lq, dh, generator=g)                   # (the backward tests draw dO here)
        if kind == "negative":
            q = torch.ones(B, H, Lq, dh)
            k = torch.randn(B, H, Lk, dh, generator=g) - 3.0
        else:
            ramp = torch.linspace(0.0, 6.0, Lk).view(1, 1, Lk, 1)
            k = k * (1 + (ramp if kind == "ramp" else ramp.flip(2)))
            q[:, :, 0] *= 8.0
            k[:, :, Lk // 2] *= 4.0
        return q.to(dtype), k.to(dtype), v.to(dtype), 1.0
    if kind in ("sink_first", "sink_last"):
        sink = 0 if kind == "sink_first" else Lk - 1
        q = 0.5 * torch.randn(B, H, Lq, dh, generator=g)
        q[..., 0] = 1.0
        k = 0.05 * torch.randn(B, H, Lk, dh, generator=g)
        k[..., 0] = 0.0
        k[:, :, sink] = 0.0
        k[:, :, sink, 0] = 15.0
        rows = torch.randn(B, H, 2, dh, generator=g)
        v = rows[:, :, :1].expand(B, H, Lk, dh).clone()
        v[:, :, sink] = rows[:, :, 1]
        return (2.0 * q).to(dtype), k.to(dtype), v.to(dtype), 0.5
    # straddle
    if dh < 8:
        raise ValueError("straddle needs a few noise channels")
    sign = lambda *s: torch.randint(0, 2, s, generator=g).float() * 2 - 1
    q = sign(B, H, Lq, dh)
    i = torch.arange(Lq)
    even = (i % 2 == 0).float()
    q[..., 0] = even
    q[..., 1] = even
    q[..., 2] = (i % 4 == 1).float() - (i % 4 == 3).float()
    pat = torch.randint(-8, 9, (B, H, 32, dh), generator=g).float() / 64
    k = pat[:, :, torch.arange(Lk) % 32].clone()
    k[..., 0], k[..., 1] = straddle_gain(Lk)
    k[..., 2] = 0.25 * (torch.arange(Lk) // 32).float()
    v = torch.randn(B, H, Lk, dh, generator=g)
    return (2.0 * q).to(dtype), k.to(dtype), v.to(dtype), 0.5
