"""fp64 references of the row-wise kernels (csrc/vl_rows.hip, the LayerNorm backward of csrc/vl_bwd.hip), in plain torch, on
the operands as the kernels read them: a bf16 or fp16 operand is converted exactly (every such value is an fp64 value), an fp32
one likewise, and nothing is rounded on the way to the result.  They run on whichever device their operands live on.

Checked on the host by tests/test_rows_ref_host.py (the backward against fp64 autograd of torch's layer_norm, the sparse form
against the dense one on a zero-filled residual gradient); used on the GPU by tests/test_hip_rows.py."""
import torch


def f64(t):
    return None if t is None else t.to(torch.float64)


def layernorm_fwd(x, w, b, eps=1e-5):
    """x [rows, D] -> (y, mean, rstd): y = (x - mean) * rstd * w + b, biased variance, eps inside the root."""
    x, w, b = f64(x), f64(w), f64(b)
    mean = x.mean(-1)
    var = ((x - mean[:, None]) ** 2).mean(-1)
    rstd = (var + eps).rsqrt()
    return (x - mean[:, None]) * rstd[:, None] * w + b, mean, rstd


def row_stats(x, eps=1e-5):
    """(mean, rstd) of the rows of x, two-pass."""
    _, mean, rstd = layernorm_fwd(x, torch.ones(x.shape[-1], device=x.device), torch.zeros(x.shape[-1], device=x.device), eps)
    return mean, rstd


def assemble(tokens, cls, pos, pos2=None):
    """Token assembly in fp64: tokens [B, T, D], cls [D], pos [T+1, D], pos2 [T, D] or None -> [B*(T+1), D];
    row (b, 0) = cls + pos[0], row (b, l) = tokens[b, l-1] + pos[l] (+ pos2[l-1])."""
    t = f64(tokens)
    B, T, D = t.shape
    if pos2 is not None:
        t = t + f64(pos2)
    x = torch.cat([f64(cls).expand(B, 1, D), t], 1) + f64(pos)
    return x.reshape(B * (T + 1), D)


def assemble_f32(tokens, cls, pos, pos2=None):
    """The same in fp32 in the kernel's order, (token + pos) + pos2: what `xpre` must hold bit for bit."""
    t = tokens.float()
    B, T, D = t.shape
    rows = t + pos[1:].float()
    if pos2 is not None:
        rows = rows + pos2.float()
    first = (cls.float() + pos[0].float()).expand(B, 1, D)
    return torch.cat([first, rows], 1).reshape(B * (T + 1), D)


def layernorm_bwd(dy, x, mean, rstd, w, dres=None):
    """dx = rstd * (g - mean(g) - xhat * mean(g * xhat)) + dres with g = dy * w, xhat = (x - mean) * rstd; mean / rstd as GIVEN
    (the kernel reads the saved statistics, it does not recompute them).  dres [rows, D] or None."""
    dy, x, w, mean, rstd = f64(dy), f64(x), f64(w), f64(mean), f64(rstd)
    g = dy * w
    xh = (x - mean[:, None]) * rstd[:, None]
    dx = rstd[:, None] * (g - g.mean(-1, keepdim=True) - xh * (g * xh).mean(-1, keepdim=True))
    return dx if dres is None else dx + f64(dres)


def layernorm_bwd_sparse(dy, x, mean, rstd, w, dres, dres_every):
    """The sparse-residual form: row i * dres_every adds row i of dres, every other row adds nothing."""
    dx = layernorm_bwd(dy, x, mean, rstd, w)
    n = (dx.shape[0] + dres_every - 1) // dres_every
    dx[::dres_every] += f64(dres)[:n]
    return dx


def batch_rowsum(x, out0, B, T, D, batch_stride_rows, row_offset):
    """out0 [T, D] + sum over b of x[b * batch_stride_rows + row_offset + t, :]; x [rows, D]."""
    x = f64(x)
    idx = (torch.arange(B, device=x.device)[:, None] * batch_stride_rows + row_offset + torch.arange(T, device=x.device)[None, :])
    return f64(out0) + x[idx.reshape(-1)].reshape(B, T, D).sum(0)


def batch_rowsum_abs(x, out0, B, T, D, batch_stride_rows, row_offset):
    """sum_b |x_b| + |out0|: what the error bound of a sequential fp32 sum scales with."""
    return batch_rowsum(x.abs(), out0.abs(), B, T, D, batch_stride_rows, row_offset)


def slice_partials(x):
    """What vl_gemm_res_rowstats_bf16 leaves per row: fp32 (sum, sum of squares) of every 64-column slice of the stored bf16
    row, flat [rows * (D // 64) * 2].  Computed in fp64 and rounded once: each partial is within half an fp32 ulp of exact."""
    rows, D = x.shape
    s = f64(x).reshape(rows, D // 64, 64)
    return torch.stack([s.sum(-1), (s * s).sum(-1)], -1).float().reshape(-1)


def _randn(rows, D, seed):
    return torch.randn(rows, D, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


def ill_conditioned_rows(D=1024):
    """The rows test_hip_rows.py plants among the main rows of ln_row_stats (bf16): four at offset 1000 with sigma 4, four at
    offset 40 with sigma 1.5, one constant row."""
    far = (1000 + 4 * _randn(4, D, 30)).bfloat16()
    near = (40 + 1.5 * _randn(4, D, 31)).bfloat16()
    const = torch.full((1, D), 3.140625).bfloat16()
    return far, near, const


def one_pass_fp32(x, eps=1e-5):
    """row_stats_kernel's first branch WITHOUT its fallback, emulated in fp32: slice partials summed in slice order,
    mean = s1 / D, var = max(E[x^2] - mean^2, 0).  Returns (mean, rstd, takes_fallback)."""
    rows, D = x.shape
    part = slice_partials(x).reshape(rows, D // 64, 2)
    s1 = torch.zeros(rows); s2 = torch.zeros(rows)
    for i in range(D // 64):
        s1 = s1 + part[:, i, 0]; s2 = s2 + part[:, i, 1]
    inv = torch.tensor(1.0 / D, dtype=torch.float32)
    mu, ex2 = s1 * inv, s2 * inv
    var = torch.clamp((ex2.double() - mu.double() * mu.double()).float(), min=0.0)      # fmaf(-mu, mu, ex2): one rounding
    return mu, (var + eps).rsqrt(), var < 1e-3 * ex2
