"""Localized comparison helpers: the relative error of every block of an output, not of the whole tensor.

A whole-tensor relative Frobenius error is an average.  A kernel bug confined to the part of the output one piece of code
owns (the lone 257th row of the attention kernels, a ragged last tile, an LDS chunk seam, the leftover-row launch of a
row-split GEMM) moves that average by sqrt(block share) times the block's own error and hides under a bf16-noise tolerance.
These helpers compute the error of each block on the device the tensors live on (outputs of 67 M elements never go to the
host) and name the worst block in the kernel's terms when it is out of tolerance.

Block error = ||out_blk - ref_blk|| / max(||ref_blk||, floor * ||ref|| * sqrt(n_blk / n)): the second term is the norm the
block would have if the reference's energy were spread evenly, so blocks that are nearly zero in the reference (ReLU, the
negative side of GELU, the last keys under a causal mask) are measured against a fraction of their fair share, not against
their own tiny norm, and cannot flake.
"""
import torch

FLOOR = 0.25


def _bounds(n, step, extra):
    """Block edges along one axis: every `step`, the end, and both ends of every extra range (which thereby gets its own
    blocks, cut out of the regular ones around it)."""
    edges = set(range(0, n, step)) | {n}
    for a, b in extra:
        if not 0 <= a < b <= n:
            raise ValueError(f"extra range {a}:{b} outside 0:{n}")
        edges |= {a, b}
    return sorted(edges)


def _segment_sums(x, edges, dim):
    """Sums of x over the segments [edges[i], edges[i+1]) of dimension dim (on x's device)."""
    n = x.shape[dim]
    idx = torch.bucketize(torch.arange(n, device=x.device), torch.tensor(edges[1:-1], device=x.device), right=True)
    shape = list(x.shape)
    shape[dim] = len(edges) - 1
    return torch.zeros(shape, dtype=x.dtype, device=x.device).index_add_(dim, idx, x)


def _ratio(d2, r2, sizes, n, floor):
    """Block errors from per-block sums of squared differences d2 and squared reference r2 (sizes: elements per block)."""
    fair = r2.sum() * sizes / float(n)
    return (d2 / torch.maximum(r2, floor * floor * fair).clamp_min(1e-300)).sqrt()


def _diff(out, ref):
    r = ref.to(torch.float64 if ref.dtype == torch.float64 else torch.float32)
    return out.to(r.dtype) - r, r


def _block_errors(out, ref, row_edges, col_edges, floor):
    if out.shape != ref.shape or out.dim() != 2:
        raise ValueError(f"block errors need two 2-D tensors of one shape, got {tuple(out.shape)} and {tuple(ref.shape)}")
    d, r = _diff(out, ref)
    d2 = _segment_sums(_segment_sums(d * d, col_edges, 1), row_edges, 0)
    del d
    r2 = _segment_sums(_segment_sums(r * r, col_edges, 1), row_edges, 0)
    rows = torch.tensor(row_edges, dtype=r2.dtype, device=r2.device).diff()
    cols = torch.tensor(col_edges, dtype=r2.dtype, device=r2.device).diff()
    return _ratio(d2, r2, rows[:, None] * cols[None, :], ref.numel(), floor)


def block_relerr(out, ref, rows, cols, extra=(), floor=FLOOR):
    """Relative error of every rows x cols block of the 2-D out against ref (plus the blocks extra cuts out).
    extra: ("rows", a, b) / ("cols", a, b) ranges that get blocks of their own.
    Returns (worst error, (r0, r1, c0, c1) of that block).  NaN in out makes the worst error NaN."""
    M, N = out.shape
    xr = [(a, b) for kind, a, b in extra if kind == "rows"]
    xc = [(a, b) for kind, a, b in extra if kind == "cols"]
    if len(xr) + len(xc) != len(extra):
        raise ValueError("extra ranges are ('rows', a, b) or ('cols', a, b)")
    re, ce = _bounds(M, rows, xr), _bounds(N, cols, xc)
    e = _block_errors(out, ref, re, ce, floor)
    flat = e.reshape(-1)
    i = int(torch.where(torch.isnan(flat), torch.full_like(flat, float("inf")), flat).argmax())
    bi, bj = divmod(i, len(ce) - 1)
    return float(flat[i]), (re[bi], re[bi + 1], ce[bj], ce[bj + 1])


def assert_blocks(out, ref, tol, rows, cols, extra=(), floor=FLOOR, what=""):
    """Every block within tol; the failure names the worst block, e.g. 'rows 10240:10496, cols 768:1024'.
    Returns the worst block error (for the measured values the tolerances are set from)."""
    worst, (r0, r1, c0, c1) = block_relerr(out, ref, rows, cols, extra, floor)
    assert worst <= tol, f"{what + ': ' if what else ''}block rows {r0}:{r1}, cols {c0}:{c1} has relative error {worst:.3e} > {tol:.1e}"
    return worst


def _heads(x, B, H, L):
    """[B, H, L, dh] (heads layout) or a token-major [B*L, H*dh] matrix -> [B, H, L, dh] view."""
    if x.dim() == 4:
        if tuple(x.shape[:3]) != (B, H, L):
            raise ValueError(f"expected [{B}, {H}, {L}, dh], got {tuple(x.shape)}")
        return x
    if x.dim() != 2 or x.shape[0] != B * L or x.shape[1] % H:
        raise ValueError(f"expected a token-major [{B * L}, H*dh] matrix, got {tuple(x.shape)}")
    return x.reshape(B, L, H, x.shape[1] // H).permute(0, 2, 1, 3)


def attn_block_relerr(out, ref, B, H, L, tile=32, floor=FLOOR):
    """Per-block relative error of an attention output or gradient; out and ref each [B, H, L, dh] or token-major
    [B*L, H*dh].  Blocks: (b, h, tile-row tile); the rows beyond whole tiles (the lone 257th row, a ragged last tile) are a
    block of their own.  Returns (worst error, (b, h, r0, r1))."""
    o, r = _heads(out, B, H, L), _heads(ref, B, H, L)
    if o.shape != r.shape:
        raise ValueError(f"shapes differ: {tuple(o.shape)} vs {tuple(r.shape)}")
    edges = _bounds(L, tile, ())
    d, rf = _diff(o, r)
    d2 = _segment_sums((d * d).sum(-1), edges, 2)
    del d
    r2 = _segment_sums((rf * rf).sum(-1), edges, 2)
    sizes = torch.tensor(edges, dtype=r2.dtype, device=r2.device).diff() * o.shape[3]
    e = _ratio(d2, r2, sizes, o.numel(), floor)
    nt = len(edges) - 1
    flat = e.reshape(-1)
    i = int(torch.where(torch.isnan(flat), torch.full_like(flat, float("inf")), flat).argmax())
    bh, t = divmod(i, nt)
    return float(flat[i]), (bh // H, bh % H, edges[t], edges[t + 1])


def assert_attn_blocks(out, ref, tol, B, H, L, rows="rows", tile=32, floor=FLOOR, what=""):
    """Every (b, h, row tile) block within tol; the failure names it in the kernel's terms, e.g. 'b=1 h=3 keys 256:257'
    (rows: what the L axis holds - 'queries' or 'keys').  Returns the worst block error."""
    worst, (b, h, r0, r1) = attn_block_relerr(out, ref, B, H, L, tile, floor)
    assert worst <= tol, f"{what + ': ' if what else ''}b={b} h={h} {rows} {r0}:{r1} has relative error {worst:.3e} > {tol:.1e}"
    return worst
