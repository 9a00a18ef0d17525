"""Contrastive-loss kernels (csrc/vl_loss.hip): float64 references, float32 models of the kernels' own order of operations,
per-element error bounds that are derived, and the seeded inputs and case lists of their tests.  Plain torch / numpy only;
nothing here needs a GPU or the package (tests/test_loss_ref_host.py runs all of it on the CPU, tests/test_hip_loss_kernels.py
holds the kernels to it).

References (float64 torch, from the fp32 logits as the kernels see them; `keep` = simmask_ref.keep_mask, None = unmasked):
    row_lse, col_lse, diag, loss, grad (G before any rounding), dscale, l2norm_bwd, split_bf16x3 (exact bits), transpose_bf16,
    colsum.  The masked loss is simmask_ref.pair_loss itself (on x = logits, y = I, scale = 1: exact in float64).

Models (numpy float32, one rounding per kernel operation, np.exp / np.log for __expf / __logf):
    row_lse_model      64 lane-strided online (max, sum) pairs, then the xor butterfly with its -inf guards
    col_lse_model      col_part_kernel's 64-row chunks, then col_comb_kernel's serial combine
    grad_model         grad_kernel's per-element formula
    dscale_model       grad_kernel's per-thread fmaf chain, wave butterfly, (red0 + red1) + (red2 + red3), part_finalize_kernel
    ce_reduce_model    ce_reduce_kernel's 256 strided partial sums
The models say what float32 arithmetic in that order gives; the bounds below have to hold for them on every input family at
every shape (checked on the CPU) before a kernel is held to them.

Bounds.  u = 2^-24 (half an fp32 ulp, relative).  Every bound is absolute, computed per element from the float64 reference:

  lse_bound    lse = m + log(s), s = sum_i exp(l_i - m) built by online rescaling.  Element i reaches s through a chain of
               factors exp(delta_k), delta_k <= 0, sum_k delta_k = l_i - m.  Each factor errs (relative) by
                   u |delta| (the subtraction) + 2 u |delta| (__expf = v_exp_f32(x * log2e): the product's rounding and the
                   constant's, both moved through 2^x) + EXP_ALLOW (v_exp_f32 itself),
               each rescale adds a multiplication and an addition (2 u), hence
                   rel(s) <= 3 u sum_i p_i |l_i - m|  +  N (EXP_ALLOW + 2 u),      p = softmax, N = rescale steps on a path:
               rows N = ceil(C / 64) + 6 (lane loop + butterfly), columns N = min(R, 64) + ceil(R / 64).  sum_i p_i |l_i - m| is
               the part that grows with the size of the logits (x e^-x <= 1 / e per element, so it stays below C / e).
               A term the hardware exponential flushes (below 2^-126) is lost against s >= 1: nothing to add.
               log: v_log_f32 and the product with ln 2: (LOG_ALLOW + 2 u) max(log s, 1); the final addition u |lse|.
               EXP_ALLOW = LOG_ALLOW = 2^-23: the instruction set documents both instructions as accurate to 1 ulp, and that is
               also what the model's np.exp / np.log give, so the CPU check of the model exercises the same allowance.  This is
               the one part of the bound that is an allowance and not a derivation; the factor is 1 (x documented accuracy).
               Worst error / bound: the float32 model on the CPU 0.473 (rows) and 0.561 (columns); the kernels on the MI355X 0.473
               (rows, descend 64 x 64) and 0.570 (columns, sink_first 4 x 63).
  grad_bound   g = sum over the two terms of w / R (exp(l - lse) - hot), lse the fp32 statistic the kernel is GIVEN (the
               reference's, rounded: u |lse| on the exponent).  delta = fp32 error of g:
                   per term |w| / R [ p (u |lse| + 4 u |l - lse| + EXP_ALLOW) + FLUSH + 5 u |p - hot| ]   +   u |g|
               p eta is ABSOLUTE on the diagonal (p - 1 cancels, the error of p does not); FLUSH = 2^-126 for a probability
               the exponential flushes to 0; 5 u: the subtraction, 1 / R, w rounded to fp32, and the two products; u |g|: the sum
               of the terms.  G and GT are bf16: |G - g| <= h(|g| + delta) + delta + FLUSH, h(v) = 2^(floor(log2 v) - 8) the
               half ulp of bf16 (8 significant bits) in v's binade: between 2^-9 v and 2^-8 v.  (A bound of 2^-9 |g| - half of
               2^-8, the constant tests/gemm_ref.py uses and its GEMMs reach to 0.99 - is not one round-to-nearest can meet:
               the exactly rounded model is at 1.99 of it on `normal` 1040 x 1040.  h is the exact figure, never larger than
               2^-8 |g|, and leaves a second ulp no room.)
  dscale_bound proportional to sum |g l|, not |sum g l|: [ (A + 3) u sum |g l| + sum |l| delta ] / scale + u (|in| + |out|),
               A = 4 + 6 + 2 + ceil(blocks / 1024) + 6 + 16 additions on a value's path through both stages.
  ce_reduce_bound, l2norm_bwd_bound, colsum_bound: rounding counts of the respective kernels, beside the functions.
No bound uses anything a kernel returns."""
import math

import numpy as np
import torch

import simmask_ref as SR

U24 = 2.0 ** -24
EXP_ALLOW = LOG_ALLOW = 2.0 ** -23
FLUSH = 2.0 ** -126
F64 = torch.float64


# ---- cases (shared by the host test, which checks them, and the GPU test, which runs them) ------------------------------------
FAMILIES = ("normal", "scale100", "ramp", "descend", "sink_first", "sink_last", "negative", "flat")
#          R,    C,   off      edge
SHAPES = [(1, 1, 0),          # C < 64: 63 idle lanes, both -inf guards of the butterfly at every level
          (3, 5, 0),          # C < 64; R % 4 != 0: a block with an idle wave
          (4, 63, 0),         # C < 64: one idle lane (guard of one side only, at the first level)
          (5, 65, 0),         # one lane with a second element
          (64, 64, 0),        # exactly one 64-row chunk, every lane one element
          (65, 257, 0),       # a second chunk of one row; a second 256-column block of one column
          (130, 300, 0),      # rectangular, three chunks, ragged everything
          (257, 257, 0),      # R above 256: ce_reduce_kernel's second sweep
          (48, 144, 96),      # --local-loss geometry: label columns 96..143
          (48, 144, 0),       # the same block as rank 0 sees it
          (1040, 1040, 0)]    # 33 x 33 = 1089 gradient blocks (34 x 34 with the pad columns): part_finalize_kernel's second sweep
GRAD_MODES = ("both", "g_only", "gt_only")
#                 R,   C,  ldo, pad (ldi - C), offset of the view in units of 4 bytes, kernel      edge
TRANSPOSE_CASES = [(70, 45, 128, 8, 0, "small"),        # the shape test_transpose_to_bf16 had
                   (255, 64, 256, 8, 0, "small"),       # R = 255: one row short of the 64-column kernel
                   (256, 64, 256, 8, 0, "tile64"),      # R = 256: the first R that takes it
                   (256, 100, 256, 8, 0, "small"),      # C % 64 != 0 at R >= 256
                   (256, 64, 256, 3, 0, "small"),       # ldi % 8 != 0 at R >= 256
                   (256, 64, 256, 8, 1, "small"),       # a view 4 bytes off 16-byte alignment at R >= 256
                   (300, 128, 304, 8, 0, "tile64"),     # ldo = R rounded up to 8, R % 64 != 0: a partly stored 64-row tile
                   (300, 64, 320, 8, 0, "tile64")]      # the second slab's loop breaks at r0 = 320 >= ldo
#               R,   C,  ldo   (nslab = ceil(ldo / 256): 1, 8, 9, 11 - the unrolled loop of colws_finalize_kernel with and without tail)
COLSUM_CASES = [(256, 64, 256), (2040, 64, 2048), (2300, 128, 2304), (2810, 64, 2816)]
L2_ROWS, L2_DIMS = (1, 4, 5, 9), (1, 63, 64, 65, 768)
#             R,   C,  off, w_col, chunk_rows
PAIR_CASES = [(70, 70, 0, 0.5, 0), (130, 300, 0, 0.5, 0), (48, 144, 96, 0.0, 0), (200, 200, 0, 0.5, 64)]
SCALES = ("f100", "f14", "dev100")          # the float 100.0, the float 14.2857, a device log-scale tensor ln 100


def transpose_kernel(R, C, ldo, ldi, ptr_in, ptr_out):
    """vl_transpose_to_bf16's dispatch, restated."""
    fused = R >= 256 and ldo % 8 == 0 and C % 64 == 0 and ldi % 8 == 0 and (ptr_in | ptr_out) % 16 == 0
    return "tile64" if fused else "small"


def grad_grid(R, C, ldg, ldgt, need_g=True, need_gt=True):
    """(gc, gr) of grad_kernel's launch: the pad columns of G and GT are written by blocks of their own."""
    return (max(ldg if need_g else 0, C) + 31) // 32, (max(ldgt if need_gt else 0, R) + 31) // 32


def branch_conditions():
    """Every branch condition of vl_loss.hip the tests claim to reach -> the cases that meet it (the host test asserts none is
    empty; the table in tests/test_hip_loss_kernels.py names the kernels)."""
    pad64 = lambda n: (n + 63) // 64 * 64
    return {
        "C < 64": [s for s in SHAPES if s[1] < 64],
        "C >= 64 and C % 64 != 0": [s for s in SHAPES if s[1] > 64 and s[1] % 64],
        "R % 4 != 0": [s for s in SHAPES if s[0] % 4],
        "R % 64 != 0": [s for s in SHAPES if s[0] % 64],
        "R > 64 (col_comb_kernel combines chunks)": [s for s in SHAPES if s[0] > 64],
        "C > 256 (a second column block)": [s for s in SHAPES if s[1] > 256],
        "ce_reduce_kernel: R < 256": [r for r in CE_REDUCE_ROWS if r < 256],
        "ce_reduce_kernel: R == 256": [r for r in CE_REDUCE_ROWS if r == 256],
        "ce_reduce_kernel: R > 256": [r for r in CE_REDUCE_ROWS if r > 256],
        "more than 1024 partials": [s for s in SHAPES if math.prod(grad_grid(s[0], s[1], pad64(s[1]), pad64(s[0]))) > 1024],
        "label_off != 0": [s for s in SHAPES if s[2]],
        "nslab % 8 != 0": [c for c in COLSUM_CASES if ((c[2] + 255) // 256) % 8 and (c[2] + 255) // 256 > 8],
        "nslab % 8 == 0": [c for c in COLSUM_CASES if ((c[2] + 255) // 256) % 8 == 0],
        "nslab < 8": [c for c in COLSUM_CASES if (c[2] + 255) // 256 < 8],
        "transpose_bf16_kernel x {f32, bf16}": [c for c in TRANSPOSE_CASES if c[5] == "small"],
        "transpose64_kernel x {f32, bf16}": [c for c in TRANSPOSE_CASES if c[5] == "tile64"],
        "transpose64_kernel: r0 >= ldo break": [c for c in TRANSPOSE_CASES if c[5] == "tile64" and (c[2] + 255) // 256 * 256 - c[2] >= 64],
        "transpose64_kernel: a partly stored tile (ldo % 64 != 0)": [c for c in TRANSPOSE_CASES if c[5] == "tile64" and c[2] % 64],
        "G-only launch": [m for m in GRAD_MODES if m == "g_only"],
        "GT-only launch": [m for m in GRAD_MODES if m == "gt_only"],
    }


CE_REDUCE_ROWS = (5, 255, 256, 257, 1040)


# ---- inputs -------------------------------------------------------------------------------------------------------------------
def make_logits(family, R, C, off=0):
    """Seeded fp32 logits [R, C] of a family.  Finite always: a row of -inf only is outside the kernels' domain."""
    g = torch.Generator().manual_seed(7919 * R + 31 * C + off + FAMILIES.index(family))
    r, c = torch.arange(R, dtype=F64)[:, None], torch.arange(C, dtype=F64)[None, :]
    if family == "normal":
        lg = 4.0 * torch.randn(R, C, generator=g, dtype=F64)
    elif family == "scale100":
        t, s = SR.clustered(C, 5000 + C)
        lg = 100.0 * (t[off:off + R].double() @ s.double().t())
    elif family in ("ramp", "descend"):          # ascending along every row AND column: every element a new running maximum
        lg = -60.0 + 120.0 * (r + c) / max(1, R + C - 2) + 1e-3 * torch.rand(R, C, generator=g, dtype=F64) / max(1, R + C)
        if family == "descend":
            lg = -lg
    elif family in ("sink_first", "sink_last"):  # one +90 per row among values near -90: exp(-180) flushes, the sum is exactly 1
        lg = -90.0 + 0.5 * torch.randn(R, C, generator=g, dtype=F64)
        lg[:, 0 if family == "sink_first" else C - 1] = 90.0
    elif family == "negative":
        lg = -95.0 + 0.5 * torch.randn(R, C, generator=g, dtype=F64)
    elif family == "flat":                       # lse = v + log C
        lg = torch.full((R, C), 3.25, dtype=F64)
    else:
        raise ValueError(family)
    return lg.float()


# ---- float64 references ------------------------------------------------------------------------------------------------------
def _masked(lg, keep):
    lg = lg.double()
    return lg if keep is None else lg * keep.to(F64)


def _hot(R, C, off):
    return torch.arange(C)[None, :] == (torch.arange(R)[:, None] + off)


def row_lse(lg, keep=None):
    return torch.logsumexp(_masked(lg, keep), dim=1)


def col_lse(lg, keep=None):
    """Every column's, before step._label_columns_only."""
    return torch.logsumexp(_masked(lg, keep), dim=0)


def diag(lg, off=0):
    """lg[r, r + off] (0 where that column does not exist, as the kernel stores)."""
    R, C = lg.shape
    c = torch.arange(R) + off
    ok = (c >= 0) & (c < C)
    return torch.where(ok, lg.double()[torch.arange(R), c.clamp(0, C - 1)], torch.zeros(R, dtype=F64))


def label_columns_only(cl, off, R):
    """step._label_columns_only: +inf for a column that is no row's label."""
    cl = cl.clone()
    cl[:max(off, 0)] = float("inf")
    cl[off + R:] = float("inf")
    return cl


def loss(lg, off=0, w_row=0.5, w_col=0.5, keep=None):
    """w_row mean_r(row_lse[r] - diag[r]) + w_col mean_r(col_lse[r + off] - diag[r])."""
    if keep is not None:
        return SR.pair_loss(lg.double(), torch.eye(lg.shape[1], dtype=F64), 1.0, keep, off, w_row, w_col)
    R = lg.shape[0]
    d = diag(lg, off)
    out = w_row * (row_lse(lg) - d).mean()
    if w_col:
        out = out + w_col * (col_lse(lg)[torch.arange(R) + off] - d).mean()
    return out


def loss_from_stats(rl, cl, dg, R, C, off, w_row, w_col):
    """The reduction alone, from GIVEN statistics (rl / cl None: that term is absent)."""
    dg = dg.double()
    out = torch.zeros((), dtype=F64)
    if rl is not None:
        out = out + w_row * (rl.double() - dg).sum()
    if cl is not None:
        c = torch.arange(R) + off
        ok = (c >= 0) & (c < C)
        out = out + w_col * (cl.double()[c[ok]] - dg[ok]).sum()
    return out / R


def grad_terms(lg, off, rl, cl, w_row, w_col, keep=None):
    """The two terms of dL/dlogits from statistics rl / cl (None: absent; cl[c] = +inf: a column term of exactly 0), before any
    rounding, and what grad_bound needs of them: [(w, p, arg, lse, hot)]."""
    R, C = lg.shape
    l = _masked(lg, keep)
    hot = _hot(R, C, off).to(F64)
    terms = []
    for w, s in ((w_row, None if rl is None else rl.double()[:, None].expand(R, C)),
                 (w_col, None if cl is None else cl.double()[None, :].expand(R, C))):
        if s is not None:
            arg = torch.where(torch.isinf(s), torch.full_like(l, -float("inf")), l - s)
            terms.append((float(w), torch.exp(arg), arg, s, hot))
    return terms


def grad(lg, off=0, w_row=0.5, w_col=0.5, keep=None, rl=None, cl=None, label_cols_only=True):
    """G = dL/dlogits, float64.  rl / cl: statistics to use instead of the exact ones (cl with +inf allowed)."""
    R, C = lg.shape
    rl = (row_lse(lg, keep) if w_row else None) if rl is None else rl
    if cl is None and w_col:
        cl = col_lse(lg, keep)
        cl = label_columns_only(cl, off, R) if label_cols_only else cl
    g = torch.zeros(R, C, dtype=F64)
    for w, p, _, _, hot in grad_terms(lg, off, rl, cl if w_col else None, w_row, w_col, keep):
        g = g + w / R * (p - hot)
    return g if keep is None else g * keep.to(F64)


def dscale(g, lg, scale, keep=None):
    """d/dscale = sum(G l) / scale."""
    return float((g * _masked(lg, keep)).sum() / scale)


def l2norm_bwd(f, df, norms, eps=1e-12):
    """Backward of F.normalize from its saved output f and norms: (df - f <f, df>) / max(norm, eps)."""
    f, df = f.double(), df.double()
    return (df - f * (f * df).sum(-1, keepdim=True)) / norms.double().clamp_min(eps)[:, None]


def split_bf16x3(x, pattern):
    """bf16 [R, 3D], the exact bits: hi = bf16(x), lo = bf16(x - hi) (round to nearest even on the stored float; x - hi is exact
    in fp32); pattern 0: [hi | lo | hi], 1: [hi | hi | lo]."""
    x = x.float()
    hi = x.bfloat16()
    lo = (x - hi.float()).bfloat16()
    return torch.cat([hi, lo, hi] if pattern == 0 else [hi, hi, lo], dim=1)


def transpose_bf16(x, ldo):
    """bf16 [C, ldo]: x^T rounded, zero pad columns."""
    R, C = x.shape
    out = torch.zeros(C, ldo, dtype=torch.bfloat16)
    out[:, :R] = x.float().t().bfloat16()
    return out


def colsum(x, init, scale):
    """init + scale * column sums of the bf16-ROUNDED x (the fused kernel sums what it stores)."""
    return init.double() + scale * x.bfloat16().double().sum(0)


# ---- float32 models ------------------------------------------------------------------------------------------------------------
_f = np.float32
_NINF = _f(-np.inf)


def _np(t):
    return t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)


def _online(m, s, v, active=True):
    """One step of the online (max, sum): s = s exp(m - mn) + exp(v - mn)."""
    mn = np.maximum(m, v)
    sn = (s * np.exp(m - mn)).astype(_f) + np.exp(v - mn)
    return np.where(active, mn, m), np.where(active, sn.astype(_f), s)


def _masked_np(lg, keep):
    lg = _np(lg).astype(_f)
    return lg if keep is None else np.where(_np(keep), lg, _f(0))


def row_lse_model(lg, keep=None, guard=True):
    """row_lse_kernel in float32.  guard=False: the butterfly WITHOUT its -inf guards (a planted error: 0 * exp(-inf + inf))."""
    x = _masked_np(lg, keep)
    R, C = x.shape
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        nk = (C + 63) // 64
        xp = np.zeros((R, nk * 64), _f)
        xp[:, :C] = x
        act = (np.arange(nk * 64) < C)[None, :]
        m, s = np.full((R, 64), _NINF), np.zeros((R, 64), _f)
        for k in range(nk):
            m, s = _online(m, s, xp[:, k * 64:(k + 1) * 64], act[:, k * 64:(k + 1) * 64])
        lane = np.arange(64)
        for o in (32, 16, 8, 4, 2, 1):
            m2, s2 = m[:, lane ^ o], s[:, lane ^ o]
            mn = np.maximum(m, m2)
            a = (s * np.exp(m - mn)).astype(_f)
            b = (s2 * np.exp(m2 - mn)).astype(_f)
            if guard:
                a, b = np.where(m == _NINF, _f(0), a), np.where(m2 == _NINF, _f(0), b)
            s, m = (a + b).astype(_f), mn
        return (m[:, 0] + np.log(s[:, 0])).astype(_f)


def col_lse_model(lg, keep=None):
    """col_part_kernel (64-row chunks, serial down the rows) + col_comb_kernel (serial over the chunks) in float32."""
    x = _masked_np(lg, keep)
    R, C = x.shape
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        nch = (R + 63) // 64
        xp = np.zeros((nch * 64, C), _f)
        xp[:R] = x
        xp = xp.reshape(nch, 64, C)
        act = (np.arange(nch * 64) < R).reshape(nch, 64, 1)
        pm, ps = np.full((nch, C), _NINF), np.zeros((nch, C), _f)
        for j in range(64):
            pm, ps = _online(pm, ps, xp[:, j], act[:, j])
        m, s = np.full(C, _NINF), np.zeros(C, _f)
        for k in range(nch):
            mn = np.maximum(m, pm[k])
            a = np.where(m == _NINF, _f(0), (s * np.exp(m - mn)).astype(_f))
            s, m = (a + (ps[k] * np.exp(pm[k] - mn)).astype(_f)).astype(_f), mn
        return (m + np.log(s)).astype(_f)


def grad_model(lg, off, rl, cl, w_row, w_col, keep=None, col_hot=True):
    """grad_kernel's g in float32, before the bf16 rounding.  rl / cl: the fp32 statistics the kernel is given (None: the term
    is absent).  col_hot=False: the column term WITHOUT its one-hot (a planted error)."""
    x = _np(lg).astype(_f)
    R, C = x.shape
    hot = _np(_hot(R, C, off)).astype(_f)
    invR = _f(1) / _f(R)
    g = np.zeros((R, C), _f)
    with np.errstate(invalid="ignore", over="ignore"):
        if rl is not None:
            g = g + (_f(w_row) * invR) * (np.exp(x - _np(rl).astype(_f)[:, None]) - hot)
        if cl is not None:
            g = g + (_f(w_col) * invR) * (np.exp(x - _np(cl).astype(_f)[None, :]) - (hot if col_hot else _f(0)))
    g = g.astype(_f)
    return g if keep is None else np.where(_np(keep), g, _f(0))


def _fma(a, b, c):
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(_f)


def _wave_sum(v):
    """wave_sum's xor butterfly over the last axis (64 lanes); every lane ends with the same value."""
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = (v + v[..., lane ^ o]).astype(_f)
    return v[..., 0]


def dscale_model(g, lg, scale, init, ldg, ldgt, need_g=True, need_gt=True, drop=None):
    """The two-stage d/dscale sum in float32 from grad_model's g: per-thread fmaf over its four rows, the wave butterfly, the
    block's (red0 + red1) + (red2 + red3), then part_finalize_kernel (1024 strided sums, butterfly, 16 serial) and
    out = init + t * (1 / scale).  drop=(block, wave): that wave's partial is left out (a planted error)."""
    g, x = _np(g).astype(_f), _np(lg).astype(_f)
    R, C = g.shape
    gc, gr = grad_grid(R, C, ldg, ldgt, need_g, need_gt)
    gp, xp = np.zeros((gr * 32, gc * 32), _f), np.zeros((gr * 32, gc * 32), _f)
    gp[:R, :C], xp[:R, :C] = g, x
    gp, xp = gp.reshape(gr, 4, 8, gc, 32), xp.reshape(gr, 4, 8, gc, 32)      # row = 8 k + ty, column = tx
    acc = np.zeros((gr, 8, gc, 32), _f)
    for k in range(4):
        acc = _fma(gp[:, k], xp[:, k], acc)
    red = _wave_sum(acc.transpose(0, 2, 1, 3).reshape(gr, gc, 4, 64))         # wave = ty >> 1, lane = 32 (ty & 1) + tx
    if drop is not None:
        red[drop[0] // gc, drop[0] % gc, drop[1]] = 0
    part = ((red[..., 0] + red[..., 1]).astype(_f) + (red[..., 2] + red[..., 3]).astype(_f)).astype(_f).reshape(-1)
    n = part.size
    pp = np.zeros((n + 1023) // 1024 * 1024, _f)
    pp[:n] = part
    a = np.zeros(1024, _f)
    for row in pp.reshape(-1, 1024):
        a = (a + row).astype(_f)
    sh = _wave_sum(a.reshape(16, 64))
    t = _f(0)
    for w in range(16):
        t = _f(t + sh[w])
    return _f(_f(init) + _f(t * (_f(1) / _f(scale))))


def ce_reduce_model(rl, cl, dg, R, C, off, w_row, w_col, init):
    """ce_reduce_kernel in float32: 256 strided sums, butterfly per wave, (sh0 + sh1 + sh2 + sh3) / R added to init."""
    dg = _np(dg).astype(_f)
    v = np.zeros(R, _f)
    if rl is not None:
        v = (v + _f(w_row) * (_np(rl).astype(_f) - dg)).astype(_f)
    if cl is not None:
        c = np.arange(R) + off
        ok = (c >= 0) & (c < C)
        with np.errstate(invalid="ignore"):
            t = (_f(w_col) * (_np(cl).astype(_f)[np.clip(c, 0, C - 1)] - dg)).astype(_f)
        v = np.where(ok, (v + t).astype(_f), v)
    vp = np.zeros((R + 255) // 256 * 256, _f)
    vp[:R] = v
    a = np.zeros(256, _f)
    for row in vp.reshape(-1, 256):
        a = (a + row).astype(_f)
    sh = _wave_sum(a.reshape(4, 64))
    tot = _f(_f(_f(sh[0] + sh[1]) + sh[2]) + sh[3])
    return _f(_f(init) + _f(tot / _f(R)))


# ---- bounds --------------------------------------------------------------------------------------------------------------------
def lse_bound(lg, dim, keep=None):
    """Absolute bound on every fp32 row (dim = 1) or column (dim = 0) log-sum-exp; the derivation is in the module docstring."""
    l = _masked(lg, keep)
    R, C = l.shape
    n_steps = ((C + 63) // 64 + 6) if dim == 1 else (min(R, 64) + (R + 63) // 64)
    lse = torch.logsumexp(l, dim=dim, keepdim=True)
    m = l.max(dim=dim, keepdim=True).values
    rel_s = 3 * U24 * (torch.exp(l - lse) * (l - m).abs()).sum(dim) + n_steps * (EXP_ALLOW + 2 * U24)
    lse, m = lse.squeeze(dim), m.squeeze(dim)
    return U24 * lse.abs() + (LOG_ALLOW + 2 * U24) * (lse - m).clamp_min(1.0) + rel_s


def bf16_half_ulp(v):
    """2^(floor(log2 v) - 8): half the spacing of bf16 (8 significant bits) in the binade of v > 0; 0 at 0."""
    _, e = torch.frexp(v.double())                       # v = m 2^e, m in [0.5, 1): floor(log2 v) = e - 1
    return torch.where(v > 0, torch.ldexp(torch.ones_like(v, dtype=F64), e - 9), torch.zeros_like(v, dtype=F64))


def grad_bound(lg, off, rl, cl, w_row, w_col, keep=None):
    """(delta, bound): the fp32 error of g and the bound on the bf16 G / GT, per element, for a kernel GIVEN rl / cl rounded to
    fp32 (None: the term is absent; +inf in cl: the term is exactly 0 and so is its error)."""
    R, C = lg.shape
    g = torch.zeros(R, C, dtype=F64)
    delta = torch.zeros(R, C, dtype=F64)
    for w, p, arg, s, hot in grad_terms(lg, off, rl, cl, w_row, w_col, keep):
        live = ~torch.isinf(s)
        fin = torch.where(live, arg.abs(), torch.zeros_like(arg))
        eta = U24 * torch.where(live, s.abs(), torch.zeros_like(s)) + 4 * U24 * fin + EXP_ALLOW
        delta = delta + abs(w) / R * torch.where(live, p * eta + FLUSH + 5 * U24 * (p - hot).abs(), torch.zeros_like(p))
        g = g + w / R * (p - hot)
    delta = delta + U24 * g.abs()
    if keep is not None:
        g, delta = g * keep.to(F64), delta * keep.to(F64)
    return delta, bf16_half_ulp(g.abs() + delta) + delta + FLUSH


def dscale_bound(g, lg, delta, scale, init, blocks, keep=None):
    """Bound on the fp32 d/dscale accumulator after the launch: sum |g l| carries the summation's roundings (every value passes
    A additions: 4 fmaf steps, 6 butterfly levels, 2 in the block, ceil(blocks / 1024) strided, 6 butterfly levels, 16 serial;
    + 3 for 1 / scale, the product and the fmaf's own rounding), sum |l| delta the error of g itself."""
    l = _masked(lg, keep).abs()
    A = 4 + 6 + 2 + (blocks + 1023) // 1024 + 6 + 16
    out = init + float((g * _masked(lg, keep)).sum()) / scale
    return ((A + 3) * U24 * float((g.abs() * l).sum()) + float((l * delta).sum())) / abs(scale) + U24 * (abs(init) + abs(out))


def ce_reduce_bound(rl, cl, dg, R, C, off, w_row, w_col, init):
    """Bound on the fp32 loss accumulator after ce_reduce_kernel, against loss_from_stats of the SAME fp32 statistics: per row one
    subtraction, one product (and w rounded to fp32) and one addition per term: 4 u; then ceil(R / 256) + 6 + 3 additions and the
    division: (ceil(R / 256) + 14) u sum_r(|w_row (rl - d)| + |w_col (cl - d)|) / R; the atomic addition u (|in| + |out|)."""
    dgd = dg.double()
    S = torch.zeros((), dtype=F64)
    if rl is not None:
        S = S + abs(w_row) * (rl.double() - dgd).abs().sum()
    if cl is not None:
        c = torch.arange(R) + off
        ok = (c >= 0) & (c < C)
        S = S + abs(w_col) * (cl.double()[c[ok]] - dgd[ok]).abs().sum()
    out = init + float(loss_from_stats(rl, cl, dg, R, C, off, w_row, w_col))
    return ((R + 255) // 256 + 14) * U24 * float(S) / R + U24 * (abs(init) + abs(out))


def l2norm_bwd_bound(f, df, norms, eps=1e-12):
    """Per element.  s = <f, df>: a lane's fmaf chain of ceil(D / 64) steps and 6 butterfly levels: ds = (ceil(D / 64) + 6) u
    sum |f df|.  dx = (df - f s) inv: |f| ds, the product f s (u |f s|), the subtraction, 1 / max(norm, eps) and the last product
    (3 u |df - f s|; the division is IEEE: no fast-math flag in the build)."""
    f, df = f.double(), df.double()
    D = f.shape[1]
    s = (f * df).sum(-1, keepdim=True)
    ds = ((D + 63) // 64 + 6) * U24 * (f * df).abs().sum(-1, keepdim=True)
    inv = 1.0 / norms.double().clamp_min(eps)[:, None]
    return (f.abs() * ds + U24 * (f * s).abs() + 3 * U24 * (df - f * s).abs()) * inv


def colsum_bound(x, init, scale):
    """Per column, of the form n 2^-24 sum |x|: a value passes 8 serial additions, 3 shuffle levels and 4 tile additions in
    transpose64_kernel, then ceil(nslab / 8) + 7 unrolled / tail steps and 3 tree levels in colws_finalize_kernel; the product
    with scale and the accumulation: 2 u |out| + u |init|."""
    nslab = (x.shape[0] + 255) // 256
    n = 8 + 3 + 4 + (nslab + 7) // 8 + 7 + 3
    a = x.bfloat16().double().abs().sum(0)
    return n * U24 * abs(scale) * a + 2 * U24 * colsum(x, init, scale).abs() + U24 * init.double().abs()


# ---- pair level ----------------------------------------------------------------------------------------------------------------
BF16X3_C = 8 + 2.0 ** -16


def logits_err_bound(x, y, scale, dev_scale=False):
    """Bound on every element of the bf16x3 logits `scale x y^T` against float64.
    x = xh + xl + rx: bf16 keeps 8 significant bits, so for x in [2^e, 2^(e+1)) |x - xh| <= 2^(e-8) <= 2^-8 |x|, xl = bf16(x - xh)
    has |xl| <= 2^-8 |x| and |rx| <= 2^(e-17) <= 2^-17 |x|; the same for y.  The GEMM forms xh yh + xl yh + xh yl, so what is
    dropped is xl yl + rx y + (xh + xl) ry: at most (2^-16 + 2^-17 + (1 + 2^-17) 2^-17) |x y| = (8 + 2^-16) 2^-18 |x y| per product:
    c = 8 + 2^-16 in units of 2^-18 (the worst case, both operands at the bottom of a binade with the largest remainders; the
    typical error is the ~2^-17 the kernel's comment names).  The K = 3 D products are exact in fp32; their accumulation and alpha: gemm_ref's budget
    (K + 2) 2^-23 S with S = sum of the |products| <= (1 + 2^-8) sum |x_i y_i|.
    Device log-scale: x exp(ls) is formed in fp32 first (vl_scale_exp_f32): __expf of |ls| <= ln 100 errs by
    3 u |ls| + EXP_ALLOW <= 16 u, the product by u: 17 u more on every |x_i y_i|."""
    S = x.double().abs() @ y.double().abs().t()
    D = x.shape[1]
    per = BF16X3_C * 2.0 ** -18 + (3 * D + 2) * 2.0 ** -23 * (1 + 2.0 ** -8) + (17 * U24 if dev_scale else 0.0)
    return abs(scale) * per * S


def pair_loss_tol(lg, E, off, w_row, w_col, init=0.0):
    """Tolerance of the pair loss against loss(): ce_reduce_bound (on the exact statistics) + the weighted mean of lse_bound (the
    statistics the reduction is given are the kernels') + the logits' error E [R, C] carried through: a log-sum-exp and a diagonal
    element each move by at most max |E| over their row / column."""
    R, C = lg.shape
    rl, cl, dg = row_lse(lg), col_lse(lg), diag(lg, off)
    c = torch.arange(R) + off
    tol = ce_reduce_bound(rl, cl if w_col else None, dg, R, C, off, w_row, w_col, init)
    tol += w_row * float((lse_bound(lg, 1) + 2 * E.max(1).values).mean())
    if w_col:
        tol += w_col * float((lse_bound(lg, 0)[c] + E.max(0).values[c] + E.max(1).values).mean())
    return tol


def dxdy_model(x, y, scale, off, w_row, w_col, keep=None):
    """(dx, dy) in float64 from G and the transposed operand ROUNDED to bf16 - what the two NT GEMMs consume - with everything
    else exact: the model of the feature gradients whose distance from the exact ones the GPU tolerances are twice of."""
    lg = scale * x.double() @ y.double().t()
    G = grad(lg, off, w_row, w_col, keep).bfloat16().double()
    return scale * G @ y.bfloat16().double(), scale * G.t() @ x.bfloat16().double()


def worst_row(out, ref):
    """Largest relative 2-norm error of a row, rows measured against no less than errloc's fair share (FLOOR = 0.25)."""
    d = (out.double() - ref.double()).norm(dim=1)
    r = ref.double().norm(dim=1)
    fair = 0.25 * ref.double().norm() / math.sqrt(ref.shape[0])
    return float((d / torch.maximum(r, fair).clamp_min(1e-300)).max())
