"""Tensor-level wrappers over the C ABI.  Every function enqueues HIP kernels on the current
torch stream and returns immediately.  Inputs must live on a GPU: there is no CPU fallback."""
import ctypes as C
import threading

import numpy as np
import torch

from ._lib import load_library, check

F32, BF16, F16 = 0, 1, 2
EPI_BF16, EPI_F32, EPI_RES_F32, EPI_RES_BF16, EPI_GEGLU, EPI_DGELU, EPI_DGEGLU = 0, 1, 2, 3, 5, 6, 7
ACT_NONE, ACT_GELU, ACT_RELU = 0, 1, 2
ACT_GELU_DSAVE = 4          # forward: out = gelu(pre), out2 = gelu'(pre);  with EPI_DGELU: res is that gelu' tensor
ACT_QGELU = 5               # QuickGELU x * sigmoid(1.702 x): the OpenAI-pretrained CLIP towers (TowerCfg / TextCfg.quick_gelu)
ACT_QGELU_DSAVE = 6         # ACT_GELU_DSAVE for QuickGELU: out2 = qgelu'(pre); EPI_DGELU takes it exactly as ACT_GELU_DSAVE


def mlp_act(quick_gelu: bool, dsave: bool = False) -> int:
    """The activation code of a transformer block's MLP: exact-erf GELU or QuickGELU, plain or with the saved derivative."""
    if quick_gelu:
        return ACT_QGELU_DSAVE if dsave else ACT_QGELU
    return ACT_GELU_DSAVE if dsave else ACT_GELU
LOG2E = 1.4426950408889634

_lib = load_library()


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t):
    if t is None:
        return None
    if not t.is_cuda:
        raise RuntimeError("vitlens_hip ops need GPU tensors (no CPU fallback)")
    return C.c_void_p(t.data_ptr())


def _dt(t):
    if t.dtype == torch.float32:
        return F32
    if t.dtype == torch.bfloat16:
        return BF16
    if t.dtype == torch.float16:
        return F16
    raise TypeError(f"unsupported dtype {t.dtype}")


def _chk2d(t, name, dtype=None):
    if t.dim() != 2 or t.stride(1) != 1:
        raise ValueError(f"{name}: need a row-major 2-D tensor, got shape {tuple(t.shape)} strides {t.stride()}")
    if dtype is not None and t.dtype != dtype:
        raise TypeError(f"{name}: expected {dtype}, got {t.dtype}")


def _gemm_operands(who, a, w, in_dtype, out, out_dtype, res, bias, out_cols=(1, 1), res_div=None, strict=True):
    """The one operand check of gemm, gemm_f16, gemm_f32 and gemm_f32_ex: a [M,K] and w [N,K] row-major of in_dtype; out row-major
    (None: allocated here, [M, N * out_cols[0] // out_cols[1]] of out_dtype); res row-major with out's row stride and, where res_div
    is given, a row for every res_div rows of out; bias f32 [N].  strict: out has to be of out_dtype and res f32 (TypeError);
    otherwise - gemm, whose epilogue decides both - res has to be of out's dtype.  Returns (M, N, K, out)."""
    _chk2d(a, f"{who}: a", in_dtype); _chk2d(w, f"{who}: w", in_dtype)
    M, K = a.shape
    N = w.shape[0]
    if w.shape[1] != K:
        raise ValueError(f"{who}: K mismatch {a.shape} vs {w.shape}")
    if out is None:
        out = torch.empty(M, N * out_cols[0] // out_cols[1], device=a.device, dtype=out_dtype)
    _chk2d(out, f"{who}: out", out_dtype if strict else None)
    if res is not None:
        _chk2d(res, f"{who}: res", torch.float32 if strict else None)
        if res.stride(0) != out.stride(0) or (not strict and res.dtype != out.dtype):
            raise ValueError(f"{who}: residual must share out's row stride" + ("" if strict else " and dtype"))
        if res_div is not None and res.shape[0] * res_div < M:
            raise ValueError(f"{who}: residual has too few rows (one for every {res_div} rows of out)")
    if bias is not None and (bias.dtype != torch.float32 or bias.numel() != N):
        raise ValueError(f"{who}: bias must be f32 [N]")
    return M, N, K, out


def gemm(a, w, bias=None, out=None, res=None, epi=EPI_BF16, act=ACT_NONE, alpha=1.0, cfg=-1, out2=None, res_div=1):
    """out = epilogue(a @ w.T).  a [M,K] bf16, w [N,K] bf16.  out2: optional pre-activation copy (bf16; with
    act=ACT_GELU_DSAVE / ACT_QGELU_DSAVE: the activation's derivative at pre instead, the operand of the backward's EPI_DGELU
    launched with the same act)."""
    if act in (ACT_GELU_DSAVE, ACT_QGELU_DSAVE) and epi == EPI_BF16 and out2 is None:
        raise ValueError("gemm: ACT_GELU_DSAVE / ACT_QGELU_DSAVE need out2")
    M, N, K, out = _gemm_operands("gemm", a, w, torch.bfloat16, out, torch.float32 if epi in (EPI_F32, EPI_RES_F32) else torch.bfloat16,
                                  res, bias, out_cols=(1, 2) if epi == EPI_GEGLU else ((2, 1) if epi == EPI_DGEGLU else (1, 1)),
                                  res_div=res_div if res_div > 1 else None, strict=False)
    if out2 is not None and (out2.stride(0) != out.stride(0) * (2 if epi == EPI_GEGLU else 1) or out2.dtype != torch.bfloat16):
        raise ValueError("gemm: out2 must be bf16 with out's row stride (twice that for GEGLU)")
    if K % 64:   # kernels stream 64-wide K slabs: zero-pad odd reduction lengths (toy configs only)
        Kp = (K + 63) // 64 * 64
        a = torch.nn.functional.pad(a, (0, Kp - K)); w = torch.nn.functional.pad(w, (0, Kp - K))
        K = Kp
    check(_lib.vl_gemm_bf16_ex(_p(a), _p(w), _p(bias), _p(out), _p(res), _p(out2), M, N, K, a.stride(0), w.stride(0),
                               out.stride(0), float(alpha), epi, act, res_div, cfg, _stream()))
    return out


def gemm_f16(a, w, bias=None, out=None, res=None, epi=EPI_BF16, act=ACT_NONE, alpha=1.0):
    """The persistent 256x256 GEMM on IEEE-half operands (vl_gemm_f16; the frozen text tower): a [M,K], w [N,K] fp16;
    epi = EPI_BF16 -> out fp16 [M,N] = act(a @ w.T + bias), epi = EPI_RES_F32 -> out f32 = res + a @ w.T + bias (in place
    allowed).  M, N multiples of 256, K a multiple of 64 and >= 512: the caller pads (TextEngine keeps whole row tiles)."""
    M, N, K, out = _gemm_operands("gemm_f16", a, w, torch.float16, out, torch.float32 if epi == EPI_RES_F32 else torch.float16, res, bias)
    check(_lib.vl_gemm_f16(_p(a), _p(w), _p(bias), _p(out), _p(res), M, N, K, a.stride(0), w.stride(0), out.stride(0),
                           float(alpha), epi, act, _stream()))
    return out


# ---- true fp32 arithmetic (inference under precision="fp32": vitlens_hip/f32.py) ----
def gemm_f32(a, w, bias=None, out=None, res=None, act=ACT_NONE, alpha=1.0):
    """out f32 = act(alpha * a @ w.T + bias) (+ res), a [M,K], w [N,K] f32, any M and N, K % 4 == 0 (vl_gemm_f32: fp32-input MFMA)."""
    M, N, K, out = _gemm_operands("gemm_f32", a, w, torch.float32, out, torch.float32, res, bias)
    check(_lib.vl_gemm_f32(_p(a), _p(w), _p(bias), _p(out), _p(res), M, N, K, a.stride(0), w.stride(0), out.stride(0),
                           float(alpha), act, _stream()))
    return out


def attn_fwd_f32(q, k, v, out, lse=None, causal=False, scale=1.0):
    """softmax(scale * q k^T [+ causal mask]) v on strided f32 [B,H,L,dh] views -> out f32 [B*Lq, H*dh] (dh = 32, 64 or a
    multiple of 8 in (64, 128]; strides multiples of 4; the library refuses anything else)."""
    import ctypes
    B, H, Lq, dh = q.shape
    Lk = k.shape[2]
    vals = []
    for t in (q, k, v):
        if t.dim() != 4 or t.stride(3) != 1 or t.dtype != torch.float32:
            raise ValueError("attn_fwd_f32: operands must be f32 [B,H,L,dh] views with unit last stride")
        vals += [t.stride(0), t.stride(1), t.stride(2)]
    if out.dtype != torch.float32:
        raise TypeError("attn_fwd_f32: out must be f32")
    check(_lib.vl_attn_fwd_f32(_p(q), _p(k), _p(v), (ctypes.c_long * 9)(*vals), _p(out), _p(lse), B, H, Lq, Lk, dh, float(scale),
                               1 if causal else 0, _stream()))
    return out


def gemm_f32_ex(a, w, bias=None, out=None, res=None, act=ACT_NONE, alpha=1.0, res_div=1, res_pre=False, geglu=False):
    """vl_gemm_f32_ex: gemm_f32 with the epilogues of the fp32 Lenses.  res_pre: out = act(alpha a @ w.T + bias + res[m // res_div])
    (res [ceil(M / res_div), N] with out's row stride).  geglu: w rows interleaved (a_j, gate_j) -> out f32 [M, N/2] =
    a * gelu(gate); no residual.  With the defaults this is gemm_f32 (the library routes it to the same kernel)."""
    M, N, K, out = _gemm_operands("gemm_f32_ex", a, w, torch.float32, out, torch.float32, res, bias,
                                  out_cols=(1, 2) if geglu else (1, 1), res_div=res_div)
    check(_lib.vl_gemm_f32_ex(_p(a), _p(w), _p(bias), _p(out), _p(res), M, N, K, a.stride(0), w.stride(0), out.stride(0),
                              float(alpha), act, int(res_div), 1 if res_pre else 0, 1 if geglu else 0, _stream()))
    return out


def im2col_f32(x, kh, kw, sh, sw, Kp, transpose_hw=False):
    """im2col with f32 patches (the conv stem under precision="fp32")."""
    if x.dtype != torch.float32 or not x.is_contiguous():
        raise ValueError("im2col_f32: need contiguous f32 input")
    N, Cc = x.shape[0], x.shape[1]
    H, W = (x.shape[3], x.shape[2]) if transpose_hw else (x.shape[2], x.shape[3])
    gh, gw = (H - kh) // sh + 1, (W - kw) // sw + 1
    out = torch.empty(N * gh * gw, Kp, device=x.device, dtype=torch.float32)
    check(_lib.vl_im2col_f32(_p(x), _p(out), N, Cc, H, W, kh, kw, sh, sw, Kp, 1 if transpose_hw else 0, _stream()))
    return out, gh, gw


# ---- LayerNorm folded into the GEMMs either side of it (frozen pre-LN blocks, bf16 residual stream; include/vitlens_hip.h) ----
def fold_ln_linear(w, b, gamma, beta):
    """Operands of  LN(x; gamma, beta) @ w.T + b  for vl_gemm_lnfold_bf16: (Wg bf16 [N,K] = bf16(w * gamma), bias_f f32 [N] =
    b + w @ beta, c f32 [N] = row sums of the ROUNDED Wg - the mean term must cancel against exactly what the MFMAs add up)."""
    w = w.detach().float()
    wg = (w * gamma.detach().float()[None, :]).to(torch.bfloat16).contiguous()
    c = wg.float().sum(1).contiguous()
    d = (b.detach().float() + (w * beta.detach().float()[None, :]).sum(1)).contiguous()       # (w @ beta without a BLAS call: build-time only)
    return wg, d, c


def _fold_rows(x, out, N, K):
    """Rows of this problem that take the folded path (0: the shape does not fit the persistent kernel)."""
    M = x.shape[0]
    if x.dtype != torch.bfloat16 or out.dtype != torch.bfloat16 or K < 512 or K % 64 or N % 256 or x.stride(0) % 8 or out.stride(0) % 8:
        return 0
    if x.data_ptr() % 16 or out.data_ptr() % 16:
        return 0
    return int(_lib.vl_gemm_main_rows(M, N))


def _leftover_cfg(rows, N, cfg):
    """cfg of the leftover rows of a GEMM whose rows the caller split: the kernel run_gemm (csrc/vl_gemm.hip) gives such rows, from
    the library itself (vl_gemm_rest_cfg; a standalone call of that size would get 128x128 tiles and a serial K)."""
    # THE ONE DIFFERENCE from run_gemm: above 512 leftover rows run_gemm launches 128x128 tiles (vl_gemm_rest_cfg says 1), while this
    # split passes cfg -1 on, so the leftover rows re-enter the auto dispatch as a problem of their own - which can pick the persistent
    # kernel again with an uneven round (N = 1024: 56 leftover row tiles x 4 = 224 tiles >= 192).  Neither choice has been measured
    # against the other; both are kept as they were.
    if cfg >= 0 or rows > 512:
        return cfg
    return int(load_library().vl_gemm_rest_cfg(rows, N))      # a pure host function: the library's own, also where `_lib` is a recorder


def gemm_lnfold(x, fold, mean, rstd, out, w, b, ln_w, ln_b, h_ws, act=ACT_NONE, out2=None, eps=1e-5, cfg=-1, h_ready=False):
    """out = act(LN(x) @ w.T + b) with the LayerNorm folded into the GEMM's epilogue for the rows the persistent kernel takes
    (x raw bf16 rows, mean / rstd their statistics, fold = fold_ln_linear(...)); the leftover rows - and every row of a shape
    that kernel refuses - go through layernorm + gemm on the plain operands (h_ws: a bf16 [>= leftover rows, K] buffer;
    h_ready: ln_row_stats(..., h_left=h_ws, h_row0=fold_rows(...)) already left their LayerNorm output there)."""
    wg, d, c = fold
    M, K = x.shape
    N = wg.shape[0]
    mm = _fold_rows(x, out, N, K)
    if mm:
        check(_lib.vl_gemm_lnfold_bf16(_p(x), _p(wg), _p(d), _p(c), _p(mean), _p(rstd), _p(out), _p(out2), mm, N, K,
                                       x.stride(0), wg.stride(0), out.stride(0), act, _stream()))
    if mm < M:
        r = M - mm
        h = h_ws[:r]
        if not h_ready:
            layernorm(x[mm:], ln_w, ln_b, h, r, K, x_row_stride=x.stride(0), mean=mean[mm:], rstd=rstd[mm:], eps=eps)
        gemm(h, w, b, out=out[mm:], epi=EPI_BF16, act=act, cfg=_leftover_cfg(r, N, cfg) if mm else cfg,
             out2=None if out2 is None else out2[mm:])
    return out


def gemm_res_rowstats(a, w, b, out, res, part, cfg=-1):
    """out = res + a @ w.T + b (bf16 residual stream, in place allowed); for the rows the persistent kernel takes it also leaves
    (sum, sum of squares) per row and 64-column slice in part f32 [rows, N/64, 2].  Returns that row count (0: none)."""
    M, K = a.shape
    N = w.shape[0]
    mm = _fold_rows(a, out, N, K) if (res.dtype == torch.bfloat16 and res.stride(0) == out.stride(0) and res.data_ptr() % 16 == 0
                                      and part.numel() >= M * (N // 64) * 2) else 0
    if mm:
        check(_lib.vl_gemm_res_rowstats_bf16(_p(a), _p(w), _p(b), _p(out), _p(res), _p(part), mm, N, K, a.stride(0), w.stride(0),
                                             out.stride(0), _stream()))
    if mm < M:
        gemm(a[mm:], w, b, out=out[mm:], res=res[mm:], epi=EPI_RES_BF16, cfg=_leftover_cfg(M - mm, N, cfg) if mm else cfg)
    return mm


def fold_rows(x, out, N):
    """Rows of `out = f(LN(x) @ W[N, K].T)` that gemm_lnfold runs through the folded epilogue (the others: layernorm + gemm)."""
    return _fold_rows(x, out, N, x.shape[1])


def ln_row_stats(part, x, m_main, mean, rstd, eps=1e-5, ln_w=None, ln_b=None, h_left=None, h_row0=None):
    """mean / rstd of the rows of x (bf16 [rows, D]): rows < m_main from the partial sums `part` of gemm_res_rowstats, the
    others from the rows themselves.  h_left (bf16 [>= rows - h_row0, D], with ln_w / ln_b): the LayerNorm output of the rows
    >= h_row0 (the consuming gemm_lnfold's leftover rows, h_row0 = fold_rows(...) >= m_main) from the same launch."""
    rows, D = x.shape
    if h_left is not None:
        if h_row0 is None or h_row0 < m_main or h_left.dtype != torch.bfloat16 or h_left.shape[0] < rows - h_row0:
            raise ValueError("ln_row_stats: h_left needs h_row0 >= m_main and a bf16 buffer of at least rows - h_row0 rows")
    check(_lib.vl_ln_row_stats(_p(part) if m_main else None, D // 64, _p(x), x.stride(0), D, m_main, rows, float(eps), _p(mean),
                               _p(rstd), _p(ln_w), _p(ln_b), _p(h_left), h_left.stride(0) if h_left is not None else 0,
                               int(h_row0 or 0), _stream()))


def logits_gemm(xb, yb, scale):
    """scale * xb @ yb^T as f32 [R, C] for ANY number of columns (a partial last batch, a batch of 6 ...): the GEMM wants
    N % 4 == 0, so the column operand is zero-padded to a multiple of 4 rows and a [R, C] view of the padded result is
    returned (the CE kernels take the row stride)."""
    Cn = yb.shape[0]
    Cp = (Cn + 3) // 4 * 4
    if Cp != Cn:
        yb = torch.cat([yb, torch.zeros(Cp - Cn, yb.shape[1], device=yb.device, dtype=yb.dtype)], 0)
    out = gemm(xb, yb, None, epi=EPI_F32, alpha=scale)
    return out if Cp == Cn else out[:, :Cn]


def gemm_dw(dyt, xt, g, cfg=-1, alpha=1.0):
    """g += dyt @ xt^T: the weight-gradient GEMM (dyt [N_out, R], xt [K_in, R] bf16 - both already transposed so
    that the token axis R is the reduction axis; g f32 [N_out, K_in], may be a strided view).  Few output tiles
    and a long reduction -> split-K over the CUs; otherwise the regular GEMM with the accumulate epilogue."""
    _chk2d(dyt, "dyt", torch.bfloat16); _chk2d(xt, "xt", torch.bfloat16); _chk2d(g, "g", torch.float32)
    M, K = dyt.shape
    N = xt.shape[0]
    nk = K // 64
    if K % 64 == 0 and M % 256 == 0 and N % 256 == 0 and nk >= 64:
        # whole 256x256 tiles: k-slices on the persistent kernel (fp32 partials + fixed-order reduce)
        t256 = (M // 256) * (N // 256)
        for splits in (1, 2, 4, 8, 16):
            if nk % splits == 0 and t256 * splits >= 192 and nk // splits >= 16:
                ws = torch.empty(splits * M * N, device=g.device, dtype=torch.float32)
                check(_lib.vl_gemm_splitk_accum_f32(_p(dyt), _p(xt), _p(g), M, N, K, dyt.stride(0), xt.stride(0), g.stride(0),
                                                    float(alpha), splits, _p(ws), _stream()))
                return g
    tiles = ((M + 127) // 128) * ((N + 127) // 128)
    if K % 64 == 0 and tiles * 2 <= 256 and nk >= 32:
        splits = max(1, min(512 // tiles, nk // 16))
        if splits > 1:
            ws = torch.empty(splits * M * N, device=g.device, dtype=torch.float32)
            check(_lib.vl_gemm_splitk_accum_f32(_p(dyt), _p(xt), _p(g), M, N, K, dyt.stride(0), xt.stride(0), g.stride(0),
                                                float(alpha), splits, _p(ws), _stream()))
            return g
    return gemm(dyt, xt, None, out=g, res=g, epi=EPI_RES_F32, cfg=cfg, alpha=alpha)


def gemm_dw_tn(dy, x, g, alpha=1.0):
    """g[N_out, K_in] += dy^T x on the operands as the backward holds them (dy [R, N_out], x [R, K_in] bf16, row = token):
    no transposed copies - the kernel stages token-major k-slabs and reads its fragments with the LDS transpose read.
    Returns False (nothing launched) when the shape does not fit (whole 256x256 tiles, R % 64 == 0, enough work items)."""
    if dy.dtype != torch.bfloat16 or x.dtype != torch.bfloat16 or g.dtype != torch.float32 or dy.dim() != 2 or x.dim() != 2:
        return False
    R, M = dy.shape
    N = x.shape[1]
    if x.shape[0] != R or R % 64 or M % 256 or N % 256 or dy.stride(1) != 1 or x.stride(1) != 1 or g.stride(1) != 1:
        return False
    if dy.stride(0) % 8 or x.stride(0) % 8 or g.stride(0) % 4 or dy.data_ptr() % 16 or x.data_ptr() % 16 or tuple(g.shape) != (M, N):
        return False
    splits = tn_splits(R // 64, (M // 256) * (N // 256))
    if not splits:
        return False
    ws = torch.empty(splits * M * N, device=g.device, dtype=torch.float32)
    check(_lib.vl_gemm_tn_splitk_accum_f32(_p(dy), _p(x), _p(g), M, N, R, dy.stride(0), x.stride(0), g.stride(0),
                                           float(alpha), splits, _p(ws), _stream()))
    return True


def tn_splits(nk: int, tiles: int, few_tiles_ok: bool = False) -> int:
    """K slices for the token-major dW kernel: the smallest of 1, 2, 4, 8, 16 that gives >= 192 work items (tiles x slices) with
    >= 16 steps of 64 tokens per slice; slices are ceil(nk / splits) steps long, the last one may be shorter but not below the
    4 steps the kernel's DMA look-ahead needs (vl_gemm_tn_splitk_accum_f32 checks the same).  0 = the shape does not fit.
    few_tiles_ok (round 6: the Perceiver's narrow projections, 1-8 output tiles over 32 k-512 k tokens): up to 64 slices, and when
    even those do not fill the chip, the largest admissible count."""
    valid = lambda splits: (nk // splits >= 16 and nk - (-(-nk // (-(-nk // splits))) - 1) * (-(-nk // splits)) >= 4)
    cands = (1, 2, 4, 8, 16, 32, 64) if few_tiles_ok else (1, 2, 4, 8, 16)
    best = 0
    for splits in cands:
        if not valid(splits):
            continue
        if tiles * splits >= 192:
            return splits
        best = splits
    return best if few_tiles_ok else 0


_pad_cache = {}


def _zero_padded(t, cols, tag):
    """t [R, c] bf16 -> a [R, cols] bf16 buffer (cached per shape and role) whose first c columns are t and the rest zero."""
    # (the source width is part of the key: the pad columns must stay zero; the stream too: two backwards run side by side;
    #  the host thread too: a buffer is filled and consumed by two separate enqueues)
    key = (tag, t.device, torch.cuda.current_stream(t.device).cuda_stream, threading.get_ident(), t.shape[0], t.shape[1], cols)
    buf = _pad_cache.get(key)
    if buf is None:
        buf = torch.zeros(t.shape[0], cols, device=t.device, dtype=torch.bfloat16)      # the pad columns are written once: zeros
        _pad_cache[key] = buf
    buf[:, :t.shape[1]].copy_(t)
    return buf


def gemm_dw_tn_any(dy, x, g, alpha=1.0):
    """g[N_out, K_in] += dy^T x like gemm_dw_tn, for operands whose column counts are NOT multiples of 256 (the Perceiver's
    cross-attention projections: 64 / 128 columns; a 384-wide context): the narrow operand is zero-padded to whole 256-column
    tiles - a copy of the SMALL matrix - instead of transposing BOTH operands for the NT kernel (a 64-134 MB round trip of the
    large one per call, `transpose64_kernel` in the C4 / C5 kernel statistics of round 5).  Returns False when the shape does
    not fit (rows not a multiple of 64, non-bf16 operands)."""
    if dy.dtype != torch.bfloat16 or x.dtype != torch.bfloat16 or g.dtype != torch.float32 or dy.dim() != 2 or x.dim() != 2:
        return False
    R, M = dy.shape
    N = x.shape[1]
    if x.shape[0] != R or R % 64 or tuple(g.shape) != (M, N) or dy.stride(1) != 1 or x.stride(1) != 1:
        return False
    Mp, Np = (M + 255) // 256 * 256, (N + 255) // 256 * 256
    if Mp == M and Np == N and gemm_dw_tn(dy, x, g, alpha):
        return True
    if dy.stride(0) % 8 or x.stride(0) % 8 or dy.data_ptr() % 16 or x.data_ptr() % 16:
        return False
    splits = tn_splits(R // 64, (Mp // 256) * (Np // 256), few_tiles_ok=True)
    if not splits:
        return False
    dyp = dy if Mp == M else _zero_padded(dy, Mp, "dy")
    xp = x if Np == N else _zero_padded(x, Np, "x")
    direct = Mp == M and Np == N and g.stride(1) == 1 and g.stride(0) % 4 == 0
    gp = g if direct else torch.zeros(Mp, Np, device=g.device, dtype=torch.float32)
    ws = torch.empty(splits * Mp * Np, device=g.device, dtype=torch.float32)
    check(_lib.vl_gemm_tn_splitk_accum_f32(_p(dyp), _p(xp), _p(gp), Mp, Np, R, dyp.stride(0), xp.stride(0), gp.stride(0),
                                           float(alpha), splits, _p(ws), _stream()))
    if not direct:
        g += gp[:M, :N]
    return True


def weight_grad(dy, x, g, bias_grad=None, narrow=True, cfg=-1):
    """g[N_out, K_in] += dy^T x on the operands as the backward holds them (dy [R, N_out], x [R, K_in], row = token) and, if
    bias_grad is given, bias_grad += the column sums of dy.  Token-major operands where the shape fits the dW kernel (narrow:
    column counts that are not whole 256-column tiles too, through gemm_dw_tn_any's zero-padded copies; otherwise gemm_dw_tn
    alone), the bias gradient from colsum; else both operands transposed to bf16 with the token axis padded to whole 64-token
    steps - the transpose of a bf16 dy reads all of dy anyway and produces the bias gradient - and gemm_dw (kernel
    configuration cfg).
    The bias gradient is the column sums of dy AS GIVEN on every route, whatever the row count: the fused transpose sums the
    bf16 values it writes, which for an fp32 dy are rounded ones, so an fp32 dy gets its sums from colsum on the fp32 values
    (the product itself is bf16 x bf16 on every route)."""
    if (gemm_dw_tn_any if narrow else gemm_dw_tn)(dy, x, g):
        if bias_grad is not None:
            colsum(dy, bias_grad)
        return g
    rp = (dy.shape[0] + 63) // 64 * 64
    if bias_grad is not None and dy.dtype != torch.bfloat16:
        colsum(dy, bias_grad)
        bias_grad = None
    return gemm_dw(transpose_colsum(dy, rp, colsum_out=bias_grad), transpose_to_bf16(x, ldo=rp), g, cfg=cfg)


def _bhld_strides(*views):
    """(batch, head, row) element strides of [B,H,L,dh] views (last stride 1) as a ctypes long array."""
    import ctypes
    vals = []
    for t in views:
        if t.dim() != 4 or t.stride(3) != 1 or t.dtype != views[0].dtype or t.dtype not in (torch.bfloat16, torch.float16):
            raise ValueError("attention operands must be bf16 (or, forward only, fp16) [B,H,L,dh] views of one dtype with unit last stride")
        vals += [t.stride(0), t.stride(1), t.stride(2)]
    return (ctypes.c_long * len(vals))(*vals)


def heads_view(x2d, B, L, H, dh, col0=0):
    """[B*L, W] token-major matrix -> the [B,H,L,dh] view of its column block [col0, col0 + H*dh) (no copy)."""
    W = x2d.stride(0)
    return x2d.as_strided((B, H, L, dh), (L * W, dh, W, 1), x2d.storage_offset() + col0)


def attn_fwd(q, k, v, out, lse=None, causal=False, qscale=1.0):
    """q [B,H,Lq,dh], k, v [B,H,Lk,dh] strided bf16 views (see heads_view) -> out [B*Lq, H*dh] bf16.
    q is multiplied by qscale (softmax_scale*log2e) inside the kernel; pass 1 for a pre-scaled q."""
    B, H, Lq, dh = q.shape
    Lk = k.shape[2]
    st = _bhld_strides(q, k, v)
    if q.dtype == torch.float16:          # the frozen text tower's operands (head dim 64, <= 288 keys)
        if k.dtype != q.dtype or v.dtype != q.dtype or out.dtype != q.dtype:
            raise TypeError("attn_fwd: fp16 q needs fp16 k, v and out")
        check(_lib.vl_attn_fwd_f16(_p(q), _p(k), _p(v), st, _p(out), _p(lse), B, H, Lq, Lk, dh, float(qscale),
                                   1 if causal else 0, _stream()))
        return out
    check(_lib.vl_attn_fwd_bf16(_p(q), _p(k), _p(v), st, _p(out), _p(lse), B, H, Lq, Lk, dh, float(qscale),
                                1 if causal else 0, _stream()))
    return out


def attn_fwd_varlen(qkv, start, lens, out, H, max_len, lse=None, qscale=1.0):
    """Causal self-attention of packed captions (vl_attn_fwd_varlen_f16): qkv fp16 [rows, 3*H*64] the packed in-projection output,
    start int32 [B+1] / lens int32 [B] the packing plan on the device, max_len >= every length (host int, <= 288)
    -> out fp16 [rows, H*64]; lse f32 [rows, H] optional."""
    import ctypes
    W = H * 64
    if qkv.dtype != torch.float16 or out.dtype != torch.float16 or qkv.dim() != 2 or qkv.shape[1] != 3 * W or qkv.stride(1) != 1:
        raise ValueError("attn_fwd_varlen: qkv must be an fp16 [rows, 3*H*64] matrix with unit column stride, out fp16")
    if out.dim() != 2 or out.shape[1] != W or not out.is_contiguous() or out.shape[0] < qkv.shape[0]:
        raise ValueError("attn_fwd_varlen: out must be a contiguous fp16 [rows, H*64] matrix")
    for t, nm in ((start, "start"), (lens, "lens")):
        if t.dtype != torch.int32 or not t.is_contiguous() or t.device != qkv.device:
            raise ValueError(f"attn_fwd_varlen: {nm} must be a contiguous int32 tensor on the operands' device")
    B = lens.numel()
    if start.numel() < B + 1:
        raise ValueError("attn_fwd_varlen: start needs B + 1 entries")
    if lse is not None and (lse.dtype != torch.float32 or not lse.is_contiguous() or lse.numel() < qkv.shape[0] * H):
        raise ValueError("attn_fwd_varlen: lse must be a contiguous f32 [rows, H]")
    ld = qkv.stride(0)
    st = (ctypes.c_long * 6)(64, ld, 64, ld, 64, ld)
    es = qkv.element_size()
    base = qkv.data_ptr()
    check(_lib.vl_attn_fwd_varlen_f16(base, base + W * es, base + 2 * W * es, st, _p(start), _p(lens), _p(out), _p(lse), B, H,
                                      int(max_len), 64, float(qscale), _stream()))
    return out


def text_pack_plan(ids, lens, start, last_row, total):
    """The packing plan of a batch of captions on the device (vl_text_pack_plan): ids int64 [B, L] -> lens int32 [B] =
    argmax + 1, start int32 [B+1], last_row int64 [B], total int32 [2] = (rows, max_len)."""
    B, L = ids.shape
    if ids.dtype != torch.int64 or not ids.is_contiguous():
        raise ValueError("text_pack_plan: ids must be a contiguous int64 [B, L] tensor")
    for t, dt, n, nm in ((lens, torch.int32, B, "lens"), (start, torch.int32, B + 1, "start"), (last_row, torch.int64, B, "last_row"),
                         (total, torch.int32, 2, "total")):
        if t.dtype != dt or not t.is_contiguous() or t.numel() < n or t.device != ids.device:
            raise ValueError(f"text_pack_plan: {nm} must be a contiguous {dt} tensor of >= {n} entries on the ids' device")
    check(_lib.vl_text_pack_plan(_p(ids), _p(lens), _p(start), _p(last_row), _p(total), B, L, _stream()))


def text_embed_packed(ids, start, lens, tok_emb, pos, out, rows, rows_pad):
    """Rows start[b] + t (t < lens[b]) of out f32 <- tok_emb[ids[b, t]] + pos[t]; rows [rows, rows_pad) <- 0 (vl_text_embed_packed)."""
    B, L = ids.shape
    D = tok_emb.shape[1]
    if ids.dtype != torch.int64 or not ids.is_contiguous() or out.dtype != torch.float32 or not out.is_contiguous():
        raise ValueError("text_embed_packed: ids contiguous int64 [B, L], out contiguous f32")
    if out.dim() != 2 or out.shape[1] != D or out.shape[0] < rows_pad or pos.shape[0] < L or pos.shape[1] != D:
        raise ValueError("text_embed_packed: out must hold rows_pad rows of the embedding width, pos L rows")
    if start.dtype != torch.int32 or lens.dtype != torch.int32 or start.numel() < B + 1 or lens.numel() < B:
        raise ValueError("text_embed_packed: start int32 [B+1], lens int32 [B]")
    check(_lib.vl_text_embed_packed(_p(ids), _p(start), _p(lens), _p(tok_emb), _p(pos), _p(out), B, L, D, tok_emb.shape[0],
                                    int(rows), int(rows_pad), _stream()))
    return out


def _q1_rows(t, H, name):
    if t.dim() != 2 or t.stride(1) != 1 or t.dtype != torch.bfloat16 or t.shape[1] != H * 64:
        raise ValueError(f"{name}: need a bf16 [B, H*64] matrix with unit column stride, got {tuple(t.shape)} {t.dtype}")


def attn_fwd_q1(q, k, v, out, lse=None, qrow=0, qscale=1.0):
    """Attention of ONE query row per (batch, head): row `qrow` of q against all keys / values.  q, k, v [B,H,L,64] strided
    bf16 views (heads_view) -> out bf16 [B, H*64], lse f32 [B, H] (optional).  Conventions of attn_fwd (qscale = scale*log2e)."""
    B, H, L, dh = q.shape
    if k.shape != q.shape or v.shape != q.shape or q.dtype != torch.bfloat16:
        raise ValueError("attn_fwd_q1: q, k, v must be bf16 views of one [B,H,L,dh] shape (self-attention)")
    _q1_rows(out, H, "attn_fwd_q1: out")
    if out.shape[0] != B or (lse is not None and (lse.dtype != torch.float32 or not lse.is_contiguous() or lse.numel() != B * H)):
        raise ValueError("attn_fwd_q1: out must have B rows, lse must be a contiguous f32 [B, H]")
    check(_lib.vl_attn_fwd_q1(_p(q), _p(k), _p(v), _bhld_strides(q, k, v), _p(out), out.stride(0), _p(lse), B, H, L, dh,
                              int(qrow), float(qscale), _stream()))
    return out


def _chk_mean_rstd(mean, rstd, who):
    if (mean is None) != (rstd is None):
        raise ValueError(f"{who}: mean and rstd are written together: give both or neither")


def layernorm(x, w, b, out, rows, D, x_row_stride=None, row_index=None, row_mul=0, mean=None, rstd=None,
              eps=1e-5):
    _chk_mean_rstd(mean, rstd, "layernorm")
    xs = D if x_row_stride is None else x_row_stride
    check(_lib.vl_layernorm_fwd(_p(x), _dt(x), xs, _p(row_index), row_mul, _p(w), _p(b), _p(out), _dt(out),
                                out.stride(-2) if out.dim() >= 2 else D, _p(mean), _p(rstd), rows, D,
                                float(eps), _stream()))
    return out


def assemble_ln_pre(tokens, cls, pos, pos2, w, b, out, B, T, D, eps=1e-5, xpre=None, mean=None, rstd=None):
    _chk_mean_rstd(mean, rstd, "assemble_ln_pre")
    check(_lib.vl_assemble_ln_pre(_p(tokens), _dt(tokens), _p(cls), _p(pos), _p(pos2), _p(w), _p(b), _p(out),
                                  _dt(out), _p(xpre), _p(mean), _p(rstd), B, T, D, float(eps), _stream()))
    return out


def assemble_tokens(tokens, cls, pos, pos2, out, B, T, D, xpre=None):
    """out [B*(T+1), D] (f32 | bf16) = [cls ; tokens] + pos (+ pos2 on rows 1..T): assemble_ln_pre without the LayerNorm, for a
    tower that has no ln_pre (the EVA ViT).  xpre: optional f32 copy of the rows."""
    for name, t in (("tokens", tokens), ("out", out)):
        if t.dtype not in (torch.float32, torch.bfloat16):
            raise ValueError(f"assemble_tokens: {name} must be f32 or bf16, got {t.dtype}")
    for name, t in (("cls", cls), ("pos", pos), ("pos2", pos2), ("xpre", xpre)):
        if t is not None and t.dtype != torch.float32:
            raise ValueError(f"assemble_tokens: {name} must be f32, got {t.dtype}")
    if tokens.numel() != B * T * D or out.numel() != B * (T + 1) * D or cls.numel() != D or pos.numel() != (T + 1) * D:
        raise ValueError("assemble_tokens: tokens [B,T,D], cls [D], pos [T+1,D] and out [B*(T+1),D] do not fit B, T, D")
    if (pos2 is not None and pos2.numel() != T * D) or (xpre is not None and xpre.numel() != out.numel()):
        raise ValueError("assemble_tokens: pos2 is [T,D] and xpre [B*(T+1),D]")
    check(_lib.vl_assemble_tokens(_p(tokens), _dt(tokens), _p(cls), _p(pos), _p(pos2), _p(out), _dt(out), _p(xpre), B, T, D,
                                  _stream()))
    return out


# ------------------------------------------------------------------------------------------------ patch dropout
PATCH_KEEP_MAX_T = 4096


def patch_keep_count(T: int, p: float) -> int:
    """Tokens a tower keeps of T at dropout probability p: the reference's `max(1, int(T * (1 - p)))` in Python floats
    (PatchDropout.forward, open_clip/transformer.py:75-76), e.g. T=10, p=0.9 -> 1 because 10 * (1 - 0.9) < 1.0."""
    p = float(p)
    if not 0.0 <= p < 1.0:
        raise ValueError(f"patch dropout probability must be in [0, 1), got {p}")
    return max(1, int(T * (1 - p)))


def patch_keep(keys, K, B=None, T=None, seed=0, sample0=0, device=None):
    """The kept tokens of a patch-dropout forward -> (keep int32 [B,K], inv int32 [B,T]): keep[b,j] = index of the j-th largest
    key of sample b (ties to the lower index; torch.topk(keys, K).indices for distinct keys), inv[b,t] = j+1 where
    keep[b,j] == t, else 0.  keys f32 [B,T] on the GPU (finite), or None: the kernel's own Philox4x32-10 keys for the samples
    sample0 .. sample0+B-1 under `seed` (then B, T and device are needed)."""
    if keys is not None:
        if keys.dim() != 2 or keys.dtype != torch.float32 or not keys.is_contiguous():
            raise ValueError("patch_keep: keys must be a contiguous f32 [B, T] tensor")
        B, T = keys.shape
        device = keys.device
    elif B is None or T is None or device is None:
        raise ValueError("patch_keep: without keys, B, T and device are needed")
    K = int(K)
    if B < 1 or not 1 <= K <= T <= PATCH_KEEP_MAX_T:      # (the entry refuses these too; no allocation of a negative size first)
        raise RuntimeError(f"libvitlens_hip: vl_patch_keep: bad shape (B >= 1, 1 <= K <= T <= {PATCH_KEEP_MAX_T}): B={B} T={T} K={K}")
    keep = torch.empty(B, K, device=device, dtype=torch.int32)
    inv = torch.empty(B, T, device=device, dtype=torch.int32)
    check(_lib.vl_patch_keep(_p(keys), int(seed) & 0xFFFFFFFFFFFFFFFF, int(sample0), B, T, K, _p(keep), _p(inv), _stream()))
    return keep, inv


def _chk_keep(keep, B, who):
    if keep.dtype != torch.int32 or keep.dim() != 2 or keep.shape[0] != B or not keep.is_contiguous():
        raise ValueError(f"{who}: need a contiguous int32 [B, *] index tensor, got {tuple(keep.shape)} {keep.dtype}")


def assemble_ln_pre_keep(tokens, keep, cls, pos, pos2, w, b, out, B, T, D, eps=1e-5, xpre=None, mean=None, rstd=None):
    """assemble_ln_pre on the class token + the kept tokens only: out [B*(K+1), D] (keep int32 [B,K] from patch_keep)."""
    _chk_keep(keep, B, "assemble_ln_pre_keep")
    _chk_mean_rstd(mean, rstd, "assemble_ln_pre_keep")
    K = keep.shape[1]
    check(_lib.vl_assemble_ln_pre_keep(_p(tokens), _dt(tokens), _p(keep), _p(cls), _p(pos), _p(pos2), _p(w), _p(b), _p(out),
                                       _dt(out), _p(xpre), _p(mean), _p(rstd), B, T, K, D, float(eps), _stream()))
    return out


def scatter_rows_keep(src, inv, K, out=None):
    """The backward of the kept-row gather: src f32 [B*(K+1), D] (rows of [class; kept tokens] per sample), inv int32 [B,T]
    -> out f32 [B*T, D], row (b,t) = src[b*(K+1) + inv[b,t]] where inv[b,t] > 0, zeros elsewhere (every row written)."""
    _chk2d(src, "src", torch.float32)
    B, T = inv.shape
    _chk_keep(inv, B, "scatter_rows_keep")
    D = src.shape[1]
    if not src.is_contiguous() or src.shape[0] != B * (K + 1):
        raise ValueError(f"scatter_rows_keep: src must be a contiguous [B*(K+1), D] = [{B * (K + 1)}, D] matrix, got {tuple(src.shape)}")
    if out is None:
        out = torch.empty(B * T, D, device=src.device, dtype=torch.float32)
    elif out.dtype != torch.float32 or not out.is_contiguous() or out.numel() != B * T * D:
        raise ValueError("scatter_rows_keep: out must be a contiguous f32 [B*T, D] tensor")
    check(_lib.vl_scatter_rows_keep(_p(src), _p(inv), _p(out), B, T, K, D, _stream()))
    return out


def l2_normalize(x, out=None, out_bf16=None, norms=None, eps=1e-12):
    _chk2d(x, "x", torch.float32)
    if out is None:
        out = torch.empty_like(x)
    check(_lib.vl_l2_normalize(_p(x), _p(out), _p(out_bf16), _p(norms), x.shape[0], x.shape[1], float(eps),
                               _stream()))
    return out


def l2_normalize_bwd(f, df, norms, eps=1e-12):
    """f, df: contiguous f32 [rows, D] (the kernel reads both with row stride D); norms: contiguous f32 [rows]."""
    _chk2d(f, "l2_normalize_bwd: f", torch.float32); _chk2d(df, "l2_normalize_bwd: df", torch.float32)
    if not f.is_contiguous() or not df.is_contiguous() or df.shape != f.shape:
        raise ValueError(f"l2_normalize_bwd: f and df must be contiguous and of one shape, got {tuple(f.shape)} strides {f.stride()} "
                         f"and {tuple(df.shape)} strides {df.stride()}")
    if norms.dtype != torch.float32 or norms.dim() != 1 or norms.shape[0] != f.shape[0] or not norms.is_contiguous():
        raise ValueError(f"l2_normalize_bwd: norms must be a contiguous f32 [{f.shape[0]}] tensor")
    if df.device != f.device or norms.device != f.device:
        raise ValueError("l2_normalize_bwd: f, df and norms must live on one device")
    dx = torch.empty_like(f)
    check(_lib.vl_l2_normalize_bwd(_p(f), _p(df), _p(norms), _p(dx), f.shape[0], f.shape[1], float(eps),
                                   _stream()))
    return dx


def im2col(x, kh, kw, sh, sw, Kp, transpose_hw=False, out=None):
    """x [N,C,H,W] f32 (or [N,C,W,H] stored when transpose_hw) -> bf16 [N*gh*gw, Kp]."""
    if x.dtype != torch.float32 or not x.is_contiguous():
        raise ValueError("im2col: need contiguous f32 input")
    N, Cc = x.shape[0], x.shape[1]
    H, W = (x.shape[3], x.shape[2]) if transpose_hw else (x.shape[2], x.shape[3])
    gh, gw = (H - kh) // sh + 1, (W - kw) // sw + 1
    if out is None:
        out = torch.empty(N * gh * gw, Kp, device=x.device, dtype=torch.bfloat16)
    check(_lib.vl_im2col_bf16(_p(x), _p(out), N, Cc, H, W, kh, kw, sh, sw, Kp, 1 if transpose_hw else 0,
                              _stream()))
    return out, gh, gw


def text_embed(ids, tok_emb, pos, out):
    B, L = ids.shape
    check(_lib.vl_text_embed(_p(ids), _p(tok_emb), _p(pos), _p(out), _dt(out), B, L, tok_emb.shape[1],
                             tok_emb.shape[0], _stream()))
    return out


def cast_bf16(x, out=None):
    if out is None:
        out = torch.empty(x.shape, device=x.device, dtype=torch.bfloat16)
    check(_lib.vl_cast_f32_bf16(_p(x), _p(out), x.numel(), _stream()))
    return out


def add_rows(x, table, out, rows, T, D):
    check(_lib.vl_add_rows(_p(x), _dt(x), _p(table), _p(out), _dt(out), rows, T, D, _stream()))
    return out


def transpose_to_bf16(x, ldo=None, out=None):
    """x [R,C] (f32|bf16, row-major) -> bf16 [C, ldo] with zero-filled tail columns."""
    _chk2d(x, "x")
    R, Cc = x.shape
    ldo = R if ldo is None else ldo
    if out is None:
        out = torch.empty(Cc, ldo, device=x.device, dtype=torch.bfloat16)
    check(_lib.vl_transpose_to_bf16(_p(x), _dt(x), x.stride(0), R, Cc, _p(out), ldo, _stream()))
    return out


def transpose_colsum(x, ldo, colsum_out=None, scale=1.0, out=None):
    """x [R,C] -> bf16 [C, ldo] (as transpose_to_bf16) and, fused, colsum_out[c] += scale * sum_r x[r, c] (bias gradient).
    Falls back to the separate kernels when the shape does not fit the fused one."""
    _chk2d(x, "x")
    R, Cc = x.shape
    ok = Cc % 64 == 0 and ldo % 8 == 0 and x.stride(0) % 8 == 0 and R >= 256 and x.data_ptr() % 16 == 0
    if not ok:
        out = transpose_to_bf16(x, ldo=ldo, out=out)
        if colsum_out is not None:
            colsum(x, colsum_out, scale)
        return out
    if out is None:
        out = torch.empty(Cc, ldo, device=x.device, dtype=torch.bfloat16)
    ws = _ws_for(x.device, ldo, Cc, 1) if colsum_out is not None else None
    check(_lib.vl_transpose_colsum_bf16(_p(x), _dt(x), x.stride(0), R, Cc, _p(out), ldo, _p(colsum_out), float(scale), _p(ws),
                                        _stream()))
    return out


def split_bf16x3(x, pattern):
    _chk2d(x, "x", torch.float32)
    out = torch.empty(x.shape[0], 3 * x.shape[1], device=x.device, dtype=torch.bfloat16)
    check(_lib.vl_split_bf16x3(_p(x.contiguous()), _p(out), x.shape[0], x.shape[1], pattern, _stream()))
    return out


def _chk_sim(logits, sim, thres, who):
    """The teacher-similarity block of the masked CE entries: f32, the logits' shape and device, unit column stride."""
    if thres is None:
        raise ValueError(f"{who}: sim needs thres")
    if not torch.is_tensor(sim) or sim.dtype != torch.float32 or sim.dim() != 2 or tuple(sim.shape) != tuple(logits.shape):
        raise ValueError(f"{who}: sim must be an f32 tensor of the logits' shape {tuple(logits.shape)}")
    if sim.device != logits.device or sim.stride(1) != 1:
        raise ValueError(f"{who}: sim must live on the logits' device with contiguous rows")


def ce_stats(logits, label_off=0, want_cols=True, sim=None, thres=None):
    """sim / thres (ClipLossSimMask): an element off the label diagonal with sim[r, c] >= thres is read as logit 0.0."""
    _chk2d(logits, "logits", torch.float32)
    if sim is None and thres is not None:
        raise ValueError("ce_stats: thres needs sim")
    if sim is not None:
        _chk_sim(logits, sim, thres, "ce_stats")
    R, Cc = logits.shape
    dev = logits.device
    row_lse = torch.empty(R, device=dev, dtype=torch.float32)
    diag = torch.empty(R, device=dev, dtype=torch.float32)
    col_lse = torch.empty(Cc, device=dev, dtype=torch.float32) if want_cols else None
    ws = torch.empty(2 * ((R + 63) // 64) * Cc, device=dev, dtype=torch.float32) if want_cols else None
    if sim is None:
        check(_lib.vl_ce_stats(_p(logits), logits.stride(0), R, Cc, label_off, _p(row_lse), _p(col_lse), _p(diag),
                               _p(ws), _stream()))
    else:
        check(_lib.vl_ce_stats_masked(_p(logits), logits.stride(0), R, Cc, label_off, _p(row_lse), _p(col_lse), _p(diag),
                                      _p(ws), _p(sim), sim.stride(0), float(thres), _stream()))
    return row_lse, col_lse, diag


def _chk_vec(t, n, name):
    """A statistic of the CE entries: contiguous f32 [n] on a GPU."""
    if not torch.is_tensor(t) or t.dtype != torch.float32 or t.dim() != 1 or t.shape[0] != n or t.stride(0) != 1:
        raise ValueError(f"{name} must be a contiguous f32 [{n}] tensor")


def ce_loss_accum(loss, row_lse, col_lse, diag, R, Cc, label_off, w_row, w_col):
    """loss[0] += w_row mean_r(row_lse[r] - diag[r]) + w_col mean_r(col_lse[r + label_off] - diag[r]); row_lse / col_lse None: that
    term is absent.  R rows are read of row_lse and diag, Cc columns may be read of col_lse."""
    if R <= 0 or Cc <= 0:
        raise ValueError(f"ce_loss_accum: empty problem ({R} x {Cc})")
    _chk_vec(diag, R, "ce_loss_accum: diag")
    if row_lse is not None:
        _chk_vec(row_lse, R, "ce_loss_accum: row_lse")
    if col_lse is not None:
        _chk_vec(col_lse, Cc, "ce_loss_accum: col_lse")
    if not torch.is_tensor(loss) or loss.dtype != torch.float32 or loss.numel() != 1:
        raise ValueError("ce_loss_accum: loss must be a 1-element f32 tensor")
    if any(t is not None and t.device != loss.device for t in (row_lse, col_lse, diag)):
        raise ValueError("ce_loss_accum: every operand must live on the device of loss")
    check(_lib.vl_ce_loss_accum(_p(row_lse), _p(col_lse), _p(diag), R, Cc, label_off, float(w_row), float(w_col),
                                _p(loss), _stream()))


def ce_grad(logits, row_lse, col_lse, label_off, w_row, w_col, logit_scale, dscale, need_g=True, need_gt=True, sim=None,
            thres=None):
    """sim / thres (ClipLossSimMask): at an element off the label diagonal with sim[r, c] >= thres the logit is read as 0.0
    and G, GT and the d/dscale term are 0 (no gradient flows through the mask)."""
    if sim is None and thres is not None:
        raise ValueError("ce_grad: thres needs sim")
    _chk2d(logits, "ce_grad: logits", torch.float32)
    if sim is not None:
        _chk_sim(logits, sim, thres, "ce_grad")
    R, Cc = logits.shape
    if row_lse is not None:
        _chk_vec(row_lse, R, "ce_grad: row_lse")
    if col_lse is not None:
        _chk_vec(col_lse, Cc, "ce_grad: col_lse")
    if dscale is not None and (not torch.is_tensor(dscale) or dscale.dtype != torch.float32 or dscale.numel() != 1):
        raise ValueError("ce_grad: dscale must be a 1-element f32 tensor")
    if any(t is not None and t.device != logits.device for t in (row_lse, col_lse, dscale)):
        raise ValueError("ce_grad: every operand must live on the logits' device")
    dev = logits.device
    ldg = (Cc + 63) // 64 * 64
    ldgt = (R + 63) // 64 * 64
    G = torch.empty(R, ldg, device=dev, dtype=torch.bfloat16) if need_g else None
    GT = torch.empty(Cc, ldgt, device=dev, dtype=torch.bfloat16) if need_gt else None
    ws = None
    if dscale is not None:
        ws = torch.empty(int(_lib.vl_ce_grad_ws_floats(R, Cc, ldg if need_g else 0, ldgt if need_gt else 0)), device=dev,
                         dtype=torch.float32)
    if sim is None:
        check(_lib.vl_ce_grad(_p(logits), logits.stride(0), R, Cc, label_off, _p(row_lse), _p(col_lse), float(w_row),
                              float(w_col), _p(G), ldg, _p(GT), ldgt, float(logit_scale), _p(dscale), _p(ws), _stream()))
    else:
        check(_lib.vl_ce_grad_masked(_p(logits), logits.stride(0), R, Cc, label_off, _p(row_lse), _p(col_lse), float(w_row),
                                     float(w_col), _p(G), ldg, _p(GT), ldgt, float(logit_scale), _p(dscale), _p(ws), _p(sim),
                                     sim.stride(0), float(thres), _stream()))
    return G, GT


def device_info(device=0):
    arch = C.create_string_buffer(64)
    cus, clk, mem = C.c_int(), C.c_int(), C.c_long()
    check(_lib.vl_device_info(device, arch, 64, C.byref(cus), C.byref(clk), C.byref(mem)))
    return {"arch": arch.value.decode(), "cus": cus.value, "clock_khz": clk.value, "hbm_bytes": mem.value}


# ------------------------------------------------------------------------------------------------ backward
def layernorm_bwd(dy, x, mean, rstd, w, rows, D, dres=None, dx=None, dx_bf16=None, x_row_stride=None,
                  dy_row_stride=None, dx_row_stride=None):
    """dx = dLN(dy) (+ dres).  dres / dx form the residual-gradient stream: f32 or bf16 (both the same dtype); dx_bf16 is
    an optional extra bf16 copy (the next GEMM operand when the stream is f32)."""
    g = dx if dx is not None else dres
    gdt = F32 if g is None else _dt(g)
    if dres is not None and dx is not None and dres.dtype != dx.dtype:
        raise TypeError("layernorm_bwd: dres and dx must share a dtype")
    check(_lib.vl_layernorm_bwd_g(_p(dy), _dt(dy), D if dy_row_stride is None else dy_row_stride, _p(x), _dt(x),
                                  D if x_row_stride is None else x_row_stride, _p(mean), _p(rstd), _p(w), _p(dres),
                                  _p(dx), gdt, _p(dx_bf16), D if dx_row_stride is None else dx_row_stride, rows, D, _stream()))


def layernorm_bwd_sparse_res(dy, x, mean, rstd, w, rows, D, dres, dres_every, dx):
    """layernorm_bwd whose upstream residual gradient exists on the rows i * dres_every only (row i of the small matrix
    `dres`); dx (all `rows` rows, same dtype as dres) = dLN(dy) + that.  No zero-filled gradient buffer is needed."""
    if dres.dtype != dx.dtype or dres.dim() != 2 or dres.stride(1) != 1 or dres.shape[0] * dres_every < rows - dres_every + 1:
        raise ValueError("layernorm_bwd_sparse_res: dres must be a row-major matrix of dx's dtype with one row per dres_every rows")
    check(_lib.vl_layernorm_bwd_sres(_p(dy), _dt(dy), D, _p(x), _dt(x), D, _p(mean), _p(rstd), _p(w), _p(dres), int(dres_every),
                                     dres.stride(0), _p(dx), _dt(dx), None, D, rows, D, _stream()))


_colreduce_ws = {}


def _ws_for(device, rows, cols, planes):
    """Workspace of the deterministic two-stage column reductions (cached per device, grown on demand)."""
    need = int(_lib.vl_colreduce_ws_floats(rows, cols, planes))             # the kernels' own slab geometry, not a copy of it
    # one workspace per device AND stream: two micro-batches' backwards run on two HIP streams (step.py, round 6)
    # (and per host thread: threads that enqueue on one stream interleave their launches - tests emulate ranks that way)
    key = (device, torch.cuda.current_stream(device).cuda_stream, threading.get_ident())
    t = _colreduce_ws.get(key)
    if t is None or t.numel() < need:
        t = torch.empty(need, device=device, dtype=torch.float32)
        _colreduce_ws[key] = t
    return t


def layernorm_bwd_params(dy, x, mean, rstd, dw, db, rows, D, x_row_stride=None, dy_row_stride=None):
    ws = _ws_for(dy.device, rows, D, 2)
    check(_lib.vl_layernorm_bwd_params(_p(dy), _dt(dy), D if dy_row_stride is None else dy_row_stride, _p(x), _dt(x),
                                       D if x_row_stride is None else x_row_stride, _p(mean), _p(rstd), _p(dw), _p(db),
                                       rows, D, _p(ws), _stream()))


def colsum(a, out, scale=1.0):
    _chk2d(a, "a")
    ws = _ws_for(a.device, a.shape[0], a.shape[1], 1)
    check(_lib.vl_colsum(_p(a), _dt(a), a.stride(0), _p(out), a.shape[0], a.shape[1], float(scale), _p(ws), _stream()))


def geglu_bf16(h, out):
    check(_lib.vl_geglu_bf16(_p(h), _p(out), h.shape[0], h.shape[1] // 2, _stream()))
    return out


def gelu_bf16(u, out):
    check(_lib.vl_gelu_bf16(_p(u), _p(out), u.numel(), _stream()))
    return out


def attn_bwd(q, k, v, dO, o, lse, delta, dq, dk, dv, ld_dq, ld_dkv, causal=False, softmax_scale=None, qscale=None, fused=None):
    """q, k, v, dO, o: strided [B,H,L,dh] bf16 views read in place (o = the forward's token-major output viewed by
    heads_view); delta [B,H,Lq] f32 workspace (filled by the two-kernel path); dq/dk/dv token-major destinations.
    fused: None = the one-kernel backward whenever the library takes the shape (vl_attn_bwd_fused_supported: head dim 64,
    self-attention, no mask, L <= 257), True = insist on it (error otherwise), False = the two-kernel path."""
    B, H, Lq, dh = q.shape
    Lk = k.shape[2]
    scale = dh ** -0.5 if softmax_scale is None else softmax_scale
    qs = scale * LOG2E if qscale is None else qscale
    st = _bhld_strides(q, k, v, dO, o)
    if fused is None:
        fused = bool(_lib.vl_attn_bwd_fused_supported(Lq, Lk, dh, 1 if causal else 0))
    if fused:
        if Lq != Lk or causal:
            raise ValueError("attn_bwd(fused=True): self-attention without a causal mask only")
        check(_lib.vl_attn_bwd_fused_bf16(_p(q), _p(k), _p(v), _p(dO), _p(o), st, _p(lse), _p(dq), _p(dk), _p(dv),
                                          ld_dq, ld_dkv, B, H, Lq, dh, float(qs), float(scale), _stream()))
        return
    check(_lib.vl_attn_bwd_bf16(_p(q), _p(k), _p(v), _p(dO), _p(o), st, _p(lse), _p(delta), _p(dq), _p(dk), _p(dv),
                                ld_dq, ld_dkv, B, H, Lq, Lk, dh, float(qs), 1 if causal else 0, float(scale), _stream()))


# ---- Perceiver dropout (csrc/vl_lens_drop.hip).  The draw is numbers, never a stored mask: p, the Philox seed, the per-sample
# number of batch row 0 (step.drop_sample0 with DROP_TOWER_LENS) and the sub-layer's position in the forward.
def check_dropout_p(p, name: str) -> float:
    """A dropout probability of the Lens: a float in [0, 1), or a ValueError that names the knob."""
    p = float(p or 0.0)
    if not 0.0 <= p < 1.0:
        raise ValueError(f"{name} must be in [0, 1), got {p}")
    return p


def attn_fwd_drop(q, k, v, out, p, seed, sample0, sublayer, lse=None, causal=False, qscale=1.0):
    """attn_fwd (bf16 operands) with dropout on the probabilities: out = (P * M / (1 - p)) V; the normaliser and lse are
    attn_fwd's."""
    B, H, Lq, dh = q.shape
    st = _bhld_strides(q, k, v)
    if q.dtype != torch.bfloat16:
        raise TypeError("attn_fwd_drop: bf16 operands only")
    check(_lib.vl_attn_fwd_drop_bf16(_p(q), _p(k), _p(v), st, _p(out), _p(lse), B, H, Lq, k.shape[2], dh, float(qscale),
                                     1 if causal else 0, float(p), int(seed), int(sample0), int(sublayer), _stream()))
    return out


def attn_bwd_drop(q, k, v, dO, o, lse, delta, dq, dk, dv, ld_dq, ld_dkv, p, seed, sample0, sublayer, causal=False,
                  softmax_scale=None, qscale=None):
    """attn_bwd (the two-kernel path) for attn_fwd_drop: the mask is redrawn from the same numbers."""
    B, H, Lq, dh = q.shape
    scale = dh ** -0.5 if softmax_scale is None else softmax_scale
    qs = scale * LOG2E if qscale is None else qscale
    st = _bhld_strides(q, k, v, dO, o)
    check(_lib.vl_attn_bwd_drop_bf16(_p(q), _p(k), _p(v), _p(dO), _p(o), st, _p(lse), _p(delta), _p(dq), _p(dk), _p(dv),
                                     ld_dq, ld_dkv, B, H, Lq, k.shape[2], dh, float(qs), 1 if causal else 0, float(scale),
                                     float(p), int(seed), int(sample0), int(sublayer), _stream()))


def _chk_ff_drop(who, B, n, *ts):
    for t in ts:
        _chk2d(t, who)
        if not t.is_contiguous() or t.shape != ts[0].shape or t.shape[0] != B * n:
            raise ValueError(f"{who}: contiguous [B*n, D] operands of one shape, got {tuple(t.shape)} for B = {B}, n = {n}")


def ff_drop_fwd(y, x0, x1, B, n, p, seed, sample0, sublayer):
    """x1 = x0 + y * M / (1 - p) on f32 [B*n, D] rows (n rows per sample): ff_dropout behind a FeedForward's second Linear."""
    _chk_ff_drop("ff_drop_fwd", B, n, y, x0, x1)
    if not (y.dtype == x0.dtype == x1.dtype == torch.float32):
        raise TypeError("ff_drop_fwd: f32 operands")
    check(_lib.vl_ff_drop_fwd(_p(y), _p(x0), _p(x1), B, n, y.shape[1], float(p), int(seed), int(sample0), int(sublayer), _stream()))
    return x1


def ff_drop_bwd(dx1, dy, B, n, p, seed, sample0, sublayer, dy_f32=None):
    """dy bf16 = dx1 f32 * M / (1 - p): the branch's share of the residual gradient, the operand of dW2 and the dGEGLU GEMM;
    dy_f32 (optional, f32): the same products unrounded - db2 is their column sum."""
    _chk_ff_drop("ff_drop_bwd", B, n, dx1, dy, *(() if dy_f32 is None else (dy_f32,)))
    if dx1.dtype != torch.float32 or dy.dtype != torch.bfloat16 or (dy_f32 is not None and dy_f32.dtype != torch.float32):
        raise TypeError("ff_drop_bwd: dx1 f32, dy bf16, dy_f32 f32")
    check(_lib.vl_ff_drop_bwd(_p(dx1), _p(dy), _p(dy_f32), B, n, dx1.shape[1], float(p), int(seed), int(sample0), int(sublayer),
                              _stream()))
    return dy


def attn_bwd_q1(q, k, v, dO, o, lse, dq, dk, dv, ld_dq, ld_dkv, qrow=0, softmax_scale=None):
    """Backward of attn_fwd_q1.  dO, o bf16 [B, H*64]; lse [B, H]; dq / dk / dv: the token-major destinations of attn_bwd.
    Writes dk, dv for every row, dq for row qrow and ZEROS to every other dq row."""
    B, H, L, dh = q.shape
    if k.shape != q.shape or v.shape != q.shape or q.dtype != torch.bfloat16:
        raise ValueError("attn_bwd_q1: q, k, v must be bf16 views of one [B,H,L,dh] shape (self-attention)")
    _q1_rows(dO, H, "attn_bwd_q1: dO"); _q1_rows(o, H, "attn_bwd_q1: o")
    if dO.shape[0] != B or o.shape[0] != B or lse.dtype != torch.float32 or not lse.is_contiguous() or lse.numel() != B * H:
        raise ValueError("attn_bwd_q1: dO and o must have B rows, lse must be a contiguous f32 [B, H]")
    for t in (dq, dk, dv):
        if t.dtype != torch.bfloat16 or t.dim() != 2 or t.shape[0] < B * L or t.shape[1] < H * 64:
            raise ValueError("attn_bwd_q1: dq / dk / dv must be bf16 [>= B*L, >= H*64] token-major destinations")
    scale = dh ** -0.5 if softmax_scale is None else softmax_scale
    check(_lib.vl_attn_bwd_q1(_p(q), _p(k), _p(v), _bhld_strides(q, k, v), _p(dO), dO.stride(0), _p(o), o.stride(0), _p(lse),
                              _p(dq), _p(dk), _p(dv), ld_dq, ld_dkv, B, H, L, dh, int(qrow), float(scale * LOG2E), float(scale),
                              _stream()))


def adamw_step(p, g, m, v, lr, beta1, beta2, eps, weight_decay, step, grad_scale=1.0):
    for t in (p, g, m, v):
        if t.dtype != torch.float32 or not t.is_contiguous():
            raise ValueError("adamw_step: contiguous f32 tensors required")
    check(_lib.vl_adamw_step(_p(p), _p(g), _p(m), _p(v), p.numel(), float(lr), float(beta1), float(beta2), float(eps),
                             float(weight_decay), int(step), float(grad_scale), _stream()))


ADAMW_MAX_SLOTS = 1024          # VL_ADAMW_MAX_SLOTS
# (device, stream handle) -> workspace of vl_sumsq_f32 (16 KiB).  Calls on one stream run in order, so they share one; two
# streams must not, hence the key.  Never pruned: one entry per stream a caller clips on, and a recycled handle is again one
# stream.  As everywhere in this module the tensor is taken to live on the current device, whose current stream _stream() gives.
_sumsq_ws = {}


def grad_sumsq(flat, out=None):
    """out[0] = sum(flat ** 2), the squared 2-norm of a contiguous f32 tensor (any shape, any element count, 0 included), as a
    1-element f32 tensor on the device: fp64 accumulation, fixed reduction order (bit-reproducible), no host read."""
    if flat.dtype != torch.float32 or not flat.is_contiguous():
        raise ValueError("grad_sumsq: contiguous f32 tensor required")
    if not flat.is_cuda:
        raise RuntimeError("vitlens_hip ops need GPU tensors (no CPU fallback)")
    if out is None:
        out = torch.empty(1, device=flat.device, dtype=torch.float32)
    elif out.dtype != torch.float32 or out.numel() != 1 or out.device != flat.device:
        raise ValueError("grad_sumsq: out must be one f32 element on the input's device")
    key = (flat.device, torch.cuda.current_stream(flat.device).cuda_stream)
    ws = _sumsq_ws.get(key)
    if ws is None:
        ws = _sumsq_ws[key] = torch.empty(int(_lib.vl_sumsq_ws_floats()) // 2, device=flat.device, dtype=torch.float64)
    check(_lib.vl_sumsq_f32(_p(flat) if flat.numel() else None, flat.numel(), _p(out), _p(ws), _stream()))
    return out


def adamw_multi(slots, nslots, lr, beta1, beta2, eps, step, grad_scale, max_norm, sumsq, norm_out=None):
    """AdamW on every tensor of a device slot table in ONE launch, the gradients multiplied by grad_scale and by
    clip_grad_norm_'s coefficient min(1, max_norm / (grad_scale * sqrt(sumsq) + 1e-6)), which is derived on the device.
    slots: int64 [nslots, 6] on the device, rows (p, g, m, v addresses, n, weight_decay's f32 bits) = struct vl_adamw_slot
    (`train.pack_adamw_slots`); sumsq: 1-element f32 device tensor (`grad_sumsq` of all gradients of the table);
    norm_out: optional 1-element f32 device tensor that receives the unclipped norm."""
    if slots.dtype != torch.int64 or slots.dim() != 2 or slots.shape[1] != 6 or not slots.is_contiguous():
        raise ValueError("adamw_multi: slots must be a contiguous int64 [nslots, 6] table")
    if not 0 <= int(nslots) <= min(slots.shape[0], ADAMW_MAX_SLOTS):
        raise ValueError(f"adamw_multi: nslots {nslots} outside the table of {slots.shape[0]} rows (at most {ADAMW_MAX_SLOTS} per launch)")
    if sumsq.dtype != torch.float32 or sumsq.numel() != 1:
        raise ValueError("adamw_multi: sumsq must be one f32 element")
    if norm_out is not None and (norm_out.dtype != torch.float32 or norm_out.numel() != 1):
        raise ValueError("adamw_multi: norm_out must be one f32 element")
    if not float(max_norm) > 0.0:
        raise ValueError(f"adamw_multi: max_norm must be positive, got {max_norm}")
    if int(step) < 1:
        raise ValueError("adamw_multi: step counts from 1")
    check(_lib.vl_adamw_multi_step(_p(slots), int(nslots), float(lr), float(beta1), float(beta2), float(eps), int(step),
                                   float(grad_scale), float(max_norm), _p(sumsq), _p(norm_out), _stream()))


def adamw_multi_step_groups(slots, groups, groups_host, nslots, lr, beta1, beta2, eps, step, grad_scale, max_norm, sumsq,
                            norm_out=None):
    """`adamw_multi` with parameter groups (vl_adamw_multi_step_groups): slot s steps with lr * lr_scale[s], and a slot whose
    no_clip is set is outside the clipped set - it sees coef = 1, and `sumsq` is the squared norm of the OTHER slots' gradients
    (`grad_sumsq` over their contiguous range).  groups: int32 [nslots, 2] on the device, rows (lr_scale's f32 bits, no_clip) =
    struct vl_adamw_group (`train.pack_adamw_groups`); groups_host: the host tensor it was uploaded from, which the library
    checks before the launch (lr_scale finite and >= 0).  norm_out: the unclipped norm of the clipped set."""
    if slots.dtype != torch.int64 or slots.dim() != 2 or slots.shape[1] != 6 or not slots.is_contiguous():
        raise ValueError("adamw_multi_step_groups: slots must be a contiguous int64 [nslots, 6] table")
    if not 0 <= int(nslots) <= min(slots.shape[0], ADAMW_MAX_SLOTS):
        raise ValueError(f"adamw_multi_step_groups: nslots {nslots} outside the table of {slots.shape[0]} rows (at most {ADAMW_MAX_SLOTS} per launch)")
    for t, name in ((groups, "groups"), (groups_host, "groups_host")):
        if t.dtype != torch.int32 or t.dim() != 2 or t.shape[1] != 2 or t.shape[0] < int(nslots) or not t.is_contiguous():
            raise ValueError(f"adamw_multi_step_groups: {name} must be a contiguous int32 [nslots, 2] table")
    if groups_host.device.type != "cpu" or groups.device != slots.device:
        raise ValueError("adamw_multi_step_groups: groups on the slots' device, groups_host on the host")
    if sumsq.dtype != torch.float32 or sumsq.numel() != 1:
        raise ValueError("adamw_multi_step_groups: sumsq must be one f32 element")
    if norm_out is not None and (norm_out.dtype != torch.float32 or norm_out.numel() != 1):
        raise ValueError("adamw_multi_step_groups: norm_out must be one f32 element")
    if not float(max_norm) > 0.0:
        raise ValueError(f"adamw_multi_step_groups: max_norm must be positive, got {max_norm}")
    if int(step) < 1:
        raise ValueError("adamw_multi_step_groups: step counts from 1")
    check(_lib.vl_adamw_multi_step_groups(_p(slots), _p(groups), groups_host.data_ptr(), int(nslots), float(lr), float(beta1),
                                          float(beta2), float(eps), int(step), float(grad_scale), float(max_norm), _p(sumsq),
                                          _p(norm_out), _stream()))


def clamp_scalar(p, lo, hi):
    check(_lib.vl_clamp_scalar(_p(p), float(lo), float(hi), _stream()))


def fill(p, value=0.0):
    """p[:] = value on a contiguous 4-byte-element tensor (f32, or int32 with value 0.0: the same bits) - a step's accumulators
    start from zero through the library, not through a framework fill."""
    if p.element_size() != 4 or not p.is_contiguous() or (p.dtype != torch.float32 and float(value) != 0.0):
        raise ValueError("fill: a contiguous f32 tensor (or an int32 one with value 0)")
    check(_lib.vl_fill_f32(_p(p), float(value), p.numel(), _stream()))
    return p


def axpy(y, x, alpha=1.0):
    check(_lib.vl_axpy_f32(_p(y), _p(x), float(alpha), y.numel(), _stream()))


def scale_exp(x, log_scale, out=None, mul=1.0):
    """out = x * exp(log_scale) * mul with log_scale a 1-element f32 tensor ON THE DEVICE (no host read)."""
    if x.dtype != torch.float32 or not x.is_contiguous() or log_scale.dtype != torch.float32:
        raise ValueError("scale_exp: contiguous f32 tensors required")
    out = torch.empty_like(x) if out is None else out
    check(_lib.vl_scale_exp_f32(_p(x), _p(out), x.numel(), _p(log_scale), float(mul), _stream()))
    return out


def batch_rowsum(x, out, B, T, D, batch_stride_rows, row_offset):
    check(_lib.vl_batch_rowsum(_p(x), _p(out), B, T, D, batch_stride_rows, row_offset, _stream()))


# ------------------------------------------------------------------------------------------------ point clouds
def fps(xyz, start, G, want_centers=True):
    B, N, _ = xyz.shape
    idx = torch.empty(B, G, device=xyz.device, dtype=torch.int64)
    centers = torch.empty(B, G, 3, device=xyz.device, dtype=torch.float32) if want_centers else None
    check(_lib.vl_fps(_p(xyz.contiguous()), _p(start.contiguous()), _p(idx), _p(centers), B, N, G, _stream()))
    return idx, centers


def pc_gather_normalize(pts, idx=None):
    """pts [B,N,C] f32, idx [B,G] int64 or None -> [B,G,C] f32: the selected points centred and scaled into the unit sphere."""
    B, N, Cc = pts.shape
    G = N if idx is None else idx.shape[1]
    out = torch.empty(B, G, Cc, device=pts.device, dtype=torch.float32)
    check(_lib.vl_pc_gather_normalize(_p(pts.contiguous()), _p(idx.contiguous() if idx is not None else None), _p(out), B, N, G, Cc,
                                      _stream()))
    return out


# one record per sample, as csrc/vl_pc_augment.hip reads it (64 bytes; include/vitlens_hip.h spells the layout out)
PC_AUGMENT_DTYPE = np.dtype([("A", "<f4", (9,)), ("t", "<f4", (3,)), ("drop_ratio", "<f4"), ("flags", "<i4"), ("seed", "<u8")])
PC_NORMALIZE, PC_NORM_GUARD, PC_FEAT_FILL = 1, 2, 4          # bits of `flags`


def pc_augment_pack(rows) -> np.ndarray:
    """rows: a PC_AUGMENT_DTYPE array (or per sample (A[9], t[3], drop_ratio, flags, seed)) -> int32 [B, 16], the words of the
    records.  A drop_ratio outside [0, 1] is refused here, on the host, where the records can still be looked at; -1 is
    admitted and means that nothing is dropped (0 still drops a point whose u is exactly 0, as the reference's <= does)."""
    a = rows if isinstance(rows, np.ndarray) and rows.dtype == PC_AUGMENT_DTYPE else np.array([tuple(r) for r in rows], dtype=PC_AUGMENT_DTYPE)
    a = np.ascontiguousarray(a.reshape(-1))
    r = a["drop_ratio"]
    if not np.all(((r >= 0) & (r <= 1)) | (r == -1)):
        raise ValueError(f"pc_augment_params: drop_ratio must be in [0, 1] (or -1: drop nothing), got {r.tolist()}")
    return a.view(np.int32).reshape(len(a), 16)


def pc_augment_params(rows, device) -> torch.Tensor:
    """The device array vl_pc_augment reads (int32 [B, 16]) from the records of `pc_augment_pack`, uploaded from pinned
    memory without waiting for the copy."""
    words = torch.from_numpy(pc_augment_pack(rows))
    device = torch.device(device)
    if device.type == "cuda":
        words = words.pin_memory()
    return words.to(device, non_blocking=True)


def pc_augment(pts, idx, params, feat_fill=0.4):
    """The 3D training transform in one launch (vl_pc_augment): pts [B,N,C] f32, idx [B,G] int64 or None (all points), params
    int32 [B,16] from `pc_augment_params` -> [B,G,C] f32 = gather, normalise, point dropout, xyz . A + t, feature fill."""
    if pts.dim() != 3 or pts.dtype != torch.float32:
        raise ValueError(f"pc_augment: pts must be f32 [B, N, C], got {tuple(pts.shape)} {pts.dtype}")
    B, N, Cc = pts.shape
    if idx is not None and (idx.dim() != 2 or idx.shape[0] != B or idx.dtype != torch.int64 or idx.device != pts.device):
        raise ValueError(f"pc_augment: idx must be int64 [B, G] on the device of pts, got {tuple(idx.shape)} {idx.dtype}")
    if params.shape != (B, 16) or params.dtype != torch.int32 or params.device != pts.device:
        raise ValueError(f"pc_augment: params must be int32 [B, 16] on the device of pts, got {tuple(params.shape)} {params.dtype}")
    G = N if idx is None else idx.shape[1]
    if B < 1 or N < 1 or G < 1:      # (the entry refuses these too; nothing of size 0 is allocated first)
        raise RuntimeError(f"libvitlens_hip: vl_pc_augment: bad shape (B, N, G >= 1, 3 <= C <= 8): B={B} N={N} G={G} C={Cc}")
    out = torch.empty(B, G, Cc, device=pts.device, dtype=torch.float32)
    check(_lib.vl_pc_augment(_p(pts.contiguous()), _p(idx.contiguous() if idx is not None else None), _p(out), B, N, G, Cc,
                             _p(params.contiguous()), float(feat_fill), _stream()))
    return out


# one record per sample, as csrc/vl_rgbd_augment.hip reads it (136 bytes; include/vitlens_hip.h spells the layout out)
RGBD_AUGMENT_DTYPE = np.dtype(
    [("rgb", "<u8"), ("depth", "<u8"), ("rgb_stride", "<i4"), ("depth_stride", "<i4"), ("H", "<i4"), ("W", "<i4"),
     ("top", "<i4"), ("left", "<i4"), ("bh", "<i4"), ("bw", "<i4"), ("row0", "<i4"), ("nrows", "<i4"),
     ("hb", "<i4"), ("hw", "<i4"), ("hks", "<i4"), ("vb", "<i4"), ("vw", "<i4"), ("vks", "<i4"), ("tmp", "<i8"), ("flags", "<i4"),
     ("b", "<f4"), ("b1", "<f4"), ("c", "<f4"), ("c1", "<f4"), ("s", "<f4"), ("s1", "<f4"), ("hue", "<f4"),
     ("ei", "<i4"), ("ej", "<i4"), ("eh", "<i4"), ("ew", "<i4")])
RGBD_FLIP, RGBD_BRIGHTNESS, RGBD_CONTRAST, RGBD_SATURATION, RGBD_HUE, RGBD_ERASE, RGBD_ORDER_SHIFT = 1, 2, 4, 8, 16, 32, 8


def rgbd_augment_pack(rows, S) -> np.ndarray:
    """rows: a RGBD_AUGMENT_DTYPE array -> int32 [n, 34], the words of the records.  The records are read on the device, where
    the entry cannot look at them, so their contents are checked here: the box inside the image, the touched rows inside
    the box, the strides, the order field a permutation of the four terms, the erase rectangle inside the S x S output."""
    a = np.ascontiguousarray(np.asarray(rows, dtype=RGBD_AUGMENT_DTYPE).reshape(-1))

    def need(ok, what):
        if not np.all(ok):
            raise ValueError(f"rgbd_augment_pack: {what} (sample {int(np.argmin(ok))})")
    need((a["rgb"] != 0) & (a["depth"] != 0), "null source pointer")
    need((a["H"] >= 1) & (a["W"] >= 1) & (a["rgb_stride"] >= 3 * a["W"]) & (a["depth_stride"] >= a["W"]), "bad source size or stride")
    need((a["top"] >= 0) & (a["bh"] >= 1) & (a["top"] + a["bh"] <= a["H"]) & (a["left"] >= 0) & (a["bw"] >= 1)
         & (a["left"] + a["bw"] <= a["W"]), "the crop box must lie inside the image")
    need((a["row0"] >= 0) & (a["nrows"] >= 1) & (a["row0"] + a["nrows"] <= a["bh"]), "the touched rows must lie inside the box")
    need((a["hks"] >= 1) & (a["vks"] >= 1) & (a["hb"] >= 0) & (a["hw"] >= 0) & (a["vb"] >= 0) & (a["vw"] >= 0) & (a["tmp"] >= 0),
         "bad table or intermediate offset")
    order = (a["flags"] >> RGBD_ORDER_SHIFT) & 0xFF
    need(sum(1 << ((order >> (2 * k)) & 3) for k in range(4)) == 15, "the order field must hold each of the four terms once")
    need((a["flags"] >> (RGBD_ORDER_SHIFT + 8)) == 0, "unknown flag bits")
    e = (a["flags"] & RGBD_ERASE) != 0
    need(~e | ((a["ei"] >= 0) & (a["eh"] >= 0) & (a["ei"] + a["eh"] <= S) & (a["ej"] >= 0) & (a["ew"] >= 0) & (a["ej"] + a["ew"] <= S)),
         "the erase rectangle must lie inside the output")
    return a.view(np.int32).reshape(len(a), RGBD_AUGMENT_DTYPE.itemsize // 4)


def rgbd_augment(records, tables, tmp, S, max_nrows, mean, std, depth_clamp, out_rgb=None, out_depth=None):
    """The depth recipe's training transform for a batch (vl_rgbd_augment, three launches): records int32 [n, 34] (the words
    of `rgbd_augment_pack`), tables int32 [*] and tmp f32 [*, 4] on the device; mean / std: 4 numbers (RGB, depth);
    depth_clamp = (lo, hi, divide_by) = DepthNorm -> (out_rgb [n,3,S,S], out_depth [n,1,S,S]) f32."""
    if records.dim() != 2 or records.shape[1] != RGBD_AUGMENT_DTYPE.itemsize // 4 or records.dtype != torch.int32 or not records.is_cuda:
        raise ValueError(f"rgbd_augment: records must be int32 [n, 34] on the GPU, got {tuple(records.shape)} {records.dtype} {records.device}")
    n, dev = records.shape[0], records.device
    if tables.dtype != torch.int32 or tables.device != dev or tmp.dtype != torch.float32 or tmp.device != dev:
        raise ValueError("rgbd_augment: tables must be int32 and tmp float32 on the device of the records")
    if len(mean) != 4 or len(std) != 4:
        raise ValueError("rgbd_augment: mean and std hold four numbers (RGB, depth)")
    if n < 1 or S < 1:                   # (the entry refuses these too; nothing of size 0 is allocated first)
        raise RuntimeError(f"libvitlens_hip: vl_rgbd_augment: bad shape: n={n} S={S}")
    if out_rgb is None:
        out_rgb = torch.empty(n, 3, S, S, device=dev, dtype=torch.float32)
    if out_depth is None:
        out_depth = torch.empty(n, 1, S, S, device=dev, dtype=torch.float32)
    for o, c in ((out_rgb, 3), (out_depth, 1)):
        if o.dtype != torch.float32 or not o.is_contiguous() or tuple(o.shape) != (n, c, S, S) or o.device != dev:
            raise ValueError(f"rgbd_augment: outputs must be contiguous f32 [n, {c}, S, S] on the device of the records")
    lo, hi, div = depth_clamp
    fl = lambda v: (C.c_float * 4)(*[float(x) for x in v])
    check(_lib.vl_rgbd_augment(_p(records.contiguous()), n, int(S), int(max_nrows), _p(tables), _p(tmp), fl(mean), fl(std), float(lo),
                               float(hi), float(div), _p(out_rgb), _p(out_depth), _stream()))
    return out_rgb, out_depth


# one record per sample, as csrc/vl_image_augment.hip reads it (368 bytes; include/vitlens_hip.h spells the layout out)
IMAGE_OP_DTYPE = np.dtype([("code", "<i4"), ("ipay", "<i4"), ("fpay", "<f4"), ("pad", "<i4"), ("m", "<f8", (6,))])
IMAGE_AUGMENT_DTYPE = np.dtype(
    [("src", "<u8"), ("stride", "<i4"), ("H", "<i4"), ("W", "<i4"), ("top", "<i4"), ("left", "<i4"), ("bh", "<i4"), ("bw", "<i4"),
     ("row0", "<i4"), ("nrows", "<i4"), ("hb", "<i4"), ("hk", "<i4"), ("hks", "<i4"), ("vb", "<i4"), ("vk", "<i4"), ("vks", "<i4"),
     ("flags", "<i4"), ("tmp", "<i8"), ("b", "<f4"), ("b1", "<f4"), ("c", "<f4"), ("c1", "<f4"), ("s", "<f4"), ("s1", "<f4"),
     ("hue", "<f4"), ("num_ops", "<i4"), ("ops", IMAGE_OP_DTYPE, (4,))])
IMAGE_MAX_OPS = 4
IMAGE_OPS = ("Identity", "ShearX", "ShearY", "TranslateX", "TranslateY", "Rotate", "Brightness", "Color", "Contrast", "Sharpness",
             "Posterize", "Solarize", "AutoContrast", "Equalize")         # the op codes, in RandAugment's own order


def image_augment_pack(rows, S, table_words, tmp_bytes) -> np.ndarray:
    """rows: an IMAGE_AUGMENT_DTYPE array for an S x S output, `table_words` int32 words of tables and `tmp_bytes` of
    intermediate -> int32 [n, 92], the words of the records.  The records are read on the device, where the entry cannot look
    at them, so their contents are checked here: the box inside the image, the touched rows inside the box, the stride, the
    tables ([S,2] bounds, [S,ks] coefficients) and the [nrows,S,3] intermediate inside their buffers, the op count and codes,
    finite matrices and factors, the order field a permutation of the four terms."""
    a = np.ascontiguousarray(np.asarray(rows, dtype=IMAGE_AUGMENT_DTYPE).reshape(-1))

    def need(ok, what):
        if not np.all(ok):
            raise ValueError(f"image_augment_pack: {what} (sample {int(np.argmin(np.asarray(ok).reshape(len(a), -1).all(axis=1)))})")
    need(a["src"] != 0, "null source pointer")
    need((a["H"] >= 1) & (a["W"] >= 1) & (a["stride"] >= 3 * a["W"]), "bad source size or stride")
    need((a["top"] >= 0) & (a["bh"] >= 1) & (a["top"] + a["bh"] <= a["H"]) & (a["left"] >= 0) & (a["bw"] >= 1)
         & (a["left"] + a["bw"] <= a["W"]), "the crop box must lie inside the image")
    need((a["row0"] >= 0) & (a["nrows"] >= 1) & (a["row0"] + a["nrows"] <= a["bh"]), "the touched rows must lie inside the box")
    S, i8 = int(S), lambda name: a[name].astype(np.int64)
    need((a["hks"] >= 1) & (a["vks"] >= 1) & (a["hb"] >= 0) & (a["hk"] >= 0) & (a["vb"] >= 0) & (a["vk"] >= 0) & (a["tmp"] >= 0)
         & (i8("hb") + 2 * S <= table_words) & (i8("vb") + 2 * S <= table_words) & (i8("hk") + S * i8("hks") <= table_words)
         & (i8("vk") + S * i8("vks") <= table_words) & (a["tmp"] + i8("nrows") * S * 3 <= tmp_bytes), "bad table or intermediate offset")
    order = (a["flags"] >> RGBD_ORDER_SHIFT) & 0xFF
    need(sum(1 << ((order >> (2 * k)) & 3) for k in range(4)) == 15, "the order field must hold each of the four terms once")
    need(((a["flags"] >> (RGBD_ORDER_SHIFT + 8)) == 0) & ((a["flags"] & (RGBD_ERASE | 0xC0)) == 0), "unknown flag bits")
    need(np.isfinite(np.stack([a[k] for k in ("b", "b1", "c", "c1", "s", "s1", "hue")], axis=1)), "a jitter factor is not finite")
    need((a["num_ops"] >= 0) & (a["num_ops"] <= IMAGE_MAX_OPS), f"num_ops must be in [0, {IMAGE_MAX_OPS}]")
    used = np.arange(IMAGE_MAX_OPS)[None, :] < a["num_ops"][:, None]
    code = a["ops"]["code"]
    need(~used | ((code >= 0) & (code < len(IMAGE_OPS))), "unknown op code")
    need(~(used & (code >= 1) & (code <= 5))[..., None] | np.isfinite(a["ops"]["m"]), "the matrix of a geometric op is not finite")
    need(~(used & (code >= 6) & (code <= 9)) | np.isfinite(a["ops"]["fpay"]), "the factor of an enhance op is not finite")
    need(~(used & (code == 10)) | ((a["ops"]["ipay"] >= 0) & (a["ops"]["ipay"] <= 255)), "the Posterize mask must be a byte")
    need(~(used & (code == 11)) | ((a["ops"]["ipay"] >= 0) & (a["ops"]["ipay"] <= 256)), "the Solarize threshold must be in [0, 256]")
    return a.view(np.int32).reshape(len(a), IMAGE_AUGMENT_DTYPE.itemsize // 4)


def _image_augment_operands(name, records, tables, tmp):
    words = IMAGE_AUGMENT_DTYPE.itemsize // 4
    if records.dim() != 2 or records.shape[1] != words or records.dtype != torch.int32 or not records.is_cuda:
        raise ValueError(f"{name}: records must be int32 [n, {words}] on the GPU, got {tuple(records.shape)} {records.dtype} {records.device}")
    dev = records.device
    if tables.dtype != torch.int32 or tables.device != dev or tmp.dtype != torch.uint8 or tmp.device != dev:
        raise ValueError(f"{name}: tables must be int32 and tmp uint8 on the device of the records")
    return records.shape[0], dev


def image_crop_resize_u8(records, tables, tmp, S, max_nrows, out_u8=None):
    """img.crop(box).resize((S, S), BILINEAR) and the flip for a batch (vl_image_crop_resize_u8, two launches): records int32
    [n, 92] (the words of `image_augment_pack`), tables int32 [*] and tmp uint8 [*] on the device -> uint8 [n, S, S, 3]."""
    n, dev = _image_augment_operands("image_crop_resize_u8", records, tables, tmp)
    if n < 1 or S < 1:                   # (the entry refuses these too; nothing of size 0 is allocated first)
        raise RuntimeError(f"libvitlens_hip: vl_image_crop_resize_u8: bad shape: n={n} S={S}")
    if out_u8 is None:
        out_u8 = torch.empty(n, S, S, 3, device=dev, dtype=torch.uint8)
    if out_u8.dtype != torch.uint8 or not out_u8.is_contiguous() or tuple(out_u8.shape) != (n, S, S, 3) or out_u8.device != dev:
        raise ValueError("image_crop_resize_u8: out_u8 must be contiguous uint8 [n, S, S, 3] on the device of the records")
    check(_lib.vl_image_crop_resize_u8(_p(records.contiguous()), n, int(S), int(max_nrows), _p(tables), _p(tmp), _p(out_u8), _stream()))
    return out_u8


def image_augment(records, tables, tmp, S, max_nrows, max_ops, mean, std, out=None, out_u8=None, want_u8=False):
    """The plain-image training transform for a batch (vl_image_augment, three launches): records int32 [n, 92] (the words of
    `image_augment_pack`), tables int32 [*] and tmp uint8 [*] on the device; mean / std: 3 numbers -> out [n,3,S,S] f32, and
    with `want_u8` (or a given `out_u8`) also the 8-bit image after RandAugment, uint8 [n,S,S,3]."""
    n, dev = _image_augment_operands("image_augment", records, tables, tmp)
    if len(mean) != 3 or len(std) != 3:
        raise ValueError("image_augment: mean and std hold three numbers")
    if n < 1 or S < 1:                   # (the entry refuses these too; nothing of size 0 is allocated first)
        raise RuntimeError(f"libvitlens_hip: vl_image_augment: bad shape: n={n} S={S}")
    if out is None:
        out = torch.empty(n, 3, S, S, device=dev, dtype=torch.float32)
    if out_u8 is None and want_u8:
        out_u8 = torch.empty(n, S, S, 3, device=dev, dtype=torch.uint8)
    if out.dtype != torch.float32 or not out.is_contiguous() or tuple(out.shape) != (n, 3, S, S) or out.device != dev:
        raise ValueError("image_augment: out must be contiguous f32 [n, 3, S, S] on the device of the records")
    if out_u8 is not None and (out_u8.dtype != torch.uint8 or not out_u8.is_contiguous() or tuple(out_u8.shape) != (n, S, S, 3)
                               or out_u8.device != dev):
        raise ValueError("image_augment: out_u8 must be contiguous uint8 [n, S, S, 3] on the device of the records")
    work = torch.empty(2, n, S, S, 3, device=dev, dtype=torch.uint8)
    fl = lambda v: (C.c_float * 3)(*[float(x) for x in v])
    check(_lib.vl_image_augment(_p(records.contiguous()), n, int(S), int(max_nrows), int(max_ops), _p(tables), _p(tmp), _p(work),
                                fl(mean), fl(std), _p(out), _p(out_u8), _stream()))
    return (out, out_u8) if out_u8 is not None else out


# one record per sample, as csrc/vl_tactile_augment.hip reads it (96 bytes; include/vitlens_hip.h spells the layout out)
TACTILE_AUGMENT_DTYPE = np.dtype(
    [("src", "<u8"), ("stride", "<i4"), ("H", "<i4"), ("W", "<i4"), ("top", "<i4"), ("left", "<i4"), ("bh", "<i4"), ("bw", "<i4"),
     ("row0", "<i4"), ("nrows", "<i4"), ("hb", "<i4"), ("hw", "<i4"), ("hks", "<i4"), ("vb", "<i4"), ("vw", "<i4"), ("vks", "<i4"),
     ("flags", "<i4"), ("tmp", "<i8"), ("t00", "<f4"), ("t01", "<f4"), ("t10", "<f4"), ("t11", "<f4")])
TACTILE_HFLIP, TACTILE_VFLIP = 1, 2


def tactile_augment_pack(rows, S, table_words, tmp_vec) -> np.ndarray:
    """rows: a TACTILE_AUGMENT_DTYPE array for an S x S output, `table_words` int32 words of tables and `tmp_vec` float4 of
    intermediate -> int32 [n, 24], the words of the records.  The records are read on the device, where the entry cannot look
    at them, so their contents are checked here: the box inside the image, the touched rows inside the box, the stride, the
    tables ([S,2] bounds, [S,ks] weights) and the [nrows,S] intermediate inside their buffers, the rotation's four floats
    finite, no flag bit beyond the two flips."""
    a = np.ascontiguousarray(np.asarray(rows, dtype=TACTILE_AUGMENT_DTYPE).reshape(-1))

    def need(ok, what):
        if not np.all(ok):
            raise ValueError(f"tactile_augment_pack: {what} (sample {int(np.argmin(np.asarray(ok).reshape(len(a), -1).all(axis=1)))})")
    need(a["src"] != 0, "null source pointer")
    need((a["H"] >= 1) & (a["W"] >= 1) & (a["stride"] >= 3 * a["W"]), "bad source size or stride")
    need((a["top"] >= 0) & (a["bh"] >= 1) & (a["top"] + a["bh"] <= a["H"]) & (a["left"] >= 0) & (a["bw"] >= 1)
         & (a["left"] + a["bw"] <= a["W"]), "the crop box must lie inside the image")
    need((a["row0"] >= 0) & (a["nrows"] >= 1) & (a["row0"] + a["nrows"] <= a["bh"]), "the touched rows must lie inside the box")
    S, i8 = int(S), lambda name: a[name].astype(np.int64)
    need((a["hks"] >= 1) & (a["vks"] >= 1) & (a["hb"] >= 0) & (a["hw"] >= 0) & (a["vb"] >= 0) & (a["vw"] >= 0) & (a["tmp"] >= 0)
         & (i8("hb") + 2 * S <= table_words) & (i8("vb") + 2 * S <= table_words) & (i8("hw") + S * i8("hks") <= table_words)
         & (i8("vw") + S * i8("vks") <= table_words) & (a["tmp"] + i8("nrows") * S <= tmp_vec), "bad table or intermediate offset")
    need((a["flags"] & ~(TACTILE_HFLIP | TACTILE_VFLIP)) == 0, "unknown flag bits")
    need(np.isfinite(np.stack([a[k] for k in ("t00", "t01", "t10", "t11")], axis=1)), "the rotation matrix is not finite")
    return a.view(np.int32).reshape(len(a), TACTILE_AUGMENT_DTYPE.itemsize // 4)


def tactile_augment(records, tables, tmp, S, max_nrows, mean, std, out=None):
    """The tactile recipe's training transform for a batch (vl_tactile_augment, two launches): records int32 [n, 24] (the words
    of `tactile_augment_pack`), tables int32 [*] and tmp f32 [*, 4] on the device; mean / std: 3 numbers -> out [n,3,S,S] f32."""
    words = TACTILE_AUGMENT_DTYPE.itemsize // 4
    if records.dim() != 2 or records.shape[1] != words or records.dtype != torch.int32 or not records.is_cuda:
        raise ValueError(f"tactile_augment: records must be int32 [n, {words}] on the GPU, got {tuple(records.shape)} {records.dtype} {records.device}")
    n, dev = records.shape[0], records.device
    if tables.dtype != torch.int32 or tables.device != dev or tmp.dtype != torch.float32 or tmp.device != dev:
        raise ValueError("tactile_augment: tables must be int32 and tmp float32 on the device of the records")
    if len(mean) != 3 or len(std) != 3:
        raise ValueError("tactile_augment: mean and std hold three numbers")
    if n < 1 or S < 1:                   # (the entry refuses these too; nothing of size 0 is allocated first)
        raise RuntimeError(f"libvitlens_hip: vl_tactile_augment: bad shape: n={n} S={S}")
    if out is None:
        out = torch.empty(n, 3, S, S, device=dev, dtype=torch.float32)
    if out.dtype != torch.float32 or not out.is_contiguous() or tuple(out.shape) != (n, 3, S, S) or out.device != dev:
        raise ValueError("tactile_augment: out must be contiguous f32 [n, 3, S, S] on the device of the records")
    fl = lambda v: (C.c_float * 3)(*[float(x) for x in v])
    check(_lib.vl_tactile_augment(_p(records.contiguous()), n, int(S), int(max_nrows), _p(tables), _p(tmp), fl(mean), fl(std), _p(out),
                                  _stream()))
    return out


def knn_group(xyz, center_idx, k, Kp=64, want_idx=False):
    B, N, _ = xyz.shape
    G = center_idx.shape[1]
    nidx = torch.empty(B, G, k, device=xyz.device, dtype=torch.int32) if want_idx else None
    patches = torch.empty(B * G * k, Kp, device=xyz.device, dtype=torch.bfloat16)
    check(_lib.vl_knn_group(_p(xyz.contiguous()), _p(center_idx.contiguous()), _p(nidx), _p(patches), B, N, G, k, Kp, _stream()))
    return patches, nidx


def ball_group(xyz, feats, center_idx, radius, nsample, Kp=64, want_idx=False):
    """Ball query + grouping of the `pnsa` tokenizer (pointnet_util.py:101-161).  xyz [B,N,3] f32, feats [B,N,D] f32 or
    None, center_idx [B,S] int64 -> (patches bf16 [B*S*nsample, Kp] = (xyz_j - centre ++ feats_j, zero padded),
    idx int32 [B,S,nsample] or None).  The radius is squared in double and rounded to f32, as `d > radius ** 2` does."""
    import numpy as np
    B, N, _ = xyz.shape
    S = center_idx.shape[1]
    D = 0 if feats is None else feats.shape[2]
    idx = torch.empty(B, S, nsample, device=xyz.device, dtype=torch.int32) if want_idx else None
    patches = torch.empty(B * S * nsample, Kp, device=xyz.device, dtype=torch.bfloat16)
    check(_lib.vl_ball_group(_p(xyz.contiguous()), _p(feats.contiguous() if feats is not None else None), _p(center_idx.contiguous()),
                             _p(idx), _p(patches), B, N, S, D, float(np.float32(float(radius) ** 2)), nsample, Kp, _stream()))
    return patches, idx


def group_max(x, M, out_dtype=torch.bfloat16):
    _chk2d(x, "x", torch.bfloat16)
    groups = x.shape[0] // M
    out = torch.empty(groups, x.shape[1], device=x.device, dtype=out_dtype)
    check(_lib.vl_group_max(_p(x), x.stride(0), _p(out), _dt(out), out.stride(0), groups, M, x.shape[1], _stream()))
    return out


def pad3(c, Kp=64):
    c = c.reshape(-1, 3).contiguous()
    out = torch.empty(c.shape[0], Kp, device=c.device, dtype=torch.bfloat16)
    check(_lib.vl_pad3_bf16(_p(c), _p(out), c.shape[0], Kp, _stream()))
    return out


# ---- fp32 point-tokenizer pieces (precision="fp32" inference, vitlens_hip/f32.py) ----
def knn_group_f32(xyz, center_idx, k, Kp=4, want_idx=False, out=None):
    """knn_group with fp32 patches [B*G*k, Kp] = x_j - centre, zero padded (Kp a multiple of 4); same neighbour sets."""
    B, N, _ = xyz.shape
    G = center_idx.shape[1]
    nidx = torch.empty(B, G, k, device=xyz.device, dtype=torch.int32) if want_idx else None
    patches = torch.empty(B * G * k, Kp, device=xyz.device, dtype=torch.float32) if out is None else out
    if patches.dtype != torch.float32 or not patches.is_contiguous() or tuple(patches.shape) != (B * G * k, Kp):
        raise ValueError(f"knn_group_f32: out must be contiguous f32 [{B * G * k}, {Kp}]")
    check(_lib.vl_knn_group_f32(_p(xyz.contiguous()), _p(center_idx.contiguous()), _p(nidx), _p(patches), B, N, G, k, Kp,
                                _stream()))
    return patches, nidx


def group_max_f32(x, M, out=None):
    """out f32 [rows / M, C] = max over the M rows of each group of x f32 [rows, C] (NaN propagates, as torch.max)."""
    _chk2d(x, "x", torch.float32)
    groups = x.shape[0] // M
    if out is None:
        out = torch.empty(groups, x.shape[1], device=x.device, dtype=torch.float32)
    _chk2d(out, "out", torch.float32)
    check(_lib.vl_group_max_f32(_p(x), x.stride(0), _p(out), out.stride(0), groups, M, x.shape[1], _stream()))
    return out


def pad3_f32(c, Kp=4):
    c = c.reshape(-1, 3).contiguous()
    out = torch.empty(c.shape[0], Kp, device=c.device, dtype=torch.float32)
    check(_lib.vl_pad3_f32(_p(c), _p(out), c.shape[0], Kp, _stream()))
    return out


def _bn_chunks(R):
    return max(1, min(1024, R // 64))


def bn_stats(x, running_mean=None, running_var=None, momentum=0.1):
    """Batch statistics of nn.BatchNorm1d over the rows of x [R,C] bf16 -> (mean, biased var) f32 [C]."""
    _chk2d(x, "x", torch.bfloat16)
    R, C = x.shape
    n = _bn_chunks(R)
    ws = torch.empty((n + 1) * 2 * C, device=x.device, dtype=torch.float32)
    mean = torch.empty(C, device=x.device, dtype=torch.float32); var = torch.empty_like(mean)
    check(_lib.vl_bn_stats(_p(x), x.stride(0), R, C, _p(ws), n, _p(mean), _p(var), _p(running_mean), _p(running_var),
                           momentum, _stream()))
    return mean, var


def bn_apply(x, mean, var, gamma, beta, eps=1e-5, relu=False, out=None):
    _chk2d(x, "x", torch.bfloat16)
    out = torch.empty_like(x) if out is None else out
    check(_lib.vl_bn_apply(_p(x), x.stride(0), _p(mean), _p(var), _p(gamma), _p(beta), eps, int(relu), _p(out), out.stride(0),
                           x.shape[0], x.shape[1], _stream()))
    return out


def bn_bwd(dy, x, mean, var, gamma, beta, dgamma, dbeta, eps=1e-5, relu=False, train=True, need_dx=True):
    """dgamma/dbeta (f32 [C]) are accumulated; returns dx bf16 [R,C] (None when need_dx is False)."""
    _chk2d(dy, "dy", torch.bfloat16); _chk2d(x, "x", torch.bfloat16)
    R, C = x.shape
    n = _bn_chunks(R)
    ws = torch.empty((n + 1) * 2 * C, device=x.device, dtype=torch.float32)
    dx = torch.empty_like(x) if need_dx else None
    check(_lib.vl_bn_bwd(_p(dy), dy.stride(0), _p(x), x.stride(0), _p(mean), _p(var), _p(gamma), _p(beta), eps, int(relu),
                         int(train), _p(ws), n, _p(dgamma), _p(dbeta), _p(dx), dx.stride(0) if need_dx else 0, R, C, _stream()))
    return dx


# ---- SyncBatchNorm: the statistics / backward passes split where the ranks exchange data (csrc/vl_bn.hip) ----
def bn_stats_local(x):
    """This rank's share of the batch statistics of x [R,C] bf16 -> f32 [2C+1]: mean, M2, row count (int bits)."""
    _chk2d(x, "x", torch.bfloat16)
    R, C = x.shape
    n = _bn_chunks(R)
    ws = torch.empty((n + 1) * 2 * C, device=x.device, dtype=torch.float32)
    local = torch.empty(2 * C + 1, device=x.device, dtype=torch.float32)
    check(_lib.vl_bn_stats_local(_p(x), x.stride(0), R, C, _p(ws), n, _p(local), _stream()))
    return local


def bn_stats_merge(gathered, running_mean=None, running_var=None, momentum=0.1):
    """gathered f32 [W, 2C+1] (all ranks' bn_stats_local) -> (mean, biased var, total) with total an int32 [1] tensor
    holding the global row count; running statistics updated with the global unbiased variance."""
    W, n = gathered.shape
    Cc = (n - 1) // 2
    mean = torch.empty(Cc, device=gathered.device, dtype=torch.float32); var = torch.empty_like(mean)
    total = torch.empty(1, device=gathered.device, dtype=torch.int32)
    check(_lib.vl_bn_stats_merge(_p(gathered.contiguous()), W, Cc, _p(mean), _p(var), _p(running_mean), _p(running_var), momentum,
                                 _p(total), _stream()))
    return mean, var, total


def bn_bwd_reduce(dy, x, mean, var, gamma, beta, dgamma, dbeta, eps=1e-5, relu=False):
    """dgamma/dbeta accumulated (local sums, as SyncBatchNorm); returns sums f32 [2C] = (sum dy', sum dy'*xhat) to all-reduce."""
    _chk2d(dy, "dy", torch.bfloat16); _chk2d(x, "x", torch.bfloat16)
    R, C = x.shape
    n = _bn_chunks(R)
    ws = torch.empty((n + 1) * 2 * C, device=x.device, dtype=torch.float32)
    sums = torch.empty(2 * C, device=x.device, dtype=torch.float32)
    check(_lib.vl_bn_bwd_reduce(_p(dy), dy.stride(0), _p(x), x.stride(0), _p(mean), _p(var), _p(gamma), _p(beta), eps, int(relu),
                                _p(ws), n, _p(dgamma), _p(dbeta), _p(sums), R, C, _stream()))
    return sums


def bn_bwd_apply(dy, x, mean, var, gamma, beta, sums, total, eps=1e-5, relu=False):
    """dx bf16 [R,C] from the globally summed `sums` and the global row count `total` (int32 [1] on the device)."""
    _chk2d(dy, "dy", torch.bfloat16); _chk2d(x, "x", torch.bfloat16)
    R, C = x.shape
    dx = torch.empty_like(x)
    check(_lib.vl_bn_bwd_apply(_p(dy), dy.stride(0), _p(x), x.stride(0), _p(mean), _p(var), _p(gamma), _p(beta), eps, int(relu),
                               _p(sums), _p(total), _p(dx), dx.stride(0), R, C, _stream()))
    return dx


def group_max_bwd(f, dg, M, base=None):
    _chk2d(f, "f", torch.bfloat16); _chk2d(dg, "dg", torch.bfloat16)
    out = torch.empty_like(f)
    check(_lib.vl_group_max_bwd(_p(f), f.stride(0), _p(dg), dg.stride(0), _p(base), base.stride(0) if base is not None else 0,
                                _p(out), out.stride(0), f.shape[0] // M, M, f.shape[1], _stream()))
    return out


def group_sum(x, M):
    _chk2d(x, "x", torch.bfloat16)
    out = torch.empty(x.shape[0] // M, x.shape[1], device=x.device, dtype=torch.bfloat16)
    check(_lib.vl_group_sum(_p(x), x.stride(0), _p(out), out.stride(0), x.shape[0] // M, M, x.shape[1], _stream()))
    return out




# ---- the linear probe (csrc/vl_linprobe.hip): Dropout -> BatchNorm1d(affine=False) -> Linear, label cross-entropy, LARS ----
LARS_MAX_SLOTS = 1024           # VL_LARS_MAX_SLOTS
LARS_TILE = 2048                # elements per work tile of vl_lars_multi_step


def _lp_pad4(n: int) -> int:
    return (int(n) + 3) // 4 * 4


def lp_bn_fwd(x, running_mean, running_var, train, p=0.0, keep=None, seed=0, sample0=0, momentum=0.1, eps=1e-6, xhat=None,
              xhatT=None, mean=None, var=None):
    """Dropout(p) -> BatchNorm1d(D, affine=False, eps) on pooled features x f32 [B, D] (row-major, any row stride that is a
    multiple of 4) -> xhat f32 [B, D]; xhatT (optional, f32 [D, ldt], ldt % 4 == 0, ldt >= B) receives the transpose with zeros
    behind column B.  train: the dropout mask is `keep` (u8 / bool [B, D], contiguous) when given, else the kernel's own
    Philox4x32-10 draw for the samples sample0 .. sample0+B-1 under `seed` (p = 0: no mask at all); batch statistics normalise,
    `mean` / `var` (f32 [D], optional) receive them and running_mean / running_var are updated as nn.BatchNorm1d does.
    Eval: the running statistics normalise and nothing else is written."""
    _chk2d(x, "lp_bn_fwd: x", torch.float32)
    B, D = x.shape
    p = float(p)
    if D < 4 or D % 4 or x.stride(0) % 4:
        raise ValueError(f"lp_bn_fwd: D and the row stride must be multiples of 4, got D={D} stride {x.stride(0)}")
    if not 0.0 <= p < 1.0:
        raise ValueError(f"lp_bn_fwd: dropout probability must be in [0, 1), got {p}")
    if train and B < 2:
        raise ValueError("lp_bn_fwd: Expected more than 1 value per channel when training (B >= 2)")
    for name, t in (("running_mean", running_mean), ("running_var", running_var), ("mean", mean), ("var", var)):
        if t is None:
            if name.startswith("running") and not train:
                raise ValueError("lp_bn_fwd: eval mode needs the running statistics")
            continue
        if t.dtype != torch.float32 or t.numel() != D or not t.is_contiguous() or t.device != x.device:
            raise ValueError(f"lp_bn_fwd: {name} must be a contiguous f32 [{D}] tensor on x's device")
    if (running_mean is None) != (running_var is None):
        raise ValueError("lp_bn_fwd: running_mean and running_var come together")
    if keep is not None:
        if keep.dtype == torch.bool:
            keep = keep.view(torch.uint8)
        if keep.dtype != torch.uint8 or tuple(keep.shape) != (B, D) or not keep.is_contiguous() or keep.device != x.device:
            raise ValueError(f"lp_bn_fwd: keep must be a contiguous u8 / bool [{B}, {D}] tensor on x's device")
    if xhat is None:
        xhat = torch.empty(B, D, device=x.device, dtype=torch.float32)
    _chk2d(xhat, "lp_bn_fwd: xhat", torch.float32)
    if tuple(xhat.shape) != (B, D) or xhat.stride(0) % 4:
        raise ValueError("lp_bn_fwd: xhat must be f32 [B, D] with a row stride that is a multiple of 4")
    ldt = 0
    if xhatT is not None:
        _chk2d(xhatT, "lp_bn_fwd: xhatT", torch.float32)
        ldt = xhatT.shape[1]
        if xhatT.shape[0] != D or ldt < B or ldt % 4 or not xhatT.is_contiguous():
            raise ValueError(f"lp_bn_fwd: xhatT must be a contiguous f32 [{D}, ldt] tensor, ldt % 4 == 0 and >= {B}")
    check(_lib.vl_lp_bn_fwd(_p(x), x.stride(0), _p(keep), p, int(seed) & 0xFFFFFFFFFFFFFFFF, int(sample0), 1 if train else 0,
                            _p(running_mean), _p(running_var), float(momentum), float(eps), _p(xhat), xhat.stride(0), _p(xhatT),
                            ldt, _p(mean), _p(var), B, D, _stream()))
    return xhat


def ce_label(logits, target, gscale=1.0, need_g=False, need_gt=False, need_dbias=False, loss=None, G=None, GT=None, dbias=None,
             ws=None):
    """torch.nn.CrossEntropyLoss() (mean) over logits f32 [B, C] (row-major, any row stride) and target int64 [B], and its
    gradient -> (loss [1], G, GT, dbias), the last three None unless asked for (need_* or a given tensor):
    G f32 [B, C] = gscale (softmax - onehot) / B, GT f32 [C, pad4(B)] = its transpose with zeros behind column B,
    dbias f32 [C] = G's column sums.  A target outside [0, C) gives NaN in its row of G and a NaN loss."""
    _chk2d(logits, "ce_label: logits", torch.float32)
    B, Cc = logits.shape
    if B < 1 or Cc < 1:
        raise ValueError("ce_label: empty problem")
    if target.dtype != torch.int64 or tuple(target.shape) != (B,) or not target.is_contiguous() or target.device != logits.device:
        raise ValueError(f"ce_label: target must be a contiguous int64 [{B}] tensor on the logits' device")
    dev = logits.device
    if loss is None:
        loss = torch.empty(1, device=dev, dtype=torch.float32)
    elif loss.dtype != torch.float32 or loss.numel() != 1:
        raise ValueError("ce_label: loss must be one f32 element")
    if G is None and need_g:
        G = torch.empty(B, Cc, device=dev, dtype=torch.float32)
    if GT is None and need_gt:
        GT = torch.empty(Cc, _lp_pad4(B), device=dev, dtype=torch.float32)
    if dbias is None and need_dbias:
        dbias = torch.empty(Cc, device=dev, dtype=torch.float32)
    ldg = ldgt = 0
    if G is not None:
        _chk2d(G, "ce_label: G", torch.float32)
        if tuple(G.shape) != (B, Cc):
            raise ValueError(f"ce_label: G must be f32 [{B}, {Cc}]")
        ldg = G.stride(0)
    if GT is not None:
        _chk2d(GT, "ce_label: GT", torch.float32)
        ldgt = GT.shape[1]
        if GT.shape[0] != Cc or ldgt < B or ldgt % 4 or (Cc > 1 and GT.stride(0) != ldgt):
            raise ValueError(f"ce_label: GT must be a contiguous f32 [{Cc}, ldgt] tensor, ldgt % 4 == 0 and >= {B}")
    if dbias is not None and (dbias.dtype != torch.float32 or dbias.numel() != Cc or not dbias.is_contiguous()):
        raise ValueError(f"ce_label: dbias must be a contiguous f32 [{Cc}] tensor")
    need = int(_lib.vl_ce_label_ws_floats(B, Cc))
    if ws is None:
        ws = torch.empty(need, device=dev, dtype=torch.float32)
    elif ws.dtype != torch.float32 or ws.numel() < need or not ws.is_contiguous():
        raise ValueError(f"ce_label: workspace of {need} f32 elements required")
    check(_lib.vl_ce_label(_p(logits), logits.stride(0), _p(target), B, Cc, float(gscale), _p(loss), _p(G), ldg, _p(GT), ldgt,
                           _p(dbias), _p(ws), _stream()))
    return loss, G, GT, dbias


def ce_label_ws_floats(B, C):
    return int(_lib.vl_ce_label_ws_floats(int(B), int(C)))


def pack_lars_slots(rows):
    """rows of (p, g, mu, weight_decay, adapt) - three contiguous f32 tensors of one shape on the GPU, a float and a flag ->
    the int64 [len, 5] image of `struct vl_lars_slot[]` (HOST tensor; 40 bytes per slot): (p, g, mu addresses, n, the f32 bits
    of weight_decay in the low word and adapt in the high word).  The caller uploads it once and keeps the tensors alive."""
    import struct
    out = torch.empty(len(rows), 5, dtype=torch.int64)
    for i, (p, g, mu, wd, adapt) in enumerate(rows):
        for name, t in (("p", p), ("g", g), ("mu", mu)):
            if t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != p.numel():
                raise ValueError(f"pack_lars_slots: slot {i}: {name} must be a contiguous f32 tensor of p's size")
            if not t.is_cuda:
                raise RuntimeError("vitlens_hip ops need GPU tensors (no CPU fallback)")
        lo = struct.unpack("<I", struct.pack("<f", float(wd)))[0]
        word = lo | ((1 if adapt else 0) << 32)
        out[i] = torch.tensor([p.data_ptr(), g.data_ptr(), mu.data_ptr(), p.numel(), word], dtype=torch.int64)
    return out


def lars_ws_floats(total_elems, nslots):
    return int(_lib.vl_lars_ws_floats(int(total_elems), int(nslots)))


def lars_multi_step(slots, nslots, lr, momentum=0.9, trust_coefficient=1e-3, grad_scale=1.0, max_norm=None, sumsq=None, ws=None,
                    total_elems=None):
    """The reference's LARS.step (training/optimizer.py) on every tensor of a device slot table (`pack_lars_slots`, uploaded) in
    one call: weight decay and the trust ratio |p| / |dp| on the adapt slots only, momentum and the update on all; the norms
    and the ratio stay on the device.  max_norm (with sumsq = `grad_sumsq` of all gradients of the table) folds
    clip_grad_norm_ in, as `adamw_multi` does.  ws: f64 workspace of lars_ws_floats(total, nslots) / 2 elements (or
    total_elems, from which it is allocated)."""
    if slots.dtype != torch.int64 or slots.dim() != 2 or slots.shape[1] != 5 or not slots.is_contiguous():
        raise ValueError("lars_multi_step: slots must be a contiguous int64 [nslots, 5] table")
    if not 0 <= int(nslots) <= min(slots.shape[0], LARS_MAX_SLOTS):
        raise ValueError(f"lars_multi_step: nslots {nslots} outside the table of {slots.shape[0]} rows (at most {LARS_MAX_SLOTS} per launch)")
    clip = max_norm is not None and float(max_norm) > 0.0
    if clip and (sumsq is None or sumsq.dtype != torch.float32 or sumsq.numel() != 1):
        raise ValueError("lars_multi_step: max_norm needs sumsq, one f32 element (grad_sumsq of the gradients)")
    if ws is None:
        if total_elems is None:
            raise ValueError("lars_multi_step: pass the workspace or total_elems")
        ws = torch.empty(lars_ws_floats(total_elems, nslots) // 2 + 1, device=slots.device, dtype=torch.float64)
    if ws.dtype != torch.float64 or not ws.is_contiguous() or ws.numel() < 2:
        raise ValueError("lars_multi_step: the workspace is a contiguous f64 tensor of lars_ws_floats(total, nslots) / 2 elements")
    check(_lib.vl_lars_multi_step(_p(slots), int(nslots), float(lr), float(momentum), float(trust_coefficient), float(grad_scale),
                                  float(max_norm) if clip else 0.0, _p(sumsq) if clip else None, _p(ws), 2 * ws.numel(), _stream()))


def topk_hits(logits, target, ks=(1, 5), hits=None, correct=None, need_correct=False):
    """Top-k hit counts of logits f32 [B, C] against target int64 [B] for the two k of `ks`, ADDED into hits (int32 [2]; a new
    zeroed tensor when None) -> (hits, correct u8 [B, 2] or None).  Ties: the lower class index ranks first."""
    _chk2d(logits, "topk_hits: logits", torch.float32)
    B, Cc = logits.shape
    if B < 1 or Cc < 1:
        raise ValueError("topk_hits: empty problem")
    if target.dtype != torch.int64 or tuple(target.shape) != (B,) or not target.is_contiguous() or target.device != logits.device:
        raise ValueError(f"topk_hits: target must be a contiguous int64 [{B}] tensor on the logits' device")
    if len(ks) != 2 or min(int(k) for k in ks) < 1:
        raise ValueError("topk_hits: two values of k, each >= 1")
    if hits is None:
        hits = torch.zeros(2, device=logits.device, dtype=torch.int32)
    elif hits.dtype != torch.int32 or hits.numel() != 2 or not hits.is_contiguous():
        raise ValueError("topk_hits: hits must be a contiguous int32 [2] tensor")
    if correct is None and need_correct:
        correct = torch.empty(B, 2, device=logits.device, dtype=torch.uint8)
    if correct is not None and (correct.dtype != torch.uint8 or tuple(correct.shape) != (B, 2) or not correct.is_contiguous()):
        raise ValueError(f"topk_hits: correct must be a contiguous u8 [{B}, 2] tensor")
    check(_lib.vl_topk_hits(_p(logits), logits.stride(0), _p(target), B, Cc, int(ks[0]), int(ks[1]), _p(hits), _p(correct), _stream()))
    return hits, correct


def _i32(t, n, name, device):
    if t.dtype != torch.int32 or t.numel() != n or not t.is_contiguous() or t.device != device:
        raise ValueError(f"{name} must be a contiguous int32 tensor of {n} elements on the logits' device")
    return t


def eval_hits(logits, target, ks=(1, 5), class_map=None, hits=None, per_class=None, pred=None, need_pred=False):
    """`topk_hits` with a class map, per-class counters and the arg-max (vl_eval_hits): logits f32 [B, C], target int64 [B] ->
    (hits, pred).  class_map: int32 [C] (None: identity) - a sample hits at k when the best-scoring member of its target's group
    ranks below k, the reference's cond_acc.  hits int32 [2] and per_class int32 [3, C] (rows: samples, hits at ks[0], hits at
    ks[1], indexed by the target) ACCUMULATE; hits is a new zeroed tensor when None.  pred int32 [B] (need_pred: allocated here):
    the row's arg-max, lowest index on ties.  A target outside [0, C) is a miss and changes no per-class counter."""
    _chk2d(logits, "eval_hits: logits", torch.float32)
    B, Cc = logits.shape
    if B < 1 or Cc < 1:
        raise ValueError("eval_hits: empty problem")
    dev = logits.device
    if target.dtype != torch.int64 or tuple(target.shape) != (B,) or not target.is_contiguous() or target.device != dev:
        raise ValueError(f"eval_hits: target must be a contiguous int64 [{B}] tensor on the logits' device")
    if len(ks) != 2 or min(int(k) for k in ks) < 1:
        raise ValueError("eval_hits: two values of k, each >= 1")
    if class_map is not None:
        _i32(class_map, Cc, "eval_hits: class_map", dev)
    hits = torch.zeros(2, device=dev, dtype=torch.int32) if hits is None else _i32(hits, 2, "eval_hits: hits", dev)
    if per_class is not None and (per_class.dim() != 2 or per_class.shape[0] != 3):
        raise ValueError(f"eval_hits: per_class must be int32 [3, {Cc}]")
    pc = [None] * 3 if per_class is None else list(_i32(per_class, 3 * Cc, "eval_hits: per_class", dev))
    if pred is None and need_pred:
        pred = torch.empty(B, device=dev, dtype=torch.int32)
    if pred is not None:
        _i32(pred, B, "eval_hits: pred", dev)
    check(_lib.vl_eval_hits(_p(logits), logits.stride(0), _p(target), _p(class_map), B, Cc, int(ks[0]), int(ks[1]), _p(hits),
                            _p(pc[0]), _p(pc[1]), _p(pc[2]), _p(pred), _stream()))
    return hits, pred


def class_map_from_merge(num_classes, idx_mapping, merge_idx, device):
    """The class map of `eval_hits` for the reference's cond_acc(idx_mapping, merge_idx): the listed classes become merge_idx."""
    m = list(range(int(num_classes)))
    for i in idx_mapping:
        if 0 <= int(i) < len(m):
            m[int(i)] = int(merge_idx)
    return torch.tensor(m, dtype=torch.int32, device=device)


def average_precision(scores, targets, out=None):
    """Per-class average precision (vl_average_precision; scikit-learn's average_precision_score(average=None) on RAW scores):
    scores f32 [N, C], targets f32 [N, C] (positive: > 0) -> f64 [C].  A class without positives scores 0.0."""
    _chk2d(scores, "average_precision: scores", torch.float32)
    _chk2d(targets, "average_precision: targets", torch.float32)
    N, Cc = scores.shape
    if N < 1 or Cc < 1 or tuple(targets.shape) != (N, Cc) or targets.device != scores.device:
        raise ValueError(f"average_precision: scores and targets must be non-empty [N, C] tensors of one shape on one device, got "
                         f"{tuple(scores.shape)} and {tuple(targets.shape)}")
    if out is None:
        out = torch.empty(Cc, device=scores.device, dtype=torch.float64)
    elif out.dtype != torch.float64 or out.numel() != Cc or not out.is_contiguous():
        raise ValueError(f"average_precision: out must be a contiguous f64 [{Cc}] tensor")
    ws = torch.empty(int(_lib.vl_average_precision_ws_bytes(N, Cc)) // 8 + 1, device=scores.device, dtype=torch.float64)
    check(_lib.vl_average_precision(_p(scores), scores.stride(0), _p(targets), targets.stride(0), N, Cc, _p(out), _p(ws), _stream()))
    return out


def clip_mean_normalize(x, n_clip, eps=1e-12):
    """x f32 [B * n_clip, D], a sample's clips in consecutive rows -> F.normalize(x.view(B, n_clip, D).mean(1), dim=-1) f32 [B, D]
    (vl_clip_mean_normalize: the audio evaluation's mean over clips and the normalisation in one launch)."""
    _chk2d(x, "clip_mean_normalize: x", torch.float32)
    n_clip = int(n_clip)
    if n_clip < 1 or x.shape[0] < n_clip or x.shape[0] % n_clip or x.shape[1] < 1:
        raise ValueError(f"clip_mean_normalize: {x.shape[0]} rows are no positive multiple of n_clip = {n_clip}")
    B, D = x.shape[0] // n_clip, x.shape[1]
    out = torch.empty(B, D, device=x.device, dtype=torch.float32)
    check(_lib.vl_clip_mean_normalize(_p(x), x.stride(0), B, n_clip, D, float(eps), _p(out), _stream()))
    return out
