"""Forward executors for the ViT / text towers on the HIP kernels.

`VitEngine` runs  tokens -> [cls;tokens]+pos -> ln_pre -> N x ResidualAttentionBlock -> ln_post(cls)
-> @proj  (open_clip/transformer.py:756-787) and `TextEngine` runs TriCLIP.encode_text
(open_clip/model.py:528-540), both as a fixed sequence of C-ABI calls on the current stream with
pre-allocated workspaces (no allocation inside the block loop -> hipGraph-capturable).

Precision contract (= the reference under torch autocast): GEMM operands bf16, accumulation fp32,
LayerNorm / softmax statistics / residual stream / final features fp32 (residual dtype selectable).
"""
from copy import copy
from dataclasses import dataclass, replace
from typing import Dict, Optional

import torch

from . import ops


@dataclass
class TowerCfg:
    width: int = 1024
    layers: int = 24
    heads: int = 16
    mlp_ratio: float = 4.0
    patch: int = 14
    image_size: int = 224
    embed_dim: int = 768
    in_chans: int = 3
    quick_gelu: bool = False     # the blocks' MLP activation: QuickGELU x * sigmoid(1.702 x) (OpenAI-pretrained CLIP) instead of erf-GELU
    ln_eps: float = 1e-5         # eps of every LayerNorm of the tower (the EVA ViT: 1e-6)
    pre_norm: bool = True        # the tower has ln_pre behind [cls; tokens] + pos (the EVA ViT has none: pos_embed, then block 0)


@dataclass
class TextCfg:
    context_length: int = 77
    vocab_size: int = 49408
    width: int = 768
    heads: int = 12
    layers: int = 12
    embed_dim: int = 768
    quick_gelu: bool = False     # as TowerCfg.quick_gelu
    ln_eps: float = 1e-5         # as TowerCfg.ln_eps (every CLIP text tower: 1e-5)


def _pad64(n):
    return (n + 63) // 64 * 64


def _dev(t, device, dtype=torch.float32):
    """Device copy owned by the engine: never an alias of the caller's tensor (a fused step updates these in place through
    raw kernels, which would otherwise modify the model's Parameters behind autograd's back)."""
    out = t.detach().to(device=device, dtype=dtype).contiguous()
    return out.clone() if out.data_ptr() == t.data_ptr() else out


def prep_block(sd: Dict[str, torch.Tensor], p: str, device, wdtype=torch.bfloat16) -> Dict[str, torch.Tensor]:
    """Device copies of one ResidualAttentionBlock: GEMM weights in `wdtype`, the rest f32; bf16 with the LayerNorm folding
    switched on: also the operands of the two LayerNorm -> Linear pairs with the LayerNorm folded in (ops.fold_ln_linear; used
    for frozen blocks on a bf16 stream)."""
    dv = lambda k: sd[p + k].detach().to(device)
    blk = block_operands(sd, p, device, wdtype)
    if LN_FOLD and wdtype == torch.bfloat16:      # (read at call time: engines built while the switch is on carry the folded operands)
        blk["in_f"] = ops.fold_ln_linear(dv("attn.in_proj_weight"), dv("attn.in_proj_bias"), dv("ln_1.weight"), dv("ln_1.bias"))
        blk["fc_f"] = ops.fold_ln_linear(dv("mlp.c_fc.weight"), dv("mlp.c_fc.bias"), dv("ln_2.weight"), dv("ln_2.bias"))
    return blk


_BLOCK_OPERANDS = {"ln1_w": "ln_1.weight", "ln1_b": "ln_1.bias", "in_w": "attn.in_proj_weight", "in_b": "attn.in_proj_bias",
                   "out_w": "attn.out_proj.weight", "out_b": "attn.out_proj.bias", "ln2_w": "ln_2.weight", "ln2_b": "ln_2.bias",
                   "fc_w": "mlp.c_fc.weight", "fc_b": "mlp.c_fc.bias", "proj_w": "mlp.c_proj.weight", "proj_b": "mlp.c_proj.bias"}


def block_operands(sd: Dict[str, torch.Tensor], p: str, device, wdtype=torch.bfloat16) -> Dict[str, torch.Tensor]:
    """Device copies of the twelve operands of one ResidualAttentionBlock: the four GEMM weights in `wdtype` (bf16; IEEE half
    for `TextEngine(arith="f16")`; f32 for the fp32 engines), LayerNorm parameters and biases f32."""
    gemm_w = ("in_w", "out_w", "fc_w", "proj_w")
    return {k: _dev(sd[p + n], device, wdtype if k in gemm_w else torch.float32) for k, n in _BLOCK_OPERANDS.items()}


def conv_weight_as_gemm(w: torch.Tensor, device, dtype=torch.bfloat16) -> torch.Tensor:
    """Conv2d weight [O,C,kh,kw] -> [O, Kp] (K = C*kh*kw zero-padded to a multiple of 64), bf16 operand or f32 master.
    Built where the weight lives (no host round trip for a parameter that is already on the GPU)."""
    O = w.shape[0]
    K = w[0].numel()
    out = torch.zeros(O, _pad64(K), dtype=torch.float32, device=w.device)
    out[:, :K] = w.detach().reshape(O, K).float()
    return out.to(device=device, dtype=dtype).contiguous()


def copy_tree(dst, src):
    """dst <- src, in place, for every tensor of two identically shaped nests of dict / list / tuple.  The engines are
    updated through this after an optimizer step: object identities (and with them the trainers' activation buffers and
    every tensor another object holds a reference to) survive, only the trainable operands are re-derived."""
    if torch.is_tensor(dst):
        dst.copy_(src)
    elif isinstance(dst, dict):
        for k in dst:
            copy_tree(dst[k], src[k])
    else:
        for d, s_ in zip(dst, src):
            copy_tree(d, s_)


class Bf16Arith:
    """The matrix products of a tower or a Perceiver on bf16 operands with fp32 accumulation.  block_forward, text_features,
    VitEngine.trunk and perceiver_forward call one of these objects and never ask which: F16Arith and Bf16x2Arith below,
    f32.F32Arith."""
    dtype = torch.bfloat16
    ln = staticmethod(ops.layernorm)           # LayerNorm into a GEMM operand (the two-term arithmetic writes it twice)

    def __init__(self, gemm_cfg=-1):
        self.cfg = gemm_cfg

    def linear(self, a, w, b, out, res=None, act=ops.ACT_NONE, out2=None):
        epi = ops.EPI_BF16 if res is None else ops.EPI_RES_F32 if res.dtype == torch.float32 else ops.EPI_RES_BF16
        ops.gemm(a, w, b, out=out, res=res, epi=epi, act=act, cfg=self.cfg, out2=out2)

    def geglu(self, a, w, b, out, out2=None):
        ops.gemm(a, w, b, out=out, epi=ops.EPI_GEGLU, cfg=self.cfg, out2=out2)

    def attn(self, q, k, v, out, lse, dh, causal=False):
        ops.attn_fwd(q, k, v, out, lse=lse, causal=causal, qscale=dh ** -0.5 * ops.LOG2E)

    # train mode with dropout (LensDrop): the attention with the mask on its probabilities, and a down-projection that leaves
    # its fp32 output apart from the residual for ops.ff_drop_fwd (also: a tower's output projection)
    def attn_drop(self, q, k, v, out, lse, dh, drop, sublayer):
        ops.attn_fwd_drop(q, k, v, out, drop.pa, drop.seed, drop.sample0, sublayer, lse=lse, qscale=dh ** -0.5 * ops.LOG2E)

    def linear_f32(self, a, w, b, out=None):
        return ops.gemm(a, w, b, out=out, epi=ops.EPI_F32, cfg=self.cfg)

    # the front of a Lens (LensEngine.cols, points.pointbert_forward): the tokenizer convolution's rows; the point patches with
    # their K padding, the group maximum and the padded centres; and the projection that adds row m // res_div of `res` in
    # front of the activation (the group's row of the split convolution)
    point_kp = 64
    im2col, knn_group, group_max, pad3 = (staticmethod(f) for f in (ops.im2col, ops.knn_group, ops.group_max, ops.pad3))

    def linear_rowres(self, a, w, out, res, res_div, act=ops.ACT_NONE):
        ops.gemm(a, w, None, out=out, res=res, res_div=res_div, epi=ops.EPI_RES_BF16, act=act, cfg=self.cfg)


class Bf16x2Arith(Bf16Arith):
    """Weights as the sum of TWO bf16 terms (prep_block_wsplit) on an fp32 stream.  A projection that writes an activation takes
    the pair K-concatenated, [N, 2K] against an operand row [a, a]: the LayerNorm in front of it writes its output into both
    halves of a [rows, 2D] buffer.  A residual projection takes the pair (hi, lo) and runs as two launches that accumulate
    into the stream: hi with the bias, then lo without."""

    def ln(self, x, w, b, out, rows, D, **kw):
        for half in (out[:, :D], out[:, D:]):
            ops.layernorm(x, w, b, half, rows, D, **kw)

    def linear(self, a, w, b, out, res=None, act=ops.ACT_NONE, out2=None):
        if res is None:
            return super().linear(a, w, b, out, act=act, out2=out2)
        super().linear(a, w[0], b, out, res=res)
        super().linear(a, w[1], None, out, res=out)


class F16Arith:
    """IEEE-half operands (the frozen text tower): vl_gemm_f16, which is the persistent kernel only - whole 256-row tiles - and
    the fp16 attention.  plan (a TextPlan): the rows are captions packed one behind the other - q is then the packed
    in-projection output [rows, 3D] itself and the attention runs caption by caption."""
    dtype = torch.float16
    ln = staticmethod(ops.layernorm)

    def __init__(self, plan=None):
        self.plan = plan

    def linear(self, a, w, b, out, res=None, act=ops.ACT_NONE, out2=None):
        ops.gemm_f16(a, w, b, out=out, res=res, epi=ops.EPI_BF16 if res is None else ops.EPI_RES_F32, act=act)

    def attn(self, q, k, v, out, lse, dh, causal=False):
        p, qscale = self.plan, dh ** -0.5 * ops.LOG2E
        if p is None:
            ops.attn_fwd(q, k, v, out, lse=lse, causal=causal, qscale=qscale)
        else:
            ops.attn_fwd_varlen(q, p.start, p.lens, out, q.shape[1] // (3 * dh), p.max_len, lse=lse, qscale=qscale)

    def linear_f32(self, a, w, b, out=None):
        """vl_gemm_f16 has no fp32-output epilogue: the product accumulates into a ZEROED fp32 buffer through EPI_RES_F32."""
        out = torch.zeros(a.shape[0], w.shape[0], device=a.device, dtype=torch.float32) if out is None else out.zero_()
        ops.gemm_f16(a, w, b, out=out, res=out, epi=ops.EPI_RES_F32)
        return out


@dataclass
class BlockSlots:
    """Where block_forward reads and writes one ResidualAttentionBlock: built once with the buffers (one for an engine's
    workspace, one per layer for a trainer's saved activations).  An optional output that is None is not written."""
    x0: torch.Tensor                  # residual stream: block input, after the attention branch, block output (an engine
    x1: torch.Tensor                  # passes one tensor three times: in place)
    x2: torch.Tensor
    h1: torch.Tensor                  # ln_1 / ln_2 output of a block that runs the LayerNorm passes ([rows, 2D]: two-term)
    h2: torch.Tensor
    h_left: torch.Tensor              # LayerNorm output of a folded GEMM's leftover rows
    qkv: torch.Tensor                 # packed in-projection output and its q / k / v views by heads (ops.heads_view)
    q: torch.Tensor                   # (a packed text batch has no such views: all three are qkv itself, _Workspace.packed)
    k: torch.Tensor
    v: torch.Tensor
    a: torch.Tensor                   # attention output
    hid: torch.Tensor                 # MLP hidden
    part: Optional[torch.Tensor]      # partial row sums between a gemm_res_rowstats and the ln_row_stats behind it
    a1: Optional[torch.Tensor]        # the class rows of a pruned last block: attention output, ln_2 output, MLP hidden
    h2c: Optional[torch.Tensor]       # (bf16 operands only)
    hid1: Optional[torch.Tensor]
    stats: Optional[tuple] = None     # (mean1, rstd1, mean2, rstd2); a folded block needs them
    lse: Optional[torch.Tensor] = None
    u: Optional[torch.Tensor] = None  # the second output of c_fc (the activation's derivative, with a *_DSAVE act)
    lse1: Optional[torch.Tensor] = None        # lse, (mean2, rstd2) and u of the class rows
    stats2c: Optional[tuple] = None
    u1: Optional[torch.Tensor] = None


class _Workspace:
    """The activations of one tower at (B, L), one in-place stream x (res_dtype) and one set of buffers in the operand `dtype`:
    LayerNorm output h (`h_width` columns: 2D for the two-term arithmetic), packed in-projection output, attention output, MLP
    hidden.  bf16 operands also get what LayerNorm folding and the pruned last block need.

    row_tile (256 for the fp16 text tower, vl_gemm_f16 being the persistent kernel only): B*L rows padded to whole row tiles,
    sized for the dense run, plus the pooled rows and the packed path's feature accumulator f.  Rows beyond the ones a call
    owns - [B*L, Mp) of a dense call, [rows, roundup(rows, 256)) of a packed one - are GEMM padding: never normalised, never read
    by the attention or the pooling, and their CONTENT is unspecified.  They start as zeros, a dense call only ever feeds zeros
    of h and a into them, but a packed call writes x, qkv and hid there from whatever h and a hold in those rows (stale rows of
    an earlier, larger call), and with roundup(rows, 256) > B*L that reaches the dense run's padding too.  Nothing depends on
    it: GEMM rows are independent of each other, and tests/test_hip_text_pack.py runs both paths on NaN-filled workspaces."""

    def __init__(self, B, L, D, H, hidden, device, res_dtype, dtype=torch.bfloat16, h_width=None, row_tile=None):
        f32 = torch.float32
        pad = (lambda n: n) if row_tile is None else (lambda n: (n + row_tile - 1) // row_tile * row_tile)
        alloc = torch.empty if row_tile is None else torch.zeros
        new = lambda *shape, dt=dtype: alloc(*shape, device=device, dtype=dt)
        self.rows, self.Mp, self.Bp = B * L, pad(B * L), pad(B)
        self.x = new(self.Mp, D, dt=res_dtype)
        self.h = new(self.Mp, h_width or D)
        self.qkv = new(self.Mp, 3 * D)                                    # packed in-projection output, read in place
        self.q, self.k, self.v = (ops.heads_view(self.qkv, B, L, H, D // H, i * D) for i in range(3))
        self.a = new(self.Mp, D)
        self.hid = new(self.Mp, hidden)
        self.pooled = new(self.Bp, D) if row_tile else None
        self.f = None                     # [Bp, E] f32, the packed path's feature accumulator (allocated at first use)
        self.mean = self.rstd = self.part = self.a1 = self.h1 = self.hid1 = None
        if dtype == torch.bfloat16:
            # LayerNorm folding: row statistics of the residual rows and the producing GEMMs' partial sums
            self.mean, self.rstd = new(B * L, dt=f32), new(B * L, dt=f32)
            self.part = new(B * L * (D // 64) * 2, dt=f32) if D % 64 == 0 else None
            # the pruned last block (PRUNE_LAST_BLOCK): attention output, LayerNorm output and MLP hidden of the class rows only
            self.a1, self.h1, self.hid1 = new(B, D), new(B, D), new(B, hidden)
        # one in-place stream, one LayerNorm buffer.  A block that runs its LayerNorm passes keeps no statistics (slots); a
        # folded one leaves both LayerNorms' in the one (mean, rstd) pair (slots_folded)
        self.slots = BlockSlots(x0=self.x, x1=self.x, x2=self.x, h1=self.h, h2=self.h, h_left=self.h, qkv=self.qkv, q=self.q,
                                k=self.k, v=self.v, a=self.a, hid=self.hid, part=self.part, a1=self.a1, h2c=self.h1, hid1=self.hid1)
        self.slots_folded = replace(self.slots, stats=(self.mean, self.rstd, self.mean, self.rstd))

    def packed(self, Mr):
        """The first Mr rows as ONE packed sequence (a TextPlan's rows in whole row tiles): row views for the GEMMs, and in place
        of the q / k / v views by heads the packed in-projection output itself (F16Arith.attn)."""
        v = copy(self)
        v.x, v.h, v.qkv, v.a, v.hid = (t[:Mr] for t in (self.x, self.h, self.qkv, self.a, self.hid))
        v.slots = replace(self.slots, x0=v.x, x1=v.x, x2=v.x, h1=v.h, h2=v.h, h_left=v.h, qkv=v.qkv, q=v.qkv, k=v.qkv, v=v.qkv,
                          a=v.a, hid=v.hid)
        return v


# LayerNorm folding is ON by default since round 5 (the whole GPU suite is green with it: profiles/r05_pytest_gpu_lnfold_on_*.log;
# it takes 88 of 96 LayerNorm passes and 270 MB of HBM traffic out of a frozen ViT-L micro-batch; +0.25 % on the C3 step - the
# chip is power-limited and gives most of the removed time back as lower GEMM clocks).  A module attribute,
# not an environment variable: `engine.LN_FOLD = False` (or `fold=False` on run_blocks, `bench.py --ln-fold off`) selects the
# separate LayerNorm passes; engines read it when they are built and when they run.
LN_FOLD = True


# A class-token-pooled tower reads ONE row per image of its last block's output (feature = proj(ln_post(x[:, 0]))): behind the
# dense in-projection (K and V need every token) the last block runs on those B rows only - single-query attention
# (ops.attn_fwd_q1), then out_proj, ln_2, c_fc and c_proj as B-row problems on the row-strided view of the class rows; the
# other rows of the block's output are NOT written and nothing reads them.  `engine.PRUNE_LAST_BLOCK = False` runs the last
# block in full (A/B runs, tests); read when a tower runs.
PRUNE_LAST_BLOCK = True
PRUNE_MAX_L = 1024          # the single-query kernels keep one row of scores in LDS


def prune_last_ok(D, H, res_dtype, L, pooled_only=True, causal=False):
    """Whether a tower of width D with H heads on a `res_dtype` residual stream runs its last block on the class rows only:
    the caller consumes nothing but the pooled class token, bf16 stream, head dim 64, no causal mask, L within the kernels'
    range.  Everything else runs the block in full."""
    return bool(PRUNE_LAST_BLOCK and pooled_only and not causal and res_dtype == torch.bfloat16 and H > 0 and D == 64 * H
                and 1 <= L <= PRUNE_MAX_L)


def cls_rows(x2d, B, L):
    """[B*L, D] token-major matrix -> the [B, D] view of its class-token rows b*L (row stride L*D, no copy)."""
    D = x2d.shape[1]
    return x2d.as_strided((B, D), (L * D, 1), x2d.storage_offset())


def _cls_tail_forward(w, s: BlockSlots, B, L, D, H, act, ar, eps=1e-5):
    """The pruned last block behind its in-projection (see PRUNE_LAST_BLOCK; bf16 stream): single-query attention, out_proj +
    residual, ln_2, c_fc + activation and c_proj + residual on the B class rows b*L of x0 / x1 / x2 (row-strided views, no
    copy); the other rows of x1 and x2 and the full-size a / hid / u are neither written nor read."""
    x0c, x1c, x2c = (cls_rows(x, B, L) for x in (s.x0, s.x1, s.x2))
    m2, r2 = s.stats2c or (None, None)
    ops.attn_fwd_q1(s.q, s.k, s.v, s.a1, lse=s.lse1, qrow=0, qscale=(D // H) ** -0.5 * ops.LOG2E)
    ar.linear(s.a1, w["out_w"], w["out_b"], x1c, res=x0c)
    ar.ln(x1c, w["ln2_w"], w["ln2_b"], s.h2c, B, D, x_row_stride=L * D, mean=m2, rstd=r2, eps=eps)
    ar.linear(s.h2c, w["fc_w"], w["fc_b"], s.hid1, act=act, out2=s.u1)
    ar.linear(s.hid1, w["proj_w"], w["proj_b"], x2c, res=x1c)


def block_forward(w, s: BlockSlots, B, L, D, H, causal, act, ar, folded, next_folded, cls_only=False, write_out=True, mm=0,
                  eps=1e-5):
    """One pre-LN ResidualAttentionBlock (transformer.py:254-272) with the operands `w` on the buffers `s` in the arithmetic
    `ar` (Bf16Arith, Bf16x2Arith, F16Arith, f32.F32Arith: ln / linear / attn):
    x1 = x0 + out_proj(attn(in_proj(ln_1(x0)))), x2 = x1 + c_proj(act(c_fc(ln_2(x1)))).  The one forward of the engines and
    the trainers: it branches on what it is given, never on who calls or which arithmetic.  B*L is the number of rows the
    LayerNorms run on (a packed text batch is one sequence: B = 1, L = its rows); the GEMMs take every row of their buffers.
    folded (Bf16Arith only): the LayerNorms are folded into the GEMMs either side of them (w carries "in_f" / "fc_f", bf16
    stream, s.stats and s.part given) - ln_1 / ln_2 are never materialised, the in-projection and c_fc read the residual rows
    and apply (mean, rstd) in their epilogues, the out-projection leaves the partial row sums of what it stores
    (ops.gemm_lnfold / gemm_res_rowstats).  Otherwise the LayerNorm passes run, and leave their statistics where s.stats is given.
    next_folded: the consumer of x2 is a folded block - c_proj leaves the partial row sums too.
    cls_only: the caller reads only the class-token rows b*L of x2 - dense up to the in-projection, then _cls_tail_forward.
    write_out=False (the recompute in front of a block's backward, which does not need x2): c_proj is skipped.
    mm: the rows of x0 whose partial sums are in s.part (what the block before returned; 0: the statistics come from the rows).
    eps: of ln_1 and ln_2 (TowerCfg / TextCfg: 1e-5; the EVA ViT's 1e-6), the folded form's row statistics included.
    Returns the rows of x2 whose partial sums it left in s.part."""
    rows = B * L
    m1, r1, m2, r2 = s.stats or (None,) * 4

    def ln_linear(x, mm, mean, rstd, ln, lin, h, out, act=ops.ACT_NONE, out2=None):
        """out = act(Linear(LayerNorm(x))) for the pair (ln, lin) of w; mm rows of x have their partial sums in s.part."""
        ln_w, ln_b, lin_w, lin_b = w[ln + "_w"], w[ln + "_b"], w[lin + "_w"], w[lin + "_b"]
        if not folded:
            ar.ln(x, ln_w, ln_b, h, rows, D, mean=mean, rstd=rstd, eps=eps)
            ar.linear(h, lin_w, lin_b, out, act=act, out2=out2)
            return
        # (the row-statistics launch also writes the LayerNorm output of the GEMM's leftover rows into s.h_left - where all of
        # them are rows whose statistics it computes from the rows themselves)
        r = ops.fold_rows(x, out, out.shape[1])
        k = dict(ln_w=ln_w, ln_b=ln_b, h_left=s.h_left, h_row0=r) if mm <= r else {}
        ops.ln_row_stats(s.part, x, mm, mean, rstd, eps=eps, **k)
        ops.gemm_lnfold(x, w[lin + "_f"], mean, rstd, out, lin_w, lin_b, ln_w, ln_b, s.h_left, act=act, out2=out2, eps=eps,
                        cfg=ar.cfg, h_ready=bool(k))

    def linear_res(a, lin, out, res, leave_sums):
        """out = res + Linear(a); returns the rows of out whose partial sums it left in s.part."""
        if leave_sums:
            return ops.gemm_res_rowstats(a, w[lin + "_w"], w[lin + "_b"], out, res, s.part, cfg=ar.cfg)
        ar.linear(a, w[lin + "_w"], w[lin + "_b"], out, res=res)
        return 0

    ln_linear(s.x0, mm, m1, r1, "ln1", "in", s.h1, s.qkv)
    if cls_only:
        _cls_tail_forward(w, s, B, L, D, H, act, ar, eps)
        return 0
    ar.attn(s.q, s.k, s.v, s.a, s.lse, D // H, causal)
    mm = linear_res(s.a, "out", s.x1, s.x0, folded)
    # s.u = act'(fc output) under a *_DSAVE act: all the backward needs of the pre-activation, evaluated next to the activation
    # from the same exp / rational pieces (+3 VALU per element here) - the dX GEMM's epilogue is then one multiplication,
    # whichever activation (erf or QuickGELU) left the derivative
    ln_linear(s.x1, mm, m2, r2, "ln2", "fc", s.h2, s.hid, act, s.u)
    if not write_out:
        return 0
    return linear_res(s.hid, "proj", s.x2, s.x1, next_folded)


def run_blocks(blocks, ws: _Workspace, B, L, D, H, ar, causal=False, fold=None, quick_gelu=False, pooled_only=False, eps=1e-5):
    """x (ws.x, residual stream) <- N pre-LN transformer blocks (transformer.py:364-371), each one block_forward in place in
    the arithmetic `ar`.
    quick_gelu: the tower's MLP activation (TowerCfg / TextCfg.quick_gelu; `act_layer`, transformer.py:217-231).
    fold (default: engine.LN_FOLD; bf16 stream and operands only): the LayerNorms folded into the GEMMs either side of them.
    pooled_only: the caller reads only the class-token rows b*L of the result (VitEngine.trunk) - the last block then runs on
    those rows alone where prune_last_ok() allows, and the other rows of ws.x are left as the block before it wrote them.
    eps: the blocks' LayerNorm eps (TowerCfg.ln_eps)."""
    prune = prune_last_ok(D, H, ws.x.dtype, L, pooled_only, causal)
    act = ops.mlp_act(quick_gelu)
    if fold is None:
        fold = LN_FOLD
    can_fold = bool(fold) and ws.x.dtype == torch.bfloat16 and ws.part is not None
    # decided PER BLOCK: a block folds when it carries the folded operands (prep_block) - a fused training step removes them
    # from the blocks it trains (their LayerNorm parameters move every step) and those run the LayerNorm passes
    folded = [can_fold and "in_f" in w for w in blocks] + [False]
    mm = 0                                            # rows of ws.x whose partial sums are in ws.part
    for i, w in enumerate(blocks):
        mm = block_forward(w, ws.slots_folded if folded[i] else ws.slots, B, L, D, H, causal, act, ar, folded[i], folded[i + 1],
                           cls_only=prune and i + 1 == len(blocks), mm=mm, eps=eps)


def _hi_lo(w: torch.Tensor, device):
    """fp32 weight -> (hi, lo) bf16 with hi + lo = w to ~2^-17 relative (hi = bf16(w), lo = bf16(w - hi))."""
    w = w.detach().float().to(device)
    hi = w.bfloat16()
    lo = (w - hi.float()).bfloat16()
    return hi.contiguous(), lo.contiguous()


def prep_block_wsplit(sd: Dict[str, torch.Tensor], p: str, device) -> Dict[str, torch.Tensor]:
    """One ResidualAttentionBlock with TWO-TERM bf16 weights (`TextEngine(arith="bf16x2")`), as Bf16x2Arith takes them: in_w and
    fc_w K-concatenated [N, 2K], out_w and proj_w the pair (hi, lo)."""
    blk = block_operands(sd, p, device)
    for key in ("in_w", "fc_w"):
        blk[key] = torch.cat(_hi_lo(sd[p + _BLOCK_OPERANDS[key]], device), dim=1).contiguous()
    for key in ("out_w", "proj_w"):
        blk[key] = _hi_lo(sd[p + _BLOCK_OPERANDS[key]], device)
    return blk


class VitEngine:
    """One ViT tower (`image.` or `visual.` prefix of the TriCLIP state_dict) on the GPU, in the arithmetic `arith` (default:
    Bf16Arith(gemm_cfg); f32.VitEngineF32 passes F32Arith): the operands are built in its dtype."""

    def __init__(self, sd, prefix: str, cfg: TowerCfg, device, res_dtype=torch.float32, gemm_cfg: int = -1,
                 n_tokens: Optional[int] = None, arith=None):
        self.cfg, self.device, self.res_dtype, self.gemm_cfg = cfg, torch.device(device), res_dtype, gemm_cfg
        self.prefix = prefix
        self.math = Bf16Arith(gemm_cfg) if arith is None else arith
        wd = self.math.dtype
        D = cfg.width
        self.cls = _dev(sd[prefix + "class_embedding"], device)
        self.pos = _dev(sd[prefix + "positional_embedding"], device)
        self.T = self.pos.shape[0] - 1
        self.ln_pre = (_dev(sd[prefix + "ln_pre.weight"], device), _dev(sd[prefix + "ln_pre.bias"], device)) if cfg.pre_norm else None
        self.ln_post = (_dev(sd[prefix + "ln_post.weight"], device), _dev(sd[prefix + "ln_post.bias"], device))
        # [E, D]; None = the tower has no output projection (`if self.proj is not None`, transformer.py:783-784;
        # CLIPBindWrap drops it when the feature width differs, VitLens-OpenShape/src/models/clip_bind.py:35-47)
        self.projT = _dev(sd[prefix + "proj"].t(), device, wd) if prefix + "proj" in sd else None
        # the bias of an output projection that is an nn.Linear (the EVA ViT's `head`, eva_tower_state); CLIP's `proj` has none
        self.proj_b = _dev(sd[prefix + "proj_bias"], device) if prefix + "proj_bias" in sd else None
        self.blocks = [prep_block(sd, f"{prefix}transformer.resblocks.{i}.", device, wd) for i in range(cfg.layers)]
        self.conv_w = None
        if prefix + "conv1.weight" in sd:
            self.conv_w = conv_weight_as_gemm(sd[prefix + "conv1.weight"], device, wd)
        self._ws = {}

    def update_params(self, sd, names):
        """Re-derive, in place, the device operands of the parameters `names` (relative to this tower's prefix) from `sd`."""
        p, dev = self.prefix, self.device
        top = {n for n in names if not n.startswith("transformer.resblocks.")}
        if "class_embedding" in top:
            self.cls.copy_(sd[p + "class_embedding"])
        if "positional_embedding" in top:
            self.pos.copy_(sd[p + "positional_embedding"])
        for nm, pair in (("ln_pre", self.ln_pre), ("ln_post", self.ln_post)):
            if pair is not None and (nm + ".weight" in top or nm + ".bias" in top):
                pair[0].copy_(sd[p + nm + ".weight"]); pair[1].copy_(sd[p + nm + ".bias"])
        if "proj" in top and self.projT is not None:
            self.projT.copy_(sd[p + "proj"].t())
        if "proj_bias" in top and self.proj_b is not None:
            self.proj_b.copy_(sd[p + "proj_bias"])
        if "conv1.weight" in top and self.conv_w is not None:
            self.conv_w.copy_(conv_weight_as_gemm(sd[p + "conv1.weight"], dev, self.math.dtype))
        for l in sorted({int(n.split(".")[2]) for n in names if n.startswith("transformer.resblocks.")}):
            copy_tree(self.blocks[l], prep_block(sd, f"{p}transformer.resblocks.{l}.", dev, self.math.dtype))

    def workspace(self, B, L):
        key = (B, L)
        if key not in self._ws:
            self._ws[key] = _Workspace(B, L, self.cfg.width, self.cfg.heads, int(self.cfg.width * self.cfg.mlp_ratio),
                                       self.device, self.res_dtype, self.math.dtype)
        return self._ws[key]

    # -- stages ---------------------------------------------------------------------------------
    def patch_tokens(self, image: torch.Tensor) -> torch.Tensor:
        """conv1 as im2col + GEMM (transformer.py:464-470,674-676): [N,C,H,W] f32 -> [N*T, D] bf16."""
        p = self.cfg.patch
        return self.conv_tokens(ops.im2col(image.contiguous().float(), p, p, p, p, self.conv_w.shape[1])[0])

    def conv_tokens(self, cols: torch.Tensor) -> torch.Tensor:
        """conv1 on its im2col rows (a trainer keeps them for the weight gradient)."""
        return ops.gemm(cols, self.conv_w, None, epi=ops.EPI_BF16, cfg=self.gemm_cfg)

    def trunk(self, tokens: torch.Tensor, B: int, pos2: Optional[torch.Tensor] = None, use_orig_pos=True,
              keep: Optional[torch.Tensor] = None, tokens_out: bool = False):
        """tokens [B*T, D] (bf16|f32; f32 for the fp32 arithmetic) -> un-normalised features f32 [B, E]: [cls; tokens] + pos
        (+ pos2) -> ln_pre -> blocks -> ln_post(cls) @ proj (transformer.py:756-787).
        keep int32 [B,K] (ops.patch_keep): patch dropout of a tower in train mode (PatchDropout, transformer.py:53-90) - the
        trunk runs on the class token + the kept tokens, L = K + 1.  bf16 operands only: the fp32 engines are eval-only.
        A tower without ln_pre (cfg.pre_norm False: the EVA ViT) enters block 0 with [cls; tokens] + pos (+ pos2) itself.
        tokens_out: return the [B, L, D] stream behind the last block and in front of ln_post instead (a copy, in the residual
        dtype) - what the EVA ViT's forward_features returns and an MLLM's ln_vision reads; the last block then runs on all rows."""
        cfg, ar = self.cfg, self.math
        if keep is not None and ar.dtype != torch.bfloat16:
            raise NotImplementedError("trunk: patch dropout (keep=) is a train-mode forward; the fp32 engines are eval-only")
        D, T = cfg.width, tokens.shape[0] // B
        L = T + 1 if keep is None else keep.shape[1] + 1
        ws = self.workspace(B, L)
        pos = self.pos if use_orig_pos else torch.zeros_like(self.pos)
        if not cfg.pre_norm:
            if keep is not None:
                raise NotImplementedError("trunk: patch dropout on a tower without ln_pre (vl_assemble_tokens is the dense form only)")
            ops.assemble_tokens(tokens, self.cls, pos, pos2, ws.x[:B * L], B, T, D)
        elif keep is None:
            ops.assemble_ln_pre(tokens, self.cls, pos, pos2, self.ln_pre[0], self.ln_pre[1], ws.x, B, T, D, eps=cfg.ln_eps)
        else:
            ops.assemble_ln_pre_keep(tokens, keep, self.cls, pos, pos2, self.ln_pre[0], self.ln_pre[1], ws.x, B, T, D, eps=cfg.ln_eps)
        # (only the class-token rows are read below: the last block may run on them alone)
        run_blocks(self.blocks, ws, B, L, D, cfg.heads, ar, quick_gelu=cfg.quick_gelu, pooled_only=not tokens_out, eps=cfg.ln_eps)
        if tokens_out:
            return ws.x[:B * L].view(B, L, D).clone()
        # (a tower without output projection: ln_post of the class rows IS the feature, fp32)
        pooled = torch.empty(B, D, device=self.device, dtype=torch.float32 if self.projT is None else ar.dtype)
        ar.ln(ws.x, self.ln_post[0], self.ln_post[1], pooled, B, D, x_row_stride=L * D, eps=cfg.ln_eps)
        return pooled if self.projT is None else ar.linear_f32(pooled, self.projT, self.proj_b)

    def encode_image(self, image: torch.Tensor, normalize: bool = False, keep: Optional[torch.Tensor] = None) -> torch.Tensor:
        B = image.shape[0]
        f = self.trunk(self.patch_tokens(image), B, keep=keep)
        return ops.l2_normalize(f) if normalize else f


# ------------------------------------------------------------------------------------------------
# The BLIP-2 / InstructBLIP EVA ViT-g as a tower (visual_arch "perceiver_blip_eva_g_vit"): width 1408 = 16 heads x 88, MLP hidden
# int(1408 * 4.3637) = 6144, 40 blocks, LayerNorm eps 1e-6, no ln_pre, a qkv bias on q and v only.  Its blocks are pre-LN
# residual blocks with an erf-GELU MLP, so they run on block_forward as they are: only the NAMES differ.
# ------------------------------------------------------------------------------------------------
_EVA_BLOCK = {"norm1.weight": "ln_1.weight", "norm1.bias": "ln_1.bias", "attn.qkv.weight": "attn.in_proj_weight",
              "attn.proj.weight": "attn.out_proj.weight", "attn.proj.bias": "attn.out_proj.bias",
              "norm2.weight": "ln_2.weight", "norm2.bias": "ln_2.bias", "mlp.fc1.weight": "mlp.c_fc.weight",
              "mlp.fc1.bias": "mlp.c_fc.bias", "mlp.fc2.weight": "mlp.c_proj.weight", "mlp.fc2.bias": "mlp.c_proj.bias"}


def eva_tower_cfg(width=1408, layers=40, heads=16, embed_dim=768, mlp_ratio=4.3637, **kw) -> TowerCfg:
    """TowerCfg of an EVA ViT: eps 1e-6, no ln_pre (defaults: ViT-g as BLIP-2 ships it, 40 blocks)."""
    return TowerCfg(width=width, layers=layers, heads=heads, mlp_ratio=mlp_ratio, embed_dim=embed_dim, ln_eps=1e-6, pre_norm=False, **kw)


def eva_tower_state(sd: Dict[str, torch.Tensor], prefix: str) -> Dict[str, torch.Tensor]:
    """The operands VitEngine and prep_block take, under VitEngine's names and the same `prefix`, out of a
    Perceiver_Blip_EVA_ViT state_dict (`prefix`eva_vit.* and `prefix`eva_vit_proj):
    cls_token [1,1,D] -> class_embedding [D]; pos_embed [1,L,D] -> positional_embedding [L,D] (absent under disable_orig_pos:
    zeros would be wrong silently, so the caller passes use_orig_pos=False and the table is sized from cls_token - see below);
    blocks.N.{norm1,norm2} -> ln_1 / ln_2; attn.qkv.weight -> in_proj_weight; cat(q_bias, 0, v_bias) -> in_proj_bias (zeros
    where the block has no qkv bias); attn.proj -> out_proj; mlp.fc1 / fc2 -> c_fc / c_proj; norm -> ln_post; the output
    projection: eva_vit_proj [D,E] -> proj, or eva_vit.head (nn.Linear(D, E), `--use_eva_pt_lin`) -> proj = weight^T and
    proj_bias.  Views where a view does (no copy of a 1408 x 6144 weight); everything else of `sd` under `prefix` (the Lens:
    visual_adapter.*, perceiver.*) is passed through."""
    e = prefix + "eva_vit."
    if e + "cls_token" not in sd:
        raise KeyError(f"eva_tower_state: no {e}cls_token in the state_dict (is the prefix right?)")
    out = {k: v for k, v in sd.items() if k.startswith(prefix) and not k.startswith((e, prefix + "eva_vit_proj"))}
    D = sd[e + "cls_token"].shape[-1]
    out[prefix + "class_embedding"] = sd[e + "cls_token"].reshape(D)
    if e + "pos_embed" in sd:
        out[prefix + "positional_embedding"] = sd[e + "pos_embed"].reshape(-1, D)
    out[prefix + "ln_post.weight"], out[prefix + "ln_post.bias"] = sd[e + "norm.weight"], sd[e + "norm.bias"]
    if prefix + "eva_vit_proj" in sd:                      # a Parameter [D, E], no bias
        out[prefix + "proj"] = sd[prefix + "eva_vit_proj"]
    elif e + "head.weight" in sd:                          # nn.Linear(D, E): y = x W^T + b
        out[prefix + "proj"] = sd[e + "head.weight"].t()
        out[prefix + "proj_bias"] = sd[e + "head.bias"]
    n = 0
    while f"{e}blocks.{n}.norm1.weight" in sd:
        src, dst = f"{e}blocks.{n}.", f"{prefix}transformer.resblocks.{n}."
        for a, b in _EVA_BLOCK.items():
            out[dst + b] = sd[src + a]
        w = sd[src + "attn.qkv.weight"]
        if src + "attn.q_bias" in sd:
            q, v = sd[src + "attn.q_bias"], sd[src + "attn.v_bias"]
            out[dst + "attn.in_proj_bias"] = torch.cat([q.detach(), torch.zeros_like(v), v.detach()])
        else:
            out[dst + "attn.in_proj_bias"] = torch.zeros(w.shape[0], dtype=w.dtype, device=w.device)
        n += 1
    return out


def eva_param_names(names) -> list:
    """Parameter names of a Perceiver_Blip_EVA_ViT (relative to its prefix) -> the names VitEngine.update_params and the
    trainers use (eva_tower_state's); Lens names pass through."""
    top = {"eva_vit.cls_token": "class_embedding", "eva_vit.pos_embed": "positional_embedding", "eva_vit.norm.weight": "ln_post.weight",
           "eva_vit.norm.bias": "ln_post.bias", "eva_vit_proj": "proj", "eva_vit.head.weight": "proj", "eva_vit.head.bias": "proj_bias",
           "eva_vit_proj.weight": "proj", "eva_vit_proj.bias": "proj_bias"}
    out = []
    for n in names:
        if n in top:
            out.append(top[n])
        elif n.startswith("eva_vit.blocks."):
            _, _, l, rest = n.split(".", 3)
            out.append(f"transformer.resblocks.{l}." + ("attn.in_proj_bias" if rest in ("attn.q_bias", "attn.v_bias") else _EVA_BLOCK[rest]))
        else:
            out.append(n)
    return sorted(set(out))


def eva_grads(grads: Dict[str, torch.Tensor], prefix: str) -> Dict[str, torch.Tensor]:
    """A trainer's gradients under VitEngine's names -> under the module's (the inverse of eva_tower_state on the names):
    the packed in_proj_bias gradient splits into q_bias and v_bias (the k third belongs to no parameter)."""
    inv = {v: k for k, v in _EVA_BLOCK.items()}
    top = {"class_embedding": "eva_vit.cls_token", "positional_embedding": "eva_vit.pos_embed", "ln_post.weight": "eva_vit.norm.weight",
           "ln_post.bias": "eva_vit.norm.bias", "proj": "eva_vit_proj"}
    out = {}
    for k, g in grads.items():
        n = k[len(prefix):]
        if not k.startswith(prefix):
            out[k] = g
        elif n in top:
            out[prefix + top[n]] = g.view(1, 1, -1) if n == "class_embedding" else g.unsqueeze(0) if n == "positional_embedding" else g
        elif n.startswith("transformer.resblocks."):
            _, _, l, rest = n.split(".", 3)
            b = f"{prefix}eva_vit.blocks.{l}."
            if rest == "attn.in_proj_bias":
                Dm = g.numel() // 3
                out[b + "attn.q_bias"], out[b + "attn.v_bias"] = g[:Dm], g[2 * Dm:]
            else:
                out[b + inv[rest]] = g
        else:
            out[k] = g
    return out


class EvaVitEngine(VitEngine):
    """VitEngine over the EVA ViT of a Perceiver_Blip_EVA_ViT state_dict: the same trunk on the same run_blocks, operands and
    updates through eva_tower_state.  cfg: eva_tower_cfg(...) - pre_norm False, ln_eps 1e-6."""

    def __init__(self, sd, prefix: str, cfg: TowerCfg, device, **kw):
        if cfg.pre_norm:
            raise ValueError("EvaVitEngine: the EVA ViT has no ln_pre - build the TowerCfg with pre_norm=False (eva_tower_cfg)")
        m = eva_tower_state(sd, prefix)
        if prefix + "positional_embedding" not in m:       # disable_orig_pos deleted the table: the trunk is then run without it
            m[prefix + "positional_embedding"] = torch.zeros(kw.get("n_tokens") or 257, cfg.width)
        super().__init__(m, prefix, cfg, device, **kw)

    def update_params(self, sd, names):
        super().update_params(eva_tower_state(sd, self.prefix), eva_param_names(names))


# The text feature is ln_final(x[b, argmax(text[b])]) @ text_projection (model.py:528-540) out of a CAUSAL tower: row t depends on
# rows <= t only, so the rows behind a caption's pooled position are work nothing reads.  With the switch on, the fp16
# TextEngine runs only the rows 0 .. argmax(text[b]) of every caption, packed one behind the other (captions are a fraction of
# the 77-token context: 14 of 77 rows on the benchmark's captions).  LayerNorm and the GEMMs are row-wise and see fewer rows,
# the attention runs caption by caption (ops.attn_fwd_varlen).  `engine.PACK_TEXT = False` runs every caption at the full
# context length (A/B runs, and what a captured graph gets: the packed form sizes its launches from the data); read per call.
PACK_TEXT = True


def text_pack_mode(arith: str, text: torch.Tensor, device) -> str:
    """How a text batch runs: "dense" (every row; PACK_TEXT off, an arithmetic other than "f16", no GPU, or the current stream
    is being captured into a graph - the packed form needs the row count on the host, and a capture must not read the device),
    "host" (packed; `text` lives on the CPU: the lengths are taken there, nothing is read back) or "device" (packed; `text`
    is on the GPU: the plan kernel runs and two integers come back)."""
    if not PACK_TEXT or arith != "f16" or torch.device(device).type != "cuda":
        return "dense"
    if torch.cuda.is_current_stream_capturing():
        return "dense"
    return "device" if text.is_cuda else "host"


def text_pack_plan_host(text: torch.Tensor):
    """The packing plan in torch, on whatever device `text` lives: (len, start, last_row, (rows, max_len)) with
    len[b] = argmax(text[b]) + 1 (first maximum), start = exclusive sum over the batch (B + 1 entries), last_row = start + len - 1.
    The engine uses it for CPU token tensors; it is also the statement of what vl_text_pack_plan computes."""
    lens = text.argmax(dim=-1).to(torch.int64) + 1
    start = torch.zeros(text.shape[0] + 1, dtype=torch.int64, device=text.device)
    start[1:] = torch.cumsum(lens, 0)
    last_row = start[:-1] + lens - 1
    return lens.to(torch.int32), start.to(torch.int32), last_row, (int(start[-1]), int(lens.max()))


@dataclass
class TextPlan:
    """Which rows a batch of captions needs (TextEngine.plan_text): host integers to size the launches, device arrays for the
    kernels."""
    B: int
    L: int
    rows: int                 # packed rows = sum of the lengths
    max_len: int
    lens: torch.Tensor        # int32 [B]
    start: torch.Tensor       # int32 [B+1]
    last_row: torch.Tensor    # int64 [B]: the pooled row of every caption


def text_features(e, ar, ws: _Workspace, text: torch.Tensor, plan: Optional[TextPlan] = None) -> torch.Tensor:
    """TriCLIP.encode_text behind the token tensor (model.py:528-540) for the engine `e` (tok, pos, blocks, ln_final, projT) in
    the arithmetic `ar` on the workspace `ws`: embed, blocks, ln_final at every caption's pooled row, projection -> the
    un-normalised features f32 [B, E].  The one text head of TextEngine and f32.TextEngineF32, in two row layouts:
    dense (plan None)  every caption at the full context, row b*L + t; the pooled row is b*L + argmax(text[b]);
    packed (a TextPlan; F16Arith(plan)) only the rows up to each caption's pooled one, one caption behind the other in whole
                       256-row tiles; the pooled rows are plan.last_row and the result is a view of ws.f."""
    cfg, (B, L), D = e.cfg, text.shape, e.cfg.width
    if plan is None:
        ops.text_embed(text, e.tok, e.pos, ws.x)
        index, mul = text.argmax(dim=-1).contiguous(), L                   # index-exact EOT position (model.py:539)
        layout, out = (ws, B, L), None
    else:
        if ws.f is None:
            ws.f = torch.empty(ws.Bp, e.projT.shape[0], device=e.device, dtype=torch.float32)
        Mr = (plan.rows + 255) // 256 * 256                                # whole row tiles of the persistent GEMM
        # (rows [rows, Mr) of x are zeroed here; of h and a they hold whatever an earlier call left: GEMM rows are independent)
        ops.text_embed_packed(text, plan.start, plan.lens, e.tok, e.pos, ws.x, plan.rows, Mr)
        index, mul = plan.last_row, 0                                      # src = r * 0 + last_row[r]
        layout, out = (ws.packed(Mr), 1, plan.rows), ws.f                  # (one sequence of plan.rows rows)
    run_blocks(e.blocks, *layout, D, cfg.heads, ar, causal=True, fold=False, quick_gelu=cfg.quick_gelu, eps=cfg.ln_eps)
    # the pooled rows: two-term [B, 2D]; fp16 in the workspace, padded to whole row tiles of zeros
    pooled = ws.pooled if ws.pooled is not None else torch.empty(B, ws.h.shape[1], device=e.device, dtype=ar.dtype)
    ar.ln(ws.x, e.ln_final[0], e.ln_final[1], pooled, B, D, x_row_stride=D, row_index=index, row_mul=mul, eps=cfg.ln_eps)
    return ar.linear_f32(pooled, e.projT, None, out)[:B]


class TextEngine:
    """TriCLIP.encode_text (model.py:528-540): embedding + causal transformer + ln_final + EOT + proj.

    The tower is frozen in every recipe (forward only) and its cosine-similarity MATRIX amplifies operand rounding: random-init
    (and trained) text features share a mutual cosine of ~0.6, so with bf16 operands - the reference's amp_bf16 arithmetic -
    that matrix is 0.8-1.9e-3 from the fp32 CPU path (the reference's own amp_bf16 forward: 1.4e-3), above the 1e-3 of
    BASELINE.json's north_star.  CPU emulation per rounding point: weights 4.6e-4, GEMM input
    activations 5.0e-4, 16-bit stores 5.7e-4, attention internals 2.2e-4 taken alone.  `arith` selects the operands:
      "f16"    (default, round 5) every GEMM / attention operand IEEE half, fp32 residual stream, fp32 accumulation: three
               more mantissa bits on ALL four sources at the bf16 MFMA rate - 1.3-2.0e-4 emulated on four seeds.  (The
               reference converts CLIP to fp16 itself: convert_weights_to_fp16, model.py:393-419.)  Needs head dim 64 and a
               width that is a multiple of 256 and >= 512 (every CLIP text tower); otherwise falls back to "bf16x2".
               This is the arithmetic that runs only the rows up to each caption's pooled position (engine.PACK_TEXT,
               `plan_text`); "bf16x2" and "bf16" run every caption at the full context length
      "bf16x2" (round 4) weights as the sum of TWO bf16 terms, fp32 residual stream: 6.1-8.1e-4 measured at twice the GEMM
               flops and twice the LayerNorm passes (+17 ms per C3 step)
      "bf16"   the reference's amp_bf16 arithmetic."""

    def __init__(self, sd, cfg: TextCfg, device, res_dtype=torch.float32, gemm_cfg: int = -1, wsplit: Optional[bool] = None,
                 arith: str = "f16"):
        self.cfg, self.device, self.gemm_cfg = cfg, torch.device(device), gemm_cfg
        if wsplit is not None:            # round-4 spelling
            arith = "bf16x2" if wsplit else "bf16"
        if arith not in ("f16", "bf16x2", "bf16"):
            raise ValueError(f"TextEngine: arith must be 'f16', 'bf16x2' or 'bf16', got {arith!r}")
        # (vl_gemm_f16 is the persistent kernel only: whole 256-wide tiles and K >= 512 - the in-projection's K is the width)
        if arith == "f16" and (cfg.width % 256 or cfg.width < 512 or cfg.width // cfg.heads != 64 or cfg.embed_dim % 256
                               or cfg.context_length > 288):
            arith = "bf16x2"
        self.arith = arith
        self.wsplit = arith == "bf16x2"
        self.res_dtype = res_dtype if arith == "bf16" else torch.float32
        self.tok = _dev(sd["token_embedding.weight"], device)
        self.pos = _dev(sd["positional_embedding"], device)
        self.ln_final = (_dev(sd["ln_final.weight"], device), _dev(sd["ln_final.bias"], device))
        # the arithmetic object (self.arith stays the name: text_pack_mode and the callers read it)
        self.math = F16Arith() if arith == "f16" else Bf16x2Arith(gemm_cfg) if self.wsplit else Bf16Arith(gemm_cfg)
        blocks = lambda prep, *a: [prep(sd, f"transformer.resblocks.{i}.", device, *a) for i in range(cfg.layers)]
        if self.wsplit:
            self.projT = torch.cat(_hi_lo(sd["text_projection"].t(), device), dim=1).contiguous()         # [E, 2D]
            self.blocks = blocks(prep_block_wsplit)
        else:
            self.projT = _dev(sd["text_projection"].t(), device, self.math.dtype)                         # [E, D]
            self.blocks = blocks(block_operands, self.math.dtype)
        self._ws = {}

    def workspace(self, B, L) -> _Workspace:
        """Sized for the dense run: no allocation depends on the data."""
        if (B, L) not in self._ws:
            D, f16 = self.cfg.width, self.arith == "f16"
            self._ws[B, L] = _Workspace(B, L, D, self.cfg.heads, 4 * D, self.device, self.res_dtype, self.math.dtype,
                                        h_width=2 * D if self.wsplit else D, row_tile=256 if f16 else None)
        return self._ws[B, L]

    def plan_text(self, text: torch.Tensor) -> Optional[TextPlan]:
        """The packing plan of a token batch, or None where the batch runs dense (text_pack_mode).  For a token tensor on the
        GPU this is the one place the host waits for the device: the plan kernel and a copy of two integers run on a stream of
        the engine's own behind an event recorded on the current stream HERE, and the host waits for that stream alone -
        request the plan before queueing other work (the fused steps do so first thing) and the wait is only for what was
        already queued.  Pass the result to encode_text(text, plan=...); the token tensor must not change in between.
        Stream order: the plan's device arrays are complete on the stream that is current HERE (a CPU token tensor's are
        copied on it; a GPU one's are waited for by the host).  encode_text on ANOTHER stream must be ordered behind this
        call by the caller - an event, or a join as the fused steps' `_side_by_side` does; encode_text only keeps the arrays'
        memory alive for its stream (record_stream), it does not order the two."""
        mode = text_pack_mode(self.arith, text, self.device)
        if mode == "dense":
            return None
        B, L = text.shape
        if mode == "host":
            lens, start, last_row, (rows, max_len) = text_pack_plan_host(text.detach().long())
            dv = lambda t: t.to(self.device)
            return TextPlan(B, L, rows, max_len, dv(lens), dv(start), dv(last_row))
        return self._plan_on_device(text, B, L)

    def _plan_on_device(self, text, B, L) -> TextPlan:
        dev = self.device
        text = text.detach().to(dev, torch.int64).contiguous()
        with torch.cuda.device(dev):
            if getattr(self, "_plan_stream", None) is None:
                self._plan_stream = torch.cuda.Stream(device=dev)
                self._plan_pin = torch.empty(2, dtype=torch.int32).pin_memory()
            cur = torch.cuda.current_stream(dev)
            i32 = lambda n: torch.empty(n, device=dev, dtype=torch.int32)
            lens, start, total = i32(B), i32(B + 1), i32(2)
            last_row = torch.empty(B, device=dev, dtype=torch.int64)
            asked = torch.cuda.Event()
            asked.record(cur)                              # `text` and the four buffers exist on the current stream
            side = self._plan_stream
            side.wait_event(asked)
            with torch.cuda.stream(side):
                ops.text_pack_plan(text, lens, start, last_row, total)
                self._plan_pin.copy_(total, non_blocking=True)
            side.synchronize()                             # the host waits for this stream alone
            rows, max_len = int(self._plan_pin[0]), int(self._plan_pin[1])
        return TextPlan(B, L, rows, max_len, lens, start, last_row)

    def encode_text(self, text: torch.Tensor, normalize: bool = False, plan=None) -> torch.Tensor:
        """plan: what plan_text(text) returned for THIS token tensor; None: made here where the batch runs packed; False: run
        every caption at the full context length (no plan is made, the host never waits)."""
        B, L = text.shape
        if plan is False:
            plan = None
        elif self.arith == "f16" and plan is None:
            plan = self.plan_text(text)                    # (before the copy below: a CPU tensor gives its lengths on the host)
        text = text.to(self.device).contiguous()
        if plan is not None and text_pack_mode(self.arith, text, self.device) == "dense":
            plan = None                                    # (not under a capture even with a plan in hand)
        if plan is not None:
            if (plan.B, plan.L) != (B, L) or not (B <= plan.rows <= B * L) or not (1 <= plan.max_len <= L):
                raise ValueError(f"encode_text: the plan was made for another batch ({plan.B} x {plan.L}, {plan.rows} rows, "
                                 f"longest {plan.max_len}; text {B} x {L})")
            cur = torch.cuda.current_stream(self.device)
            for t in (plan.lens, plan.start, plan.last_row):                 # (made on the stream the plan was requested on)
                t.record_stream(cur)
            text = text.long()
        f = text_features(self, self.math if plan is None else F16Arith(plan), self.workspace(B, L), text, plan)
        # (the packed path's result lives in the workspace: hand out a copy)
        return ops.l2_normalize(f) if normalize else f.clone() if plan is not None else f


# ------------------------------------------------------------------------------------------------
# The "Lens": modality tokenizer + Perceiver resampler in front of the frozen ViT
# ------------------------------------------------------------------------------------------------
@dataclass
class LensCfg:
    """Mirror of the exp_args fields VisionTransformer.forward reads (module_cfg.py:37-92)."""
    modality: str = "depth"            # depth | audio | pc | image
    perceiver_identity: bool = True    # perceiver.py:370-371
    depth: int = 2
    self_per_cross: int = 3
    num_latents: int = 256
    latent_dim: int = 1024
    input_chan: int = 1024
    cross_heads: int = 1
    cross_dim_head: int = 64
    latent_heads: int = 16
    latent_dim_head: int = 64
    audio_fstride: int = 10
    audio_tstride: int = 10
    audio_mel_bins: int = 128
    audio_target_length: int = 512
    pc_num_group: int = 512
    pc_group_size: int = 32
    pc_encoder_dims: int = 256
    pc_trans_dim: int = 384
    pc_tokenizer: str = "pointbert"        # "pointbert" (FPS + kNN mini-PointNet) | "pnsa" (FPS + ball query set abstraction)
    pc_radius: float = 0.2                 # ball-query radius of the pnsa tokenizer
    pc_in_dim: int = 3                     # point feature channels of the pnsa tokenizer (its convs see 3 + pc_in_dim)
    use_orig_pos: bool = True
    disable_adapter_pos: bool = False
    eeg_chans: int = 128               # modal_eeg/models/EEG_tokenizer.py (PatchEmbed1D)
    eeg_time_len: int = 512
    eeg_window_size: int = 1
    eeg_stride: int = 1
    weight_tie_layers: bool = False    # perceiver.py:249-254: layers >= 1 share one set of modules
    attn_dropout: float = 0.0          # --perceiver_attn_dropout: on the probabilities of every cross / latent attention
    ff_dropout: float = 0.0            # --perceiver_ff_dropout: behind the second Linear of every FeedForward (train mode only)


@dataclass(frozen=True)
class LensDrop:
    """One train-mode forward's dropout draw in the Perceiver - numbers, never masks: the Philox seed, the per-sample number of
    batch row 0 (step.drop_sample0 with DROP_TOWER_LENS) and the two probabilities.  The forward, the backward and any
    recompute that are handed the same LensDrop draw the same bits (csrc/vl_lens_drop.hip has the counter layout)."""
    seed: int
    sample0: int
    pa: float = 0.0
    pf: float = 0.0


def lens_sublayer(c: "LensCfg", li: int, sj: int = -1, ff: bool = False) -> int:
    """The position of a sub-layer in the Perceiver's forward, the `sublayer` word of its dropout draw: layer li's cross
    attention (sj = -1) or its sj-th latent self-attention, or the FeedForward behind it.  Weight-tied layers share modules,
    not positions: every call draws a mask of its own, as nn.Dropout does."""
    return li * (2 + 2 * c.self_per_cross) + 2 * (sj + 1) + (1 if ff else 0)


def interleave_geglu(w: torch.Tensor, b: torch.Tensor):
    """Linear(D, 8D) rows [a(0..4D) ; gate(4D..8D)] -> interleaved (a_j, gate_j) so the GEGLU epilogue
    finds both halves of a pair in one lane (perceiver.py:85-89 `x, gates = x.chunk(2, dim=-1)`)."""
    half = w.shape[0] // 2
    wi = torch.stack([w[:half], w[half:]], dim=1).reshape(w.shape[0], w.shape[1])
    bi = torch.stack([b[:half], b[half:]], dim=1).reshape(-1)
    return wi, bi


def deinterleave_geglu(g: torch.Tensor, *more):
    """Inverse of interleave_geglu for a weight, a bias or a gradient in the kernels' interleaved (a_j, gate_j) row order ->
    the reference's [a ; gate] order; several tensors -> a tuple."""
    out = tuple(torch.cat([t[0::2], t[1::2]], dim=0) for t in (g,) + more)
    return out if more else out[0]


def perceiver_operands(sd: Dict[str, torch.Tensor], prefix: str, cfg: LensCfg, device, wdtype=torch.bfloat16) -> list:
    """Device copies of the Perceiver's layers: one dict per layer (cross attention "x_*", its FeedForward "x_ff*", the latent
    "selfs"), GEMM weights in `wdtype` (bf16; f32 for the fp32 engine), LayerNorm parameters and biases f32.  to_q / to_kv of a
    latent self-attention are one packed "qkv_w"; the GEGLU's first Linear is row-interleaved (interleave_geglu)."""
    dv = lambda k, dt=torch.float32: _dev(sd[k], device, dt)
    ln = lambda q: (dv(q + ".weight"), dv(q + ".bias"))

    def attn(p, packed):
        d = {"to_out_w": dv(p + "to_out.weight", wdtype), "to_out_b": dv(p + "to_out.bias")}
        if packed:
            d["qkv_w"] = _dev(torch.cat([sd[p + "to_q.weight"], sd[p + "to_kv.weight"]], 0), device, wdtype)
        else:
            d["q_w"], d["kv_w"] = dv(p + "to_q.weight", wdtype), dv(p + "to_kv.weight", wdtype)
        return d

    def ff(p):
        w0, b0 = interleave_geglu(sd[p + "net.0.weight"].detach().float(), sd[p + "net.0.bias"].detach().float())
        return {"w0": _dev(w0, device, wdtype), "b0": _dev(b0, device), "w2": dv(p + "net.2.weight", wdtype), "b2": dv(p + "net.2.bias")}
    layers = []
    for i in range(cfg.depth):
        if cfg.weight_tie_layers and i >= 2:
            # perceiver.py:249-254 (`cache_fn`): layers 1 .. depth-1 ARE one set of modules; the state_dict repeats their
            # tensors under every layer index.  Sharing the objects here makes an update of layer 1 an update of all.
            layers.append(layers[1])
            continue
        q = f"{prefix}layers.{i}."
        lay = {"x_norm": ln(q + "0.norm"), "x_norm_ctx": ln(q + "0.norm_context"), "x_attn": attn(q + "0.fn.", False),
               "x_ff_norm": ln(q + "1.norm"), "x_ff": ff(q + "1.fn."), "selfs": []}
        for j in range(cfg.self_per_cross):
            r = f"{q}2.{j}."
            lay["selfs"].append({"norm": ln(r + "0.norm"), "attn": attn(r + "0.fn.", True), "ff_norm": ln(r + "1.norm"),
                                 "ff": ff(r + "1.fn.")})
        layers.append(lay)
    return layers


@dataclass
class LensAttnSlots:
    """Where perceiver_forward reads and writes one attention sub-layer x1 = x0 + to_out(attn(...)).  Cross attention: q2 and
    the context's kv2 apart, cn = LN_ctx(data); latent self-attention: q2 is the packed [q|k|v], kv2 and cn are None.  An
    optional output that is None is not written (an engine's)."""
    x0: torch.Tensor
    x1: torch.Tensor
    hn: torch.Tensor                           # LN(x0)
    q2: torch.Tensor                           # token-major projection outputs and their views by heads (ops.heads_view)
    kv2: Optional[torch.Tensor]
    q: torch.Tensor
    k: torch.Tensor
    v: torch.Tensor
    a: torch.Tensor                            # attention output
    cn: Optional[torch.Tensor] = None
    stats: Optional[tuple] = None              # (mean, rstd) of LN(x0), of LN_ctx(data)
    cstats: Optional[tuple] = None
    lse: Optional[torch.Tensor] = None
    av: Optional[torch.Tensor] = None          # a trainer's backward: a by heads, the out-projection's input gradient, delta
    dOm: Optional[torch.Tensor] = None
    dO: Optional[torch.Tensor] = None
    delta: Optional[torch.Tensor] = None


@dataclass
class LensFFSlots:
    """One GEGLU FeedForward sub-layer x1 = x0 + W2 geglu(W0 LN(x0) + b0) + b2."""
    x0: torch.Tensor
    x1: torch.Tensor
    hn: torch.Tensor                           # LN(x0)
    hid: torch.Tensor                          # geglu(...)
    stats: Optional[tuple] = None
    h: Optional[torch.Tensor] = None           # the GEGLU's pre-activation
    y: Optional[torch.Tensor] = None           # ff_dropout > 0: the down-projection's fp32 output in front of the mask


def perceiver_residuals(c: LensCfg) -> int:
    """How many residual snapshots a Perceiver has: one in front of the first sub-layer and one behind every sub-layer."""
    return c.depth * (2 + 2 * c.self_per_cross) + 1


def perceiver_slots(c: LensCfg, B, Tc, device, dtype, X=None):
    """-> (X, layers): the residual snapshots in front of and behind every sub-layer and, per layer, the slots of its
    sub-layers under the operand table's keys ("x_attn", "x_ff", "selfs"[j]["attn" | "ff"]).  An engine's workspace (X None):
    ONE in-place fp32 stream and one set of `dtype` temporaries shared by all sub-layers, nothing optional.  A trainer's
    (X: its perceiver_residuals(c) snapshots): saved operands, statistics and lse per sub-layer, and the backward's
    per-attention buffers - allocated in the order the trainer's state has always had."""
    n, D, C, f32 = c.num_latents, c.latent_dim, c.input_chan, torch.float32
    R, save = B * n, X is not None
    new = lambda *s, dt=dtype: torch.empty(*s, device=device, dtype=dt)
    if not save:
        X = [new(R, D, dt=f32)] * perceiver_residuals(c)
    shared = {}

    def tmp(name, *s):
        """A trainer's buffer: a new one per sub-layer.  An engine's temporary: one per name, shared by the sub-layers."""
        if save:
            return new(*s)
        if name not in shared:
            shared[name] = new(*s)
        return shared[name]
    stats = lambda rows: (new(rows, dt=f32), new(rows, dt=f32)) if save else None
    xi = iter(range(len(X)))

    def attn(H, dh, cross):
        i, inner = next(xi), H * dh
        st, cst = stats(R), stats(B * Tc) if cross else None
        if cross:
            hn, cn, q2, kv2 = tmp("h", R, D), tmp("ctx", B * Tc, C), tmp("xq2", R, inner), tmp("xkv2", B * Tc, 2 * inner)
            q, k, v = ops.heads_view(q2, B, n, H, dh), ops.heads_view(kv2, B, Tc, H, dh), ops.heads_view(kv2, B, Tc, H, dh, inner)
        else:
            q2, kv2, cn = tmp("sqkv2", R, 3 * inner), None, None
            q, k, v = (ops.heads_view(q2, B, n, H, dh, j * inner) for j in range(3))
        a = tmp("xa" if cross else "sa", R, inner)
        lse, dOm, delta = (new(B, H, n, dt=f32), new(R, inner), new(B, H, n, dt=f32)) if save else (None, None, None)
        if not cross:
            hn = tmp("h", R, D)
        by_heads = lambda m: ops.heads_view(m, B, n, H, dh) if save else None
        return LensAttnSlots(x0=X[i], x1=X[i + 1], hn=hn, q2=q2, kv2=kv2, q=q, k=k, v=v, a=a, cn=cn, stats=st, cstats=cst, lse=lse,
                             av=by_heads(a), dOm=dOm, dO=by_heads(dOm), delta=delta)

    # ONE fp32 [R, D] buffer for every FeedForward of these slots, of a trainer too.  Forward: the down-projection's output, dead
    # once the row kernel has added its masked copy to the residual - the backward redraws the mask and never reads it.
    # Backward (PerceiverTrainer._ff_bwd): scratch for the unrounded branch gradient, written and column-summed within one
    # sub-layer.  So nothing may expect y to hold a value across sub-layers; every trainer owns its own slots.
    y = new(R, D, dt=f32) if c.ff_dropout > 0.0 else None

    def ff():
        i = next(xi)
        st, h = stats(R), new(R, 8 * D) if save else None
        return LensFFSlots(x0=X[i], x1=X[i + 1], hn=tmp("h", R, D), hid=tmp("hid", R, 4 * D), stats=st, h=h, y=y)
    layers = [{"x_attn": attn(c.cross_heads, c.cross_dim_head, True), "x_ff": ff(),
               "selfs": [{"attn": attn(c.latent_heads, c.latent_dim_head, False), "ff": ff()} for _ in range(c.self_per_cross)]}
              for _ in range(c.depth)]
    return X, layers


def perceiver_forward(layers, slots, data, B, c: LensCfg, ar, drop: Optional[LensDrop] = None):
    """Perceiver.forward(return_embeddings=True) behind the latents' broadcast (open_clip/perceiver.py:289-328,
    fourier_encode_data=False) with the operands `layers` (perceiver_operands) on the buffers `slots` (perceiver_slots) in the
    arithmetic `ar` (linear / geglu / attn: Bf16Arith, f32.F32Arith).  Per layer: cross attention of the latents over
    data [B*Tc, C], FeedForward, then self_per_cross x (latent self-attention, FeedForward), each with its residual.  The one
    forward of the engines and the trainer: it branches on what it is given, never on who calls.

    drop (a train-mode forward: LensDrop): with drop.pa > 0 every attention drops probabilities (ar.attn_drop), with
    drop.pf > 0 every FeedForward's down-projection leaves its fp32 output in s.y and a row kernel adds its masked, scaled
    copy to the residual (perceiver.py:91-102, 105-154).  None - eval mode, or both probabilities 0 - is the calls without
    it, to the same symbols in the same order."""
    rows, D = B * c.num_latents, c.latent_dim
    pa, pf = (drop.pa, drop.pf) if drop is not None else (0.0, 0.0)
    if (pa > 0.0 or pf > 0.0) and not hasattr(ar, "attn_drop"):
        raise ValueError("perceiver_forward: dropout runs on bf16 operands only (the fp32 engines are eval-only and never drop)")
    if pf > 0.0 and any(S["x_ff"].y is None for S in slots):
        raise ValueError("perceiver_forward: ff dropout needs slots built for a LensCfg with ff_dropout > 0")
    sub = iter(range(perceiver_residuals(c) - 1))       # every sub-layer's position in this forward

    def attn(w, norm, s, dh, norm_ctx=None):
        if ("qkv_w" in w) != (s.kv2 is None):
            raise ValueError("perceiver_forward: packed (self) operands need packed slots, cross operands q2 / kv2 slots")
        m, r = s.stats or (None, None)
        ops.layernorm(s.x0, norm[0], norm[1], s.hn, rows, D, mean=m, rstd=r)
        if s.kv2 is None:                      # latent self-attention: bias-free to_q / to_kv as one packed projection
            ar.linear(s.hn, w["qkv_w"], None, s.q2)
        else:
            m, r = s.cstats or (None, None)
            ops.layernorm(data, norm_ctx[0], norm_ctx[1], s.cn, data.shape[0], c.input_chan, mean=m, rstd=r)
            ar.linear(s.hn, w["q_w"], None, s.q2)
            ar.linear(s.cn, w["kv_w"], None, s.kv2)
        k = next(sub)
        if pa > 0.0:
            ar.attn_drop(s.q, s.k, s.v, s.a, s.lse, dh, drop, k)
        else:
            ar.attn(s.q, s.k, s.v, s.a, s.lse, dh)
        ar.linear(s.a, w["to_out_w"], w["to_out_b"], s.x1, res=s.x0)

    def ff(w, norm, s):
        m, r = s.stats or (None, None)
        ops.layernorm(s.x0, norm[0], norm[1], s.hn, rows, D, mean=m, rstd=r)
        ar.geglu(s.hn, w["w0"], w["b0"], s.hid, s.h)
        k = next(sub)
        if pf > 0.0:
            ar.linear_f32(s.hid, w["w2"], w["b2"], s.y)
            ops.ff_drop_fwd(s.y, s.x0, s.x1, B, c.num_latents, pf, drop.seed, drop.sample0, k)
        else:
            ar.linear(s.hid, w["w2"], w["b2"], s.x1, res=s.x0)

    for lay, S in zip(layers, slots):
        attn(lay["x_attn"], lay["x_norm"], S["x_attn"], c.cross_dim_head, lay["x_norm_ctx"])
        ff(lay["x_ff"], lay["x_ff_norm"], S["x_ff"])
        for sl, T in zip(lay["selfs"], S["selfs"]):
            attn(sl["attn"], sl["norm"], T["attn"], c.latent_dim_head)
            ff(sl["ff"], sl["ff_norm"], T["ff"])


class PerceiverEngine:
    """Perceiver.forward(return_embeddings=True) (open_clip/perceiver.py:289-328), fourier_encode_data=False."""

    def __init__(self, sd, prefix: str, cfg: LensCfg, device, gemm_cfg=-1, arith=None):
        self.cfg, self.device, self.gemm_cfg = cfg, torch.device(device), gemm_cfg
        ops.check_dropout_p(cfg.attn_dropout, "perceiver_attn_dropout"); ops.check_dropout_p(cfg.ff_dropout, "perceiver_ff_dropout")
        self.arith = Bf16Arith(gemm_cfg) if arith is None else arith
        self.latents = _dev(sd[prefix + "latents"], device)
        self.layers = perceiver_operands(sd, prefix, cfg, device, self.arith.dtype)
        self._ws = {}

    def update_params(self, sd, prefix: str):
        """All Perceiver operands re-derived from `sd`, in place (the Perceiver is trainable as a whole in every recipe)."""
        self.latents.copy_(sd[prefix + "latents"].detach())
        copy_tree(self.layers, perceiver_operands(sd, prefix, self.cfg, self.device, self.arith.dtype))

    def draw(self, seed: int, sample0: int) -> Optional[LensDrop]:
        """The dropout draw of ONE train-mode forward whose batch row 0 has the per-sample number `sample0`; None when the
        configuration drops nothing, so that the default is the code path without the argument."""
        c = self.cfg
        if not (c.attn_dropout > 0.0 or c.ff_dropout > 0.0):
            return None
        return LensDrop(int(seed), int(sample0), float(c.attn_dropout), float(c.ff_dropout))

    def forward(self, data: torch.Tensor, B: int, drop: Optional[LensDrop] = None) -> torch.Tensor:
        """data [B*Tc, C] (bf16|f32; f32 for the fp32 arithmetic) -> latents [B*n, D] f32 (view of an internal workspace).
        drop: a train-mode forward without autograd (nn.Dropout follows .training, not requires_grad)."""
        c, key = self.cfg, (B, data.shape[0] // B)
        if key not in self._ws:
            self._ws[key] = perceiver_slots(c, *key, self.device, self.arith.dtype)
        X, slots = self._ws[key]
        X[0].view(B, c.num_latents, c.latent_dim).copy_(self.latents)          # repeat(latents, 'n d -> b n d')
        perceiver_forward(self.layers, slots, data, B, c, self.arith, drop)
        return X[-1]


def lens_cols(im2col, x: torch.Tensor, lens: LensCfg, patch: int, Kp: int) -> torch.Tensor:
    """The GEMM rows [B*T, Kp] of a Lens tokenizer's convolution, by `im2col` (ops.im2col: bf16, ops.im2col_f32), column order
    (c, i, j) = the conv weight's.  depth (DepthTokenizer.py:35-60): patch x patch, stride patch.  audio (AST_tokenizer.py:
    44-57): [N,T,F] -> a conv over [N,1,F,T] with the f / t strides.  eeg (EEG_tokenizer.py:35-42, PatchEmbed1D): windows of the
    time axis of [N, chans, time] = a conv over [N, chans, 1, time]."""
    L, p = lens, patch
    if L.modality not in ("depth", "audio", "eeg"):
        raise NotImplementedError(L.modality)
    kh, kw, sh, sw, transpose_hw, unsqueeze = {"depth": (p, p, p, p, False, None),
                                               "audio": (p, p, L.audio_fstride, L.audio_tstride, True, 1),
                                               "eeg": (1, L.eeg_window_size, 1, L.eeg_stride, False, 2)}[L.modality]
    x = x.contiguous().float()
    return im2col(x if unsqueeze is None else x.unsqueeze(unsqueeze), kh, kw, sh, sw, Kp, transpose_hw=transpose_hw)[0]


class LensEngine:
    """`visual.` tower of TriCLIP for a non-image modality: visual_adapter -> (+pos) -> Perceiver -> ViT trunk
    (VisionTransformer.forward, open_clip/transformer.py:723-792), in the arithmetic `arith` (default: Bf16Arith(gemm_cfg);
    f32.LensEngineF32 passes F32Arith): tower, Perceiver and tokenizer are built in its dtype."""

    def __init__(self, sd, prefix: str, tower: TowerCfg, lens: LensCfg, device, res_dtype=torch.float32, gemm_cfg=-1, arith=None):
        self.tower, self.lens, self.device, self.gemm_cfg = tower, lens, torch.device(device), gemm_cfg
        self.arith = Bf16Arith(gemm_cfg) if arith is None else arith
        # a tower without ln_pre is the EVA ViT of a Perceiver_Blip_EVA_ViT (its state_dict names, eva_tower_state)
        eva = {} if tower.pre_norm else {"n_tokens": lens.num_latents + 1}
        self.vit = (EvaVitEngine if eva else VitEngine)(sd, prefix, tower, device, res_dtype=res_dtype, gemm_cfg=gemm_cfg,
                                                        arith=self.arith, **eva)
        a = self.prefix_adapter = prefix + "visual_adapter."
        self.conv_w = self.conv_b = self.adapter_pos = self.points = None
        self._points_pending = None             # the parameters a PointBERT tokenizer is rebuilt from at its next use (update_params)
        if lens.modality in ("depth", "audio", "eeg"):
            self.conv_w, self.conv_b, self.adapter_pos = self._adapter_operands(sd, a)
        elif lens.modality == "pc":
            self.points = self._point_tokenizer(sd)
        else:
            raise NotImplementedError(lens.modality)
        self.perceiver = None if lens.perceiver_identity else PerceiverEngine(sd, prefix + "perceiver.", lens, device, gemm_cfg, self.arith)

    def _adapter_operands(self, sd, a: str):
        """-> (conv weight as a GEMM operand, bias f32 or None, pos_emb f32 scaled by disable_adapter_pos) of the depth / audio
        (conv1, no bias) or EEG tokenizer (PatchEmbed1D: Conv1d(chans -> width, kernel = window, stride, bias) over time = a conv
        over [N, C, 1, T]), as new device tensors."""
        eeg = self.lens.modality == "eeg"
        w = sd[a + "proj.weight"].unsqueeze(2) if eeg else sd[a + "conv1.weight"]
        pos = sd[a + "pos_emb"].detach().float() * (0.0 if self.lens.disable_adapter_pos else 1.0)
        return (conv_weight_as_gemm(w, self.device, self.arith.dtype), _dev(sd[a + "proj.bias"], self.device) if eeg else None,
                _dev(pos, self.device))

    def _point_tokenizer(self, sd):
        from .points import PNSATokenizerTrainer, PointTokenizerEngine
        if self.lens.pc_tokenizer == "pnsa":       # inference = the trainer class with the running BatchNorm statistics
            return PNSATokenizerTrainer(sd, self.prefix_adapter, self.lens, self.device, gemm_cfg=self.gemm_cfg, bn_training=False)
        return PointTokenizerEngine(sd, self.prefix_adapter, self.lens, self.device, gemm_cfg=self.gemm_cfg)

    def update_params(self, sd, prefix: str, names):
        """In-place refresh after the parameters `names` (relative to `prefix`) changed, e.g. by an optimizer step."""
        a = prefix + "visual_adapter."
        self.vit.update_params(sd, [n for n in names if not n.startswith(("visual_adapter.", "perceiver."))])    # (EVA names: EvaVitEngine maps them)
        if any(n.startswith("visual_adapter.") for n in names):
            if self.points is None:
                for dst, src in zip((self.conv_w, self.conv_b, self.adapter_pos), self._adapter_operands(sd, a)):
                    if dst is not None:
                        dst.copy_(src)
            elif self.lens.pc_tokenizer == "pnsa":
                self.points.load_params(sd)
            else:
                # the inference tokenizer (BatchNorm folded into the convolutions, a host round trip) is rebuilt at its next
                # USE: while training every optimizer step lands here and the trainer runs its own tokenizer copy
                self._points_pending = {k: v for k, v in sd.items() if k.startswith(a)}
        if self.perceiver is not None and any(n.startswith("perceiver.") for n in names):
            self.perceiver.update_params(sd, prefix + "perceiver.")

    def cols(self, x: torch.Tensor) -> torch.Tensor:
        if self.lens.modality == "pc":          # (no convolution tokenizer: the point cloud's is self.points)
            raise NotImplementedError(self.lens.modality)
        return lens_cols(self.arith.im2col, x.to(self.device), self.lens, self.tower.patch, self.conv_w.shape[1])

    def conv_tokens(self, cols: torch.Tensor) -> torch.Tensor:
        """The tokenizer convolution on its im2col rows (a trainer keeps them for the weight gradient) -> tokens [B*T, C]."""
        tok = torch.empty(cols.shape[0], self.conv_w.shape[0], device=cols.device, dtype=self.arith.dtype)
        self.arith.linear(cols, self.conv_w, self.conv_b, tok)
        return tok

    def tokens(self, x: torch.Tensor):
        """-> (tokens [B*T, C] in the arithmetic's dtype, pos table [T, C] f32)."""
        return self.conv_tokens(self.cols(x)), self.adapter_pos

    def encode(self, x: torch.Tensor, normalize: bool = False, keep: Optional[torch.Tensor] = None,
               drop: Optional[LensDrop] = None, tokens_out: bool = False, **kw) -> torch.Tensor:
        """keep int32 [B,K] (ops.patch_keep): patch dropout on the tokens that enter the ViT trunk (VitEngine.trunk).
        drop (PerceiverEngine.draw): the Perceiver's dropout of a train-mode forward without autograd.
        tokens_out: the trunk's [B, L, D] token stream instead of the pooled feature (VitEngine.trunk)."""
        return self._encode(x, normalize, keep, drop, tokens_out, **kw)

    def _encode(self, x, normalize=False, keep=None, drop=None, tokens_out=False, **kw):
        B = x.shape[0]
        if tokens_out:
            if normalize:
                raise ValueError("LensEngine.encode: tokens_out returns the un-pooled stream, there is nothing to normalise")
            trunk = lambda *a, **k: self.vit.trunk(*a, tokens_out=True, **k)
        else:
            trunk = self.vit.trunk
        pos2 = None
        if self.points is not None:
            if self._points_pending is not None:
                self.points, self._points_pending = self._point_tokenizer(self._points_pending), None
            tok = self.points.forward(x, **kw)                 # already x + pos, [B*G, C]
        else:
            tok, pos2 = self.tokens(x)
            if self.perceiver is not None:
                tok, pos2 = ops.add_rows(tok, pos2, torch.empty_like(tok), tok.shape[0], tok.shape[0] // B, tok.shape[1]), None
        if self.perceiver is not None:
            tok = self.perceiver.forward(tok, B, drop)
        f = trunk(tok, B, pos2=pos2, use_orig_pos=self.lens.use_orig_pos, keep=keep)
        return ops.l2_normalize(f) if normalize else f
