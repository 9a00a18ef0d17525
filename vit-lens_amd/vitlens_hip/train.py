"""Forward-with-saved-activations and backward of the trainable `visual.` tower on the HIP kernels.

Implements the autograd of VisionTransformer.forward (open_clip/transformer.py:723-792) for the lock
recipes of the reference (`VisionTransformer.lock`, transformer.py:553-627): dX flows through every
ResidualAttentionBlock, dW is produced only for the unlocked subset (depth recipe: visual_adapter +
the first n blocks; TRAIN_INFERENCE.md:229-242).  No torch autograd graph is built inside the tower:
`TowerTrainer.forward` stores exactly the tensors the backward kernels need and `backward` replays
the blocks in reverse with hand-written kernels (GEMM dX with fused dGELU, attention backward,
LayerNorm backward); weight gradients are NT GEMMs over transposed activation copies accumulated in
fp32 (`EPI_RES_F32` into the gradient buffer).
"""
import math
from typing import Dict, Iterable, Optional

import torch

from . import ops
from . import engine as _engine
from .engine import VitEngine, deinterleave_geglu  # noqa: F401  (re-exported: the inverse of engine.interleave_geglu)

BF = torch.bfloat16


class _Saved:
    """Per-(B, L) activation store: residual-stream snapshots and attention operands of every block."""

    def __init__(self, B, L, D, H, hidden, layers, device, res_dtype=torch.float32, keep_blocks=(), checkpoint=False):
        """checkpoint=True (set_grad_checkpointing, transformer.py:366-368): only the block INPUTS are kept per layer; every
        other per-layer buffer is ONE tensor shared by all layers (the lists below repeat the same object), refilled by
        re-running a block's forward right before its backward.  ViT-L at 256 samples: 3.4 GB instead of 36 GB."""
        dh = D // H
        T = B * L
        Lp = (L + 7) // 8 * 8
        f32 = lambda *s: torch.empty(*s, device=device, dtype=torch.float32)
        bf = lambda *s: torch.empty(*s, device=device, dtype=BF)
        self.Lp = Lp
        xres = f32 if res_dtype == torch.float32 else bf

        def per_layer(make):
            if not checkpoint:
                return [make() for _ in range(layers)]
            one = make()
            return [one] * layers
        mids = per_layer(lambda: xres(T, D))
        self.X = [None] * (2 * layers + 1)                            # X[2l]=block input, X[2l+1]=after attention
        for l in range(layers):
            self.X[2 * l] = xres(T, D); self.X[2 * l + 1] = mids[l]
        self.X[2 * layers] = xres(T, D)
        # mean1, rstd1, mean2, rstd2.  Defined from the start as the identity (mean 0, rstd 1), not uninitialised memory: the
        # pruned last block (engine.PRUNE_LAST_BLOCK) never runs ln_2 on the rows that are not class tokens and keeps the class
        # rows' statistics in stats2c, so its (mean2, rstd2) slot is never written
        ident = lambda: [torch.zeros(T, device=device), torch.ones(T, device=device), torch.zeros(T, device=device),
                         torch.ones(T, device=device)]
        self.stats = per_layer(ident)
        # the packed in-projection output of every block; the attention kernels read q / k / v out of it in place
        self.qkv = per_layer(lambda: bf(T, 3 * D))
        hv = lambda m, i=0: ops.heads_view(m, B, L, H, dh, i * D)
        self.q = [hv(m, 0) for m in self.qkv]; self.k = [hv(m, 1) for m in self.qkv]; self.v = [hv(m, 2) for m in self.qkv]
        self.a = per_layer(lambda: bf(T, D))
        self.av = [hv(m) for m in self.a]
        self.lse = per_layer(lambda: f32(B, H, L))
        self.u = per_layer(lambda: bf(T, hidden))
        # temporaries shared by all blocks
        self.h = bf(T, D); self.hid = bf(T, hidden)
        # trainable blocks keep their GEMM inputs (LN outputs, GELU output) for the weight gradients: 1.3 GB per block and
        # micro-batch at b = 256 instead of two LayerNorm passes and one GELU pass in the backward (HBM is 288 GB)
        if checkpoint and keep_blocks:
            k1, k2, k3 = bf(T, D), bf(T, D), bf(T, hidden)
            self.h1 = {l: k1 for l in keep_blocks}; self.h2 = {l: k2 for l in keep_blocks}; self.hidk = {l: k3 for l in keep_blocks}
        else:
            self.h1 = {l: bf(T, D) for l in keep_blocks}; self.h2 = {l: bf(T, D) for l in keep_blocks}
            self.hidk = {l: bf(T, hidden) for l in keep_blocks}
        # LayerNorm folding (frozen blocks, bf16 stream): partial row sums between a GEMM and the row statistics behind it
        self.part = f32(T * (D // 64) * 2) if (D % 64 == 0 and res_dtype == BF) else None
        self.xpre = f32(T, D); self.pre_stats = [f32(T), f32(T)]
        self.post_stats = [f32(B), f32(B)]
        self.pooled = bf(B, D)
        # backward temporaries
        # residual-gradient stream in the residual dtype (the reference's autocast: bf16 activations -> bf16 gradients);
        # with an f32 stream the GEMM operand is a separate bf16 copy
        self.dx = xres(T, D); self.dxb = bf(T, D) if res_dtype == torch.float32 else self.dx
        self.du = bf(T, hidden); self.dh = bf(T, D)
        self.dOm = bf(T, D); self.dO = hv(self.dOm)          # out-projection input gradient, read by heads in place
        self.delta = f32(B, H, L); self.dqkv = bf(T, 3 * D)
        # the pruned last block (engine.PRUNE_LAST_BLOCK): everything behind its in-projection exists for the B class rows only,
        # in buffers of its own - forward: attention output + lse, ln_2 output + statistics, MLP hidden, act'; backward: the
        # residual gradient of those rows (dxc) and the three small GEMM outputs
        self.a1 = bf(B, D); self.lse1 = f32(B, H); self.h2c = bf(B, D); self.stats2c = [f32(B), f32(B)]
        self.hid1 = bf(B, hidden); self.u1 = bf(B, hidden)
        self.dxc = bf(B, D); self.du1 = bf(B, hidden); self.dhc = bf(B, D); self.dO1 = bf(B, D)
        # what engine.block_forward reads and writes for layer l: the shared temporaries, or the kept copies of a trainable block
        self.slots = [_engine.BlockSlots(
            x0=self.X[2 * l], x1=self.X[2 * l + 1], x2=self.X[2 * l + 2], h1=self.h1.get(l, self.h), h2=self.h2.get(l, self.h),
            h_left=self.h, qkv=self.qkv[l], q=self.q[l], k=self.k[l], v=self.v[l], a=self.a[l], hid=self.hidk.get(l, self.hid),
            part=self.part, stats=tuple(self.stats[l]), lse=self.lse[l], u=self.u[l], a1=self.a1, h2c=self.h2c, hid1=self.hid1,
            lse1=self.lse1, stats2c=tuple(self.stats2c), u1=self.u1) for l in range(layers)]


def prunes_last_block(layers, train_blocks, checkpoint, causal, res_dtype, D, H, L) -> bool:
    """Whether a class-token-pooled trainer runs its last block on the class rows only (forward AND backward): the block is
    frozen and not recomputed, and the tower qualifies (engine.prune_last_ok: switch on, bf16 stream, head dim 64, no mask)."""
    return bool(layers > 0 and (layers - 1) not in set(train_blocks) and not checkpoint
                and _engine.prune_last_ok(D, H, res_dtype, L, True, causal))


class TowerTrainer:
    def __init__(self, eng: VitEngine, train_blocks: Iterable[int] = (), train_cls=False, train_pos=False,
                 param_prefix: str = "visual.", train_ln_pre=False, train_ln_post=False, train_proj=False, checkpoint=False):
        self.eng, self.prefix = eng, param_prefix
        self.causal = False                         # (TextTowerTrainer: the text transformer's additive causal mask, transformer.py:870-876)
        self.checkpoint = bool(checkpoint)          # activation recompute per block (Transformer.forward, transformer.py:366-368)
        self.train_blocks = sorted(set(train_blocks))
        self.train_cls, self.train_pos = train_cls, train_pos
        # the stem / head pieces of the grouped (LiT) unlock, VisionTransformer.lock open_clip/transformer.py:564-597
        self.train_ln_pre, self.train_ln_post, self.train_proj = train_ln_pre, train_ln_post, train_proj
        c = eng.cfg
        self.D, self.H, self.hidden, self.layers = c.width, c.heads, int(c.width * c.mlp_ratio), c.layers
        # the MLP activation of this tower with its derivative saved by the forward: exact-erf GELU, or QuickGELU (cfg.quick_gelu)
        self.act_dsave = ops.mlp_act(bool(getattr(c, "quick_gelu", False)), dsave=True)
        dev = eng.device
        # transposed bf16 weights for the dX GEMMs (C = dY . W  ==  NT GEMM against W^T)
        self.wT = [{k: w[k].t().contiguous() for k in ("in_w", "out_w", "fc_w", "proj_w")} for w in eng.blocks]
        # [D, E]: the NT "W" operand of dpooled = dfeat . proj^T (None: a tower without output projection)
        self.proj = eng.projT.t().contiguous() if eng.projT is not None else None
        self._saved = {}
        self.grads: Dict[str, torch.Tensor] = {}
        self.ctx = None
        self._pruned = False                        # the decision of the last forward(), kept for its backward()
        self._drop = None                           # (T, inv) of the last forward() when it dropped tokens, else None

    def refresh_derived(self, blocks=(), proj=False):
        """The engine's weights of `blocks` (and proj) were updated in place: redo their transposes."""
        for l in blocks:
            for k in ("in_w", "out_w", "fc_w", "proj_w"):
                self.wT[l][k].copy_(self.eng.blocks[l][k].t())
        if proj and self.proj is not None:
            self.proj.copy_(self.eng.projT.t())

    # ------------------------------------------------------------------------------------------ helpers
    def saved(self, B, L):
        key = (B, L)
        if key not in self._saved:
            self._saved[key] = _Saved(B, L, self.D, self.H, self.hidden, self.layers, self.eng.device, self.eng.res_dtype,
                                      keep_blocks=tuple(self.train_blocks), checkpoint=self.checkpoint)
        return self._saved[key]

    def grad_buffer(self, name, like):
        g = self.grads.get(name)
        if g is None:
            g = torch.zeros(like.shape, device=self.eng.device, dtype=torch.float32)
            self.grads[name] = g
        return g

    def zero_grads(self):
        for g in self.grads.values():
            g.zero_()

    # ------------------------------------------------------------------------------------------ forward
    def forward(self, tokens: torch.Tensor, B: int, pos2: Optional[torch.Tensor] = None, keep: Optional[torch.Tensor] = None,
                inv: Optional[torch.Tensor] = None) -> torch.Tensor:
        """tokens [B*T, D] -> un-normalised features f32 [B, E]; keeps what backward() needs.
        keep / inv (ops.patch_keep; PatchDropout in train mode, open_clip/transformer.py:53-90, applied after the positional
        add and before ln_pre, :770-771): the trunk runs on the class token + the K kept tokens of every sample - L = K + 1
        everywhere behind the assembly, which gathers the kept rows itself and never writes the T + 1 row stream."""
        e, D, H = self.eng, self.D, self.H
        T = tokens.shape[0] // B
        if (keep is None) != (inv is None):
            raise ValueError("TowerTrainer.forward: keep and inv come together (ops.patch_keep)")
        if keep is not None and (tuple(inv.shape) != (B, T) or keep.shape[0] != B or not 1 <= keep.shape[1] <= T):
            raise ValueError(f"TowerTrainer.forward: keep [B,K] / inv [B,T] do not fit B={B}, T={T}: {tuple(keep.shape)}, {tuple(inv.shape)}")
        L = T + 1 if keep is None else keep.shape[1] + 1
        S = self.saved(B, L)
        cfg, eps = e.gemm_cfg, e.cfg.ln_eps
        if not e.cfg.pre_norm:          # a tower without ln_pre (the EVA ViT): block 0 reads [cls; tokens] + pos (+ pos2) itself
            if keep is not None:
                raise NotImplementedError("TowerTrainer.forward: patch dropout on a tower without ln_pre (vl_assemble_tokens is dense only)")
            ops.assemble_tokens(tokens, e.cls, e.pos, pos2, S.X[0], B, T, D)
        elif keep is None:
            ops.assemble_ln_pre(tokens, e.cls, e.pos, pos2, e.ln_pre[0], e.ln_pre[1], S.X[0], B, T, D, eps=eps,
                                xpre=S.xpre, mean=S.pre_stats[0], rstd=S.pre_stats[1])
        else:
            ops.assemble_ln_pre_keep(tokens, keep, e.cls, e.pos, pos2, e.ln_pre[0], e.ln_pre[1], S.X[0], B, T, D, eps=eps,
                                     xpre=S.xpre, mean=S.pre_stats[0], rstd=S.pre_stats[1])
        self._drop = None if keep is None else (T, inv)
        # only the class rows of the last block's output are read (ln_post below, and its backward)
        self._pruned = prunes_last_block(self.layers, self.train_blocks, self.checkpoint, self.causal, e.res_dtype, D, H, L)
        mm = 0                                      # rows of X[2l] whose partial sums are in S.part
        for l in range(self.layers):
            mm = self._block_forward(S, l, B, L, cls_only=self._pruned and l == self.layers - 1, mm=mm)
        xl = S.X[2 * self.layers]
        ops.layernorm(xl, e.ln_post[0], e.ln_post[1], S.pooled, B, D, x_row_stride=L * D,
                      mean=S.post_stats[0], rstd=S.post_stats[1], eps=eps)
        if e.projT is None:          # features = ln_post(cls) itself (bf16 activation, returned as f32)
            feat = S.pooled.float()
        else:                        # (proj_b: the bias of an nn.Linear head - frozen in every recipe, it only enters the forward)
            feat = ops.gemm(S.pooled, e.projT, getattr(e, "proj_b", None), epi=ops.EPI_F32, cfg=cfg)
        self.ctx = (B, L, tokens, pos2 is not None)
        return feat

    def _block_forward(self, S, l, B, L, write_out=True, cls_only=False, mm=0):
        """engine.block_forward of layer l into its saved-activation slots; returns what that returns (the rows of X[2l+2] whose
        partial sums are in S.part, for the next block's `mm`).  write_out=False: the recompute in front of a block's backward
        (X[2l+2] is already there from the forward pass); cls_only: the last block of a class-token-pooled tower
        (prunes_last_block)."""
        e = self.eng
        # LayerNorm folding (round 4): a FROZEN block never materialises ln_1 / ln_2 - its backward needs only (mean, rstd),
        # which ln_row_stats leaves in S.stats; a trainable block keeps its LayerNorm outputs (the operands of its weight
        # gradients).  Either kind leaves the partial row sums of its output when the next block is folded.
        def folds(k):
            return bool(_engine.LN_FOLD and S.part is not None and k < self.layers and "in_f" in e.blocks[k]
                        and k not in self.train_blocks)
        return _engine.block_forward(e.blocks[l], S.slots[l], B, L, self.D, self.H, self.causal, self.act_dsave, e.math,
                                     folds(l), folds(l + 1), cls_only=cls_only, write_out=write_out, mm=mm, eps=e.cfg.ln_eps)

    # ------------------------------------------------------------------------------------------ backward
    def _dw(self, name, dy, x, bias_name=None):
        """grads[name] += dy^T x  (dy [rows, N], x [rows, K] -> [N, K]), grads[bias_name] += the column sums of dy."""
        g = self.grad_buffer(name, torch.empty(dy.shape[1], x.shape[1]))
        gb = self.grad_buffer(bias_name, torch.empty(dy.shape[1])) if bias_name else None
        ops.weight_grad(dy, x, g, bias_grad=gb, narrow=False, cfg=self.eng.gemm_cfg)

    def backward(self, dfeat: torch.Tensor, on_block_done=None) -> torch.Tensor:
        """dfeat f32 [B, E] -> gradient w.r.t. the input tokens, f32 [B*T, D]; fills self.grads.  After a forward that dropped
        tokens (keep / inv) the result is still the dense [B*T, D] gradient: the rows of dropped tokens are exact zeros.
        on_block_done(l) is called as soon as every gradient of trainable block l has been enqueued (the multi-GPU step
        starts that block's gradient all-reduce there, under the backward of the blocks below it)."""
        e, D, H = self.eng, self.D, self.H
        B, L, tokens, has_pos2 = self.ctx
        dh = D // H
        T = L - 1 if self._drop is None else self._drop[0]
        S = self.saved(B, L)
        rows = B * L
        cfg = e.gemm_cfg
        P = self.prefix
        # feat = pooled @ proj ; pooled = ln_post(x[:, 0])
        dfb = ops.cast_bf16(dfeat.contiguous())
        dpooled = dfb if self.proj is None else ops.gemm(dfb, self.proj, None, epi=ops.EPI_BF16, cfg=cfg)   # [B, D]
        if self.train_proj and self.proj is not None:          # feat = pooled @ proj  ->  dproj[D, E] += pooled^T dfeat
            bp = (B + 63) // 64 * 64
            ops.gemm_dw(ops.transpose_to_bf16(S.pooled, ldo=bp), ops.transpose_to_bf16(dfb, ldo=bp),
                        self.grad_buffer(P + "proj", torch.empty(D, dfeat.shape[1])), cfg=cfg)
        if self.train_ln_post:
            ops.layernorm_bwd_params(dpooled, S.X[2 * self.layers], S.post_stats[0], S.post_stats[1],
                                     self.grad_buffer(P + "ln_post.weight", e.ln_post[0]),
                                     self.grad_buffer(P + "ln_post.bias", e.ln_post[1]), B, D, x_row_stride=L * D)
        if self._pruned:
            # only the cls rows (row b*L) of the final residual receive gradient, and the pruned last block carries it in a
            # [B, D] buffer of its own: no zero fill of the full-size stream (its ln_1 backward writes every row of S.dx)
            ops.layernorm_bwd(dpooled, S.X[2 * self.layers], S.post_stats[0], S.post_stats[1], e.ln_post[0], B, D,
                              dx=S.dxc, x_row_stride=L * D)
        else:
            S.dx.zero_()
            # only the cls rows (row b*L) of the final residual receive gradient: write them in place
            ops.layernorm_bwd(dpooled, S.X[2 * self.layers], S.post_stats[0], S.post_stats[1], e.ln_post[0], B, D,
                              dx=S.dx, x_row_stride=L * D, dx_row_stride=L * D)
        self._blocks_backward(S, B, L, on_block_done, cls_only=self._pruned)
        # ---- ln_pre and the [cls; tokens] + pos assembly ----
        if not e.cfg.pre_norm:
            # no ln_pre: the gradient of block 0's input IS the gradient of the assembled rows (fp32 for the reductions below)
            dxpre = S.dx.float() if S.dx.dtype != torch.float32 else S.dx.clone()
        else:
            dxpre = torch.empty(S.dx.shape, device=S.dx.device, dtype=torch.float32)
            if self.train_ln_pre:
                ops.layernorm_bwd_params(S.dx, S.xpre, S.pre_stats[0], S.pre_stats[1], self.grad_buffer(P + "ln_pre.weight", e.ln_pre[0]),
                                         self.grad_buffer(P + "ln_pre.bias", e.ln_pre[1]), rows, D)
            ops.layernorm_bwd(S.dx, S.xpre, S.pre_stats[0], S.pre_stats[1], e.ln_pre[0], rows, D, dx=dxpre)
        if self.train_cls:
            ops.batch_rowsum(dxpre, self.grad_buffer(P + "class_embedding", e.cls).view(1, D), B, 1, D, L, 0)
        self.dxpre = dxpre
        if self._drop is not None:
            # the gather's backward: the compact rows back to their tokens' places, zeros for the dropped ones (one pass, every
            # row written).  pos[0] takes the class rows of the compact gradient, pos[1:] the dense scattered rows
            dtok = ops.scatter_rows_keep(dxpre, self._drop[1], L - 1)
            if self.train_pos:
                gpos = self.grad_buffer(P + "positional_embedding", e.pos)
                ops.batch_rowsum(dxpre, gpos[:1], B, 1, D, L, 0)
                ops.batch_rowsum(dtok, gpos[1:], B, T, D, T, 0)
            return dtok
        if self.train_pos:
            ops.batch_rowsum(dxpre, self.grad_buffer(P + "positional_embedding", e.pos), B, L, D, L, 0)
        return dxpre.view(B, L, D)[:, 1:, :].reshape(B * T, D)

    def _cls_block_backward(self, S, l, B, L):
        """Backward of the pruned last block (engine._cls_tail_forward): S.dxc [B, D] = the gradient of the class rows of its output
        (every other row's is zero) -> S.dx = the gradient of ALL rows of its input.  The MLP branch, ln_2, out_proj and the
        attention run on B rows; dK / dV, the dX GEMM of the in-projection and the ln_1 backward are dense.  Additions in the
        order of the full path: dLN_2 + dres on the class rows, then dLN_1 + that on the class rows, dLN_1 alone elsewhere."""
        e, D = self.eng, self.D
        w, wT, cfg = e.blocks[l], self.wT[l], e.gemm_cfg
        m1, r1 = S.stats[l][0], S.stats[l][1]
        x1c = _engine.cls_rows(S.X[2 * l + 1], B, L)
        ops.gemm(S.dxc, wT["proj_w"], None, out=S.du1, res=S.u1, epi=ops.EPI_DGELU, act=self.act_dsave, cfg=cfg)
        ops.gemm(S.du1, wT["fc_w"], None, out=S.dhc, epi=ops.EPI_BF16, cfg=cfg)
        ops.layernorm_bwd(S.dhc, x1c, S.stats2c[0], S.stats2c[1], w["ln2_w"], B, D, dres=S.dxc, dx=S.dxc, x_row_stride=L * D)
        ops.gemm(S.dxc, wT["out_w"], None, out=S.dO1, epi=ops.EPI_BF16, cfg=cfg)
        # (also writes the dQ rows of the other tokens as zeros: S.dqkv is fully defined for the dense GEMM below)
        ops.attn_bwd_q1(S.q[l], S.k[l], S.v[l], S.dO1, S.a1, S.lse1, S.dqkv, S.dqkv[:, D:], S.dqkv[:, 2 * D:], 3 * D, 3 * D, qrow=0)
        ops.gemm(S.dqkv, wT["in_w"], None, out=S.dh, epi=ops.EPI_BF16, cfg=cfg)
        ops.layernorm_bwd_sparse_res(S.dh, S.X[2 * l], m1, r1, w["ln1_w"], B * L, D, dres=S.dxc, dres_every=L, dx=S.dx)

    def _blocks_backward(self, S, B, L, on_block_done=None, cls_only=False):
        """S.dx (the gradient of the last block's output, residual-stream dtype) -> S.dx = the gradient of the first block's
        input, through every ResidualAttentionBlock in reverse; parameter gradients of the trainable blocks into self.grads.
        cls_only: the last block was pruned by the forward (S.dxc holds the gradient of its class rows instead)."""
        e, D, H = self.eng, self.D, self.H
        rows = B * L
        cfg = e.gemm_cfg
        P = self.prefix
        f32_stream = S.dx.dtype == torch.float32
        dxb_out = S.dxb if f32_stream else None
        if f32_stream:
            ops.cast_bf16(S.dx, out=S.dxb)
        for l in reversed(range(self.layers)):
            if cls_only and l == self.layers - 1:
                self._cls_block_backward(S, l, B, L)
                continue
            if self.checkpoint:          # refill the shared per-layer buffers with block l's activations
                self._block_forward(S, l, B, L, write_out=False)
            w, wT = e.blocks[l], self.wT[l]
            m1, r1, m2, r2 = S.stats[l]
            trainable = l in self.train_blocks
            bp = f"{P}transformer.resblocks.{l}."
            # ---- MLP branch: x2 = x1 + proj(gelu(fc(ln2(x1)))) ----
            ops.gemm(S.dxb, wT["proj_w"], None, out=S.du, res=S.u[l], epi=ops.EPI_DGELU, act=self.act_dsave, cfg=cfg)   # du = (dx W_proj) * act'(u)
            if trainable:
                self._dw(bp + "mlp.c_proj.weight", S.dx, S.hidk[l], bp + "mlp.c_proj.bias")
                self._dw(bp + "mlp.c_fc.weight", S.du, S.h2[l], bp + "mlp.c_fc.bias")
            ops.gemm(S.du, wT["fc_w"], None, out=S.dh, epi=ops.EPI_BF16, cfg=cfg)                           # dh2
            if trainable:
                ops.layernorm_bwd_params(S.dh, S.X[2 * l + 1], m2, r2, self.grad_buffer(bp + "ln_2.weight", w["ln2_w"]),
                                         self.grad_buffer(bp + "ln_2.bias", w["ln2_b"]), rows, D)
            ops.layernorm_bwd(S.dh, S.X[2 * l + 1], m2, r2, w["ln2_w"], rows, D, dres=S.dx, dx=S.dx, dx_bf16=dxb_out)
            # ---- attention branch: x1 = x0 + out(attn(qkv(ln1(x0)))) ----
            if trainable:
                self._dw(bp + "attn.out_proj.weight", S.dx, S.a[l], bp + "attn.out_proj.bias")
            ops.gemm(S.dxb, wT["out_w"], None, out=S.dOm, epi=ops.EPI_BF16, cfg=cfg)                        # dO
            ops.attn_bwd(S.q[l], S.k[l], S.v[l], S.dO, S.av[l], S.lse[l], S.delta,
                         S.dqkv, S.dqkv[:, D:], S.dqkv[:, 2 * D:], 3 * D, 3 * D, causal=self.causal)
            if trainable:
                self._dw(bp + "attn.in_proj_weight", S.dqkv, S.h1[l], bp + "attn.in_proj_bias")
            ops.gemm(S.dqkv, wT["in_w"], None, out=S.dh, epi=ops.EPI_BF16, cfg=cfg)                         # dh1
            if trainable:
                ops.layernorm_bwd_params(S.dh, S.X[2 * l], m1, r1, self.grad_buffer(bp + "ln_1.weight", w["ln1_w"]),
                                         self.grad_buffer(bp + "ln_1.bias", w["ln1_b"]), rows, D)
            ops.layernorm_bwd(S.dh, S.X[2 * l], m1, r1, w["ln1_w"], rows, D, dres=S.dx, dx=S.dx, dx_bf16=dxb_out)
            if trainable and on_block_done is not None:
                on_block_done(l)


def conv_weight_grad(dtok: torch.Tensor, cols: torch.Tensor, g: torch.Tensor, gemm_cfg: int = -1):
    """g[D, Kp] += dtok^T cols: the weight gradient of a stride-patch convolution run as im2col + GEMM (dtok f32 [R, D] = the
    gradient of its output tokens, cols bf16 [R, Kp] = the im2col rows the forward kept).  Token-major operands for the dW
    kernel (the fp32 gradient cast to bf16 - the values a transposed copy would hold too); the transposing NT path where the
    shape does not fit."""
    ops.weight_grad(ops.cast_bf16(dtok.contiguous()), cols, g, cfg=gemm_cfg)


class DepthLensTrainer:
    """`visual.` tower of the depth recipe: DepthTokenizer conv1 + pos_emb -> ViT trunk (Perceiver = Identity)."""

    def __init__(self, lens_engine, unlock_first_n: int = 4, tower_kw=None):
        self.le = lens_engine
        kw = dict(train_blocks=range(unlock_first_n)) if tower_kw is None else dict(tower_kw)
        self.tower = TowerTrainer(lens_engine.vit, param_prefix="visual.", **kw)
        self.ctx = None

    @property
    def grads(self):
        return self.tower.grads

    def forward(self, x: torch.Tensor, keep=None, inv=None) -> torch.Tensor:
        """keep / inv: patch dropout in front of the ViT trunk (TowerTrainer.forward); the tokenizer stays dense."""
        le = self.le
        cols = le.cols(x)
        tok = le.conv_tokens(cols)
        self.ctx = (cols, x.shape[0])
        return self.tower.forward(tok, x.shape[0], pos2=le.adapter_pos, keep=keep, inv=inv)

    def backward(self, dfeat: torch.Tensor, on_block_done=None):
        cols, B = self.ctx
        dtok = self.tower.backward(dfeat, on_block_done)         # f32 [B*T, D]
        T, D = dtok.shape[0] // B, dtok.shape[1]
        t = self.tower
        g = t.grad_buffer("visual.visual_adapter.conv1.weight_gemm", torch.empty(D, cols.shape[1]))
        conv_weight_grad(dtok, cols, g, self.le.gemm_cfg)
        gpos = t.grad_buffer("visual.visual_adapter.pos_emb", self.le.adapter_pos)
        if t._drop is not None:          # (t.dxpre holds the K + 1 kept rows: the dense scattered gradient instead)
            ops.batch_rowsum(dtok, gpos, B, T, D, T, 0)
        else:
            ops.batch_rowsum(t.dxpre, gpos, B, T, D, T + 1, 1)


class ImageTowerTrainer:
    """An image-modality tower (conv1 patchify -> ViT trunk) under any lock recipe; the stem convolution's weight
    gradient is produced when `train_conv` (grouped unlock reaching the stem, transformer.py:566-573)."""

    def __init__(self, vit_engine, tower_kw=None, train_conv: bool = False):
        self.eng = vit_engine
        self.tower = TowerTrainer(vit_engine, param_prefix="visual.", **(tower_kw or {}))
        self.train_conv = train_conv
        self.ctx = None

    @property
    def grads(self):
        return self.tower.grads

    def forward(self, x: torch.Tensor, keep=None, inv=None) -> torch.Tensor:
        e = self.eng
        p = e.cfg.patch
        cols, gh, gw = ops.im2col(x.contiguous().float(), p, p, p, p, e.conv_w.shape[1])
        tok = e.conv_tokens(cols)
        self.ctx = cols
        return self.tower.forward(tok, x.shape[0], keep=keep, inv=inv)

    def backward(self, dfeat: torch.Tensor):
        dtok = self.tower.backward(dfeat)
        if self.train_conv:
            cols = self.ctx
            g = self.tower.grad_buffer("visual.conv1.weight_gemm", torch.empty(dtok.shape[1], cols.shape[1]))
            conv_weight_grad(dtok, cols, g, self.eng.gemm_cfg)


class _TextAsTower:
    """What TowerTrainer reads of an engine, for the text tower (a `TextEngine(arith="bf16")`: bf16 operands, fp32 residual stream)."""

    def __init__(self, te):
        from types import SimpleNamespace
        c = te.cfg
        self.cfg = SimpleNamespace(width=c.width, heads=c.heads, mlp_ratio=4.0, layers=c.layers, quick_gelu=c.quick_gelu,
                                   ln_eps=c.ln_eps, pre_norm=False)
        self.device, self.res_dtype, self.gemm_cfg, self.math = te.device, torch.float32, te.gemm_cfg, te.math
        self.blocks, self.projT, self.ln_post = te.blocks, te.projT, te.ln_final
        self.tok, self.pos = te.tok, te.pos


class TextTowerTrainer(TowerTrainer):
    """Forward with saved activations and backward of the TEXT tower (TriCLIP.encode_text, open_clip/model.py:528-540: token
    embedding + positional embedding -> 12 causal ResidualAttentionBlocks -> ln_final -> the EOT token's row @ text_projection)
    for runs that do NOT lock it (every ViT-Lens recipe does; `training/train.py:212-235` trains whatever requires grad).  The
    blocks are TowerTrainer's, with the additive causal mask (transformer.py:870-876) in the attention kernels; gradients come
    out under the reference's parameter names: token_embedding.weight, positional_embedding, transformer.resblocks.*, ln_final.*,
    text_projection.  bf16 operands on an fp32 residual stream (the frozen tower's fp16 operands are an inference choice)."""

    def __init__(self, text_engine):
        if getattr(text_engine, "arith", "bf16") != "bf16":
            raise ValueError("TextTowerTrainer needs a TextEngine(arith='bf16')")
        eng = _TextAsTower(text_engine)
        super().__init__(eng, train_blocks=range(eng.cfg.layers), param_prefix="", train_ln_post=True, train_proj=True)
        self.causal = True

    def forward(self, text: torch.Tensor) -> torch.Tensor:
        e, D = self.eng, self.D
        B, L = text.shape
        S = self.saved(B, L)
        text = text.to(e.device).contiguous()
        ops.text_embed(text, e.tok, e.pos, S.X[0])
        mm = 0
        for l in range(self.layers):
            mm = self._block_forward(S, l, B, L, mm=mm)
        eot = text.argmax(dim=-1).contiguous()            # index-exact EOT position (model.py:539)
        ops.layernorm(S.X[2 * self.layers], e.ln_post[0], e.ln_post[1], S.pooled, B, D, x_row_stride=D, row_index=eot, row_mul=L,
                      mean=S.post_stats[0], rstd=S.post_stats[1], eps=e.cfg.ln_eps)
        feat = ops.gemm(S.pooled, e.projT, None, epi=ops.EPI_F32, cfg=e.gemm_cfg)
        self.ctx = (B, L, text, eot)
        return feat

    def backward(self, dfeat: torch.Tensor):
        """dfeat f32 [B, E]; fills self.grads (every text parameter)."""
        e, D = self.eng, self.D
        B, L, text, eot = self.ctx
        S = self.saved(B, L)
        cfg = e.gemm_cfg
        dfb = ops.cast_bf16(dfeat.contiguous())
        dpooled = ops.gemm(dfb, self.proj, None, epi=ops.EPI_BF16, cfg=cfg)                                  # [B, D]
        bp = (B + 63) // 64 * 64
        ops.gemm_dw(ops.transpose_to_bf16(S.pooled, ldo=bp), ops.transpose_to_bf16(dfb, ldo=bp),
                    self.grad_buffer("text_projection", torch.empty(D, dfeat.shape[1])), cfg=cfg)
        # ln_final acts on ONE row per caption, the EOT token's (an arbitrary position: gathered / scattered by index)
        rows = torch.arange(B, device=e.device) * L + eot
        x_eot = S.X[2 * self.layers].index_select(0, rows).contiguous()
        ops.layernorm_bwd_params(dpooled, x_eot, S.post_stats[0], S.post_stats[1], self.grad_buffer("ln_final.weight", e.ln_post[0]),
                                 self.grad_buffer("ln_final.bias", e.ln_post[1]), B, D)
        dx_eot = torch.empty(B, D, device=e.device, dtype=torch.float32)
        ops.layernorm_bwd(dpooled, x_eot, S.post_stats[0], S.post_stats[1], e.ln_post[0], B, D, dx=dx_eot)
        S.dx.zero_()
        S.dx.index_copy_(0, rows, dx_eot)
        self._blocks_backward(S, B, L)
        # x0 = token_embedding[text] + positional_embedding
        ops.batch_rowsum(S.dx, self.grad_buffer("positional_embedding", e.pos), B, L, D, L, 0)
        self.grad_buffer("token_embedding.weight", e.tok).index_add_(0, text.reshape(-1), S.dx)


def clip_coef(sumsq: torch.Tensor, max_norm: float, grad_scale: float = 1.0) -> torch.Tensor:
    """What vl_adamw_multi_step derives on the device, restated on tensors (f32 arithmetic, the same operations):
    min(1, max_norm / (grad_scale * sqrt(sumsq) + 1e-6)) = torch.nn.utils.clip_grad_norm_'s coefficient for the gradient
    grad_scale * g; a NaN norm gives NaN (error_if_nonfinite=False), an infinite one 0."""
    norm = torch.sqrt(sumsq.float()) * float(grad_scale)          # (a Python scalar: no host-to-device copy)
    return torch.clamp(max_norm / (norm + 1e-6), max=1.0)


def clip_grad_norm_(flat_or_tensors, max_norm: float) -> torch.Tensor:
    """torch.nn.utils.clip_grad_norm_(norm_type=2, error_if_nonfinite=False) for callers that hold the gradients themselves
    (a fused step's `flat_grad` / `reduced_grads()`) and run their own optimizer: the squared norm comes from the
    sum-of-squares kernel (`ops.grad_sumsq`, one launch pair per tensor - pass the flat buffer where there is one), the
    coefficient is derived and applied on the device (an in-place multiplication by a device scalar).  Takes one f32 tensor,
    a list of them or a dict (its values); scales them in place; returns the unclipped norm as a 0-d device tensor."""
    if not float(max_norm) > 0.0:
        raise ValueError(f"clip_grad_norm_: max_norm must be positive, got {max_norm}")
    if torch.is_tensor(flat_or_tensors):
        ts = [flat_or_tensors]
    else:
        ts = [t for t in (flat_or_tensors.values() if isinstance(flat_or_tensors, dict) else flat_or_tensors) if t is not None]
    if not ts:
        raise ValueError("clip_grad_norm_: no tensors")
    parts = [ops.grad_sumsq(t) for t in ts]          # (argument checks: contiguous f32 on a GPU)
    sumsq = parts[0] if len(parts) == 1 else torch.cat(parts).sum(dtype=torch.float64).float().reshape(1)
    coef = clip_coef(sumsq, float(max_norm)).reshape(())
    for t in ts:
        t.mul_(coef)
    return torch.sqrt(sumsq).reshape(())


def pack_adamw_slots(rows) -> torch.Tensor:
    """rows of (p, g, m, v addresses, n, weight_decay) -> the int64 [len, 6] image of `struct vl_adamw_slot[]` (host tensor):
    four pointers, the element count, and the f32 bits of the weight decay in the low half of the last word."""
    import struct
    t = torch.empty(len(rows), 6, dtype=torch.int64)
    for i, (p, g, m, v, n, wd) in enumerate(rows):
        t[i] = torch.tensor([p, g, m, v, n, struct.unpack("<I", struct.pack("<f", wd))[0]], dtype=torch.int64)
    return t


def pack_adamw_groups(rows) -> torch.Tensor:
    """rows of (lr_scale, no_clip) -> the int32 [len, 2] image of `struct vl_adamw_group[]` (host tensor): the f32 bits of the
    scale, then the flag."""
    import struct
    return torch.tensor([[struct.unpack("<i", struct.pack("<f", ls))[0], int(bool(nc))] for ls, nc in rows],
                        dtype=torch.int32).reshape(len(rows), 2)


def _f32_mul(a: float, b: float) -> float:
    """a * b as the kernels form it: both operands and the product rounded to fp32."""
    import struct
    r = lambda x: struct.unpack("<f", struct.pack("<f", x))[0]
    return r(r(a) * r(b))


class AdamW:
    """torch.optim.AdamW semantics on f32 master tensors, one fused kernel launch per tensor
    (reference: depth_tri_main.py:394-419 -- two groups: no weight decay for ndim<2 / bn / ln / bias / logit_scale).
    `step(..., max_norm=c)` clips the global gradient norm first (torch.nn.utils.clip_grad_norm_(params, c), the reference's
    --grad-clip-norm / training.grad_clip_norm) and updates every tensor in ONE launch; the norm and the coefficient stay
    on the device, `last_grad_norm` holds the unclipped norm.

    Parameter groups, per tensor by name: `lr_scale` {name: s} - the tensor steps with lr * s (torch's groups with an lr of
    their own; `lr` stays what a scheduler assigns); `no_clip` names - tensors outside clip_grad_norm_'s parameter list: they
    are updated unclipped and their gradients are not in the norm; `decay` {name: bool} - overrides `decays` (a master whose
    name is not the reference parameter's).  Defaults: 1.0, clipped, `decays`.  With any of the first two given the clipped
    step is vl_adamw_multi_step_groups, and `sumsq` (where the caller passes it) is the squared norm of the clipped set."""

    def __init__(self, params: Dict[str, torch.Tensor], lr=5e-4, betas=(0.9, 0.98), eps=1e-6, weight_decay=0.2,
                 lr_scale: Optional[Dict[str, float]] = None, no_clip: Iterable[str] = (), decay: Optional[Dict[str, bool]] = None):
        self.lr_scale, self.no_clip, self.decay = dict(lr_scale or {}), frozenset(no_clip), dict(decay or {})
        for k in (*self.lr_scale, *self.no_clip, *self.decay):
            if k not in params:
                raise ValueError(f"AdamW: {k!r} is not a parameter of this optimizer")
        for k, v in self.lr_scale.items():
            if not (math.isfinite(float(v)) and float(v) >= 0.0):
                raise ValueError(f"AdamW: lr_scale of {k} must be finite and >= 0, got {v}")
        self._grouped = bool(self.no_clip) or any(float(v) != 1.0 for v in self.lr_scale.values())
        self._groups = self._groups_host = None
        self._slots, self._slot_key = None, None      # the device table of the clipped step, kept while no tensor moves
        self.last_grad_norm = None                    # 0-d f32 device tensor after a clipped step
        # `param_groups[i]["lr"]` is what the reference's schedulers assign (training/scheduler.py:4-6); one group here,
        # weight decay is decided per tensor by `decays`
        self.param_groups = [{"lr": lr}]
        self.params, self.betas, self.eps, self.wd = params, betas, eps, weight_decay
        self.m = {k: torch.zeros_like(v) for k, v in params.items()}
        self.v = {k: torch.zeros_like(v) for k, v in params.items()}
        self.t = 0

    @property
    def lr(self) -> float:
        return float(self.param_groups[0]["lr"])

    @lr.setter
    def lr(self, value):
        self.param_groups[0]["lr"] = float(value)

    @staticmethod
    def decays(name: str, p: torch.Tensor) -> bool:
        return not (p.ndim < 2 or "bn" in name or "ln" in name or "bias" in name or "logit_scale" in name)

    def slot_rows(self, grads: Dict[str, torch.Tensor]):
        """One (p, g, m, v addresses, n, weight_decay) row per parameter that has a gradient, in `params` order."""
        rows = []
        for k, p in self.params.items():
            g = grads.get(k)
            if g is None:
                continue
            for t in (p, g, self.m[k], self.v[k]):
                if t.dtype != torch.float32 or not t.is_contiguous():
                    raise ValueError(f"AdamW: contiguous f32 tensors required ({k})")
            if g.numel() != p.numel():
                raise ValueError(f"AdamW: gradient of {k} has {g.numel()} elements, the parameter {p.numel()}")
            rows.append((p.data_ptr(), g.data_ptr(), self.m[k].data_ptr(), self.v[k].data_ptr(), p.numel(), self._wd(k, p)))
        return rows

    def _wd(self, k, p) -> float:
        return self.wd if self.decay.get(k, self.decays(k, p)) else 0.0

    def group_rows(self, grads: Dict[str, torch.Tensor]):
        """One (lr_scale, no_clip) row per row of `slot_rows`."""
        return [(float(self.lr_scale.get(k, 1.0)), k in self.no_clip) for k in self.params if grads.get(k) is not None]

    def _clipped_step(self, grads, grad_scale, max_norm, sumsq):
        if not float(max_norm) > 0.0:
            raise ValueError(f"AdamW.step: max_norm must be positive, got {max_norm}")
        rows = self.slot_rows(grads)
        if not rows:
            return
        dev = next(iter(self.params.values())).device
        key = tuple(rows)
        if key != self._slot_key:          # first step, or a tensor was re-allocated: one small host-to-device copy
            self._slots, self._slot_key = pack_adamw_slots(rows).to(dev), key
            if self._grouped:
                self._groups_host = pack_adamw_groups(self.group_rows(grads))
                self._groups = self._groups_host.to(dev)
        if sumsq is None:                  # gradients in separate allocations: one reduction each, added on the device
            parts = [ops.grad_sumsq(g) for k, g in grads.items() if k in self.params and g is not None and k not in self.no_clip]
            sumsq = torch.cat(parts).sum(dtype=torch.float64).float().reshape(1)
        if self.last_grad_norm is None:
            self.last_grad_norm = torch.zeros((), device=dev, dtype=torch.float32)
        self.t += 1
        for a in range(0, len(rows), ops.ADAMW_MAX_SLOTS):
            n = min(ops.ADAMW_MAX_SLOTS, len(rows) - a)
            if self._grouped:
                ops.adamw_multi_step_groups(self._slots[a:a + n], self._groups[a:a + n], self._groups_host[a:a + n], n, self.lr,
                                            self.betas[0], self.betas[1], self.eps, self.t, grad_scale, max_norm, sumsq,
                                            self.last_grad_norm)
                continue
            ops.adamw_multi(self._slots[a:a + n], n, self.lr, self.betas[0], self.betas[1], self.eps, self.t, grad_scale,
                            max_norm, sumsq, self.last_grad_norm)

    def step(self, grads: Dict[str, torch.Tensor], grad_scale: float = 1.0, max_norm: Optional[float] = None,
             sumsq: Optional[torch.Tensor] = None):
        """max_norm=None: the per-tensor loop.  With a max_norm: the gradients' global 2-norm (of grad_scale * g) is clipped to
        it; `sumsq` is the squared norm of ALL gradients as `ops.grad_sumsq` leaves it on the device (the fused steps pass the
        one of their flat buffer; None = computed here, one reduction per tensor)."""
        if max_norm is not None:
            return self._clipped_step(grads, grad_scale, max_norm, sumsq)
        self.t += 1
        for k, p in self.params.items():
            g = grads.get(k)
            if g is None:
                continue
            wd = self._wd(k, p)
            lr = _f32_mul(self.lr, self.lr_scale[k]) if k in self.lr_scale else self.lr
            ops.adamw_step(p.view(-1), g.view(-1), self.m[k].view(-1), self.v[k].view(-1), lr, self.betas[0],
                           self.betas[1], self.eps, wd, self.t, grad_scale)


# ------------------------------------------------------------------------------------------------
# Perceiver ("Lens") training: autograd of Perceiver.forward (open_clip/perceiver.py:289-328)
# ------------------------------------------------------------------------------------------------
def at_path(node, path):
    """node[path[0]][path[1]]... of a nest of dicts and lists."""
    for k in path:
        node = node[k]
    return node


class PerceiverTrainer:
    def __init__(self, pe, param_prefix: str = "visual.perceiver."):
        if pe.arith.dtype != BF:
            raise ValueError("PerceiverTrainer needs a PerceiverEngine with bf16 operands")
        self.pe, self.P = pe, param_prefix
        self.grads: Dict[str, torch.Tensor] = {}
        # transposed bf16 weights for the dX GEMMs (C = dY . W  ==  NT GEMM against W^T); tied layers
        # (perceiver_weight_tie_layers) share one entry
        self.wT = []
        for li, lay in enumerate(pe.layers):
            if self.layer_name(li) != li:
                self.wT.append(self.wT[1])
                continue
            d = {"x": {}, "xff": {}, "selfs": [{} for _ in lay["selfs"]]}
            for path, operand in self.wT_table(len(lay["selfs"])):
                w = at_path(lay, operand)
                at_path(d, path[:-1])[path[-1]] = w.new_empty(w.shape[1], w.shape[0])
            self.wT.append(d)
        self.refresh_derived()
        self._st = {}
        self.drop = None          # the last forward's dropout draw (engine.LensDrop), redrawn by the backward

    @staticmethod
    def wT_table(n_selfs: int):
        """(key path in wT[li], key path of the operand in pe.layers[li]) of every transposed weight of one layer."""
        t = [(("x", "q"), ("x_attn", "q_w")), (("x", "kv"), ("x_attn", "kv_w")), (("x", "out"), ("x_attn", "to_out_w")),
             (("xff", "w0"), ("x_ff", "w0")), (("xff", "w2"), ("x_ff", "w2"))]
        for j in range(n_selfs):
            t += [(("selfs", j, "qkv"), ("selfs", j, "attn", "qkv_w")), (("selfs", j, "out"), ("selfs", j, "attn", "to_out_w")),
                  (("selfs", j, "w0"), ("selfs", j, "ff", "w0")), (("selfs", j, "w2"), ("selfs", j, "ff", "w2"))]
        return t

    def refresh_derived(self):
        """The Perceiver engine's operands were set or updated in place: (re)do the transposes."""
        for li, lay in enumerate(self.pe.layers):
            if self.layer_name(li) == li:
                for path, operand in self.wT_table(len(lay["selfs"])):
                    at_path(self.wT[li], path).copy_(at_path(lay, operand).t())

    def grad_buffer(self, name, shape):
        g = self.grads.get(name)
        if g is None:
            g = torch.zeros(tuple(shape), device=self.pe.device, dtype=torch.float32)
            self.grads[name] = g
        return g

    def layer_name(self, li: int) -> int:
        """Index under which layer li's parameters are named: tied layers (>= 2) are layer 1's modules, so their
        gradients accumulate in layer 1's buffers (what autograd does for the reference's shared modules)."""
        return 1 if li >= 2 and self.pe.layers[li] is self.pe.layers[1] else li

    def _state(self, B, Tc):
        key = (B, Tc)
        if key in self._st:
            return self._st[key]
        c, dev = self.pe.cfg, self.pe.device
        R, D = B * c.num_latents, c.latent_dim
        f32 = lambda *s: torch.empty(*s, device=dev, dtype=torch.float32)
        bf = lambda *s: torch.empty(*s, device=dev, dtype=BF)
        st = {"X": [f32(R, D) for _ in range(_engine.perceiver_residuals(c))],
              "dx": f32(R, D), "dxb": bf(R, D), "dh8": bf(R, 8 * D), "dhn": bf(R, D), "dqkv": bf(R, 3 * c.latent_heads * c.latent_dim_head),
              "dq": bf(R, c.cross_heads * c.cross_dim_head), "dkv": bf(B * Tc, 2 * c.cross_heads * c.cross_dim_head),
              "dctx": bf(B * Tc, c.input_chan), "ddata": f32(B * Tc, c.input_chan)}
        # (kept per sub-layer for the backward's weight gradients: every LayerNorm output `hn` / `cn` and every GEGLU output
        #  `hid` - recomputing them was 2 % of the C4 step's kernel time for 2-7 GB of a 288 GB card)
        st["layers"] = _engine.perceiver_slots(c, B, Tc, dev, BF, X=st["X"])[1]
        self._st[key] = st
        return st

    # ---- forward ----------------------------------------------------------------------------------
    def forward(self, data: torch.Tensor, B: int, drop=None) -> torch.Tensor:
        """engine.perceiver_forward into the per-sub-layer slots: residual snapshots, LayerNorm outputs and statistics,
        projection outputs, lse, GEGLU pre-activation and output are what the backward reads.  drop (engine.LensDrop, from
        PerceiverEngine.draw): this forward's dropout; the backward keeps the numbers and redraws the masks from them."""
        pe, c = self.pe, self.pe.cfg
        st = self._state(B, data.shape[0] // B)
        st["X"][0].view(B, c.num_latents, c.latent_dim).copy_(pe.latents)
        _engine.perceiver_forward(pe.layers, st["layers"], data, B, c, pe.arith, drop)
        self.ctx = (B, data.shape[0] // B, data)
        self.drop = drop
        return st["X"][-1]

    # ---- backward ---------------------------------------------------------------------------------
    def _dw(self, name, dy, x):
        ops.weight_grad(dy, x, self.grad_buffer(name, (dy.shape[1], x.shape[1])), cfg=self.pe.gemm_cfg)

    def _ln_params(self, name, dy, x, stats, rows, D):
        ops.layernorm_bwd_params(dy, x, stats[0], stats[1], self.grad_buffer(name + ".weight", (D,)),
                                 self.grad_buffer(name + ".bias", (D,)), rows, D)

    def _ff_bwd(self, st, s, norm, wT, pname, sub=0):
        """x1 = x0 + W2 geglu(W0 LN(x0) + b0) + b2 on the slots `s` ; st['dx'] holds dL/dx1 on entry, dL/dx0 on exit.
        s.hn = LN(x0), s.h = the GEGLU's pre-activation, s.hid = geglu(...) as the forward left them.  With ff dropout
        (sub = the sub-layer's position in the forward) the branch sees the masked, scaled gradient, the residual the whole."""
        cfg, (rows, D) = self.pe.gemm_cfg, s.x0.shape
        # (dy = the bf16 copy of the residual gradient the dX GEMMs read: token-major operands for the dW kernel - the fp32
        #  stream would be rounded to the same bf16 values on its way through a transposed copy)
        drop = self.drop
        if drop is not None and drop.pf > 0.0:
            # st['dxb'] becomes the branch gradient dx1 M / (1 - pf) (the LayerNorm backward below rewrites it): dW2 and the
            # dGEGLU GEMM read that one; db2 is the column sum of its unrounded copy, in the forward's free s.y (p = 0 sums
            # the fp32 residual gradient there, not a bf16 copy)
            n = self.pe.cfg.num_latents
            ops.ff_drop_bwd(st["dx"], st["dxb"], rows // n, n, drop.pf, drop.seed, drop.sample0, sub, dy_f32=s.y)
            self._dw(pname + "1.fn.net.2.weight", st["dxb"], s.hid)
            ops.colsum(s.y, self.grad_buffer(pname + "1.fn.net.2.bias", (D,)))
        else:
            self._dw(pname + "1.fn.net.2.weight", st["dxb"], s.hid)
            ops.colsum(st["dx"], self.grad_buffer(pname + "1.fn.net.2.bias", (D,)))
        ops.gemm(st["dxb"], wT["w2"], None, out=st["dh8"], res=s.h, epi=ops.EPI_DGEGLU, cfg=cfg)     # d(pre-activation), interleaved
        self._dw(pname + "1.fn.net.0.weight_il", st["dh8"], s.hn)
        ops.colsum(st["dh8"], self.grad_buffer(pname + "1.fn.net.0.bias_il", (8 * D,)))
        ops.gemm(st["dh8"], wT["w0"], None, out=st["dhn"], epi=ops.EPI_BF16, cfg=cfg)
        self._ln_params(pname + "1.norm", st["dhn"], s.x0, s.stats, rows, D)
        ops.layernorm_bwd(st["dhn"], s.x0, s.stats[0], s.stats[1], norm[0], rows, D, dres=st["dx"], dx=st["dx"], dx_bf16=st["dxb"])

    def _attn_bwd(self, st, s, norm, wT, pname, dq, dkv=None, data=None, norm_ctx=None, sub=0):
        """x1 = x0 + to_out(attn(to_q(LN(x0)), to_kv(context))) on the slots `s` ; st['dx'] holds dL/dx1 on entry, dL/dx0 on exit.
        Latent self-attention (dkv None; the context is LN(x0) itself): dq is the packed [dq|dk|dv], one to_qkv gradient with
        rows [to_q ; to_kv].  Cross attention: dq and dkv = [dk|dv] apart, and the context side LN_ctx(data) -> to_kv, whose
        input gradient is ADDED to st['ddata'] (every cross layer reads the same data)."""
        cfg, (rows, D), inner = self.pe.gemm_cfg, s.x0.shape, s.a.shape[1]
        packed = dkv is None
        self._dw(pname + "0.fn.to_out.weight", st["dxb"], s.a)
        ops.colsum(st["dx"], self.grad_buffer(pname + "0.fn.to_out.bias", (D,)))
        ops.gemm(st["dxb"], wT["out"], None, out=s.dOm, epi=ops.EPI_BF16, cfg=cfg)
        dk, dv, lds = (dq[:, inner:], dq[:, 2 * inner:], (3 * inner, 3 * inner)) if packed else (dkv, dkv[:, inner:], (inner, 2 * inner))
        drop = self.drop
        if drop is not None and drop.pa > 0.0:
            # (the two-kernel backward also where p = 0 has the one-kernel one: sub = the sub-layer's position in the forward)
            ops.attn_bwd_drop(s.q, s.k, s.v, s.dO, s.av, s.lse, s.delta, dq, dk, dv, *lds, drop.pa, drop.seed, drop.sample0, sub)
        else:
            ops.attn_bwd(s.q, s.k, s.v, s.dO, s.av, s.lse, s.delta, dq, dk, dv, *lds)
        # query side: LN(x0) -> to_q (packed: -> [to_q ; to_kv])
        self._dw(pname + ("0.fn.to_qkv.weight" if packed else "0.fn.to_q.weight"), dq, s.hn)
        ops.gemm(dq, wT["qkv" if packed else "q"], None, out=st["dhn"], epi=ops.EPI_BF16, cfg=cfg)
        self._ln_params(pname + "0.norm", st["dhn"], s.x0, s.stats, rows, D)
        ops.layernorm_bwd(st["dhn"], s.x0, s.stats[0], s.stats[1], norm[0], rows, D, dres=st["dx"], dx=st["dx"], dx_bf16=st["dxb"])
        if packed:
            return
        crows, C = data.shape
        self._dw(pname + "0.fn.to_kv.weight", dkv, s.cn)
        ops.gemm(dkv, wT["kv"], None, out=st["dctx"], epi=ops.EPI_BF16, cfg=cfg)
        self._ln_params(pname + "0.norm_context", st["dctx"], data, s.cstats, crows, C)
        ops.layernorm_bwd(st["dctx"], data, s.cstats[0], s.cstats[1], norm_ctx[0], crows, C, dres=st["ddata"], dx=st["ddata"])

    def backward(self, dlat: torch.Tensor) -> torch.Tensor:
        """dlat f32 [B*n, D] = dL/d(latent output) -> returns dL/d(data) f32 [B*Tc, C]; fills self.grads
        (GEGLU first-layer gradients are kept in the kernels' interleaved row order under '*_il' names)."""
        pe, c = self.pe, self.pe.cfg
        B, Tc, data = self.ctx
        st = self._state(B, Tc)
        st["dx"].copy_(dlat)
        ops.cast_bf16(st["dx"], out=st["dxb"])
        st["ddata"].zero_()
        for li in reversed(range(c.depth)):
            lay, S, wT = pe.layers[li], st["layers"][li], self.wT[li]
            pn = f"{self.P}layers.{self.layer_name(li)}."
            for sj in reversed(range(c.self_per_cross)):
                sl, T, w = lay["selfs"][sj], S["selfs"][sj], wT["selfs"][sj]
                self._ff_bwd(st, T["ff"], sl["ff_norm"], w, f"{pn}2.{sj}.", sub=_engine.lens_sublayer(c, li, sj, ff=True))
                self._attn_bwd(st, T["attn"], sl["norm"], w, f"{pn}2.{sj}.", st["dqkv"], sub=_engine.lens_sublayer(c, li, sj))
            self._ff_bwd(st, S["x_ff"], lay["x_ff_norm"], wT["xff"], pn, sub=_engine.lens_sublayer(c, li, ff=True))
            self._attn_bwd(st, S["x_attn"], lay["x_norm"], wT["x"], pn, st["dq"], st["dkv"], data, lay["x_norm_ctx"],
                           sub=_engine.lens_sublayer(c, li))
        n, D = c.num_latents, c.latent_dim
        ops.batch_rowsum(st["dx"], self.grad_buffer(self.P + "latents", (n, D)), B, n, D, n, 0)
        return st["ddata"]

    def reference_named_grads(self, grads: Optional[Dict[str, torch.Tensor]] = None) -> Dict[str, torch.Tensor]:
        """Gradients under the reference's parameter names/layouts (de-interleaved GEGLU, split to_q/to_kv); `grads`: another
        dictionary in the kernels' layout (a fused step's merged buffer) instead of this trainer's own."""
        out = {}
        c = self.pe.cfg
        for k, g in (self.grads if grads is None else grads).items():
            if k.endswith(("net.0.weight_il", "net.0.bias_il")):
                out[k[:-3]] = deinterleave_geglu(g)
            elif k.endswith("to_qkv.weight"):
                inner = c.latent_heads * c.latent_dim_head
                out[k.replace("to_qkv", "to_q")] = g[:inner]; out[k.replace("to_qkv", "to_kv")] = g[inner:]
            else:
                out[k] = g
        return out


class AudioLensTrainer:
    """`visual.` tower of the audio recipe (TRAIN_INFERENCE.md:283-299): AST tokenizer + Perceiver trainable,
    ViT blocks locked, class_embedding unlocked (--lock-visual --unlock-cls)."""

    conv_w_name = "visual.visual_adapter.conv1.weight_gemm"

    def __init__(self, lens_engine, tower_kw=None):
        self.le = lens_engine
        kw = dict(train_blocks=(), train_cls=True) if tower_kw is None else dict(tower_kw)
        self.tower = TowerTrainer(lens_engine.vit, param_prefix="visual.", **kw)
        self.perc = PerceiverTrainer(lens_engine.perceiver, "visual.perceiver.")
        self.perc.grads = self.tower.grads            # one gradient dictionary
        self.ctx = None

    @property
    def grads(self):
        return self.tower.grads

    def _conv_bias_grad(self, ddata):
        pass                                          # (the AST convolution's bias is not in the trainable set)

    def forward(self, x: torch.Tensor, keep=None, inv=None, drop=None) -> torch.Tensor:
        """keep / inv: patch dropout on the Perceiver's latents, the tokens that enter the ViT trunk; tokenizer and Perceiver
        stay dense.  drop (PerceiverEngine.draw): the Perceiver's own attention / FeedForward dropout."""
        le = self.le
        B = x.shape[0]
        cols = le.cols(x)                             # (the im2col rows bf16 [B*T, Kp], which the backward keeps)
        tok = le.conv_tokens(cols)
        T = tok.shape[0] // B
        xin = torch.empty_like(tok)
        ops.add_rows(tok, le.adapter_pos, xin, tok.shape[0], T, tok.shape[1])
        lat = self.perc.forward(xin, B, drop)
        self.ctx = (cols, B, T)
        return self.tower.forward(lat, B, keep=keep, inv=inv)

    def backward(self, dfeat: torch.Tensor):
        cols, B, T = self.ctx
        dlat = self.tower.backward(dfeat)
        ddata = self.perc.backward(dlat)                          # f32 [B*T, D]: gradient of tokens + pos
        D = ddata.shape[1]
        g = self.tower.grad_buffer(self.conv_w_name, torch.empty(D, cols.shape[1]))
        conv_weight_grad(ddata, cols, g, self.le.gemm_cfg)
        self._conv_bias_grad(ddata)
        ops.batch_rowsum(ddata, self.tower.grad_buffer("visual.visual_adapter.pos_emb", self.le.adapter_pos), B, T, D, T, 0)


class EEGLensTrainer(AudioLensTrainer):
    """`visual.` tower of the EEG recipe (mm_vit_lens/model_cfg.py:153-178): PatchEmbed1D (Conv1d with bias over the
    time axis) + pos_emb + Perceiver trainable in front of the locked ViT - the audio recipe with a 1-D tokenizer."""

    conv_w_name = "visual.visual_adapter.proj.weight_gemm"

    def _conv_bias_grad(self, ddata):
        ops.colsum(ddata, self.tower.grad_buffer("visual.visual_adapter.proj.bias", self.le.conv_b))


class PCLensTrainer:
    """`visual.` tower of the point-cloud recipe: PointBERT tokenizer + Perceiver trainable, ViT blocks locked.
    `tok` is the shared PointTokenizerTrainer (masters, bf16 operands, running statistics); each micro-batch gets
    a shallow copy that only owns its saved activations."""

    def __init__(self, lens_engine, tok, train_cls: bool = False, tower_kw=None):
        import copy
        self.le = lens_engine
        kw = dict(train_blocks=(), train_cls=train_cls) if tower_kw is None else dict(tower_kw)
        self.tower = TowerTrainer(lens_engine.vit, param_prefix="visual.", **kw)
        self.perc = PerceiverTrainer(lens_engine.perceiver, "visual.perceiver.")
        self.perc.grads = self.tower.grads
        self.tok = copy.copy(tok)
        self.tok.ctx = None
        self.tok.grads = self.tower.grads

    @property
    def grads(self):
        return self.tower.grads

    def forward(self, pts: torch.Tensor, fps_start=None, keep=None, inv=None, drop=None, **kw) -> torch.Tensor:
        """pts [B,N,3] (PointBERT tokenizer) or point features [B,N,in_dim] with xyz=[B,N,3] (pnsa tokenizer).
        keep / inv: patch dropout on the Perceiver's latents (TowerTrainer.forward); drop: the Perceiver's own dropout
        (PerceiverEngine.draw)."""
        B = pts.shape[0]
        ctx = self.tok.forward(pts, fps_start=fps_start, **kw)    # tokens (+ pos), bf16 [B*G, C]
        return self.tower.forward(self.perc.forward(ctx, B, drop), B, keep=keep, inv=inv)

    def backward(self, dfeat: torch.Tensor, on_block_done=None):
        """on_block_done: `TowerTrainer.backward`'s, for a recipe with unlocked blocks (tower_kw train_blocks)."""
        self.tok.backward(self.perc.backward(self.tower.backward(dfeat, on_block_done)))


def refresh_trainer(tr, sd, names):
    """After the engine under trainer `tr` was updated in place for the parameters `names` (relative to the tower prefix):
    refresh what the trainer derived from them - transposed weights, the point tokenizer's masters - keeping the trainer
    and its activation buffers (a rebuild re-allocates tens of GB at ViT-L size)."""
    names = _engine.eva_param_names(names)      # (a no-op on the CLIP tower's names)
    tower = getattr(tr, "tower", None)
    if tower is not None:
        tower.refresh_derived({int(n.split(".")[2]) for n in names if n.startswith("transformer.resblocks.")}, "proj" in names)
    perc = getattr(tr, "perc", None)
    if perc is not None and any(n.startswith("perceiver.") for n in names):
        perc.refresh_derived()
    tok = getattr(tr, "tok", None)
    if tok is not None and any(n.startswith("visual_adapter.") for n in names):
        tok.load_params(sd)
