"""True fp32 INFERENCE executors: what `precision="fp32"` of the reference's factory means (open_clip/factory.py:260-295,
training/precision.py:5-12 - no autocast, fp32 parameters, fp32 nn.Linear / attention).  Rounds 1-4 ran bf16 operands under
that precision and warned; these classes run every matrix product on gfx950's fp32-input MFMA (`vl_gemm_f32`, exact fmaf
chains, 157 TFLOP/s peak = 1/16 of the bf16 rate), attention in fp32 on the VALU (`vl_attn_fwd_f32`: head dims 32, 64 and the
multiples of 8 in (64, 128] - ViT-H-14's 80, ViT-bigG-14's 104), LayerNorm / token
assembly / embedding on the existing f32 kernels.  Forward only - a tower whose parameters require grad under an enabled
autograd keeps the bf16-operand trainers with fp32 residual and gradient streams (open_clip/model.py says so in
`precision_effective`).  Covered: the image / tactile towers (conv stem + ViT), the depth Lens with an identity Perceiver
(DepthTokenizer -> ViT) and the text tower wherever the head dim is one of those (f32_supported), and the Lenses with a
Perceiver - audio, EEG, point cloud (pointbert) and depth (LensEngineF32) - over such a trunk when the Perceiver's cross and
latent head dims are 32 or 64 (f32_lens_supported); anything else stays on the 16-bit engines.

Reference ops: VisionTransformer.forward (open_clip/transformer.py:723-792), ResidualAttentionBlock (:254-272),
TriCLIP.encode_text (open_clip/model.py:528-540), Perceiver.forward (open_clip/perceiver.py:289-328), PointTokenizer.forward
(modal_3d/models/pointbert/point_encoder.py:350-362)."""
from typing import Optional

import torch

from . import ops
from .engine import (LensCfg, PerceiverEngine, TextCfg, TowerCfg, VitEngine, _dev, _Workspace, block_operands, conv_weight_as_gemm,
                     deinterleave_geglu, interleave_geglu, lens_cols, text_features)  # noqa: F401  (the two GEGLU helpers: re-exported)


def f32_head_dim_ok(dh: int) -> bool:
    """The head dims vl_attn_fwd_f32 takes: 32, 64, or a multiple of 8 in (64, 128] (ViT-H-14: 80, ViT-bigG-14: 104)."""
    return dh in (32, 64) or (64 < dh <= 128 and dh % 8 == 0)


def f32_supported(width: int, heads: int) -> bool:
    return width % heads == 0 and f32_head_dim_ok(width // heads) and width % 4 == 0


class F32Arith:
    """engine.Bf16Arith in fp32: every matrix product on the fp32-input MFMA (the GEGLU FeedForward's first Linear as ONE GEMM
    with the GEGLU epilogue, vl_gemm_f32_ex), attention on vl_attn_fwd_f32.  Inference only: no second outputs, no dropout."""
    dtype = torch.float32
    ln = staticmethod(ops.layernorm)

    def linear(self, a, w, b, out, res=None, act=ops.ACT_NONE, out2=None):
        ops.gemm_f32(a, w, b, out=out, res=res, act=act)

    def geglu(self, a, w, b, out, out2=None):
        ops.gemm_f32_ex(a, w, b, out=out, geglu=True)

    def attn(self, q, k, v, out, lse, dh, causal=False):
        ops.attn_fwd_f32(q, k, v, out, causal=causal, scale=dh ** -0.5)

    def linear_f32(self, a, w, b, out=None):
        return ops.gemm_f32(a, w, b, out=out)


def conv_as_gemm_f32(w: torch.Tensor, device="cpu") -> torch.Tensor:
    """Conv weight [O, C, *kernel] -> f32 [O, Kp] (K = C * prod(kernel) zero-padded to a multiple of 64, as the 16-bit stem
    lays it out; column order (c, i, j) = im2col's)."""
    return conv_weight_as_gemm(w, device, torch.float32)


def fold_bn_f32(w, b, gamma, beta, running_mean, running_var, eps=1e-5):
    """Eval-mode BatchNorm after a 1x1 conv, folded into it IN FP32: bn(x W^T + b) = x (s W)^T + (b - mean) s + beta with
    s = gamma / sqrt(var + eps) (dvae.py:183-194 in eval mode).  -> (W' [O, K], b' [O]) f32."""
    f = lambda t: t.detach().float()
    s = f(gamma) / torch.sqrt(f(running_var) + eps)
    return f(w) * s[:, None], (f(b) - f(running_mean)) * s + f(beta)


def pad_k4(w: torch.Tensor) -> torch.Tensor:
    """[O, K] -> f32 [O, K rounded up to a multiple of 4], zero columns (the fp32 GEMM reads 16-byte rows)."""
    K = w.shape[1]
    out = torch.zeros(w.shape[0], (K + 3) // 4 * 4, dtype=torch.float32, device=w.device)
    out[:, :K] = w.float()
    return out


def f32_lens_supported(tower: TowerCfg, lens: Optional[LensCfg]) -> bool:
    """Does LensEngineF32 take this `visual` tower?  Audio / EEG / pointbert point cloud / depth, a trunk that f32_supported
    takes (head dim 32, 64 or a multiple of 8 in (64, 128]), Perceiver cross and latent head dims 32 or 64, widths that the fp32
    GEMM's 16-byte rows take.  pnsa, other head dims, other modalities: no (they keep the 16-bit engines)."""
    if lens is None or lens.modality not in ("audio", "eeg", "pc", "depth"):
        return False
    if not f32_supported(tower.width, tower.heads):
        return False
    if lens.modality == "pc" and (lens.pc_tokenizer != "pointbert" or lens.perceiver_identity):
        return False
    if not lens.perceiver_identity:
        if lens.cross_dim_head not in (32, 64) or lens.latent_dim_head not in (32, 64):
            return False
        if lens.latent_dim % 4 or lens.input_chan % 4:
            return False
    return True


class VitEngineF32(VitEngine):
    """One ViT tower in fp32 - engine.VitEngine on fp32 operands, an fp32 stream and F32Arith: `image.` / `visual.` of TriCLIP for
    the image and tactile modalities, and - with `depth=True` - the depth Lens with an identity Perceiver (visual_adapter.conv1 +
    pos_emb in front of the same trunk).  A `visual.` tower of the other Lenses has no stem of its own: LensEngineF32 feeds
    `trunk` the Perceiver's latents."""

    def __init__(self, sd, prefix: str, cfg: TowerCfg, device, depth: bool = False, use_orig_pos: bool = True,
                 disable_adapter_pos: bool = False):
        if not f32_supported(cfg.width, cfg.heads):
            raise NotImplementedError("fp32 inference: head dim must be 32, 64 or a multiple of 8 in (64, 128]")
        super().__init__(sd, prefix, cfg, device, res_dtype=torch.float32, arith=F32Arith())
        self.depth, self.use_orig_pos, self.pos2 = depth, use_orig_pos, None
        if depth:
            a = prefix + "visual_adapter."
            self.conv_w = conv_as_gemm_f32(sd[a + "conv1.weight"], device)
            self.pos2 = _dev(sd[a + "pos_emb"].detach().float() * (0.0 if disable_adapter_pos else 1.0), device)

    def encode(self, x: torch.Tensor, normalize: bool = False, **kw) -> torch.Tensor:
        if self.conv_w is None:
            raise RuntimeError("VitEngineF32.encode: this tower has no conv stem (a Lens tower: use LensEngineF32)")
        p = self.cfg.patch
        cols, gh, gw = ops.im2col_f32(x.to(self.device).contiguous().float(), p, p, p, p, self.conv_w.shape[1])
        tok = ops.gemm_f32(cols, self.conv_w)
        f = self.trunk(tok, x.shape[0], pos2=self.pos2, use_orig_pos=self.use_orig_pos or not self.depth)
        return ops.l2_normalize(f) if normalize else f

    encode_image = encode


class TextEngineF32:
    """TriCLIP.encode_text in fp32 (model.py:528-540): embedding, causal transformer, ln_final at the EOT token, projection -
    engine.text_features on fp32 operands in F32Arith."""

    def __init__(self, sd, cfg: TextCfg, device):
        if not f32_supported(cfg.width, cfg.heads):
            raise NotImplementedError("fp32 inference: head dim must be 32, 64 or a multiple of 8 in (64, 128]")
        self.cfg, self.device = cfg, torch.device(device)
        self.tok = _dev(sd["token_embedding.weight"], device)
        self.pos = _dev(sd["positional_embedding"], device)
        self.ln_final = (_dev(sd["ln_final.weight"], device), _dev(sd["ln_final.bias"], device))
        self.projT = _dev(sd["text_projection"].t(), device)                                          # [E, D]
        self.blocks = [block_operands(sd, f"transformer.resblocks.{i}.", device, torch.float32) for i in range(cfg.layers)]
        self.arith = "f32"
        self._ws = {}

    def encode_text(self, text: torch.Tensor, normalize: bool = False) -> torch.Tensor:
        B, L = text.shape
        D, f32 = self.cfg.width, torch.float32
        if (B, L) not in self._ws:
            self._ws[B, L] = _Workspace(B, L, D, self.cfg.heads, 4 * D, self.device, f32, f32)
        f = text_features(self, F32Arith(), self._ws[B, L], text.to(self.device).contiguous())
        return ops.l2_normalize(f) if normalize else f


# ------------------------------------------------------------------------------------------------
# The Lenses with a Perceiver (audio, EEG, point cloud, depth): tokenizer -> (+pos) -> Perceiver -> trunk, all in fp32
# ------------------------------------------------------------------------------------------------
class PerceiverEngineF32(PerceiverEngine):
    """Perceiver.forward(return_embeddings=True) (open_clip/perceiver.py:289-328) in fp32: engine.perceiver_forward on fp32
    operands and an fp32 workspace in F32Arith.  data f32 [B*Tc, C] -> latents f32 [B*n, D]."""

    def __init__(self, sd, prefix: str, cfg: LensCfg, device):
        for dh in (cfg.cross_dim_head, cfg.latent_dim_head):
            if dh not in (32, 64):
                raise NotImplementedError("fp32 inference: Perceiver head dims must be 32 or 64")
        super().__init__(sd, prefix, cfg, device, arith=F32Arith())


def point_tokenizer_operands_f32(sd, a: str, eps: float = 1e-5):
    """fp32 operands of PointTokenizerEngineF32 from the reference's parameters (prefix `a` = "...visual_adapter."), on the
    device the parameters live on: the two eval-mode BatchNorms folded in fp32 into the convs before them, the 3-channel
    inputs zero-padded to K = 4, second_conv.0 split into its global (first half of the input channels: the broadcast group
    maximum, dvae.py:207-209) and local halves."""
    f = lambda k: sd[a + k].detach().float()
    bn = lambda k: [f(k + n) for n in (".weight", ".bias", ".running_mean", ".running_var")]
    w1, b1 = fold_bn_f32(f("encoder.first_conv.0.weight")[:, :, 0], f("encoder.first_conv.0.bias"), *bn("encoder.first_conv.1"), eps=eps)
    w3, b3 = fold_bn_f32(f("encoder.second_conv.0.weight")[:, :, 0], f("encoder.second_conv.0.bias"), *bn("encoder.second_conv.1"), eps=eps)
    half = w3.shape[1] // 2
    return {"w1": pad_k4(w1), "b1": b1, "w2": f("encoder.first_conv.3.weight")[:, :, 0], "b2": f("encoder.first_conv.3.bias"),
            "w3g": w3[:, :half], "w3l": w3[:, half:], "b3": b3,
            "w4": f("encoder.second_conv.3.weight")[:, :, 0], "b4": f("encoder.second_conv.3.bias"),
            "wr": f("reduce_dim.weight"), "br": f("reduce_dim.bias"),
            "wp0": pad_k4(f("pos_embed.0.weight")), "bp0": f("pos_embed.0.bias"), "wp2": f("pos_embed.2.weight"), "bp2": f("pos_embed.2.bias")}


class PointTokenizerEngineF32:
    """PointTokenizer.forward (point_encoder.py:350-362) in fp32, BatchNorm in eval mode: FPS (vl_fps, bit-exact fp32), kNN
    grouping into fp32 centred patches (vl_knn_group_f32: the 16-bit engine's neighbour sets), the mini-PointNet (dvae.py:
    196-212) with the BatchNorms folded in fp32, the two group maxima in fp32, reduce_dim, and the centre MLP with exact GELU.
    forward -> tokens + pos, f32 [B*G, trans_dim]."""

    def __init__(self, sd, a: str, lens: LensCfg, device):
        self.lens, self.device = lens, torch.device(device)
        self.op = {k: _dev(v, device) for k, v in point_tokenizer_operands_f32(sd, a).items()}

    def group(self, pts: torch.Tensor, fps_start=None, want_idx=False):
        L = self.lens
        pts = pts.to(self.device).contiguous().float()
        if fps_start is None:   # misc.py:60 draws the first centre at random
            fps_start = torch.randint(0, pts.shape[1], (pts.shape[0],), device=self.device, dtype=torch.long)
        cidx, centers = ops.fps(pts, fps_start.to(self.device), L.pc_num_group)
        patches, nidx = ops.knn_group_f32(pts, cidx, L.pc_group_size, Kp=self.op["w1"].shape[1], want_idx=want_idx)
        return cidx, centers, patches, nidx

    def forward(self, pts: torch.Tensor, fps_start=None) -> torch.Tensor:
        M, o = self.lens.pc_group_size, self.op
        _, centers, patches, _ = self.group(pts, fps_start)
        h1 = ops.gemm_f32(patches, o["w1"], o["b1"], act=ops.ACT_RELU)                       # conv 3->128 + BN + ReLU
        f = ops.gemm_f32(h1, o["w2"], o["b2"])                                               # conv 128->256
        t = ops.gemm_f32(ops.group_max_f32(f, M), o["w3g"], o["b3"])                         # global half of conv 512->512 (+ BN)
        h2 = ops.gemm_f32_ex(f, o["w3l"], None, res=t, res_div=M, res_pre=True, act=ops.ACT_RELU)   # + local half, ReLU
        tok = ops.gemm_f32(ops.group_max_f32(ops.gemm_f32(h2, o["w4"], o["b4"]), M), o["wr"], o["br"])
        p1 = ops.gemm_f32(ops.pad3_f32(centers, o["wp0"].shape[1]), o["wp0"], o["bp0"], act=ops.ACT_GELU)
        return ops.gemm_f32(p1, o["wp2"], o["bp2"], res=tok)                                 # tokens + pos


class LensEngineF32:
    """The `visual.` tower of a Lens under precision="fp32", eval mode (VisionTransformer.forward, transformer.py:723-792):
    audio (AST conv over [N,1,F,T] with f / t strides), EEG (PatchEmbed1D: Conv1d with bias), point cloud (pointbert) or depth
    tokens -> + adapter pos -> PerceiverEngineF32 -> VitEngineF32.trunk.  Every matrix product on the fp32-input MFMA."""

    def __init__(self, sd, prefix: str, tower: TowerCfg, lens: LensCfg, device):
        if not f32_lens_supported(tower, lens):
            raise NotImplementedError("fp32 inference: this Lens is not covered (f32_lens_supported)")
        self.tower, self.lens, self.device = tower, lens, torch.device(device)
        self.vit = VitEngineF32(sd, prefix, tower, device)
        a = prefix + "visual_adapter."
        scale = 0.0 if lens.disable_adapter_pos else 1.0
        self.adapter_pos = self.points = None
        if lens.modality in ("depth", "audio"):
            self.conv_w, self.conv_b = conv_as_gemm_f32(sd[a + "conv1.weight"], device), None
        elif lens.modality == "eeg":
            self.conv_w = conv_as_gemm_f32(sd[a + "proj.weight"].unsqueeze(2), device)
            self.conv_b = _dev(sd[a + "proj.bias"], device)
        else:
            self.points = PointTokenizerEngineF32(sd, a, lens, device)
        if self.points is None:
            self.adapter_pos = _dev(sd[a + "pos_emb"].detach().float() * scale, device)
        self.perceiver = None if lens.perceiver_identity else PerceiverEngineF32(sd, prefix + "perceiver.", lens, device)

    def tokens(self, x: torch.Tensor) -> torch.Tensor:
        """-> tokens f32 [B*T, width] of the depth / audio / EEG tokenizer (without the adapter pos)."""
        cols = lens_cols(ops.im2col_f32, x.to(self.device), self.lens, self.tower.patch, self.conv_w.shape[1])
        return ops.gemm_f32(cols, self.conv_w, self.conv_b)

    def encode(self, x: torch.Tensor, normalize: bool = False, fps_start=None, **kw) -> torch.Tensor:
        B = x.shape[0]
        if self.points is not None:
            tok = self.points.forward(x, fps_start)                   # tokens + pos, f32 [B*G, trans_dim]
        else:
            t = self.tokens(x)
            if self.perceiver is None:
                f = self.vit.trunk(t, B, pos2=self.adapter_pos, use_orig_pos=self.lens.use_orig_pos)
                return ops.l2_normalize(f) if normalize else f
            tok = torch.empty_like(t)
            ops.add_rows(t, self.adapter_pos, tok, t.shape[0], t.shape[0] // B, t.shape[1])
        lat = self.perceiver.forward(tok, B)
        f = self.vit.trunk(lat, B, use_orig_pos=self.lens.use_orig_pos)
        return ops.l2_normalize(f) if normalize else f
