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
from .engine import (LensCfg, LensEngine, PerceiverEngine, TextCfg, TowerCfg, VitEngine, _dev, _Workspace, block_operands,
                     conv_weight_as_gemm, deinterleave_geglu, interleave_geglu, text_features)  # noqa: F401  (the two GEGLU helpers: re-exported)
from .points import PointTokenizerEngine, fold_bn as fold_bn_f32, point_tokenizer_operands  # noqa: F401  (fold_bn_f32: its name here)


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

    point_kp = 4                # (the fp32 GEMM reads 16-byte rows)
    im2col, knn_group, group_max, pad3 = (staticmethod(f) for f in (ops.im2col_f32, ops.knn_group_f32, ops.group_max_f32, ops.pad3_f32))

    def linear_rowres(self, a, w, out, res, res_div, act=ops.ACT_NONE):
        ops.gemm_f32_ex(a, w, None, out=out, res=res, act=act, res_div=res_div, res_pre=True)


def conv_as_gemm_f32(w: torch.Tensor, device="cpu") -> torch.Tensor:
    """Conv weight [O, C, *kernel] -> f32 [O, Kp] (K = C * prod(kernel) zero-padded to a multiple of 64, as the 16-bit stem
    lays it out; column order (c, i, j) = im2col's)."""
    return conv_weight_as_gemm(w, device, torch.float32)


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
    """fp32 operands of PointTokenizerEngineF32: points.point_tokenizer_operands in fp32 with the 3-channel inputs zero-padded
    to K = 4, on the device the parameters live on."""
    return point_tokenizer_operands(sd, a, torch.float32, F32Arith.point_kp, eps)


class PointTokenizerEngineF32(PointTokenizerEngine):
    """PointTokenizer.forward (point_encoder.py:350-362) in fp32, BatchNorm in eval mode - points.pointbert_forward in F32Arith:
    FPS (vl_fps, bit-exact fp32), kNN grouping into fp32 centred patches (vl_knn_group_f32: the 16-bit engine's neighbour sets),
    the mini-PointNet (dvae.py:196-212) with the BatchNorms folded in fp32 where the parameters live, the two group maxima in
    fp32, reduce_dim, and the centre MLP with exact GELU.  forward -> tokens + pos, f32 [B*G, trans_dim]."""
    fold_on_host = False

    def __init__(self, sd, a: str, lens: LensCfg, device):
        super().__init__(sd, a, lens, device, arith=F32Arith())


class LensEngineF32(LensEngine):
    """The `visual.` tower of a Lens under precision="fp32", eval mode (VisionTransformer.forward, transformer.py:723-792) -
    engine.LensEngine on fp32 operands in F32Arith: audio (AST conv over [N,1,F,T] with f / t strides), EEG (PatchEmbed1D: Conv1d
    with bias), point cloud (pointbert) or depth tokens -> + adapter pos -> Perceiver -> trunk.  Every matrix product on the
    fp32-input MFMA."""

    def __init__(self, sd, prefix: str, tower: TowerCfg, lens: LensCfg, device):
        if not f32_lens_supported(tower, lens):
            raise NotImplementedError("fp32 inference: this Lens is not covered (f32_lens_supported)")
        super().__init__(sd, prefix, tower, lens, device, arith=F32Arith())

    def _point_tokenizer(self, sd):
        return PointTokenizerEngineF32(sd, self.prefix_adapter, self.lens, self.device)

    def encode(self, x: torch.Tensor, normalize: bool = False, fps_start=None, **kw) -> torch.Tensor:
        """The one body of LensEngine.encode, for an eval-mode forward.  Every other keyword is accepted and IGNORED, as it always
        was here: keep (patch dropout), drop (the Perceiver's dropout) and tokens_out belong to train-mode or token-stream
        forwards, which the fp32 engines do not run."""
        return self._encode(x, normalize, **({} if self.points is None else {"fps_start": fps_start}))
