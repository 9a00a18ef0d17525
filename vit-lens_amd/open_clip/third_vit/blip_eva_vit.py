"""`visual_arch = "perceiver_blip_eva_g_vit"`: the Lens (tokenizer + Perceiver) in front of the frozen BLIP-2 / InstructBLIP
EVA ViT-g, "trained for subsequent plug-in for MFM/MLLM".  Interface and parameter names of the reference's
open_clip/third_vit/blip_eva_vit.py; the arithmetic runs on the HIP engines (vitlens_hip.engine.EvaVitEngine on run_blocks).

    VisionTransformer        parameter holder of the EVA ViT: cls_token [1,1,D], pos_embed [1,L,D], blocks.N.{norm1, attn.{qkv,
                             q_bias, v_bias, proj}, norm2, mlp.{fc1, fc2}}, norm, head (nn.Linear(D, num_classes) or Identity)
    create_eva_vit_g         ViT-g: width 1408 = 16 heads x 88, MLP hidden int(1408 * 4.3637) = 6144, LayerNorm eps 1e-6,
                             qkv bias on q and v; loads `eva_vit_g.pth` from cache_dir when it is there - never from the network
    Perceiver_Blip_EVA_ViT   visual_adapter.* + perceiver.* + eva_vit.* + eva_vit_proj (a [D, E] Parameter, or eva_vit.head itself)

Out of scope here: modalities that keep EVA's patch embedding (image / video / tactile: its biased patch convolution), relative
position biases, layer scale (init_values), stochastic depth - none of which ViT-g as BLIP-2 ships it uses."""
import logging
import math
import os
from typing import Optional

import torch
import torch.nn as nn

from ..model import CLIPVisionCfg, VisionTransformer as _LensTower, _g

EVA_G = dict(embed_dim=1408, num_heads=16, mlp_ratio=4.3637, patch_size=14, eps=1e-6)
CKPT_NAME = "eva_vit_g.pth"


class _Holder(nn.Module):
    """Parameters only: the forward is the engine's."""


def _linear(i, o):
    m = nn.Linear(i, o)
    nn.init.trunc_normal_(m.weight, std=0.02)
    nn.init.zeros_(m.bias)
    return m


class Attention(_Holder):
    def __init__(self, dim, num_heads, qkv_bias=True):
        super().__init__()
        self.num_heads = num_heads
        self.qkv = nn.Linear(dim, 3 * dim, bias=False)
        nn.init.trunc_normal_(self.qkv.weight, std=0.02)
        self.q_bias = nn.Parameter(torch.zeros(dim)) if qkv_bias else None
        self.v_bias = nn.Parameter(torch.zeros(dim)) if qkv_bias else None
        self.proj = _linear(dim, dim)


class Mlp(_Holder):
    def __init__(self, dim, hidden):
        super().__init__()
        self.fc1, self.fc2 = _linear(dim, hidden), _linear(hidden, dim)


class Block(_Holder):
    def __init__(self, dim, num_heads, mlp_ratio, qkv_bias, eps):
        super().__init__()
        self.norm1 = nn.LayerNorm(dim, eps=eps)
        self.attn = Attention(dim, num_heads, qkv_bias)
        self.norm2 = nn.LayerNorm(dim, eps=eps)
        self.mlp = Mlp(dim, int(dim * mlp_ratio))


class VisionTransformer(_Holder):
    """The EVA ViT's parameters under the reference's names, initialised as the reference does: trunc-normal(0.02) Linear
    weights, cls_token and pos_embed, zero biases, unit LayerNorms, then `fix_init_weight` (attn.proj and mlp.fc2 of block l
    divided by sqrt(2 (l + 1)))."""

    def __init__(self, img_size=224, patch_size=14, embed_dim=1408, depth=40, num_heads=16, mlp_ratio=4.3637, qkv_bias=True,
                 num_classes=1024, eps=1e-6, num_tokens: Optional[int] = None):
        super().__init__()
        self.image_size, self.patch_size = img_size, patch_size
        self.embed_dim = self.num_features = embed_dim
        self.num_heads, self.mlp_ratio, self.eps, self.num_classes = num_heads, mlp_ratio, eps, num_classes
        L = (img_size // patch_size) ** 2 + 1 if num_tokens is None else num_tokens
        self.patch_embed = None            # (modalities that would keep it are refused by Perceiver_Blip_EVA_ViT)
        self.cls_token = nn.Parameter(torch.zeros(1, 1, embed_dim))
        self.pos_embed = nn.Parameter(torch.zeros(1, L, embed_dim))
        self.rel_pos_bias = None
        self.blocks = nn.ModuleList([Block(embed_dim, num_heads, mlp_ratio, qkv_bias, eps) for _ in range(depth)])
        self.norm = nn.LayerNorm(embed_dim, eps=eps)
        self.fc_norm = None
        self.head = _linear(embed_dim, num_classes) if num_classes > 0 else nn.Identity()
        nn.init.trunc_normal_(self.pos_embed, std=0.02)
        nn.init.trunc_normal_(self.cls_token, std=0.02)
        self.fix_init_weight()

    def fix_init_weight(self):
        for layer_id, blk in enumerate(self.blocks):
            blk.attn.proj.weight.data.div_(math.sqrt(2.0 * (layer_id + 1)))
            blk.mlp.fc2.weight.data.div_(math.sqrt(2.0 * (layer_id + 1)))

    def forward(self, *a, **k):
        raise NotImplementedError("the EVA ViT runs inside Perceiver_Blip_EVA_ViT on the HIP engines; on its own it would need "
                                  "its patch convolution, which is out of scope")


def load_eva_state(model: VisionTransformer, path: str):
    """load_state_dict(strict=False) of an EVA checkpoint: fp16 tensors are accepted (cast to the parameters' dtype), keys of
    the patch embedding are ignored, a position table of another size is refused."""
    sd = torch.load(path, map_location="cpu", weights_only=True)
    if "pos_embed" in sd and tuple(sd["pos_embed"].shape) != tuple(model.pos_embed.shape):
        raise ValueError(f"{path}: pos_embed is {tuple(sd['pos_embed'].shape)}, this tower has {tuple(model.pos_embed.shape)} - "
                         "interpolating the position table is not implemented; build the tower for the checkpoint's image size")
    sd = {k: v.float() if v.is_floating_point() else v for k, v in sd.items() if not k.startswith("patch_embed.")}
    return model.load_state_dict(sd, strict=False)


def create_eva_vit_g(img_size=224, depth=39, drop_path_rate=0.0, use_checkpoint=False, precision="fp32", use_nnlinear=True,
                     cache_dir: Optional[str] = None):
    """EVA ViT-g/14 (`depth` of its 40 blocks; BLIP-2 drops the last).  use_nnlinear: an nn.Linear(1408, 1024) head.  The
    weights are loaded from `cache_dir`/eva_vit_g.pth only when that file exists: nothing is ever fetched."""
    if drop_path_rate:
        raise NotImplementedError("create_eva_vit_g: stochastic depth (drop_path_rate > 0) is not implemented")
    model = VisionTransformer(img_size=img_size, patch_size=EVA_G["patch_size"], embed_dim=EVA_G["embed_dim"], depth=depth,
                              num_heads=EVA_G["num_heads"], mlp_ratio=EVA_G["mlp_ratio"], qkv_bias=True,
                              num_classes=1024 if use_nnlinear else 0, eps=EVA_G["eps"])
    if cache_dir is None:
        from ..constants import CKPT_CACHE_DIR as cache_dir      # noqa: N811
    path = os.path.join(str(cache_dir), CKPT_NAME)
    if os.path.exists(path):
        logging.info("EVA-ViT-g14: %s", load_eva_state(model, path))
    else:
        logging.info("EVA-ViT-g14: %s not found, the tower keeps its initialisation", path)
    return model


class Perceiver_Blip_EVA_ViT(_LensTower):
    """The Lens tower over an EVA ViT.  The Lens parameters (visual_adapter.*, perceiver.*) are built from `args` as in the
    CLIP tower - `visual_adapter` and `perceiver` are accepted as None only - at the EVA ViT's width."""

    def __init__(self, visual_adapter, perceiver, eva_vit: VisionTransformer, args=None, vision_cfg=None, **kwargs):
        if visual_adapter is not None or perceiver is not None:
            raise NotImplementedError("Perceiver_Blip_EVA_ViT builds its visual adapter and Perceiver from `args`: pass None for both")
        embed_dim = kwargs.pop("embed_dim")
        modality = str(_g(args, "visual_modality_type", "")).lower()
        if modality in ("image", "video", "tactile"):       # the reference's keep_patch_embed
            raise NotImplementedError(f"Perceiver_Blip_EVA_ViT: modality {modality!r} keeps the EVA ViT's patch embedding "
                                      "(keep_patch_embed): its biased patch convolution is out of scope, only Lens modalities "
                                      "(pc / audio / depth / eeg) run here")
        D = eva_vit.embed_dim
        latent = _g(args, "perceiver_latent_dim", D)
        if _g(args, "use_perceiver", True) and not _g(args, "perceiver_as_identity", False) and latent != D:
            raise ValueError(f"Perceiver_Blip_EVA_ViT: perceiver_latent_dim is {latent}, the EVA ViT's width is {D}: the latents "
                             f"enter the tower as its tokens, so the Perceiver latent dim must be {D}")
        cfg = CLIPVisionCfg(layers=len(eva_vit.blocks), width=D, head_width=D // eva_vit.num_heads, mlp_ratio=eva_vit.mlp_ratio,
                            patch_size=_g(vision_cfg, "patch_size", eva_vit.patch_size), image_size=_g(vision_cfg, "image_size", eva_vit.image_size),
                            visual_modality_type=_g(args, "visual_modality_type", "pc"), use_perceiver=bool(_g(args, "use_perceiver", True)),
                            visual_arch="perceiver_blip_eva_g_vit", exp_args=args, patch_dropout=0.0)
        object.__setattr__(self, "_eva_src", eva_vit)
        super().__init__(embed_dim, cfg)
        object.__delattr__(self, "_eva_src")
        self.args = args
        self.eva_vit = eva_vit
        self.keep_patch_embed = False
        n_tok = _g(args, "perceiver_num_latents", None) if self.use_perceiver else None
        if n_tok is not None and eva_vit.pos_embed is not None and eva_vit.pos_embed.shape[1] != n_tok + 1:
            raise ValueError(f"Perceiver_Blip_EVA_ViT: the EVA ViT has {eva_vit.pos_embed.shape[1]} positions (class token + patches), "
                             f"the Perceiver hands it {n_tok} latents: perceiver_num_latents must be {eva_vit.pos_embed.shape[1] - 1}")
        if isinstance(eva_vit.head, nn.Linear):
            self.eva_vit_proj = eva_vit.head                  # the SAME module: state_dict lists it under both names, as the reference's
        else:
            self.eva_vit_proj = nn.Parameter(D ** -0.5 * torch.randn(D, embed_dim))
        if _g(args, "disable_orig_pos", False):
            eva_vit.pos_embed = None
        skip = _g(args, "skip_trans_first_n_layers", None)
        if skip is not None:
            assert skip < len(eva_vit.blocks)
            n_keep = len(eva_vit.blocks) - skip
            logging.info("Using last %d out of %d transformer layers.", n_keep, len(eva_vit.blocks))
            eva_vit.blocks = eva_vit.blocks[-n_keep:]
            import dataclasses
            self.cfg = dataclasses.replace(self.cfg, layers=n_keep)

    # ---- the base class's view of the tower ------------------------------------------------------
    def _tower_params(self, D, n_tok, embed_dim):
        return {}                                             # the EVA ViT brings its own (attached as `eva_vit`)

    @property
    def class_embedding(self):
        return self.eva_vit.cls_token

    @property
    def positional_embedding(self):
        return self.eva_vit.pos_embed

    def _engine_names(self, names):
        from vitlens_hip.engine import eva_param_names
        return eva_param_names(names)

    def _module_grads(self, raw):
        from vitlens_hip.engine import eva_grads
        for pre in ("visual.", "t."):
            raw = eva_grads(raw, pre)
        return raw

    def _cfgs(self):
        from vitlens_hip import engine as E
        _, lens = super()._cfgs()
        tower = E.eva_tower_cfg(width=self.cfg.width, layers=len(self.eva_vit.blocks), heads=self.heads, embed_dim=self.embed_dim,
                                mlp_ratio=self.cfg.mlp_ratio, patch=self.cfg.patch_size, image_size=self.cfg.image_size)
        tower.ln_eps = float(self.eva_vit.eps)
        return tower, lens

    def _engine_f32(self):
        return None                                           # (the fp32 engines over an EVA tower are out of scope)

    def keep_last_layers(self, n_keep: int):
        raise NotImplementedError("Perceiver_Blip_EVA_ViT drops its first layers at construction (args.skip_trans_first_n_layers)")

    def drop_output_projection(self):
        raise NotImplementedError("Perceiver_Blip_EVA_ViT: the tower without output projection (OpenShape's CLIPBindWrap) is out of scope")

    def forward_tokens(self, x, **kwargs):
        """eva_vit.forward_features behind the Lens: the [B, L, D] stream in front of `norm`, without a graph."""
        x = x.to(self.class_embedding.device)
        with torch.no_grad():
            return self.engine().encode(x, tokens_out=True, **kwargs)

    # ---- lock --------------------------------------------------------------------------------------
    def lock(self, unlocked_groups=0, freeze_bn_stats=False, unlock_cls=False, unlock_pos_emb=False,
             unlock_trans_first_n_layers=None):
        """The reference's Perceiver_Blip_EVA_ViT.lock: everything frozen; the grouped unlock over [cls_token, pos_embed],
        one group per block but the last, [last block, norm] - the first k with args.unlock_from_head, else the last k; then
        always the Perceiver, the visual adapter and an eva_vit_proj that is a Parameter (a Linear head stays frozen), and what
        the three flags name."""
        for p in self.parameters():
            p.requires_grad = False
        self._freeze_bn = bool(freeze_bn_stats)
        ev = self.eva_vit

        def unlock(x):
            if x is None:
                return
            if isinstance(x, (list, tuple)):
                for y in x:
                    unlock(y)
            elif isinstance(x, nn.Parameter):
                x.requires_grad = True
            else:
                for p in x.parameters():
                    p.requires_grad = True
        if unlocked_groups != 0:
            first = [m for m in (ev.patch_embed, ev.cls_token, ev.pos_embed, ev.rel_pos_bias) if m is not None]
            last = [m for m in (ev.blocks[-1], ev.norm, ev.fc_norm) if m is not None]
            groups = [first, *ev.blocks[:-1], last]
            unlock(groups[:unlocked_groups] if _g(self.args, "unlock_from_head", False) else groups[-unlocked_groups:])
        always = [m for m in (getattr(self, "perceiver", None), getattr(self, "visual_adapter", None)) if m is not None]
        if not isinstance(self.eva_vit_proj, nn.Linear):
            always.append(self.eva_vit_proj)
        if unlock_cls:
            always.append(ev.cls_token)
        if unlock_pos_emb:
            always.append(ev.pos_embed)
        if unlock_trans_first_n_layers is not None:
            always.extend(ev.blocks[i] for i in range(unlock_trans_first_n_layers))
        unlock(always)
