#!/usr/bin/env python
"""Writes tests/golden/eva_tiny.npz: what the reference's Perceiver_Blip_EVA_ViT computes, in fp64 on the CPU, for two tiny Lens
towers over a tiny EVA ViT (width 176 = 2 heads x 88, 3 blocks, MLP hidden int(176 * 4.3637) = 768, 16 latents, LayerNorm eps
1e-6): a point-cloud Lens with cross head dim 64 and the `eva_vit_proj` Parameter, an audio Lens with cross head dim 88 and the
nn.Linear head.  Data only.  The weights are NOT stored (1.6 M numbers per tower would not fit a fixture): they are the seeded
state of tests/eva_ref.init_state + the oracle's init_lens, loaded into the reference's modules with strict=True - which is
also the check that our names and shapes are the reference's - and the tests rebuild them from the seeds in `meta`.  Stored per
tower: inputs, features, the forward_features tokens, the loss sum(features * dfeat), per parameter the gradient's 2-norm, sum
and its dot product with a seeded probe (tests/eva_ref.probe), the state_dict's names and shapes, and the trainable names after
`lock` for five flag combinations with `unlock_from_head` both ways.

usage: python tools/gen_eva_golden.py        (needs the reference tree; see oracle/ref_loader.py)"""
import json
import os
import sys
from functools import partial

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]
import ref_loader  # noqa: E402
import eva_ref  # noqa: E402
import vitlens_oracle as O  # noqa: E402

P = "visual."
D, HEADS, DEPTH, LATENTS, E = 176, 2, 3, 16, 32
LOCKS = [dict(), dict(unlock_cls=True, unlock_pos_emb=True), dict(unlock_trans_first_n_layers=2), dict(unlocked_groups=1),
         dict(unlocked_groups=2, unlock_cls=True)]


def lens_args(modality, linear_head):
    common = dict(perceiver_num_latents=LATENTS, perceiver_latent_dim=D, perceiver_latent_heads=HEADS, perceiver_latent_dim_head=88,
                  perceiver_cross_heads=1, use_eva_pt_lin=linear_head, visual_arch="perceiver_blip_eva_g_vit",
                  disable_orig_pos=False, skip_trans_first_n_layers=None, disable_visual_adapter_pos=False)
    if modality == "audio":
        return ref_loader.lens_args("audio", audio_mel_bins=32, audio_target_length=48, audio_fstride=6, audio_tstride=6,
                                    perceiver_input_chan=D, perceiver_depth=2, perceiver_self_per_cross_attn=1,
                                    perceiver_cross_dim_head=88, **common)
    return ref_loader.lens_args("pc", pc_num_group=16, pc_group_size=8, pc_encoder_dims=64, pc_trans_dim=64, pc_npoints=256,
                                perceiver_input_chan=64, perceiver_depth=2, perceiver_self_per_cross_attn=1,
                                pc_tokenizer="pointbert", pc_in_channel=3, pc_radius=0.2, perceiver_cross_dim_head=64, **common)


def build(oc, modality, linear_head, seed):
    """The reference's modules with our seeded state loaded into them (strict), in fp64."""
    import timm.models.layers as tl
    import types
    if not hasattr(tl, "to_2tuple"):        # the three names the shells lack, in this process only
        tl.drop_path = lambda x, p=0.0, training=False: x
        tl.to_2tuple = lambda v: tuple(v) if isinstance(v, (tuple, list)) else (v, v)
        reg = types.ModuleType("timm.models.registry"); reg.register_model = lambda f: f
        sys.modules["timm.models.registry"] = reg
    from open_clip.third_vit import blip_eva_vit as R
    from open_clip.module_cfg import get_input_adapter_cfg, get_perceiver_cfg
    from open_clip.perceiver import get_perceiver
    from open_clip.visual_adapter import get_visual_adapter
    from open_clip.transformer import LayerNorm
    args = lens_args(modality, linear_head)
    adapter = get_visual_adapter(get_input_adapter_cfg(args), grid_size=(4, 4), patch_size=(14, 14), width=D, input_patchnorm=False,
                                 exp_args=args)
    perceiver = get_perceiver(get_perceiver_cfg(args), args=args, transformer_width=D, transformer_heads=HEADS,
                              transformer_mlp_ratio=4.3637, transformer_ls_init_value=None, transformer_act_layer=torch.nn.GELU,
                              transformer_norm_layer=LayerNorm)
    eva = R.VisionTransformer(img_size=56, patch_size=14, use_mean_pooling=False, embed_dim=D, num_classes=E if linear_head else 0,
                              depth=DEPTH, num_heads=HEADS, mlp_ratio=4.3637, qkv_bias=True, norm_layer=partial(torch.nn.LayerNorm, eps=1e-6))
    model = R.Perceiver_Blip_EVA_ViT(adapter, perceiver, eva, args, embed_dim=E)
    sd = eva_ref.fixture_state(modality, linear_head, seed)
    own = {k[len(P):]: v for k, v in sd.items()}
    if linear_head:                         # the head is registered under both names
        own["eva_vit_proj.weight"], own["eva_vit_proj.bias"] = own["eva_vit.head.weight"], own["eva_vit.head.bias"]
    have = {k: v for k, v in model.state_dict().items() if "num_batches_tracked" not in k}
    assert set(have) == set(own), sorted(set(have) ^ set(own))
    for k in have:
        assert tuple(have[k].shape) == tuple(own[k].shape), (k, have[k].shape, own[k].shape)
    model.load_state_dict(own, strict=False)
    return model.double().eval(), args, sd


def case(oc, modality, linear_head, seed, res):
    model, args, sd = build(oc, modality, linear_head, seed)
    x, extra = eva_ref.fixture_inputs(modality, seed)
    tag = modality + "/"
    if modality == "pc":                    # the reference draws the FPS start inside the tokenizer (torch.randint)
        torch.manual_seed(seed + 7)
        extra["fps_start"] = torch.randint(0, 256, (x.shape[0],), dtype=torch.long)
    def fwd():
        if modality == "pc":
            torch.manual_seed(seed + 7)
        return model(x.double())
    feat = fwd()
    dfeat = extra["dfeat"].double()
    loss = (feat * dfeat).sum()
    model.zero_grad()
    loss.backward()
    # the tokens: the same forward up to eva_vit.forward_features
    grabbed = {}
    h = model.eva_vit.blocks[-1].register_forward_hook(lambda m, i, o: grabbed.__setitem__("x", o.detach()))
    with torch.no_grad():
        fwd()
    h.remove()
    res[tag + "in/x"] = x.numpy()
    for k, v in extra.items():
        res[tag + "in/" + k] = v.numpy()
    res[tag + "out/features"] = feat.detach().numpy(); res[tag + "out/tokens"] = grabbed["x"].numpy()
    res[tag + "out/loss"] = loss.detach().numpy()
    names, shapes, stats = [], [], []
    for n, p in model.named_parameters():
        g = p.grad.detach()
        stats.append([float(g.norm()), float(g.sum()), float((g.reshape(-1) * eva_ref.probe(n, g.numel())).sum())])
        names.append(n); shapes.append(list(p.shape))
    res[tag + "grad/stats"] = np.array(stats, dtype=np.float64)
    locks = {}
    for from_head in (False, True):
        args["unlock_from_head"] = from_head
        for i, kw in enumerate(LOCKS):
            model.lock(**kw)
            locks[f"{int(from_head)}/{i}"] = sorted(n for n, p in model.named_parameters() if p.requires_grad)
    return {"seed": seed, "linear_head": linear_head, "grad_names": names, "grad_shapes": shapes,
            "state_names": [k for k in model.state_dict() if "num_batches_tracked" not in k],
            "state_shapes": [list(v.shape) for k, v in model.state_dict().items() if "num_batches_tracked" not in k],
            "locks": locks, "lock_flags": LOCKS,
            "args": {k: v for k, v in args.items() if isinstance(v, (int, float, str, bool, type(None)))}}


def main():
    oc = ref_loader.load()
    res, meta = {}, {"width": D, "heads": HEADS, "depth": DEPTH, "latents": LATENTS, "embed_dim": E, "eps": 1e-6}
    meta["pc"] = case(oc, "pc", False, 11, res)
    meta["audio"] = case(oc, "audio", True, 12, res)
    res["meta"] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    out = os.path.join(ROOT, "tests", "golden", "eva_tiny.npz")
    np.savez_compressed(out, **res)
    print(f"{out}: {len(res)} arrays, {os.path.getsize(out)} bytes; losses {float(res['pc/out/loss']):.6f} {float(res['audio/out/loss']):.6f}")


if __name__ == "__main__":
    main()
