#!/usr/bin/env python
"""The OpenShape recipe at the published geometry (TRAIN_INFERENCE.md:108-133: ViT-bigG-14 trunk - 40 blocks, the last 24
kept, the first 2 of those unlocked - behind a pnsa tokenizer over 10 000 points in 512 groups of 64, trans dim 256, and a
Perceiver of depth 4 with 256 latents of 1664 = 16 x 104), seeded random weights and inputs, micro-batch 16:

  module   openshape.openclip_step (CLIPBindWrap + torch.optim.AdamW with the recipe's four groups, clip over the tower) at
           batch 16 - the drop-in path, which this tree leaves as it was;
  fused    vitlens_hip.step.OpenShapeStep at batch 16 and at larger batches in micro-batches of 16 (--batches);
  adamw    the optimizer launch alone on the step's own slot table: vl_adamw_multi_step_groups against vl_adamw_multi_step.

Times are host clocks around work that ends in a device synchronise, after warm-up steps of the same shape; the variants
alternate within one process and every line is repeated (--reps), so the spread is in the log.  Not a bench.py workload.

usage: python tools/bench_openshape_step.py [--batches 16,64,256] [--steps 4] [--warmup 2] [--reps 3] [--out FILE] [--small]"""
import argparse
import json
import os
import sys
import tempfile
import time
import warnings
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "vit-lens_amd"))

import torch  # noqa: E402

LR, BETAS, EPS, WD, CLIP = 1e-4, (0.9, 0.98), 1e-8, 0.2, 10.0


def geometry(small: bool):
    if small:          # a rehearsal size: every code path, no meaning in its times
        vis = dict(image_size=32, layers=4, width=64, head_width=32, mlp_ratio=4.0, patch_size=8)
        return dict(embed_dim=32, vision_cfg=vis, skip=1, points=600,
                    lens=dict(pc_in_channel=3, pc_radius=0.3, pc_num_group=32, pc_group_size=16, pc_trans_dim=64, pc_encoder_dims=64,
                              perceiver_input_chan=64, perceiver_cross_dim_head=64, perceiver_latent_dim=64, perceiver_latent_dim_head=32,
                              perceiver_latent_heads=2, perceiver_num_latents=16, perceiver_self_per_cross_attn=1, perceiver_depth=2))
    vis = dict(image_size=224, layers=40, width=1664, head_width=104, mlp_ratio=4.9231, patch_size=14)
    return dict(embed_dim=1280, vision_cfg=vis, skip=16, points=10000,
                lens=dict(pc_in_channel=6, pc_radius=0.2, pc_num_group=512, pc_group_size=64, pc_trans_dim=256, pc_encoder_dims=256,
                          perceiver_input_chan=256, perceiver_cross_dim_head=104, perceiver_latent_dim=1664, perceiver_latent_dim_head=104,
                          perceiver_latent_heads=16, perceiver_num_latents=256, perceiver_self_per_cross_attn=1, perceiver_depth=4))


def build_wrap(geo, device):
    """CLIPBindWrap over a seeded tower of the geometry, locked as the recipe locks it.  The text side of the TriCLIP factory
    is as small as it goes: nothing in this recipe runs it."""
    import open_clip as oc
    import openshape
    cfg = dict(embed_dim=geo["embed_dim"], vision_cfg=geo["vision_cfg"],
               text_cfg=dict(context_length=8, vocab_size=64, width=64, heads=2, layers=1))
    args = SimpleNamespace(visual_modality_type="3dpc", pc_tokenizer="pnsa", use_perceiver=True, use_visual_adapter=True,
                           visual_arch="perceiver_vit", v_key="pc", skip_trans_first_n_layers=geo["skip"], unlock_cls=False,
                           perceiver_as_identity=False, perceiver_attn_dropout=0.0, perceiver_ff_dropout=0.0, perceiver_cross_heads=1,
                           perceiver_weight_tie_layers=False, disable_orig_pos=False, disable_visual_adapter_pos=False,
                           pc_npoints=geo["points"], model=SimpleNamespace(out_channel=geo["embed_dim"]), **geo["lens"])
    with tempfile.TemporaryDirectory() as td:
        with open(os.path.join(td, "openshape-bench.json"), "w") as f:
            json.dump(cfg, f)
        oc.add_model_config(td)
        torch.manual_seed(0)
        with warnings.catch_warnings(), torch.device(device):          # parameters are drawn on the device: 1.6 G of them
            warnings.simplefilter("ignore")
            tri = oc.tri_create_model("openshape-bench", None, precision="fp32", device=device, output_dict=True, args=args)
    tri.image = None                                                     # (the wrapper keeps the `visual` tower only)
    wrap = openshape.CLIPBindWrap(args, model=tri).to(device)
    wrap.lock(unlocked_groups=0, freeze_bn_stats=False, unlock_cls=False, unlock_trans_first_n_layers=2)
    wrap.train()
    return wrap, openshape


def inputs(geo, batch, device, seed=1):
    g = torch.Generator(device=device).manual_seed(seed)
    n, c, e = geo["points"], geo["lens"]["pc_in_channel"], geo["embed_dim"]
    xyz = torch.rand(batch, n, 3, device=device, generator=g) * 2 - 1
    feats = torch.cat([xyz, torch.rand(batch, n, c - 3, device=device, generator=g)], -1) if c > 3 else xyz.clone()
    return dict(xyz=xyz, feats=feats, img=torch.randn(batch, e, device=device, generator=g),
                text=torch.randn(batch, e, device=device, generator=g),
                start=torch.randint(0, n, (batch,), device=device, generator=g))


def timed(fn, warmup, steps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="16,64,256")
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--small", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_openshape_step: needs an MI355X; a CPU run measures nothing")
    from vitlens_hip import engine, ops
    from vitlens_hip.step import OpenShapeStep, openshape_param_group
    dev, geo = "cuda", geometry(a.small)
    lines = []

    def say(**kw):
        line = json.dumps(kw)
        lines.append(line)
        print(line, flush=True)
    wrap, openshape = build_wrap(geo, dev)
    v = geo["vision_cfg"]
    tower = engine.TowerCfg(width=v["width"], layers=v["layers"] - geo["skip"], heads=v["width"] // v["head_width"],
                            mlp_ratio=v["mlp_ratio"], patch=v["patch_size"], image_size=v["image_size"], embed_dim=geo["embed_dim"])
    lens = wrap.backbone._cfgs()[1]
    sd = {"visual." + k: t.detach() for k, t in wrap.backbone.state_dict().items()}
    sd["logit_scale"] = torch.tensor(2.659, device=dev)
    say(what="geometry", small=a.small, kept_blocks=tower.layers, unlocked=2, width=tower.width, points=geo["points"],
        trainable=sum(p.numel() for p in wrap.parameters() if p.requires_grad), micro_batch=16)
    # ---- the module path at batch 16 ----
    scale_net = openshape.LogitScaleNetwork().to(dev)
    named = [(n, p) for n, p in list(wrap.named_parameters()) + list(scale_net.named_parameters()) if p.requires_grad]
    groups = {}
    for n, p in named:
        groups.setdefault(openshape_param_group(n, p.ndim, WD), []).append(p)

    class Clipped(torch.optim.AdamW):
        def step(self):
            torch.nn.utils.clip_grad_norm_(wrap.parameters(), CLIP, norm_type=2.0)
            super().step()
    opt = Clipped([{"params": ps, "lr": LR * ls, "weight_decay": wd} for (ls, wd), ps in groups.items()], lr=LR, betas=BETAS, eps=EPS)
    x16 = inputs(geo, 16, dev)
    data = {"xyz_dense": x16["xyz"], "features_dense": x16["feats"], "text_feat": x16["text"], "img_feat": x16["img"]}
    loss_fn = openshape.TriClipLoss()
    module = lambda: openshape.openclip_step(wrap, scale_net, loss_fn, opt, data, device=dev, fps_start=x16["start"])
    # ---- the fused step ----
    st = OpenShapeStep(sd, tower, lens, dev, micro_batch=16, unlock_trans_first_n_layers=2, lr=LR, betas=BETAS, eps=EPS,
                       weight_decay=WD, grad_clip_norm=CLIP)
    fused16 = lambda: st.step(x16["feats"], x16["xyz"], x16["img"], x16["text"], fps_start=x16["start"])
    for rep in range(a.reps):
        ms = timed(module, a.warmup if rep == 0 else 1, a.steps)
        say(what="module openclip_step", batch=16, rep=rep, ms_per_step=round(ms, 3), ms_per_sample=round(ms / 16, 3))
        ms = timed(fused16, a.warmup if rep == 0 else 1, a.steps)
        say(what="fused OpenShapeStep", batch=16, micro_batch=16, rep=rep, ms_per_step=round(ms, 3), ms_per_sample=round(ms / 16, 3))
    del module, opt, wrap, groups, named
    torch.cuda.empty_cache()
    for batch in [int(b) for b in a.batches.split(",") if int(b) > 16]:
        try:
            xb = inputs(geo, batch, dev, seed=batch)
            fn = lambda: st.step(xb["feats"], xb["xyz"], xb["img"], xb["text"], fps_start=xb["start"])
            for rep in range(a.reps):
                ms = timed(fn, 1, max(1, a.steps * 16 // batch))
                say(what="fused OpenShapeStep", batch=batch, micro_batch=16, rep=rep, ms_per_step=round(ms, 3),
                    ms_per_sample=round(ms / batch, 3), gb_allocated=round(torch.cuda.max_memory_allocated() / 2 ** 30, 1))
        except torch.OutOfMemoryError:
            say(what="fused OpenShapeStep", batch=batch, micro_batch=16, result="does not fit")
            break
    # ---- the optimizer launch alone, on the step's table (lr 0: the weights stay where they are) ----
    o = st.opt
    n = o._slots.shape[0]
    elems = sum(m.numel() for m in st.masters.values())
    plain = lambda: ops.adamw_multi(o._slots, n, 0.0, BETAS[0], BETAS[1], EPS, 3, 1.0, CLIP, st._sumsq)
    grouped = lambda: ops.adamw_multi_step_groups(o._slots, o._groups, o._groups_host, n, 0.0, BETAS[0], BETAS[1], EPS, 3, 1.0, CLIP,
                                                  st._sumsq)
    for rep in range(max(a.reps, 3)):
        for name, fn in (("vl_adamw_multi_step", plain), ("vl_adamw_multi_step_groups", grouped)):
            ms = timed(fn, 5, 50)
            # bytes the update needs: p, m, v read and written, g read (fp32)
            say(what=name, slots=n, elements=elems, rep=rep, us=round(ms * 1e3, 2), gb_per_s=round(7 * 4 * elems / (ms * 1e-3) / 1e9, 1))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
