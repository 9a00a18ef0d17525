"""GPU: the backward of a tower without ln_pre (`TowerTrainer` over `engine.EvaVitEngine`): the gradients of cls_token,
pos_embed, norm, eva_vit_proj, one unlocked block (its q_bias / v_bias included) and of the input tokens against fp64 autograd
through tests/eva_ref.py on the bf16-rounded weights, under the module's parameter names (`engine.eva_grads`).

Criteria: those of the tower-backward tests of tests/test_hip_train.py - relative 2-norm error per tensor below 5e-2 at the
tiny configuration (test_depth_tower_backward_vs_reference_grads) and below 3e-2 at full width
(test_vitl_block_backward_vs_oracle_autograd)."""
import pytest
import torch

import eva_ref
from test_hip_eva_tower import P, case, engine_for, relerr

pytestmark = pytest.mark.gpu


def _grads_case(name, tol, res_dtype):
    from vitlens_hip import engine as E, train as TR
    c = case(name)
    B, T, D = c["tok"].shape
    unlocked = f"{P}eva_vit.blocks.0."
    want = lambda k: k.startswith(unlocked) or k in (P + "eva_vit.cls_token", P + "eva_vit.pos_embed", P + "eva_vit.norm.weight",
                                                      P + "eva_vit.norm.bias", P + "eva_vit_proj")
    sd = {k: v.cuda().double().requires_grad_(want(k)) for k, v in eva_ref.rounded(c["sd"]).items()}
    tok = c["tok"].cuda().double().requires_grad_(True)
    dfeat = torch.randn(B, c["E"], generator=torch.Generator().manual_seed(11))
    feat, _ = eva_ref.tower(sd, P, tok, c["H"])
    (feat * dfeat.cuda().double()).sum().backward()

    eng = engine_for(c, res_dtype)
    tr = TR.TowerTrainer(eng, train_blocks=[0], train_cls=True, train_pos=True, train_ln_post=True, train_proj=True, param_prefix=P)
    got_feat = tr.forward(c["tok"].cuda().bfloat16().reshape(B * T, D), B)
    e = relerr(got_feat, feat.detach())
    print(f"MEASURED {name} {res_dtype} trainer features: {e:.3e}")
    assert e < 2e-2 if res_dtype == torch.float32 else e < 4e-2, e
    dtok = tr.backward(dfeat.cuda())
    e = relerr(dtok.reshape(B, T, D), tok.grad)
    print(f"MEASURED {name} {res_dtype} token gradient: {e:.3e} (bound {tol:.0e})")
    assert e < tol, e
    named = E.eva_grads(tr.grads, P)
    expected = {k for k in sd if want(k)}
    assert set(named) == expected, set(named) ^ expected
    for k in sorted(expected):
        assert tuple(named[k].shape) == tuple(sd[k].shape), (k, named[k].shape)
        e = relerr(named[k], sd[k].grad)
        print(f"MEASURED {name} {res_dtype} grad {k}: {e:.3e} (bound {tol:.0e})")
        assert e < tol, (k, e)


@pytest.mark.parametrize("res_dtype", [torch.float32, torch.bfloat16])
def test_eva_tower_backward_tiny(res_dtype):
    """176 = 2 x 88, 3 blocks, 17 tokens, B = 4: block 0 unlocked behind two frozen ones, no ln_pre backward."""
    _grads_case("tiny", 5e-2, res_dtype)


def test_eva_tower_backward_width_1408():
    """1408 = 16 x 88, 257 tokens, B = 2, block 0 of 2 unlocked: the D = 1408 LayerNorm backward, the head-dim-88 attention
    backward at L = 257 and the N = 4224 / 6144 weight-gradient GEMMs."""
    _grads_case("full", 3e-2, torch.float32)


# ------------------------------------------------------------------------------------------------ the module path
def tiny_args(modality, **kw):
    """exp_args of a tiny Lens at the EVA test width 176 = 2 x 88: 16 latents, cross head dim 88 (audio) / 64 (pc, eeg)."""
    from types import SimpleNamespace
    a = dict(visual_modality_type=modality, use_perceiver=True, perceiver_as_identity=False, perceiver_num_latents=16,
             perceiver_latent_dim=176, perceiver_latent_heads=2, perceiver_latent_dim_head=88, perceiver_cross_heads=1,
             perceiver_depth=2, perceiver_self_per_cross_attn=1, unlock_from_head=False, disable_orig_pos=False,
             skip_trans_first_n_layers=None, use_eva_pt_lin=False, visual_arch="perceiver_blip_eva_g_vit")
    if modality == "audio":
        a.update(audio_mel_bins=32, audio_target_length=48, audio_fstride=6, audio_tstride=6, perceiver_input_chan=176,
                 perceiver_cross_dim_head=88)
    elif modality == "eeg":
        a.update(eeg_chans=8, eeg_time_len=40, eeg_window_size=3, eeg_stride=2, perceiver_input_chan=176, perceiver_cross_dim_head=64)
    else:
        a.update(pc_num_group=16, pc_group_size=8, pc_encoder_dims=64, pc_trans_dim=64, pc_npoints=256, perceiver_input_chan=64,
                 perceiver_cross_dim_head=64, pc_tokenizer="pointbert", pc_in_channel=3)
    a.update(kw)
    return SimpleNamespace(**a)


def tiny_module(modality, linear_head, seed=0):
    from open_clip.third_vit import blip_eva_vit as B
    torch.manual_seed(seed)
    args = tiny_args(modality)
    ev = B.VisionTransformer(img_size=56, patch_size=14, embed_dim=176, depth=3, num_heads=2, num_classes=32 if linear_head else 0,
                             num_tokens=17)
    m = B.Perceiver_Blip_EVA_ViT(None, None, ev, args, embed_dim=32)
    with torch.no_grad():               # away from the trivial initial values (zero biases, unit LayerNorms)
        g = torch.Generator().manual_seed(seed + 1)
        for n, p in m.named_parameters():
            if n.startswith("eva_vit"):
                p.add_(torch.randn(p.shape, generator=g) * (0.05 if p.dim() > 1 and "cls" not in n and "pos" not in n else 0.1))
        for n, b in m.named_buffers():
            if n.endswith("running_var"):
                b.uniform_(0.8, 1.2, generator=g)
            elif n.endswith("running_mean"):
                b.normal_(0, 0.1, generator=g)
    return m.cuda(), args


def oracle_forward(sd, x, args, heads, fps_start=None):
    """Lens (the oracle's tokenizer and Perceiver, on whatever dtype `sd` has) -> eva_ref.tower, all fp64."""
    import vitlens_oracle as O
    a = args
    lens = O.LensSpec(modality=a.visual_modality_type, perceiver_identity=False, depth=a.perceiver_depth,
                      self_per_cross=a.perceiver_self_per_cross_attn, num_latents=a.perceiver_num_latents,
                      latent_dim=a.perceiver_latent_dim, input_chan=a.perceiver_input_chan, cross_heads=a.perceiver_cross_heads,
                      cross_dim_head=a.perceiver_cross_dim_head, latent_heads=a.perceiver_latent_heads,
                      latent_dim_head=a.perceiver_latent_dim_head, audio_fstride=getattr(a, "audio_fstride", 10),
                      audio_tstride=getattr(a, "audio_tstride", 10), audio_mel_bins=getattr(a, "audio_mel_bins", 128),
                      audio_target_length=getattr(a, "audio_target_length", 512), pc_num_group=getattr(a, "pc_num_group", 512),
                      pc_group_size=getattr(a, "pc_group_size", 32), pc_encoder_dims=getattr(a, "pc_encoder_dims", 256),
                      pc_trans_dim=getattr(a, "pc_trans_dim", 384), eeg_chans=getattr(a, "eeg_chans", 128),
                      eeg_time_len=getattr(a, "eeg_time_len", 512), eeg_window_size=getattr(a, "eeg_window_size", 1),
                      eeg_stride=getattr(a, "eeg_stride", 1))
    if lens.modality == "audio":
        t, pos = O.audio_tokens(sd, P, x, lens)
    elif lens.modality == "eeg":
        t, pos = O.eeg_tokens(sd, P, x, lens)
    else:
        t, pos, _, _ = O.point_tokens(sd, P, x, lens, fps_start, False, None)
    lat = O.perceiver(sd, P + "perceiver.", t + pos, lens)
    return eva_ref.tower(sd, P, lat, heads)


@pytest.mark.parametrize("modality,linear_head", [("audio", False), ("pc", True), ("eeg", False)])
def test_eva_module_forward_tokens_backward_and_adamw(modality, linear_head):
    """Perceiver_Blip_EVA_ViT on the module path (forward under grad mode, loss.backward(), torch AdamW - the body of
    tri_train_one_epoch): features and tokens against the fp64 oracle Lens + eva_ref tower (bounds of tests/test_hip_towers.py),
    the gradients of every trainable parameter - Lens, cls_token, pos_embed, eva_vit_proj; an nn.Linear head stays frozen
    and its bias enters the forward - against fp64 autograd (5e-2, test_depth_tower_backward_vs_reference_grads), and the
    state after one AdamW step against torch AdamW on those fp64 gradients (see the comment there); a second step then runs on
    the updated engine."""
    m, args = tiny_module(modality, linear_head)
    m.train()
    m.lock(freeze_bn_stats=True, unlock_cls=True, unlock_pos_emb=True)
    g = torch.Generator().manual_seed(3)
    B = 4
    kw = {}
    if modality == "audio":
        x = torch.randn(B, 48, 32, generator=g).cuda()
    elif modality == "eeg":
        x = torch.randn(B, 8, 40, generator=g).cuda()
    else:
        x = (torch.rand(B, 256, 3, generator=g) * 2 - 1).cuda()
        kw["fps_start"] = torch.randint(0, 256, (B,), generator=g).cuda()
    dfeat = torch.randn(B, 32, generator=g).cuda()
    names = [n for n, p in m.named_parameters() if p.requires_grad]
    assert ("eva_vit_proj" in names) == (not linear_head) and "eva_vit.cls_token" in names and "eva_vit.pos_embed" in names
    assert not any(n.startswith(("eva_vit.blocks", "eva_vit.head", "eva_vit.norm")) for n in names)
    # (the fp64 reference runs on the CPU: the oracle's farthest-point sampling lives there, and the model is tiny)
    sd = {P + k: v.detach().cpu().double().requires_grad_(k in names) for k, v in m.state_dict().items()}
    ref_f, ref_x = oracle_forward(sd, x.cpu().double(), args, 2, **{k: v.cpu() for k, v in kw.items()})
    (ref_f * dfeat.cpu().double()).sum().backward()

    tok = m.forward_tokens(x, **kw)
    assert tuple(tok.shape) == (B, 17, 176)
    e = relerr(tok.reshape(B * 17, 176), ref_x.detach().reshape(B * 17, 176))
    print(f"MEASURED {modality} module tokens: {e:.3e} (bound 2e-2)")
    assert e < 2e-2, e
    opt = torch.optim.AdamW([p for p in m.parameters() if p.requires_grad], lr=1e-3)
    before = {n: p.detach().clone() for n, p in m.named_parameters() if p.requires_grad}
    feat = m(x, **kw)
    e = relerr(feat, ref_f.detach())
    print(f"MEASURED {modality} module features: {e:.3e} (bound 2e-2)")
    assert e < 2e-2, e
    (feat * dfeat).sum().backward()
    # the point tokenizer and what sits behind its two max-pools keep the bounds of the existing module-path test
    # (tests/test_hip_api.py _pc_tol: arg-max routing noise over bf16 activations); everything on the EVA side holds 5e-2
    from test_hip_api import _pc_tol
    tol = lambda n: 5e-2 if modality != "pc" or n.startswith("eva_vit") else _pc_tol(n)
    for n, p in m.named_parameters():
        assert (p.grad is not None) == (n in names), n
        if n in names:
            e = relerr(p.grad, sd[P + n].grad)
            print(f"MEASURED {modality} module grad {n}: {e:.3e} (bound {tol(n):.0e})")
            assert e < tol(n), (n, e)
    opt.step()
    # torch AdamW on the fp64 gradients, from the same start
    ref_p = {n: before[n].cpu().requires_grad_(True) for n in names}
    ref_opt = torch.optim.AdamW(list(ref_p.values()), lr=1e-3)
    for n in names:
        ref_p[n].grad = sd[P + n].grad.float()
    ref_opt.step()
    # AdamW's first step is -lr (sign(g) + wd p) up to eps: discontinuous in g where g crosses 0, so the PARAMETERS are compared
    # only where the asserted gradient bound rules a sign flip out - |g_ref| > tol ||g_ref|| >= |g - g_ref| - and there they must
    # agree to fp32 rounding; the optimizer's moments are smooth in g and are compared everywhere: exp_avg is linear in g (the
    # gradient's own bound), exp_avg_sq quadratic (twice that).  No bound is taken from what the code gave.
    state = {id(p): opt.state[p] for p in opt.state}
    checked = 0
    for n, p in m.named_parameters():
        if n not in names:
            continue
        assert not torch.equal(p.detach(), before[n]), n
        st, rst = state[id(p)], ref_opt.state[ref_p[n]]
        assert relerr(st["exp_avg"], rst["exp_avg"]) < tol(n), n
        assert relerr(st["exp_avg_sq"], rst["exp_avg_sq"]) < 2 * tol(n), n
        gref = sd[P + n].grad
        safe = gref.abs() > tol(n) * gref.norm()
        if bool(safe.any()):
            d = (p.detach().cpu() - ref_p[n].detach())[safe].abs().max()
            assert float(d) < 1e-6, (n, float(d))
            checked += int(safe.sum())
    print(f"MEASURED {modality} module AdamW: {checked} parameter elements compared exactly")
    assert checked > 0
    opt.zero_grad()
    feat2 = m(x, **kw)
    assert bool(torch.isfinite(feat2).all()) and float((feat2 - feat).abs().max()) > 0      # the engine follows the step
    (feat2 * dfeat).sum().backward()
    opt.step()
