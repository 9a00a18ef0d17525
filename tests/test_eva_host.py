"""CPU: the EVA ViT-g Lens tower (visual_arch "perceiver_blip_eva_g_vit") below the kernels - the fp64 restatement against
torch's own layers, `engine.eva_tower_state` (names, shapes, the [q, 0, v] bias) and its inverse on the gradient names, the
module's state_dict names, `lock`, `create_eva_vit_g` without a file, the refusals with their reasons, and the new C entry
under ABI version 610 in header, exports and binding table."""
import os
import re
from types import SimpleNamespace

import pytest
import torch

import eva_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = "visual."


def args_for(modality="audio", **kw):
    a = dict(visual_modality_type=modality, use_perceiver=True, perceiver_as_identity=False, perceiver_num_latents=16,
             perceiver_latent_dim=176, perceiver_latent_heads=2, perceiver_latent_dim_head=88, perceiver_cross_heads=1,
             perceiver_cross_dim_head=88, perceiver_depth=1, perceiver_self_per_cross_attn=1, perceiver_input_chan=176,
             audio_mel_bins=32, audio_target_length=48, audio_fstride=6, audio_tstride=6, unlock_from_head=False,
             disable_orig_pos=False, skip_trans_first_n_layers=None, use_eva_pt_lin=False)
    a.update(kw)
    return SimpleNamespace(**a)


def tiny(linear_head=False, depth=3, **kw):
    from open_clip.third_vit import blip_eva_vit as B
    torch.manual_seed(0)
    ev = B.VisionTransformer(img_size=56, patch_size=14, embed_dim=176, depth=depth, num_heads=2,
                             num_classes=24 if linear_head else 0, num_tokens=17)
    return B.Perceiver_Blip_EVA_ViT(None, None, ev, args_for(**kw), embed_dim=32)


def test_restatement_equals_torch_layers():
    """eva_ref.tower against the same tower written with torch's own LayerNorm / softmax / gelu / linear in fp64."""
    F = torch.nn.functional
    sd = {k: v.double() for k, v in eva_ref.init_state(P, 176, 2, 3, 17, 32, seed=1).items()}
    tok = torch.randn(3, 16, 176, dtype=torch.float64, generator=torch.Generator().manual_seed(2))
    f, x = eva_ref.tower(sd, P, tok, 2)
    e = P + "eva_vit."
    y = torch.cat([sd[e + "cls_token"].expand(3, 1, 176), tok], 1) + sd[e + "pos_embed"]
    for n in range(3):
        p = f"{e}blocks.{n}."
        h = F.layer_norm(y, (176,), sd[p + "norm1.weight"], sd[p + "norm1.bias"], 1e-6)
        bias = torch.cat([sd[p + "attn.q_bias"], torch.zeros(176, dtype=torch.float64), sd[p + "attn.v_bias"]])
        q, k, v = F.linear(h, sd[p + "attn.qkv.weight"], bias).reshape(3, 17, 3, 2, 88).permute(2, 0, 3, 1, 4)
        a = F.scaled_dot_product_attention(q, k, v).transpose(1, 2).reshape(3, 17, 176)
        y = y + F.linear(a, sd[p + "attn.proj.weight"], sd[p + "attn.proj.bias"])
        h = F.layer_norm(y, (176,), sd[p + "norm2.weight"], sd[p + "norm2.bias"], 1e-6)
        y = y + F.linear(F.gelu(F.linear(h, sd[p + "mlp.fc1.weight"], sd[p + "mlp.fc1.bias"])), sd[p + "mlp.fc2.weight"], sd[p + "mlp.fc2.bias"])
    want = F.layer_norm(y[:, 0], (176,), sd[e + "norm.weight"], sd[e + "norm.bias"], 1e-6) @ sd[P + "eva_vit_proj"]
    assert float((x - y).norm() / y.norm()) < 1e-10 and float((f - want).norm() / want.norm()) < 1e-10
    assert int(176 * 4.3637) == 768 and int(1408 * 4.3637) == 6144


@pytest.mark.parametrize("linear_head", [False, True])
def test_eva_tower_state_round_trip(linear_head):
    from vitlens_hip import engine as E
    sd = eva_ref.init_state(P, 176, 2, 3, 17, 32, seed=3, linear_head=linear_head)
    sd[P + "perceiver.latents"] = torch.zeros(16, 176)
    m = E.eva_tower_state(sd, P)
    assert m[P + "class_embedding"].shape == (176,) and m[P + "positional_embedding"].shape == (17, 176)
    assert torch.equal(m[P + "class_embedding"], sd[P + "eva_vit.cls_token"].reshape(176))
    assert m[P + "perceiver.latents"] is sd[P + "perceiver.latents"]
    assert not any("eva_vit" in k for k in m) and P + "ln_pre.weight" not in m
    for n in range(3):
        b, s = f"{P}transformer.resblocks.{n}.", f"{P}eva_vit.blocks.{n}."
        bias = m[b + "attn.in_proj_bias"]
        assert bias.shape == (528,)
        assert torch.equal(bias[:176], sd[s + "attn.q_bias"]) and torch.equal(bias[352:], sd[s + "attn.v_bias"])
        assert float(bias[176:352].abs().max()) == 0.0
        assert m[b + "attn.in_proj_weight"].shape == (528, 176) and m[b + "mlp.c_fc.weight"].shape == (768, 176)
        assert m[b + "mlp.c_proj.weight"].shape == (176, 768) and m[b + "ln_2.bias"] is sd[s + "norm2.bias"]
    assert f"{P}transformer.resblocks.3.ln_1.weight" not in m
    assert m[P + "proj"].shape == (176, 32)
    if linear_head:
        assert torch.equal(m[P + "proj"], sd[P + "eva_vit.head.weight"].t()) and torch.equal(m[P + "proj_bias"], sd[P + "eva_vit.head.bias"])
    else:
        assert m[P + "proj"] is sd[P + "eva_vit_proj"] and P + "proj_bias" not in m
    # the names, there and back
    names = [k[len(P):] for k in sd if "eva_vit" in k and "head" not in k]
    mapped = E.eva_param_names(names)
    assert "transformer.resblocks.1.attn.in_proj_bias" in mapped and "class_embedding" in mapped and not any("eva" in n for n in mapped)
    grads = {P + n: torch.zeros(m[P + n].shape) for n in mapped if P + n in m}
    back = E.eva_grads(grads, P)
    assert {k[len(P):] for k in back} == set(names) - ({"eva_vit_proj"} if linear_head else set())
    for k, g in back.items():
        assert tuple(g.shape) == tuple(sd[k].shape), k
    cfg = E.eva_tower_cfg(width=176, layers=3, heads=2, embed_dim=32)
    assert cfg.ln_eps == 1e-6 and cfg.pre_norm is False and int(cfg.width * cfg.mlp_ratio) == 768
    assert E.TowerCfg().ln_eps == 1e-5 and E.TowerCfg().pre_norm is True
    full = E.eva_tower_cfg()
    assert (full.width, full.layers, full.heads, int(full.width * full.mlp_ratio)) == (1408, 40, 16, 6144)


def test_module_state_dict_names_and_shapes():
    m = tiny()
    sd = m.state_dict()
    want = {"eva_vit_proj": (176, 32), "eva_vit.cls_token": (1, 1, 176), "eva_vit.pos_embed": (1, 17, 176),
            "eva_vit.norm.weight": (176,), "eva_vit.blocks.2.attn.qkv.weight": (528, 176), "eva_vit.blocks.2.attn.q_bias": (176,),
            "eva_vit.blocks.2.attn.v_bias": (176,), "eva_vit.blocks.0.attn.proj.bias": (176,), "eva_vit.blocks.0.mlp.fc1.weight": (768, 176),
            "eva_vit.blocks.0.mlp.fc2.weight": (176, 768), "eva_vit.blocks.1.norm1.bias": (176,), "perceiver.latents": (16, 176),
            "visual_adapter.conv1.weight": (176, 1, 14, 14)}
    for k, shp in want.items():
        assert tuple(sd[k].shape) == shp, k
    assert not any(k.startswith(("class_embedding", "transformer.", "ln_pre", "ln_post", "proj", "eva_vit.patch_embed")) for k in sd)
    assert "eva_vit.blocks.0.attn.qkv.bias" not in sd and "eva_vit.blocks.3.norm1.weight" not in sd
    lin = tiny(linear_head=True).state_dict()
    assert tuple(lin["eva_vit.head.weight"].shape) == (24, 176) and "eva_vit_proj.weight" in lin and "eva_vit_proj" not in lin
    assert lin["eva_vit_proj.bias"].data_ptr() == lin["eva_vit.head.bias"].data_ptr()
    # the reference's initialisation: fix_init_weight scales block l's two output projections by 1 / sqrt(2 (l + 1))
    s0, s2 = float(sd["eva_vit.blocks.0.attn.proj.weight"].std()), float(sd["eva_vit.blocks.2.attn.proj.weight"].std())
    assert 0.85 < s0 / (0.02 / 2 ** 0.5) < 1.15 and 0.85 < s2 / (0.02 / 6 ** 0.5) < 1.15
    assert float(sd["eva_vit.blocks.0.attn.qkv.weight"].abs().max()) <= 2.0 and float(sd["eva_vit.blocks.0.mlp.fc1.bias"].abs().max()) == 0
    assert tiny(disable_orig_pos=True).eva_vit.pos_embed is None
    assert len(tiny(skip_trans_first_n_layers=2).eva_vit.blocks) == 1


def trainable(m):
    return sorted(n for n, p in m.named_parameters() if p.requires_grad)


def test_lock_semantics():
    lens = lambda m: [n for n in trainable(m) if n.startswith(("perceiver.", "visual_adapter."))]
    eva = lambda m: [n for n in trainable(m) if n.startswith("eva_vit")]
    m = tiny()
    m.lock()
    assert eva(m) == ["eva_vit_proj"] and len(lens(m)) == len([n for n, _ in m.named_parameters() if not n.startswith("eva_vit")])
    m.lock(unlock_cls=True, unlock_pos_emb=True)
    assert eva(m) == ["eva_vit.cls_token", "eva_vit.pos_embed", "eva_vit_proj"]
    m.lock(unlock_trans_first_n_layers=2)
    assert {n.split(".")[2] for n in eva(m) if "blocks" in n} == {"0", "1"}
    m.lock(unlocked_groups=1)                       # from the tail: [last block, norm]
    assert {n.rsplit(".", 2)[0] if "blocks" in n else n for n in eva(m)} >= {"eva_vit.norm.weight", "eva_vit.norm.bias"}
    assert {n.split(".")[2] for n in eva(m) if "blocks" in n} == {"2"} and "eva_vit.cls_token" not in eva(m)
    m.lock(unlocked_groups=2)
    assert {n.split(".")[2] for n in eva(m) if "blocks" in n} == {"1", "2"}
    h = tiny(unlock_from_head=True)
    h.lock(unlocked_groups=1)                       # from the head: [cls_token, pos_embed]
    assert eva(h) == ["eva_vit.cls_token", "eva_vit.pos_embed", "eva_vit_proj"]
    h.lock(unlocked_groups=2)
    assert {n.split(".")[2] for n in eva(h) if "blocks" in n} == {"0"}
    lin = tiny(linear_head=True)
    lin.lock(unlock_cls=True)
    assert eva(lin) == ["eva_vit.cls_token"]        # a Linear head is always frozen


def test_create_eva_vit_g_without_a_file(tmp_path):
    from open_clip.third_vit import blip_eva_vit as B
    g = B.create_eva_vit_g(depth=1, cache_dir=str(tmp_path))
    assert (g.embed_dim, g.num_heads, g.eps) == (1408, 16, 1e-6) and tuple(g.pos_embed.shape) == (1, 257, 1408)
    assert tuple(g.blocks[0].mlp.fc1.weight.shape) == (6144, 1408) and tuple(g.head.weight.shape) == (1024, 1408)
    assert isinstance(B.create_eva_vit_g(depth=1, use_nnlinear=False, cache_dir=str(tmp_path)).head, torch.nn.Identity)
    # a checkpoint that IS there is loaded: fp16 accepted, another position table refused with the reason
    sd = {k: v.half() for k, v in g.state_dict().items()}
    sd["cls_token"] = torch.full_like(sd["cls_token"], 0.25)
    torch.save(sd, tmp_path / B.CKPT_NAME)
    g2 = B.create_eva_vit_g(depth=1, cache_dir=str(tmp_path))
    assert g2.cls_token.dtype == torch.float32 and float(g2.cls_token.detach().mean()) == 0.25
    sd["pos_embed"] = sd["pos_embed"][:, :197]
    torch.save(sd, tmp_path / B.CKPT_NAME)
    with pytest.raises(ValueError, match="pos_embed is .*197.*interpolating"):
        B.create_eva_vit_g(depth=1, cache_dir=str(tmp_path))


def test_refusals_carry_their_reasons():
    from open_clip.third_vit import blip_eva_vit as B
    from vitlens_hip import engine as E
    for modality in ("image", "video", "tactile"):
        with pytest.raises(NotImplementedError, match="keep_patch_embed.*patch convolution"):
            tiny(modality=modality)
    with pytest.raises(ValueError, match="perceiver_latent_dim is 128.*must be 176"):
        tiny(perceiver_latent_dim=128)
    with pytest.raises(ValueError, match="perceiver_num_latents must be 16"):
        tiny(perceiver_num_latents=32)
    with pytest.raises(NotImplementedError, match="HIP engines"):
        B.VisionTransformer(embed_dim=176, depth=1, num_heads=2, num_tokens=17)(torch.zeros(1))
    sd = eva_ref.init_state(P, 176, 2, 1, 17, 32, seed=0)
    with pytest.raises(ValueError, match="pre_norm=False"):
        E.EvaVitEngine(sd, P, E.TowerCfg(width=176, layers=1, heads=2), "cpu")
    with pytest.raises(KeyError, match="cls_token"):
        E.eva_tower_state(sd, "image.")


def test_triclip_refuses_a_latent_dim_other_than_1408(monkeypatch):
    """TriCLIP builds the EVA arch through _build_visual_arch; the check fires before the 40-block tower is used (the tower
    itself is replaced by a one-block one here: a billion parameters are no unit test)."""
    from open_clip import model as M
    from open_clip.third_vit import blip_eva_vit as B
    real = B.create_eva_vit_g
    monkeypatch.setattr(B, "create_eva_vit_g", lambda depth=40, **kw: real(depth=1, cache_dir="/nonexistent", **kw))
    a = args_for(perceiver_latent_dim=1024, perceiver_num_latents=256)
    with pytest.raises(ValueError, match="perceiver_latent_dim is 1024.*1408"):
        M._build_visual_arch("perceiver_blip_eva_g_vit", a, embed_dim=768)
    with pytest.raises(NotImplementedError, match="visual_arch 'mystery'"):
        M._build_visual_arch("mystery", a, embed_dim=768)
    a = args_for(perceiver_latent_dim=1408, perceiver_num_latents=256, perceiver_input_chan=1408)
    v = M._build_visual_arch("perceiver_blip_eva_g_vit", a, embed_dim=768)
    assert tuple(v.state_dict()["eva_vit_proj"].shape) == (1408, 768) and v.heads == 16 and v._cfgs()[0].ln_eps == 1e-6
    assert tuple(v.state_dict()["visual_adapter.conv1.weight"].shape)[0] == 1408


def test_new_entry_is_declared_exported_and_bound_under_610():
    import ctypes
    from vitlens_hip import _lib
    hdr = open(os.path.join(ROOT, "include", "vitlens_hip.h")).read()
    assert int(re.search(r"#define\s+VL_ABI_VERSION\s+(\d+)", hdr).group(1)) == 610 == _lib.ABI_VERSION
    decl = re.search(r"int vl_assemble_tokens\((.*?)\);", hdr, re.S).group(1)
    assert len(decl.split(",")) == len(_lib.SIGNATURES["vl_assemble_tokens"]) == 12
    note = hdr[:hdr.index("int vl_assemble_tokens(")].rsplit("/*", 1)[1]
    for word in ("NOTE on the version", "610", "D = 1408", "No existing entry changes"):
        assert word in note, word
    lib = ctypes.CDLL(_lib.lib_path())
    assert hasattr(lib, "vl_assemble_tokens") and int(_lib.load_library().vl_version()) == 610
    from vitlens_hip import ops
    assert callable(ops.assemble_tokens)
    # a refusal launches nothing, so it runs here too
    assert _lib.load_library().vl_assemble_tokens(None, 0, None, None, None, None, 0, None, 0, 1, 8, None) != 0
    assert b"empty problem" in _lib.load_library().vl_last_error()


# ------------------------------------------------------------------------------------------------ the reference's fixture
def _fixture():
    import json
    import numpy as np
    z = np.load(os.path.join(ROOT, "tests", "golden", "eva_tiny.npz"))
    return z, json.loads(bytes(z["meta"]).decode())


def _module_for(modality, meta, **kw):
    """Our module at the fixture's configuration (the EVA ViT tiny, the Lens from the recorded args)."""
    from open_clip.third_vit import blip_eva_vit as B
    a = dict(meta[modality]["args"])
    a.update(kw)
    ev = B.VisionTransformer(img_size=56, patch_size=14, embed_dim=meta["width"], depth=meta["depth"], num_heads=meta["heads"],
                             num_classes=meta["embed_dim"] if meta[modality]["linear_head"] else 0, num_tokens=meta["latents"] + 1)
    return B.Perceiver_Blip_EVA_ViT(None, None, ev, SimpleNamespace(**a), embed_dim=meta["embed_dim"])


@pytest.mark.parametrize("modality", ["pc", "audio"])
def test_restatement_equals_the_reference_fixture(modality):
    """tests/golden/eva_tiny.npz (the reference's own modules in fp64, tools/gen_eva_golden.py): features, forward_features
    tokens, the loss, and every parameter's gradient - recorded as (2-norm, sum, dot with a seeded probe) - against the oracle's
    Lens + eva_ref.tower with fp64 autograd, to 1e-10 relative."""
    z, meta = _fixture()
    m = meta[modality]
    sd = {k: v.double().requires_grad_(v.is_floating_point() and "running_" not in k)
          for k, v in eva_ref.fixture_state(modality, m["linear_head"], m["seed"]).items()}
    x = torch.from_numpy(z[modality + "/in/x"]).double()
    fps = torch.from_numpy(z[modality + "/in/fps_start"]) if modality == "pc" else None
    feat, tok = eva_ref.lens_tower(sd, modality, x, meta["heads"], fps)
    rel = lambda a, b: float((a - b).norm() / b.norm())
    assert rel(feat.detach(), torch.from_numpy(z[modality + "/out/features"])) < 1e-10
    assert rel(tok.detach(), torch.from_numpy(z[modality + "/out/tokens"])) < 1e-10
    loss = (feat * torch.from_numpy(z[modality + "/in/dfeat"]).double()).sum()
    assert abs(float(loss.detach()) - float(z[modality + "/out/loss"])) < 1e-10 * abs(float(z[modality + "/out/loss"]))
    loss.backward()
    stats = torch.from_numpy(z[modality + "/grad/stats"])
    assert len(m["grad_names"]) == stats.shape[0] >= 90
    for i, n in enumerate(m["grad_names"]):
        key = "visual." + ("eva_vit.head." + n.split(".", 1)[1] if n.startswith("eva_vit_proj.") else n)
        g = sd[key].grad
        assert g is not None and list(g.shape) == m["grad_shapes"][i], n
        got = torch.stack([g.norm(), g.sum(), (g.reshape(-1) * eva_ref.probe(n, g.numel())).sum()])
        # (|sum| and |dot| are bounded by ||g|| sqrt(n) and ||g|| ||probe|| ~ ||g|| sqrt(n): 1e-10 relative to that scale)
        scale = float(stats[i, 0]) + 1e-300
        assert float((got - stats[i]).abs().max()) < 1e-10 * scale * max(1.0, g.numel() ** 0.5), (n, got.tolist(), stats[i].tolist())


@pytest.mark.parametrize("modality", ["pc", "audio"])
def test_module_equals_the_fixture_names_shapes_and_lock(modality):
    z, meta = _fixture()
    m = meta[modality]
    ours = {k: list(v.shape) for k, v in _module_for(modality, meta).state_dict().items() if "num_batches_tracked" not in k}
    assert ours == dict(zip(m["state_names"], m["state_shapes"])), set(ours) ^ set(m["state_names"])
    for from_head in (False, True):
        mod = _module_for(modality, meta, unlock_from_head=from_head)
        assert [n for n, _ in mod.named_parameters()] == m["grad_names"] or set(n for n, _ in mod.named_parameters()) == set(m["grad_names"])
        for i, kw in enumerate(m["lock_flags"]):
            mod.lock(**kw)
            assert trainable(mod) == m["locks"][f"{int(from_head)}/{i}"], (from_head, kw)
