"""fp64 restatement of the EVA ViT tower of `Perceiver_Blip_EVA_ViT` (open_clip/third_vit/blip_eva_vit.py), in plain torch on
the module's own state_dict names (`eva_vit.cls_token`, `eva_vit.blocks.N.attn.q_bias`, `eva_vit_proj` ...): ours, in the
style of the other *_ref.py.  Every operand is converted to fp64 exactly and nothing is rounded on the way, so autograd through
these functions is the fp64 gradient.  `rounded(sd)` gives the state as a bf16-operand engine reads it (GEMM weights rounded to
bf16, everything else fp32), which is what the GPU tests compare against.

    tokens [B, T, D] -> x = [cls ; tokens] + pos_embed (+ pos2 on rows 1..T)              (no ln_pre)
    per block:  x = x + proj(softmax(q k^T / sqrt(dh)) v),  [q|k|v] = norm1(x) W_qkv^T + [q_bias, 0, v_bias]
                x = x + fc2(gelu_erf(fc1(norm2(x))))
    stream = x                                                (forward_features: what an MLLM's ln_vision reads)
    feature = norm(x[:, 0]) @ eva_vit_proj        or        head(norm(x[:, 0]))           (LayerNorm eps 1e-6 throughout)"""
import math

import torch

GEMM_WEIGHTS = ("attn.qkv.weight", "attn.proj.weight", "mlp.fc1.weight", "mlp.fc2.weight", "eva_vit_proj", "eva_vit.head.weight")


def f64(t):
    return t.to(torch.float64)


def layer_norm(x, w, b, eps):
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + eps) * f64(w) + f64(b)


def gelu_erf(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def block(sd, p, x, heads, eps):
    B, L, D = x.shape
    dh = D // heads
    h = layer_norm(x, sd[p + "norm1.weight"], sd[p + "norm1.bias"], eps)
    bias = torch.cat([f64(sd[p + "attn.q_bias"]), torch.zeros(D, dtype=torch.float64, device=x.device), f64(sd[p + "attn.v_bias"])])
    qkv = (h @ f64(sd[p + "attn.qkv.weight"]).t() + bias).reshape(B, L, 3, heads, dh).permute(2, 0, 3, 1, 4)
    att = torch.softmax(qkv[0] @ qkv[1].transpose(-2, -1) * dh ** -0.5, dim=-1)
    a = (att @ qkv[2]).transpose(1, 2).reshape(B, L, D)
    x = x + a @ f64(sd[p + "attn.proj.weight"]).t() + f64(sd[p + "attn.proj.bias"])
    h = layer_norm(x, sd[p + "norm2.weight"], sd[p + "norm2.bias"], eps)
    h = gelu_erf(h @ f64(sd[p + "mlp.fc1.weight"]).t() + f64(sd[p + "mlp.fc1.bias"]))
    return x + h @ f64(sd[p + "mlp.fc2.weight"]).t() + f64(sd[p + "mlp.fc2.bias"])


def depth_of(sd, prefix):
    n = 0
    while f"{prefix}eva_vit.blocks.{n}.norm1.weight" in sd:
        n += 1
    return n


def tower(sd, prefix, tokens, heads, eps=1e-6, use_pos=True, pos2=None):
    """-> (feature [B, E], stream [B, T+1, D]) in fp64."""
    e = prefix + "eva_vit."
    t = f64(tokens)
    B, T, D = t.shape
    if pos2 is not None:
        t = t + f64(pos2)
    x = torch.cat([f64(sd[e + "cls_token"]).reshape(1, 1, D).expand(B, 1, D), t], 1)
    if use_pos and e + "pos_embed" in sd:
        x = x + f64(sd[e + "pos_embed"]).reshape(1, T + 1, D)
    for n in range(depth_of(sd, prefix)):
        x = block(sd, f"{e}blocks.{n}.", x, heads, eps)
    pooled = layer_norm(x[:, 0], sd[e + "norm.weight"], sd[e + "norm.bias"], eps)
    if prefix + "eva_vit_proj" in sd:
        return pooled @ f64(sd[prefix + "eva_vit_proj"]), x
    return pooled @ f64(sd[e + "head.weight"]).t() + f64(sd[e + "head.bias"]), x


def init_state(prefix, D, heads, depth, L, E, seed, linear_head=False):
    """A seeded EVA ViT state under the module's names, with every parameter away from its trivial value (LayerNorm weights
    1 +- 0.1, biases +- 0.1, a q / v bias) so that nothing can be dropped unnoticed.  hidden = int(D * 4.3637)."""
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s, std=1.0: torch.randn(*s, generator=g) * std
    hidden = int(D * 4.3637)
    e = prefix + "eva_vit."
    sd = {e + "cls_token": rn(1, 1, D, std=0.5), e + "pos_embed": rn(1, L, D, std=0.5),
          e + "norm.weight": 1 + rn(D, std=0.1), e + "norm.bias": rn(D, std=0.1)}
    for n in range(depth):
        p = f"{e}blocks.{n}."
        for nm in ("norm1", "norm2"):
            sd[p + nm + ".weight"], sd[p + nm + ".bias"] = 1 + rn(D, std=0.1), rn(D, std=0.1)
        sd[p + "attn.qkv.weight"] = rn(3 * D, D, std=D ** -0.5)
        sd[p + "attn.q_bias"], sd[p + "attn.v_bias"] = rn(D, std=0.1), rn(D, std=0.1)
        sd[p + "attn.proj.weight"], sd[p + "attn.proj.bias"] = rn(D, D, std=D ** -0.5), rn(D, std=0.1)
        sd[p + "mlp.fc1.weight"], sd[p + "mlp.fc1.bias"] = rn(hidden, D, std=D ** -0.5), rn(hidden, std=0.1)
        sd[p + "mlp.fc2.weight"], sd[p + "mlp.fc2.bias"] = rn(D, hidden, std=hidden ** -0.5), rn(D, std=0.1)
    if linear_head:
        sd[e + "head.weight"], sd[e + "head.bias"] = rn(E, D, std=D ** -0.5), rn(E, std=0.1)
    else:
        sd[prefix + "eva_vit_proj"] = rn(D, E, std=D ** -0.5)
    return sd


def rounded(sd):
    """The state as a bf16-operand engine reads it: the GEMM weights rounded to bf16 (and back to fp32), the rest untouched."""
    return {k: (v.bfloat16().float() if k.endswith(GEMM_WEIGHTS) else v.clone()) for k, v in sd.items()}


# ---- the seeded towers of tests/golden/eva_tiny.npz (tools/gen_eva_golden.py loads these into the reference's modules) ----
def fixture_state(modality, linear_head, seed, D=176, heads=2, depth=3, latents=16, E=32):
    """The whole tower's state under `visual.`: init_state for the EVA ViT and the oracle's init_lens for the Lens in front of it."""
    import vitlens_oracle as O
    sd = init_state("visual.", D, heads, depth, latents + 1, E, seed, linear_head=linear_head)
    spec = O.TowerSpec(width=D, layers=depth, heads=heads, patch=14, image_size=56, embed_dim=E)
    sd.update(O.init_lens(spec, fixture_lens(modality, D, heads, latents), torch.Generator().manual_seed(seed + 1), "visual."))
    return sd


def fixture_lens(modality, D=176, heads=2, latents=16):
    import vitlens_oracle as O
    common = dict(perceiver_identity=False, depth=2, self_per_cross=1, num_latents=latents, latent_dim=D, cross_heads=1,
                  latent_heads=heads, latent_dim_head=88)
    if modality == "audio":
        return O.LensSpec(modality="audio", input_chan=D, cross_dim_head=88, audio_fstride=6, audio_tstride=6, audio_mel_bins=32,
                          audio_target_length=48, **common)
    return O.LensSpec(modality="pc", input_chan=64, cross_dim_head=64, pc_num_group=16, pc_group_size=8, pc_encoder_dims=64,
                      pc_trans_dim=64, **common)


def fixture_inputs(modality, seed, B=4, E=32):
    g = torch.Generator().manual_seed(seed + 100)
    x = torch.randn(B, 48, 32, generator=g) if modality == "audio" else torch.rand(B, 256, 3, generator=g) * 2 - 1
    return x, {"dfeat": torch.randn(B, E, generator=g)}


def probe(name, n):
    """A seeded fp64 probe vector for the parameter `name`: a gradient is recorded as (2-norm, sum, dot with this)."""
    seed = sum((i + 1) * ord(c) for i, c in enumerate(name)) % (2 ** 31)
    return torch.randn(n, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


def lens_tower(sd, modality, x, heads=2, fps_start=None):
    """The oracle's tokenizer and Perceiver in front of `tower`, on the dtype of `sd` -> (features, tokens)."""
    import vitlens_oracle as O
    lens = fixture_lens(modality)
    if modality == "audio":
        t, pos = O.audio_tokens(sd, "visual.", x, lens)
    else:
        t, pos, _, _ = O.point_tokens(sd, "visual.", x, lens, fps_start, False, None)
    return tower(sd, "visual.", O.perceiver(sd, "visual.perceiver.", t + pos, lens), heads)
