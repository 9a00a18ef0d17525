"""GPU: the EVA ViT tower (`engine.EvaVitEngine`: no ln_pre, LayerNorm eps 1e-6, qkv bias on q and v only, head dim 88) on the
existing run_blocks, against the fp64 restatement tests/eva_ref.py evaluated on the bf16-rounded GEMM weights.

Criteria and bounds are those of tests/test_hip_towers.py: relative 2-norm error of the raw features below 2e-2 on an fp32
residual stream and 4e-2 on a bf16 one (its bound at 24 to 48 blocks; these towers have 2 or 3), 1 - cosine below 1e-3 per
sample.  The token stream (`trunk(..., tokens_out=True)`, what forward_features returns) is held to the same relative bound.

Worst values of the first MI355X run (all below half the bound: 2 / 3 blocks against the 24 - 48 the bound was set at):
  tiny tower (176 = 2 x 88, 3 blocks, 17 tokens)  fp32 stream: features 4.3e-3, tokens 2.7e-3;  bf16 stream: 6.0e-3 / 5.2e-3
  full width (1408 = 16 x 88, 2 blocks, 257 tokens, B = 2)  fp32 stream: features 2.7e-3, tokens 1.7e-3;  bf16 stream: 4.7e-3 / 4.1e-3
  1 - cosine at most 2.9e-5.  The eps pair: fp64 features at eps 1e-6 and 1e-5 are 0.24 (tiny) and 0.14 (full) apart, the
  engine is 3.0 - 3.3e-3 from the one it was given."""
import dataclasses

import pytest
import torch

import eva_ref

pytestmark = pytest.mark.gpu

P = "visual."
F32, BF16 = torch.float32, torch.bfloat16
TOL = {F32: 2e-2, BF16: 4e-2}


def _E():
    from vitlens_hip import engine
    return engine


def relerr(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / b.norm())


def check(got, ref, tol, what, cosine=True):
    e = relerr(got, ref)
    c = float((1 - torch.nn.functional.cosine_similarity(got.double().cpu(), ref.double().cpu(), dim=-1)).max())
    print(f"MEASURED {what}: relative error {e:.3e} (bound {tol:.1e}), 1 - cosine {c:.3e}")
    assert e < tol, (what, e)
    if cosine:
        assert c < 1e-3, (what, c)


_CASES = {}


def case(name):
    """(state, tokens f32 [B,T,D], heads, E) of a seeded tower; the fp64 results are added by the tests and shared."""
    if name not in _CASES:
        D, H, depth, L, E, B, lin = {"tiny": (176, 2, 3, 17, 32, 4, False), "tiny_linear": (176, 2, 3, 17, 32, 4, True),
                                     "full": (1408, 16, 2, 257, 768, 2, False)}[name]
        sd = eva_ref.init_state(P, D, H, depth, L, E, seed=len(name), linear_head=lin)
        tok = torch.randn(B, L - 1, D, generator=torch.Generator().manual_seed(5)).bfloat16().float()
        _CASES[name] = dict(sd=sd, tok=tok, H=H, E=E, D=D, depth=depth, ref={})
    return _CASES[name]


def reference(c, eps=1e-6):
    """fp64 on the bf16-rounded weights, on the GPU (torch's fp64 matmul: the reference, not the code under test), once."""
    if eps not in c["ref"]:
        sd = {k: v.cuda() for k, v in eva_ref.rounded(c["sd"]).items()}
        with torch.no_grad():
            f, x = eva_ref.tower(sd, P, c["tok"].cuda(), c["H"], eps)
        c["ref"][eps] = (f.cpu(), x.cpu())
    return c["ref"][eps]


def engine_for(c, res_dtype, **cfg_kw):
    E = _E()
    cfg = E.eva_tower_cfg(width=c["D"], layers=c["depth"], heads=c["H"], embed_dim=c["E"])
    return E.EvaVitEngine(c["sd"], P, dataclasses.replace(cfg, **cfg_kw), "cuda", res_dtype=res_dtype)


@pytest.mark.parametrize("res_dtype", [F32, BF16])
@pytest.mark.parametrize("name", ["tiny", "tiny_linear", "full"])
def test_eva_tower_features_and_tokens(name, res_dtype):
    """Pooled features (eva_vit_proj, and the nn.Linear head with its bias) and the token stream.  `full`: the GEMMs are
    N = 1408 / 4224 / 6144 with K = 1408 / 6144 on 514 rows, the attention runs head dim 88 at L = 257, every LayerNorm is the
    D = 1408 form (fp32 stream) and the tower has no ln_pre."""
    c = case(name)
    eng = engine_for(c, res_dtype)
    B, T, D = c["tok"].shape
    tok = c["tok"].cuda().bfloat16().reshape(B * T, D)
    ref_f, ref_x = reference(c)
    got = eng.trunk(tok, B)
    assert tuple(got.shape) == (B, c["E"]) and got.dtype == F32
    check(got, ref_f, TOL[res_dtype], f"{name} {res_dtype} features")
    x = eng.trunk(tok, B, tokens_out=True)
    assert tuple(x.shape) == (B, T + 1, D) and x.dtype == res_dtype
    check(x.reshape(B * (T + 1), D), ref_x.reshape(B * (T + 1), D), TOL[res_dtype], f"{name} {res_dtype} tokens")
    # the token call ran the last block on every row and left the workspace as the pooled call needs it
    again = eng.trunk(tok, B)
    assert torch.equal(again, got)


def test_eva_tower_head_bias_enters_the_forward():
    c = case("tiny_linear")
    eng = engine_for(c, F32)
    B, T, D = c["tok"].shape
    tok = c["tok"].cuda().bfloat16().reshape(B * T, D)
    with_bias = eng.trunk(tok, B)
    eng.proj_b.zero_()
    without = eng.trunk(tok, B)
    bias = c["sd"][P + "eva_vit.head.bias"].cuda()
    assert float((with_bias - without - bias).abs().max()) < 1e-5 and float(bias.abs().max()) > 0.05


@pytest.mark.parametrize("name", ["tiny", "full"])
def test_eva_tower_reads_ln_eps(name):
    """Rows whose variance is near 1e-5 in front of block 0 (everything = 0.5 + 3e-3 noise, fp32 tokens on an fp32 stream): the
    fp64 results at eps 1e-6 and 1e-5 are further apart than the bound, so an engine that dropped TowerCfg.ln_eps anywhere in
    block 0 - the LayerNorm pass, ln_post - fails one of the two."""
    c = dict(case(name))
    g = torch.Generator().manual_seed(9)
    sd = dict(c["sd"])
    L, D = sd[P + "eva_vit.pos_embed"].shape[1:]
    sd[P + "eva_vit.pos_embed"] = 0.5 + 3e-3 * torch.randn(1, L, D, generator=g)
    sd[P + "eva_vit.cls_token"] = 3e-3 * torch.randn(1, 1, D, generator=g)
    B = c["tok"].shape[0]
    c.update(sd=sd, tok=3e-3 * torch.randn(B, L - 1, D, generator=g), ref={})
    var = float((sd[P + "eva_vit.pos_embed"][0, 1:] + c["tok"][0]).var(-1, unbiased=False).mean())
    assert 5e-6 < var < 4e-5, var
    refs = {eps: reference(c, eps)[0] for eps in (1e-6, 1e-5)}
    apart = relerr(refs[1e-6], refs[1e-5])
    print(f"MEASURED {name}: fp64 features at eps 1e-6 and 1e-5 are {apart:.3e} apart (bound {TOL[F32]:.1e})")
    assert apart > 2 * TOL[F32], apart
    tok = c["tok"].cuda().reshape(-1, D)
    for eps in (1e-6, 1e-5):
        got = engine_for(c, F32, ln_eps=eps).trunk(tok, B)
        check(got, refs[eps], TOL[F32], f"{name} eps={eps:g}", cosine=False)
