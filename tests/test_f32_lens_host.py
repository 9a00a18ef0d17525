"""CPU: the plain-torch operand preparation of the fp32 Lenses (vitlens_hip/f32.py) and the predicate that routes a Lens to
them.  BatchNorm folded in fp32 against conv -> BatchNorm at float64; GEGLU interleave / de-interleave; conv-as-GEMM; the
point tokenizer's fp32 operands composed as LensEngineF32 runs them against the oracle's PointTokenizer arithmetic."""
import pytest
import torch

import vitlens_oracle as O
from vitlens_hip import f32 as F
from vitlens_hip.engine import LensCfg, TowerCfg


def rel(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm())


@pytest.mark.parametrize("O_, K", [(128, 3), (512, 512)])
def test_fold_bn_f32_against_conv_then_bn_in_float64(O_, K):
    """The two BatchNorms of the mini-PointNet (dvae.py:183-194, eval mode) folded into the convs before them, in fp32:
    the folded conv evaluated at float64 within 1e-6 relative of conv -> BatchNorm at float64 (the fold itself rounds
    W * s and (b - mean) * s + beta once each in fp32: ~6e-8)."""
    g = torch.Generator().manual_seed(O_ + K)
    w, b = torch.randn(O_, K, generator=g) * K ** -0.5, torch.randn(O_, generator=g) * 0.1
    gamma, beta = 1.0 + 0.05 * torch.randn(O_, generator=g), 0.05 * torch.randn(O_, generator=g)
    rm, rv = 0.1 * torch.randn(O_, generator=g), 1.0 + 0.2 * torch.rand(O_, generator=g)
    x = torch.randn(256, K, generator=g, dtype=torch.float64)
    ref = ((x @ w.double().t() + b.double()) - rm.double()) / torch.sqrt(rv.double() + 1e-5) * gamma.double() + beta.double()
    wf, bf = F.fold_bn_f32(w, b, gamma, beta, rm, rv)
    assert wf.dtype == torch.float32 and bf.dtype == torch.float32
    got = x @ wf.double().t() + bf.double()
    e = rel(got, ref)
    print(f"fp32 BatchNorm fold [{O_}x{K}]: {e:.2e} relative to conv -> BN at float64")
    assert e <= 1e-6, e


def test_geglu_interleave_round_trips_exactly():
    g = torch.Generator().manual_seed(1)
    D = 48
    w, b = torch.randn(8 * D, D, generator=g), torch.randn(8 * D, generator=g)
    wi, bi = F.interleave_geglu(w, b)
    half = 4 * D
    assert torch.equal(wi[0::2], w[:half]) and torch.equal(wi[1::2], w[half:])       # rows (a_j, gate_j)
    assert torch.equal(bi[0::2], b[:half]) and torch.equal(bi[1::2], b[half:])
    w2, b2 = F.deinterleave_geglu(wi, bi)
    assert torch.equal(w2, w) and torch.equal(b2, b)
    # the GEGLU of the interleaved product is the reference's chunk(2) form (perceiver.py:85-89)
    x = torch.randn(5, D, generator=g, dtype=torch.float64)
    h = x @ wi.double().t() + bi.double()
    a, gates = (x @ w.double().t() + b.double()).chunk(2, dim=-1)
    assert torch.equal(h[:, 0::2] * O.gelu_erf(h[:, 1::2]), a * O.gelu_erf(gates))


@pytest.mark.parametrize("kernel,stride,transpose", [((14, 14), (10, 10), True), ((1, 3), (1, 2), False)])
def test_conv_as_gemm_f32(kernel, stride, transpose):
    """AST conv (transpose_hw, f / t strides) and the EEG Conv1d as [O, K padded to 64] GEMM operands: unfold columns
    (c, i, j) times the operand = the convolution."""
    g = torch.Generator().manual_seed(2)
    C = 1 if transpose else 8
    w = torch.randn(32, C, *kernel, generator=g)
    x = torch.randn(2, C, 40 if transpose else 1, 64 if transpose else 40, generator=g)
    wg = F.conv_as_gemm_f32(w)
    K = w[0].numel()
    assert wg.shape == (32, (K + 63) // 64 * 64) and float(wg[:, K:].abs().max()) == 0.0
    cols = torch.nn.functional.unfold(x, kernel, stride=stride).transpose(1, 2)           # [N, T, K]
    got = cols @ wg[:, :K].t()
    ref = torch.nn.functional.conv2d(x, w, stride=stride).flatten(2).transpose(1, 2)
    assert rel(got, ref) < 1e-6


def _tower():
    return TowerCfg()                       # ViT-L/14: width 1024, 16 heads (head dim 64)


def test_f32_lens_supported_predicate():
    t = _tower()
    released = [LensCfg(modality="audio", perceiver_identity=False, depth=2, self_per_cross=3),
                LensCfg(modality="eeg", perceiver_identity=False, depth=1, self_per_cross=1),
                LensCfg(modality="pc", perceiver_identity=False, depth=4, self_per_cross=1, input_chan=384),
                LensCfg(modality="depth", perceiver_identity=False)]
    assert all(F.f32_lens_supported(t, L) for L in released)
    assert F.f32_lens_supported(TowerCfg(width=64, heads=2), LensCfg(modality="audio", perceiver_identity=False, latent_dim=64,
                                                                    input_chan=64, latent_heads=2, latent_dim_head=32))
    no = [LensCfg(modality="pc", perceiver_identity=False, pc_tokenizer="pnsa"),
          LensCfg(modality="audio", perceiver_identity=False, latent_dim_head=48),
          LensCfg(modality="audio", perceiver_identity=False, cross_dim_head=128),
          LensCfg(modality="pc", perceiver_identity=True),
          LensCfg(modality="image")]
    assert not any(F.f32_lens_supported(t, L) for L in no)
    assert not F.f32_lens_supported(TowerCfg(width=768, heads=16), released[0])        # tower head dim 48
    assert not F.f32_lens_supported(t, None)


def test_point_tokenizer_operands_compose_to_the_oracle():
    """point_tokenizer_operands_f32 run in PointTokenizerEngineF32's dataflow (padded K, folded BatchNorms, global / local
    halves of second_conv.0 with the broadcast group maximum added before the ReLU, tokens + pos) in fp32 torch, on the
    oracle's own neighbour sets: within 1e-5 of O.point_tokens (tokens + pos)."""
    g = torch.Generator().manual_seed(3)
    spec = O.TowerSpec(width=64, layers=1, heads=2, patch=8, image_size=32, embed_dim=32)
    lens = O.LensSpec(modality="pc", perceiver_identity=True, pc_num_group=16, pc_group_size=8, pc_encoder_dims=64, pc_trans_dim=96)
    sd = O.init_lens(spec, lens, g)
    B, N, G, M = 2, 256, 16, 8
    pts = torch.randn(B, N, 3, generator=g)
    start = torch.zeros(B, dtype=torch.long)
    tok, pos, cidx, nidx = O.point_tokens(sd, "visual.", pts, lens, start)
    op = F.point_tokenizer_operands_f32(sd, "visual.visual_adapter.")
    center = torch.gather(pts, 1, cidx[:, :, None].expand(B, G, 3))
    nb = torch.gather(pts[:, None].expand(B, G, N, 3), 2, nidx[..., None].expand(B, G, M, 3)) - center[:, :, None]
    patches = torch.zeros(B * G * M, op["w1"].shape[1])
    patches[:, :3] = nb.reshape(-1, 3)
    h1 = torch.relu(patches @ op["w1"].t() + op["b1"])
    f = h1 @ op["w2"].t() + op["b2"]
    t = f.view(B * G, M, -1).max(1).values @ op["w3g"].t() + op["b3"]
    h2 = torch.relu(f @ op["w3l"].t() + t.repeat_interleave(M, 0))
    f2 = h2 @ op["w4"].t() + op["b4"]
    tk = f2.view(B * G, M, -1).max(1).values @ op["wr"].t() + op["br"]
    c = torch.zeros(B * G, op["wp0"].shape[1])
    c[:, :3] = center.reshape(-1, 3)
    got = O.gelu_erf(c @ op["wp0"].t() + op["bp0"]) @ op["wp2"].t() + op["bp2"] + tk
    e = rel(got, (tok + pos).reshape(B * G, -1))
    assert e < 1e-5, e
    assert op["w1"].shape[1] % 4 == 0 and op["wp0"].shape[1] % 4 == 0
    assert op["w3g"].shape == op["w3l"].shape == (512, 256)
