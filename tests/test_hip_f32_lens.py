"""GPU: true fp32 inference for the Lenses with a Perceiver - audio, EEG, point cloud (pointbert) and depth - under
precision="fp32" (vitlens_hip/f32.py: LensEngineF32, PerceiverEngineF32, PointTokenizerEngineF32) and the kernels they added:
vl_gemm_f32_ex (GEGLU epilogue; broadcast residual before the activation), vl_knn_group_f32, vl_group_max_f32, vl_pad3_f32.

Per-kernel checks are against float64 per block (tests/errloc.py).  The tolerance of each is 4x the worst block of the same op
computed by torch float32 on the CPU on the same inputs: the kernels sum K as one sequential fmaf chain, a blocked CPU sum
rounds less.  Where the CPU op is exact (one key: softmax weight 1), the tolerance is 4x one fp32 rounding unit (2^-24): a
bound below the format's own resolution could not be shown to fail.  Every check is shown to fail on the kernel's own output
with one block scaled by 1 + 3 tol.  Outputs start as NaN; every case runs twice and must be bit-identical."""
import json
import os
import tempfile
import warnings
from types import SimpleNamespace

import pytest
import torch

import vitlens_oracle as O
from errloc import assert_attn_blocks, assert_blocks, attn_block_relerr, block_relerr
from golden_util import load_npz, specs_from_meta, split

pytestmark = pytest.mark.gpu

EPS32 = 2.0 ** -24


def _ops():
    from vitlens_hip import ops
    return ops


def rnd(*shape, scale=1.0, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def relerr(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-300))


def nan_like(*shape):
    return torch.full(shape, float("nan"), device="cuda")


def _tol(cpu_worst):
    return 4.0 * max(cpu_worst, EPS32)


def _scaled_block_fails(out, r0, r1, c0, c1, tol, check):
    bad = out.clone()
    bad[r0:r1, c0:c1] *= 1.0 + 3.0 * tol
    with pytest.raises(AssertionError):
        check(bad)


# ------------------------------------------------------------------------------------------------ GEGLU epilogue
def _geglu64(a, w, b):
    h = a.double() @ w.double().t() + b.double()
    return h[:, 0::2] * O.gelu_erf(h[:, 1::2])


@pytest.mark.parametrize("M,N,K", [(300, 8192, 1024), (77, 200, 36), (128, 128, 16), (1, 2, 4)])
def test_gemm_f32_geglu_per_block(M, N, K):
    """out[m, j] = (acc[2j] + b[2j]) * gelu(acc[2j+1] + b[2j+1]) on interleaved rows, per block of 128 rows x 64 output columns."""
    ops = _ops()
    a, w, b = rnd(M, K, seed=1), rnd(N, K, scale=K ** -0.5, seed=2), rnd(N, scale=0.5, seed=3)
    ref = _geglu64(a, w, b)
    h32 = a @ w.t() + b
    cpu = h32[:, 0::2] * O.gelu_erf(h32[:, 1::2])
    cw, _ = block_relerr(cpu, ref, 128, 64)
    tol = _tol(cw)
    ac, wc, bc = a.cuda(), w.cuda(), b.cuda()
    outs = []
    for _ in range(2):
        out = nan_like(M, N // 2)
        ops.gemm_f32_ex(ac, wc, bc, out=out, geglu=True)
        outs.append(out)
    assert torch.equal(outs[0], outs[1])
    got = outs[0].cpu()
    assert bool(torch.isfinite(got).all())
    kw, (r0, r1, c0, c1) = block_relerr(got, ref, 128, 64)
    print(f"GEGLU [{M}x{N}x{K}]: kernel worst block {kw:.3e}, CPU fp32 {cw:.3e}, ratio {kw / max(cw, EPS32):.2f}, tol {tol:.3e}")
    check = lambda o: assert_blocks(o, ref, tol, 128, 64, what="GEGLU")
    check(got)
    _scaled_block_fails(got, r0, r1, c0, c1, tol, check)


def test_gemm_f32_ex_refusals_write_nothing():
    ops = _ops()
    a, w, b = rnd(64, 32, seed=1).cuda(), rnd(64, 32, seed=2).cuda(), rnd(64, seed=3).cuda()
    out = nan_like(64, 64)
    res = torch.zeros(64, 64, device="cuda")
    with pytest.raises(RuntimeError):
        ops.gemm_f32_ex(a, w, b, out=out[:, :32], geglu=True, res=res[:, :32])            # residual with GEGLU
    with pytest.raises(RuntimeError):
        ops.gemm_f32_ex(a, w[:63], b[:63], out=out[:, :32], geglu=True)                    # odd N
    big = torch.zeros(64, 33, device="cuda")
    with pytest.raises(RuntimeError):
        ops.gemm_f32_ex(big[:, 1:], w, b, out=out, res=res, res_pre=True)                  # A not 16-byte aligned (row stride 33)
    with pytest.raises(RuntimeError):
        ops.gemm_f32_ex(a, w, b, out=out, res=res, res_div=2)                              # res_div without res_pre
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())


@pytest.mark.parametrize("act", [0, 1, 2])
def test_gemm_f32_ex_defaults_are_gemm_f32_bit_for_bit(act):
    ops = _ops()
    M, N, K = 300, 130, 68
    a, w, b, r = (rnd(*s, seed=i).cuda() for i, s in enumerate([(M, K), (N, K), (N,), (M, N)]))
    for res in (None, r):
        x = ops.gemm_f32(a, w, b, act=act, res=res, out=nan_like(M, N))
        y = ops.gemm_f32_ex(a, w, b, act=act, res=res, out=nan_like(M, N))
        assert torch.equal(x, y)


# ------------------------------------------------------------------------------------------------ residual before ReLU
@pytest.mark.parametrize("res_div,M", [(32, 32 * 39 + 5), (8, 8 * 150 + 3), (32, 32 * 64)])
def test_gemm_f32_broadcast_residual_before_relu_per_block(res_div, M):
    """PointBERT's second conv: relu(f @ W3l^T + t[row / res_div]), per block of 128 x 128, ragged M."""
    ops = _ops()
    N, K = 512, 256
    G = (M + res_div - 1) // res_div
    f, w, t = rnd(M, K, seed=4), rnd(N, K, scale=K ** -0.5, seed=5), rnd(G, N, seed=6)
    rows = torch.arange(M) // res_div
    ref = torch.relu(f.double() @ w.double().t() + t.double()[rows])
    cpu = torch.relu(f @ w.t() + t[rows])
    cw, _ = block_relerr(cpu, ref, 128, 128)
    tol = _tol(cw)
    outs = []
    for _ in range(2):
        out = nan_like(M, N)
        ops.gemm_f32_ex(f.cuda(), w.cuda(), None, out=out, res=t.cuda(), res_div=res_div, res_pre=True, act=ops.ACT_RELU)
        outs.append(out)
    assert torch.equal(outs[0], outs[1])
    got = outs[0].cpu()
    kw, (r0, r1, c0, c1) = block_relerr(got, ref, 128, 128)
    print(f"residual before ReLU res_div={res_div} M={M}: kernel worst block {kw:.3e}, CPU fp32 {cw:.3e}, "
          f"ratio {kw / max(cw, EPS32):.2f}, tol {tol:.3e}")
    check = lambda o: assert_blocks(o, ref, tol, 128, 128, what="residual before ReLU")
    check(got)
    _scaled_block_fails(got, r0, r1, c0, c1, tol, check)


# ------------------------------------------------------------------------------------------------ cross attention
@pytest.mark.parametrize("Lk", [1, 65, 512, 600, 1212])
def test_attn_fwd_f32_cross_attention_per_tile(Lk):
    """Perceiver cross attention on attn_fwd_f32: Lq = 256 latents, Lk context tokens, per (b, h, 32-query tile)."""
    ops = _ops()
    B, H, dh, Lq = 2, 2, 64, 256
    D = H * dh
    q2, kv2 = rnd(B * Lq, D, seed=7), rnd(B * Lk, 2 * D, seed=8)
    hv = lambda x, L, c0: x.reshape(B, L, x.shape[1])[:, :, c0:c0 + D].reshape(B, L, H, dh).permute(0, 2, 1, 3)
    q, k, v = hv(q2, Lq, 0), hv(kv2, Lk, 0), hv(kv2, Lk, D)
    s64 = (q.double() @ k.double().transpose(-1, -2)) * dh ** -0.5
    ref = torch.softmax(s64, -1) @ v.double()
    cpu = torch.softmax((q @ k.transpose(-1, -2)) * dh ** -0.5, -1) @ v
    cw, _ = attn_block_relerr(cpu, ref, B, H, Lq)
    tol = _tol(cw)
    qc, kvc = q2.cuda(), kv2.cuda()
    outs = []
    for _ in range(2):
        out = nan_like(B * Lq, D)
        ops.attn_fwd_f32(ops.heads_view(qc, B, Lq, H, dh), ops.heads_view(kvc, B, Lk, H, dh), ops.heads_view(kvc, B, Lk, H, dh, D),
                         out, scale=dh ** -0.5)
        outs.append(out)
    assert torch.equal(outs[0], outs[1])
    got = outs[0].cpu()
    kw, (b, h, r0, r1) = attn_block_relerr(got, ref, B, H, Lq)
    print(f"cross attention Lk={Lk}: kernel worst block {kw:.3e}, CPU fp32 {cw:.3e}, ratio {kw / max(cw, EPS32):.2f}, tol {tol:.3e}")
    check = lambda o: assert_attn_blocks(o, ref, tol, B, H, Lq, rows="queries", what="cross attention")
    check(got)
    bad = got.clone()
    bad.view(B, Lq, H, dh)[b, r0:r1, h] *= 1.0 + 3.0 * tol
    with pytest.raises(AssertionError):
        check(bad)


# ------------------------------------------------------------------------------------------------ point-tokenizer pieces
@pytest.mark.parametrize("B,N,G,k", [(2, 8192, 512, 32), (2, 1024, 20, 16), (1, 320, 16, 8)])
def test_knn_group_f32_patches_exact(B, N, G, k):
    """fp32 patches = x_j - centre of the selected points, bit for bit; the same neighbour lists (and order) as the bf16 entry
    (LDS-staged register form, register form, LDS-key form)."""
    ops = _ops()
    g = torch.Generator().manual_seed(N + G)
    pts = torch.randn(B, N, 3, generator=g)
    pts = (pts / pts.norm(dim=-1).max()).cuda()
    cidx, centers = ops.fps(pts, torch.zeros(B, dtype=torch.long, device="cuda"), G)
    runs = []
    for _ in range(2):
        out = nan_like(B * G * k, 4)
        p, nidx = ops.knn_group_f32(pts, cidx, k, Kp=4, want_idx=True, out=out)
        runs.append((p.clone(), nidx.clone()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    p, nidx = runs[0]
    _, nidx16 = ops.knn_group(pts, cidx, k, Kp=64, want_idx=True)
    assert torch.equal(nidx, nidx16)
    nb = torch.gather(pts[:, None].expand(B, G, N, 3), 2, nidx.long()[..., None].expand(B, G, k, 3)) - centers[:, :, None]
    assert torch.equal(p[:, :3], nb.reshape(-1, 3))
    assert bool((p[:, 3] == 0).all())
    with pytest.raises(RuntimeError):
        ops.knn_group_f32(pts, cidx, k, Kp=3)


@pytest.mark.parametrize("groups,M,C", [(65536 // 32, 32, 256), (37, 8, 5)])
def test_group_max_f32_exact_with_nan_and_inf(groups, M, C):
    ops = _ops()
    x = rnd(groups * M, C, seed=9)
    x[3 * M + 1, 2] = float("nan")                                   # a NaN in a group: the group's max is NaN
    x[5 * M:6 * M, 1] = float("-inf")                                # an all -inf group
    x[7 * M + M - 1, 0] = float("inf")
    ref = x.view(groups, M, C).max(1).values
    xc = x.cuda()
    a, b = ops.group_max_f32(xc, M, out=nan_like(groups, C)), ops.group_max_f32(xc, M, out=nan_like(groups, C))
    got = a.cpu()
    nan = torch.isnan(ref)
    assert torch.equal(torch.isnan(got), nan) and int(nan.sum()) == 1          # exactly the group with the NaN
    assert torch.equal(got[~nan], ref[~nan])                                    # everything else exact, +-inf included
    assert float(got[5, 1]) == float("-inf") and float(got[7, 0]) == float("inf")
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_pad3_f32_exact():
    ops = _ops()
    c = rnd(2, 37, 3, seed=10).cuda()
    out = ops.pad3_f32(c, 8)
    assert torch.equal(out[:, :3], c.reshape(-1, 3)) and bool((out[:, 3:] == 0).all())
    with pytest.raises(RuntimeError):
        ops.pad3_f32(c, 3)


# ------------------------------------------------------------------------------------------------ the Perceiver alone
def _lens_spec(modality):
    kw = dict(modality=modality, perceiver_identity=False)
    if modality == "audio":
        kw.update(depth=2, self_per_cross=3)
    if modality == "pc":
        kw.update(depth=4, self_per_cross=1, input_chan=384)
    return O.LensSpec(**kw)


@pytest.mark.parametrize("modality,Tc", [("audio", 600), ("pc", 512)])
def test_fullsize_perceiver_against_float64(modality, Tc):
    """PerceiverEngineF32 at the released audio / pc geometry against the oracle's perceiver() at float64, per 128-latent-row
    block; tolerance 4x the fp32 oracle's own worst block on the same inputs."""
    from vitlens_hip import engine as E, f32 as F
    spec, lens = O.TowerSpec(), _lens_spec(modality)
    g = torch.Generator().manual_seed(5)
    sd = O.init_lens(spec, lens, g)
    B = 2
    data = torch.randn(B, Tc, lens.input_chan, generator=g)
    p = "visual.perceiver."
    ref = O.perceiver({k: v.double() for k, v in sd.items()}, p, data.double(), lens).reshape(B * lens.num_latents, -1)
    cpu = O.perceiver(sd, p, data, lens).reshape(B * lens.num_latents, -1)
    D = ref.shape[1]
    cw, _ = block_relerr(cpu, ref, 128, D)
    tol = _tol(cw)
    lc = E.LensCfg(**{k: getattr(lens, k) for k in O.LensSpec.__dataclass_fields__ if k in E.LensCfg.__dataclass_fields__})
    eng = F.PerceiverEngineF32(sd, p, lc, "cuda")
    dc = data.reshape(B * Tc, -1).cuda()
    got = eng.forward(dc, B).clone()
    again = eng.forward(dc, B).clone()
    assert torch.equal(got, again)
    got = got.cpu()
    kw, (r0, r1, c0, c1) = block_relerr(got, ref, 128, D)
    print(f"Perceiver {modality}: kernel worst block {kw:.3e}, fp32 oracle {cw:.3e}, ratio {kw / cw:.2f}, tol {tol:.3e}")
    check = lambda o: assert_blocks(o, ref, tol, 128, D, what=f"{modality} Perceiver")
    check(got)
    _scaled_block_fails(got, r0, r1, c0, c1, tol, check)


# ------------------------------------------------------------------------------------------------ tiny goldens
def _pc_tokens_on_sets(sd, a, pts, cidx, nidx, lens):
    """The oracle's PointTokenizer arithmetic (vitlens_oracle.point_tokens, eval-mode BatchNorm) on GIVEN fps / kNN index sets:
    kNN may legitimately swap near-equidistant points (test_hip_points.py::test_knn_sets)."""
    B, N, _ = pts.shape
    G, M = cidx.shape[1], nidx.shape[2]
    center = torch.gather(pts, 1, cidx[:, :, None].expand(B, G, 3))
    nb = torch.gather(pts[:, None].expand(B, G, N, 3), 2, nidx[..., None].expand(B, G, M, 3)) - center[:, :, None, :]
    x = nb.reshape(B * G, M, 3).transpose(1, 2)
    conv1 = lambda x, name: torch.einsum("oc,bcn->bon", sd[a + name + ".weight"][:, :, 0], x) + sd[a + name + ".bias"].view(1, -1, 1)
    f = torch.relu(O.batch_norm_1d(conv1(x, "encoder.first_conv.0"), sd, a + "encoder.first_conv.1.", False))
    f = conv1(f, "encoder.first_conv.3")
    f = torch.cat([f.max(dim=2, keepdim=True).values.expand(-1, -1, M), f], dim=1)
    f = torch.relu(O.batch_norm_1d(conv1(f, "encoder.second_conv.0"), sd, a + "encoder.second_conv.1.", False))
    f = conv1(f, "encoder.second_conv.3")
    tok = O.linear(f.max(dim=2).values.reshape(B, G, -1), sd[a + "reduce_dim.weight"], sd[a + "reduce_dim.bias"])
    pos = O.linear(O.gelu_erf(O.linear(center, sd[a + "pos_embed.0.weight"], sd[a + "pos_embed.0.bias"])),
                   sd[a + "pos_embed.2.weight"], sd[a + "pos_embed.2.bias"])
    return tok + pos


def _encode_visual_on_sets(sd, x, spec, lens, cidx, nidx, prefix="visual."):
    tok = _pc_tokens_on_sets(sd, prefix + "visual_adapter.", x, cidx, nidx, lens)
    tok = O.perceiver(sd, prefix + "perceiver.", tok, lens)
    return O.vit_trunk(sd, prefix, tok, spec, lens.use_orig_pos)


def _check_knn_sets(pts, cidx, got, k):
    """The kernel's neighbour sets equal O.knn_indices in every group, except where the swapped points are near-equidistant
    (as test_hip_points.py::test_knn_sets defines it), in at most 1 % of the groups."""
    B, G = cidx.shape
    center = torch.gather(pts, 1, cidx[:, :, None].expand(B, G, 3))
    ref = O.knn_indices(pts, center, k)
    d = ((center[:, :, None, :] - pts[:, None, :, :]) ** 2).sum(-1)
    bad = 0
    for b in range(B):
        for c in range(G):
            s1, s2 = set(ref[b, c].tolist()), set(got[b, c].tolist())
            assert len(s2) == k
            if s1 != s2:
                dd = d[b, c, list(s1 ^ s2)]
                assert float(dd.max() - dd.min()) < 1e-5 * max(1.0, float(dd.max())), (b, c, dd)
                bad += 1
    assert bad <= 0.01 * B * G, bad
    return bad


@pytest.mark.parametrize("modality", ["audio", "audio_tied", "pc", "eeg"])
def test_tiny_goldens_through_lens_engine_f32(modality):
    """LensEngineF32 on the tiny golden models (weight tying, EEG window 3 / stride 2, a ragged audio grid) within 1e-5 of the
    fp32 oracle."""
    from vitlens_hip import engine as E, f32 as F
    sd, ins, outs, grads, meta = split(load_npz(f"tiny_{modality}.npz"))
    tower, text, lens = specs_from_meta(meta)
    tc = E.TowerCfg(width=tower.width, layers=tower.layers, heads=tower.heads, patch=tower.patch, image_size=tower.image_size,
                    embed_dim=tower.embed_dim)
    lc = E.LensCfg(**{k: getattr(lens, k) for k in E.LensCfg.__dataclass_fields__ if hasattr(lens, k)})
    sdo = O.tie_perceiver_layers(dict(sd), lens.depth) if lens.weight_tie_layers else sd
    eng = F.LensEngineF32(sd, "visual.", tc, lc, "cuda")
    x = ins["visual_x"]
    kw = {"fps_start": ins["fps_start"].cuda()} if modality == "pc" else {}
    got = eng.encode(x.cuda(), **kw)
    assert torch.equal(got, eng.encode(x.cuda(), **kw))
    if modality == "pc":
        cidx, _, _, nidx = eng.points.group(x.cuda(), ins["fps_start"].cuda(), want_idx=True)
        assert torch.equal(cidx.cpu(), O.fps_indices(x, lens.pc_num_group, ins["fps_start"]))
        _check_knn_sets(x, cidx.cpu(), nidx.cpu().long(), lens.pc_group_size)
        ref = _encode_visual_on_sets(sdo, x, tower, lens, cidx.cpu(), nidx.cpu().long())
    else:
        ref = O.encode_visual(sdo, x, tower, lens)
    e = relerr(got, ref)
    print(f"tiny {modality}: LensEngineF32 {e:.2e} relative to the fp32 oracle")
    assert e < 1e-5, e


# ------------------------------------------------------------------------------------------------ full size through the API
def _fullsize_model(modality):
    import open_clip as oc
    from mm_vit_lens.model_cfg import fetch_model_cfg
    torch.manual_seed(0)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        model = oc.tri_create_model("ViT-L-14", None, precision="fp32", device="cuda", output_dict=True,
                                    args=fetch_model_cfg(modality=modality))
    tower, lens = model.visual._cfgs()
    spec = O.TowerSpec(**{k: getattr(tower, k) for k in O.TowerSpec.__dataclass_fields__})
    ls = O.LensSpec(**{k: getattr(lens, k) for k in O.LensSpec.__dataclass_fields__})
    g = torch.Generator().manual_seed(5)
    sd = O.init_tower(spec, g, "visual.", with_conv=False)
    sd.update(O.init_lens(spec, ls, g))
    miss = model.load_state_dict(sd, strict=False)
    assert not [k for k in miss.missing_keys if k.startswith("visual.") and not k.endswith("num_batches_tracked")], miss.missing_keys
    model.eval()
    return model, sd, spec, ls


@pytest.mark.parametrize("modality", ["audio", "pc", "eeg"])
def test_fullsize_lens_features_in_fp32_arithmetic(modality):
    """Released ViT-L Lens (fetch_model_cfg), B = 2, seeded weights, tri_create_model(precision="fp32"), .eval(), encode_visual
    under no_grad: within 1e-5 relative of O.encode_visual in fp32 on the CPU, on the new engine.  Point cloud: the reference
    is the oracle's tokenizer arithmetic on the kernel's neighbour sets, which first must equal the oracle's own."""
    from vitlens_hip import f32 as F, ops
    model, sd, spec, ls = _fullsize_model(modality)
    assert "true fp32 arithmetic" in model.precision_effective
    g = torch.Generator().manual_seed(6)
    B = 2
    kw = {}
    if modality == "audio":
        x = torch.randn(B, ls.audio_target_length, ls.audio_mel_bins, generator=g)
    elif modality == "eeg":
        x = torch.randn(B, ls.eeg_chans, ls.eeg_time_len, generator=g)
    else:
        x = torch.randn(B, 8192, 3, generator=g)
        x = x / x.norm(dim=-1).max()
        kw = {"fps_start": torch.zeros(B, dtype=torch.long)}
    with torch.no_grad():
        got = model.encode_visual(x.cuda(), **{k: v.cuda() for k, v in kw.items()})
        again = model.encode_visual(x.cuda(), **{k: v.cuda() for k, v in kw.items()})
    assert torch.equal(got, again)
    eng = model.visual._engine_f32()
    assert isinstance(eng, F.LensEngineF32)
    if modality == "pc":
        cidx = O.fps_indices(x, ls.pc_num_group, kw["fps_start"])
        gc, _ = ops.fps(x.cuda(), kw["fps_start"].cuda(), ls.pc_num_group)
        assert torch.equal(gc.cpu(), cidx)
        _, nidx = ops.knn_group(x.cuda(), gc, ls.pc_group_size, want_idx=True)
        bad = _check_knn_sets(x, cidx, nidx.cpu().long(), ls.pc_group_size)
        ref = _encode_visual_on_sets(sd, x, spec, ls, cidx, nidx.cpu().long())
        print(f"pc: {bad} kNN groups differ from the oracle's (near-equidistant swaps)")
    else:
        ref = O.encode_visual(sd, x, spec, ls)
    e = relerr(got, ref)
    print(f"fp32 arithmetic, ViT-L {modality} Lens: features {e:.2e} relative to the fp32 CPU path")
    assert e < 1e-5, e


# ------------------------------------------------------------------------------------------------ routing
def _tiny_model(name, **over):
    import open_clip as oc
    sd, ins, outs, grads, meta = split(load_npz(f"tiny_{name}.npz"))
    a = dict(meta["args"]); a.update(over)
    with tempfile.TemporaryDirectory() as td:
        with open(os.path.join(td, "tiny-lens.json"), "w") as f:
            json.dump(meta["model_cfg"], f)
        oc.add_model_config(td)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            model = oc.tri_create_model("tiny-lens", None, precision="fp32", device="cuda", output_dict=True, args=SimpleNamespace(**a))
    if not over:
        model.load_state_dict(sd, strict=False)
    return model, ins


@pytest.mark.parametrize("case", ["audio", "pc", "eeg", "pnsa", "latent_dh48", "train_mode", "grad_trainable"])
def test_routing_through_the_engine_used(case, monkeypatch):
    """Eval-mode, no-grad calls of audio / pc / eeg run LensEngineF32; pnsa, a latent head dim of 48, train mode and
    grad-enabled calls with trainable parameters keep the 16-bit engine or the trainer - read off the engine object that ran."""
    from vitlens_hip import engine as E, f32 as F
    used = []

    def spy(cls):
        orig = cls.encode

        def enc(self, x, *a, **k):
            used.append(cls)
            if case in ("pnsa", "latent_dh48"):          # routing only: the 16-bit kernels are not asked to run these
                return torch.zeros(x.shape[0], self.tower.embed_dim, device="cuda")
            return orig(self, x, *a, **k)
        monkeypatch.setattr(cls, "encode", enc)
    spy(E.LensEngine); spy(F.LensEngineF32)
    over = {}
    name = case if case in ("audio", "pc", "eeg") else "audio"
    if case == "pnsa":
        name, over = "pc", {"pc_tokenizer": "pnsa"}
    elif case == "latent_dh48":
        over = {"perceiver_latent_dim_head": 48}
    model, ins = _tiny_model(name, **over)
    x = ins["visual_x"].cuda()
    kw = {"fps_start": ins["fps_start"].cuda()} if name == "pc" else {}
    if case == "pnsa":
        kw = {"xyz": x, "fps_start": ins["fps_start"].cuda()}
    model.eval()
    if case == "train_mode":
        model.train()
    if case == "grad_trainable":
        assert any(p.requires_grad for p in model.visual.parameters())
        f = model.encode_visual(x, **kw)
        assert f.requires_grad and model.visual._trainer_obj is not None and used == []
        return
    with torch.no_grad():
        model.encode_visual(x, **kw)
    want = F.LensEngineF32 if case in ("audio", "pc", "eeg") else E.LensEngine
    assert used == [want], used
    assert (model.visual._engine_f32() is not None) == (want is F.LensEngineF32) or case == "train_mode"
