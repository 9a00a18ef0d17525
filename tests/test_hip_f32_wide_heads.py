"""GPU: true fp32 attention at head dims 72-128 (vl_attn_fwd_f32 -> attn_f32_wide_kernel: one query row per quad of lanes,
zero-padded to 80 / 96 / 112 / 128 in registers and LDS) and the fp32 ViT-H-14 / ViT-bigG-14 towers it completes.

Kernel checks follow tests/test_hip_f32_lens.py: per (b, h, 32-query tile) block against float64 (tests/errloc.py, reference
tests/attn_ref.py), tolerance 4 x max(the worst block of the same attention in torch float32 on the CPU on the same inputs,
2^-24).  lse is checked per query row against float64 logsumexp by the same rule, the error of a row being |lse - ref| /
max(|ref|, 1) (relative; absolute below 1, where a relative error of a value near 0 says nothing).  Outputs start as NaN and
sit between NaN guard rows; every case runs twice and must be bit-identical; every check is shown to fail on the kernel's own
output with its worst block (row, for lse) scaled by 1 + 3 tol.  Operands are strided views of one packed allocation whose
columns after the last head are NaN (self-attention: the engines' [tokens, 3 D] qkv; cross attention: the Perceiver's q rows
and packed k|v rows), so a read past the real head dim shows up as NaN in out."""
import json
import os
import tempfile
import warnings
from types import SimpleNamespace

import pytest
import torch

import attn_ref as A
import vitlens_oracle as O
from errloc import assert_attn_blocks, attn_block_relerr
from golden_util import load_npz, split

pytestmark = pytest.mark.gpu

EPS32 = 2.0 ** -24
TAIL = 8        # NaN columns after the last head of a packed buffer
GUARD = 4       # NaN rows before and after out
NAN = float("nan")


def _ops():
    from vitlens_hip import ops
    return ops


def relerr(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-300))


def _tol(cpu_worst):
    return 4.0 * max(cpu_worst, EPS32)


def _token_major(t):
    B, H, L, dh = t.shape
    return t.permute(0, 2, 1, 3).reshape(B * L, H * dh)


def _packed(q, k, v, cross):
    """Contiguous CPU [B, H, L, dh] q, k, v -> (allocation, (q, k, v) strided device views into it)."""
    ops = _ops()
    B, H, Lq, dh = q.shape
    Lk, D = k.shape[2], H * dh
    if not cross:
        buf = torch.full((B * Lq, 3 * D + TAIL), NAN, device="cuda")
        for i, t in enumerate((q, k, v)):
            buf[:, i * D:(i + 1) * D] = _token_major(t).cuda()
        return buf, tuple(ops.heads_view(buf, B, Lq, H, dh, i * D) for i in range(3))
    nq = B * Lq * (D + TAIL)
    buf = torch.full((nq + B * Lk * (2 * D + TAIL),), NAN, device="cuda")
    q2, kv2 = buf[:nq].view(B * Lq, D + TAIL), buf[nq:].view(B * Lk, 2 * D + TAIL)
    q2[:, :D] = _token_major(q).cuda()
    kv2[:, :D] = _token_major(k).cuda()
    kv2[:, D:2 * D] = _token_major(v).cuda()
    return buf, (ops.heads_view(q2, B, Lq, H, dh), ops.heads_view(kv2, B, Lk, H, dh), ops.heads_view(kv2, B, Lk, H, dh, D))


def _bits(t):
    return t.contiguous().view(torch.int32)


def _launch_twice(q, k, v, scale, causal, cross):
    ops = _ops()
    B, H, Lq, dh = q.shape
    _, (qd, kd, vd) = _packed(q, k, v, cross)
    runs = []
    for _ in range(2):
        ob = torch.full((B * Lq + 2 * GUARD, H * dh), NAN, device="cuda")
        lse = torch.full((B, H, Lq), NAN, device="cuda")
        ops.attn_fwd_f32(qd, kd, vd, ob[GUARD:GUARD + B * Lq], lse=lse, causal=causal, scale=scale)
        torch.cuda.synchronize()
        assert bool(torch.isnan(ob[:GUARD]).all()) and bool(torch.isnan(ob[-GUARD:]).all()), "guard rows were written"
        runs.append((ob[GUARD:GUARD + B * Lq].cpu(), lse.cpu()))
    (o1, l1), (o2, l2) = runs
    assert torch.equal(_bits(o1), _bits(o2)) and torch.equal(_bits(l1), _bits(l2)), "a second launch differs"
    assert bool(torch.isfinite(o1).all()), "out has non-finite elements (a NaN column was read, or a row was not written)"
    assert bool(torch.isfinite(l1).all()), "lse has non-finite elements"
    return o1, l1


def _lse_err(lse, ref):
    return (lse.double() - ref).abs() / ref.abs().clamp_min(1.0)


def _assert_lse(lse, ref, tol, what):
    e = _lse_err(lse, ref)
    i = int(torch.where(torch.isnan(e), torch.full_like(e, float("inf")), e).reshape(-1).argmax())
    worst = float(e.reshape(-1)[i])
    B, H, Lq = ref.shape
    b, r = divmod(i, H * Lq)
    assert worst <= tol, f"{what} lse: b={b} h={r // Lq} query {r % Lq} has error {worst:.3e} > {tol:.1e}"
    return worst, i


def run_case(kind, B, H, Lq, Lk, dh, causal):
    cross = Lq != Lk
    q, k, v, scale = A.make_scores(kind, B, H, Lq, Lk, dh, seed=1000 * Lq + Lk + dh, dtype=torch.float32)
    if kind == "normal":
        scale /= A.LOG2E                                       # vl_attn_fwd_f32 takes the natural-log softmax scale
    ref, ref_lse = A.attn_fwd_ref(q, k, v, scale, causal, torch.float32, log2=False)
    cpu, cpu_lse = A.attn_fwd_model(q, k, v, scale, causal, torch.float32, log2=False)
    cw, _ = attn_block_relerr(cpu, ref, B, H, Lq)
    tol = _tol(cw)
    lcw = float(_lse_err(cpu_lse, ref_lse).max())
    ltol = _tol(lcw)
    got, lse = _launch_twice(q, k, v, scale, causal, cross)
    kw, (b, h, r0, r1) = attn_block_relerr(got, ref, B, H, Lq)
    lkw = float(_lse_err(lse, ref_lse).max())
    what = f"{kind} B={B} H={H} Lq={Lq} Lk={Lk} dh={dh}{' causal' if causal else ''}"
    print(f"{what}: out worst block {kw:.3e}, CPU fp32 {cw:.3e}, ratio {kw / max(cw, EPS32):.2f}, tol {tol:.3e}; "
          f"lse worst row {lkw:.3e}, CPU fp32 {lcw:.3e}, ratio {lkw / max(lcw, EPS32):.2f}, tol {ltol:.3e}")
    check = lambda o: assert_attn_blocks(o, ref, tol, B, H, Lq, rows="queries", what=what)
    check(got)
    bad = got.clone()
    bad.view(B, Lq, H, dh)[b, r0:r1, h] *= 1.0 + 3.0 * tol
    with pytest.raises(AssertionError):
        check(bad)
    _, i = _assert_lse(lse, ref_lse, ltol, what)
    bad = lse.clone().reshape(-1)
    if abs(float(ref_lse.reshape(-1)[i])) >= 1.0:
        bad[i] *= 1.0 + 3.0 * ltol
    else:                                                      # |ref| < 1: the row's error is absolute; move it by 3 tol
        bad[i] += 3.0 * ltol
    with pytest.raises(AssertionError):
        _assert_lse(bad.view_as(lse), ref_lse, ltol, what)


def _cases():
    c = []
    for dh in (72, 80, 88, 96, 104, 112, 120, 128):
        c.append(("normal", 2, 16, 257, 257, dh, False))
    for dh in (80, 104, 128):
        c.append(("normal", 2, 16, 77, 77, dh, True))
    for dh in (104, 128):
        for Lk in (1, 65, 600):
            c.append(("normal", 2, 16, 256, Lk, dh, False))
    c.append(("normal", 2, 16, 1, 1, 104, False))
    c.append(("normal", 2, 16, 1, 257, 104, False))
    for kind in ("ramp", "descend", "negative", "sink_first", "sink_last"):
        for dh in (80, 104, 128):
            c.append((kind, 2, 4, 257, 257, dh, False))
    return [pytest.param(*a, id=f"{a[0]}-B{a[1]}H{a[2]}-{a[3]}x{a[4]}-dh{a[5]}{'-causal' if a[6] else ''}") for a in c]


@pytest.mark.parametrize("kind,B,H,Lq,Lk,dh,causal", _cases())
def test_attn_fwd_f32_wide_heads_per_tile(kind, B, H, Lq, Lk, dh, causal):
    run_case(kind, B, H, Lq, Lk, dh, causal)


# ------------------------------------------------------------------------------------------------ refusals
def _refused(call, *bufs):
    with pytest.raises(RuntimeError):
        call()
    torch.cuda.synchronize()
    for t in bufs:
        assert bool(torch.isnan(t).all()), "a refused call wrote"


@pytest.mark.parametrize("dh", [48, 100, 136])
def test_refused_head_dims_write_nothing(dh):
    ops = _ops()
    B, H, L = 2, 2, 40
    D = H * dh
    buf = torch.randn(B * L, 3 * D + TAIL, device="cuda")
    q, k, v = (ops.heads_view(buf, B, L, H, dh, i * D) for i in range(3))
    out, lse = torch.full((B * L, D), NAN, device="cuda"), torch.full((B, H, L), NAN, device="cuda")
    _refused(lambda: ops.attn_fwd_f32(q, k, v, out, lse=lse, scale=dh ** -0.5), out, lse)


def test_refused_strides_write_nothing():
    """A row stride of q, k or v that is not a multiple of 4 elements (16-byte rows), at head dim 104."""
    ops = _ops()
    B, H, L, dh = 2, 2, 40, 104
    D = H * dh
    good = torch.randn(B * L, 3 * D + TAIL, device="cuda")
    odd = torch.randn(B * L, 3 * D + 2, device="cuda")
    g = [ops.heads_view(good, B, L, H, dh, i * D) for i in range(3)]
    o = [ops.heads_view(odd, B, L, H, dh, i * D) for i in range(3)]
    out, lse = torch.full((B * L, D), NAN, device="cuda"), torch.full((B, H, L), NAN, device="cuda")
    for i in range(3):
        trio = [o[j] if j == i else g[j] for j in range(3)]
        _refused(lambda: ops.attn_fwd_f32(*trio, out, lse=lse, scale=dh ** -0.5), out, lse)


# ------------------------------------------------------------------------------------------------ full-size towers
GEOMETRY = {"ViT-H-14": dict(width=1280, layers=32, heads=16, mlp_ratio=4.0, embed_dim=1024),
            "ViT-bigG-14": dict(width=1664, layers=48, heads=16, mlp_ratio=4.9231, embed_dim=1280)}


@pytest.mark.parametrize("name", list(GEOMETRY))
def test_fullsize_tower_in_fp32_arithmetic(name):
    """VitEngineF32 at the real geometry (open_clip/model_configs: ViT-H-14 32 x 1280, 16 heads of 80, MLP 5120; ViT-bigG-14
    48 x 1664, 16 heads of 104, MLP 8192, embed 1280), seeded O.init_tower weights, 2 images: features within 1e-5 relative of
    O.encode_image in fp32 on the CPU (the fp32 mode's bar)."""
    from vitlens_hip import engine as E, f32 as F
    geo = GEOMETRY[name]
    spec = O.TowerSpec(patch=14, image_size=224, **geo)
    g = torch.Generator().manual_seed(3)
    sd = O.init_tower(spec, g, "image.")
    image = torch.randn(2, 3, 224, 224, generator=g)
    eng = F.VitEngineF32(sd, "image.", E.TowerCfg(patch=14, image_size=224, **geo), "cuda")
    got = eng.encode(image.cuda())
    assert torch.equal(got, eng.encode(image.cuda()))
    ref = O.encode_image(sd, image, spec)
    e = relerr(got, ref)
    print(f"fp32 arithmetic, {name}: image features {e:.2e} relative to the fp32 CPU path")
    assert e < 1e-5, e


# ------------------------------------------------------------------------------------------------ routing
def _tiny_wide_model():
    """The tiny audio golden's config with a vision width of 208 = 2 heads of 104 and an audio Lens whose Perceiver heads are
    32 (latents of width 208), built by tri_create_model(precision="fp32") with its own seeded initialisation."""
    import open_clip as oc
    _, ins, _, _, meta = split(load_npz("tiny_audio.npz"))
    cfg = json.loads(json.dumps(meta["model_cfg"]))
    cfg["vision_cfg"].update(width=208, head_width=104, layers=2)
    a = dict(meta["args"])
    a.update(perceiver_input_chan=208, perceiver_latent_dim=208, perceiver_cross_dim_head=32, perceiver_latent_dim_head=32)
    torch.manual_seed(0)
    with tempfile.TemporaryDirectory() as td:
        with open(os.path.join(td, "tiny-wide-heads.json"), "w") as f:
            json.dump(cfg, f)
        oc.add_model_config(td)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            model = oc.tri_create_model("tiny-wide-heads", None, precision="fp32", device="cuda", output_dict=True,
                                        args=SimpleNamespace(**a))
    return model, ins


def _specs(tower, lens=None):
    spec = O.TowerSpec(**{k: getattr(tower, k) for k in O.TowerSpec.__dataclass_fields__})
    return spec, (None if lens is None else O.LensSpec(**{k: getattr(lens, k) for k in O.LensSpec.__dataclass_fields__}))


def test_routing_head_dim_104_through_the_api(monkeypatch):
    """Eval mode + no_grad: encode_image of a head-dim-104 tower runs VitEngineF32, and an audio Lens (Perceiver heads of 32)
    over such a trunk runs LensEngineF32, both within 1e-5 of the fp32 oracle; train mode keeps the 16-bit engine - read off
    the engine object that ran."""
    from vitlens_hip import engine as E, f32 as F
    used = []

    def spy(cls, meth):
        orig = getattr(cls, meth)

        def run(self, *a, **k):
            used.append(cls)
            return orig(self, *a, **k)
        monkeypatch.setattr(cls, meth, run)
    spy(F.VitEngineF32, "encode"); spy(E.VitEngine, "encode_image"); spy(F.LensEngineF32, "encode"); spy(E.LensEngine, "encode")
    model, ins = _tiny_wide_model()
    assert "true fp32 arithmetic" in model.precision_effective
    model.eval()
    sd = {k: v.detach().float().cpu() for k, v in model.state_dict().items()}
    ispec, _ = _specs(*model.image._cfgs())
    vspec, lspec = _specs(*model.visual._cfgs())
    assert ispec.width // ispec.heads == 104 and vspec.width // vspec.heads == 104
    assert lspec.cross_dim_head == 32 and lspec.latent_dim_head == 32 and not lspec.perceiver_identity
    g = torch.Generator().manual_seed(4)
    image = torch.randn(2, 3, ispec.image_size, ispec.image_size, generator=g)
    with torch.no_grad():
        fi = model.encode_image(image.cuda())
    assert used == [F.VitEngineF32], used
    assert isinstance(model.image._engine_f32(), F.VitEngineF32)
    ei = relerr(fi, O.encode_image(sd, image, ispec))
    x = ins["visual_x"]
    used.clear()
    with torch.no_grad():
        fv = model.encode_visual(x.cuda())
    assert used == [F.LensEngineF32], used
    ev = relerr(fv, O.encode_visual(sd, x, vspec, lspec))
    print(f"head dim 104 through the API: image features {ei:.2e}, audio Lens features {ev:.2e} relative to the fp32 oracle")
    assert ei < 1e-5 and ev < 1e-5, (ei, ev)
    model.train()
    used.clear()
    with torch.no_grad():
        model.encode_image(image.cuda())
    assert used == [E.VitEngine], used
