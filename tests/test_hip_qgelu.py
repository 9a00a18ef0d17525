"""GPU: QuickGELU (x * sigmoid(1.702 x), the OpenAI-pretrained CLIP activation; VL_ACT_QGELU / VL_ACT_QGELU_DSAVE) in every GEMM
family that carries an activation, and at tower level through the executors, the trainers and the public interface.

Op level: against fp32 torch on the same 16-bit operands (fp64 for the fp32 engine), per 256x256 block through tests/errloc.py,
with the bounds the neighbouring erf assertions use for the same output type (tests/test_hip_gemm_park.py, test_hip_f16.py,
test_hip_f32.py, test_hip_lnfold.py).  Pre-activations are scaled to a standard deviation of 4, so every tile holds both saturated
ends (|u| up to ~12-16).  Every case pins its kernel with an explicit cfg (an unsupported shape is an error there, not another
kernel); the one auto-dispatch case checks its row split with vl_gemm_main_rows.
Tower level: the tiny geometry of the goldens against the oracle with its GELU swapped for QuickGELU (tests/qgelu_ref.py, pinned
to the imported reference by tests/test_qgelu_reference.py), within the envelopes the erf towers have in tests/test_hip_towers.py,
test_hip_train.py, test_hip_api.py and test_hip_f32.py."""
import json
import os
import tempfile
import warnings
from types import SimpleNamespace

import pytest
import torch

import vitlens_oracle as O
from errloc import assert_blocks
from golden_util import load_npz, split, specs_from_meta
from qgelu_ref import qgelu, qgelu_grad, quick_gelu_oracle

pytestmark = pytest.mark.gpu

TILE_TOL_BF16 = 5e-3           # tests/test_hip_gemm_park.py
SD_PRE = 4.0                   # standard deviation of the pre-activations


def _ops():
    from vitlens_hip import ops
    return ops


def rnd(*shape, scale=1.0, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def relerr(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def _operands(M, N, K, seed=0, dtype=torch.bfloat16):
    a = rnd(M, K, seed=seed + 1).to(dtype).cuda()
    w = rnd(N, K, seed=seed + 2, scale=SD_PRE * K ** -0.5).to(dtype).cuda()
    bias = rnd(N, seed=seed + 3).cuda()
    acc = a.float() @ w.float().t() + bias
    assert float(acc.min()) < -11 and float(acc.max()) > 11           # both saturated ends are there
    return a, w, bias, acc


def _buf(M, N, pad=0):
    """NaN-poisoned bf16 [M, N] output; pad > 0: a view of a wider buffer (row stride N + pad: rows not 16-byte aligned)."""
    return torch.full((M, N + pad), float("nan"), device="cuda", dtype=torch.bfloat16)[:, :N]


def _check_forward(out, acc, what, extra=()):
    """The bounds of the erf GELU assertions of tests/test_hip_gemm_park.py::test_p4_bf16_epilogues."""
    ref = qgelu(acc).float()
    assert bool(torch.isfinite(out).all()), what
    e = relerr(out, ref)
    worst = assert_blocks(out, ref, TILE_TOL_BF16, 256, 256, extra=extra, what=what)
    print(f"{what}: relerr {e:.2e}, worst block {worst:.2e}")
    assert e < 4e-3, (what, e)
    assert bool(((out.float() - ref).abs() <= ref.abs() * 2.0 ** -7 + 2e-3).all()), what


def _check_dsave_and_backward(ops, a, w, bias, acc, cfg, what, extra=(), pad=0):
    """VL_ACT_QGELU_DSAVE on one kernel family: out = qgelu, out2 = qgelu' of the bf16-rounded pre-activation (which the same
    kernel's plain epilogue stores: same products, same rounding point), then VL_EPI_DGELU with that tensor."""
    M, N = acc.shape
    pre = ops.gemm(a, w, bias, epi=ops.EPI_BF16, cfg=cfg, out=_buf(M, N, pad))
    d = _buf(M, N, pad)
    y = ops.gemm(a, w, bias, epi=ops.EPI_BF16, act=ops.ACT_QGELU_DSAVE, cfg=cfg, out2=d, out=_buf(M, N, pad))
    _check_forward(y, acc, what + " dsave out", extra)
    want_y, want_d = qgelu(pre), qgelu_grad(pre)                       # fp64 of the bf16-rounded pre-activation
    assert bool(torch.isfinite(d).all()), what
    ey = float(((y.double() - want_y).abs() - want_y.abs() * 2.0 ** -8).max())
    ed = float(((d.double() - want_d).abs() - want_d.abs() * 2.0 ** -8).max())
    print(f"{what}: out - qgelu(pre) beyond one bf16 ulp by {ey:.2e}, out2 - qgelu'(pre) by {ed:.2e} (allowed 1e-6)")
    # bf16 of an fp32-accurate value: at most one bf16 ulp from fp64 (the bound of the erf gelu' assertion)
    assert ey <= 1e-6 and ed <= 1e-6, (what, ey, ed)
    # the saturated ends: qgelu' is 1 / 0 there, never NaN
    assert bool((d[pre > 20].float() == 1).all()) and bool((d[pre < -20].float().abs() < 1e-12).all())
    # backward: (dy W) * qgelu'
    K = a.shape[1]
    dy = rnd(M, K, seed=34).bfloat16().cuda(); wt = rnd(N, K, seed=35, scale=K ** -0.5).bfloat16().cuda()
    accb = dy.float() @ wt.float().t()
    got = _buf(M, N, pad)
    ops.gemm(dy, wt, None, res=d, epi=ops.EPI_DGELU, act=ops.ACT_QGELU_DSAVE, cfg=cfg, out=got)
    ref = accb * want_d.float()
    e = relerr(got, ref)
    worst = assert_blocks(got, ref, TILE_TOL_BF16, 256, 256, extra=extra, what=what + " dgelu")
    print(f"{what}: dgelu relerr {e:.2e}, worst block {worst:.2e}")
    assert e < 5e-3, (what, e)
    # the same multiplication as the erf code: one kernel for both
    same = ops.gemm(dy, wt, None, res=d, epi=ops.EPI_DGELU, act=ops.ACT_GELU_DSAVE, cfg=cfg, out=_buf(M, N, pad))
    assert torch.equal(got, same), what


# ---- op level -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg,M,N,K,pad", [(8, 768, 512, 512, 0),           # persistent 256x256 kernel
                                           (10, 768, 384, 512, 0),          # N % 256 == 128: the 256x128-tile kernel
                                           (1, 2 * 256 + 77, 512, 512, 0),  # plain 128x128 tiles, ragged rows (direct epilogue)
                                           (11, 2 * 256 + 77, 512, 512, 0),  # 64x64 tiles
                                           (9, 2 * 256 + 77, 512, 512, 0),  # split-K leftover-row kernel
                                           (5, 2 * 256 + 77, 512, 512, 0),  # round-1 persistent kernel: 16-byte LDS-transpose epilogue
                                           (5, 2 * 256 + 77, 512, 512, 4)])  # ... its 8-byte epilogue (row stride 516: not 16-byte rows)
def test_qgelu_and_dsave_on_every_kernel_family(cfg, M, N, K, pad):
    ops = _ops()
    a, w, bias, acc = _operands(M, N, K, seed=10 * cfg)
    what = f"cfg {cfg} ({M}, {N}, {K}) pad {pad}"
    out = _buf(M, N, pad)
    ops.gemm(a, w, bias, out=out, epi=ops.EPI_BF16, act=ops.ACT_QGELU, cfg=cfg)
    _check_forward(out, acc, what + " qgelu")
    _check_dsave_and_backward(ops, a, w, bias, acc, cfg, what, pad=pad)


def test_qgelu_auto_dispatch_with_leftover_rows():
    """cfg = -1 with M % 256 != 0: whole row tiles on the persistent kernel, the 77 leftover rows on the small-tile kernels."""
    ops = _ops()
    M, N, K = 96 * 256 + 77, 512, 512
    mm = int(ops._lib.vl_gemm_main_rows(M, N))
    assert 0 < mm < M and mm % 256 == 0, mm                           # the row split the dispatcher makes: both paths run
    a, w, bias, acc = _operands(M, N, K, seed=77)
    extra = [("rows", mm, M)]
    out = torch.full((M, N), float("nan"), device="cuda", dtype=torch.bfloat16)
    ops.gemm(a, w, bias, out=out, epi=ops.EPI_BF16, act=ops.ACT_QGELU, cfg=-1)
    _check_forward(out, acc, "auto qgelu", extra)
    _check_dsave_and_backward(ops, a, w, bias, acc, -1, "auto", extra)


def _lnfold_case(M, N, K):
    ops = _ops()
    x = (rnd(M, K, seed=3) * (0.5 + rnd(M, 1, seed=4).abs() * 2) + rnd(M, 1, seed=5) * 0.7).bfloat16().cuda()
    w = rnd(N, K, seed=6, scale=SD_PRE * K ** -0.5).cuda()
    b = rnd(N, seed=7, scale=0.2).cuda()
    gamma, beta = (1.0 + 0.3 * rnd(K, seed=8)).cuda(), (0.2 * rnd(K, seed=9)).cuda()
    mean, rstd = torch.empty(M, device="cuda"), torch.empty(M, device="cuda")
    ops.ln_row_stats(None, x, 0, mean, rstd)
    pre = torch.nn.functional.layer_norm(x.float(), (K,), gamma, beta, 1e-5) @ w.t() + b
    assert float(pre.min()) < -11 and float(pre.max()) > 11
    return ops, x, w, b, gamma, beta, mean, rstd, ops.fold_ln_linear(w, b, gamma, beta), pre


@pytest.mark.parametrize("dsave", [False, True])
def test_qgelu_layernorm_folded_kernel(dsave):
    """vl_gemm_lnfold_bf16 (the persistent kernel's row-statistics epilogue) at (768, 512, 512), both codes.  Called through the
    binding table: ops.gemm_lnfold gives a problem of six tiles to layernorm + gemm (vl_gemm_main_rows is 0 below three quarters
    of a round of tiles), which is checked next to it - the flag rides through that path too."""
    M, N, K = 768, 512, 512
    ops, x, w, b, gamma, beta, mean, rstd, fold, pre = _lnfold_case(M, N, K)
    from vitlens_hip.ops import _lib, _p, _stream, check
    act = ops.ACT_QGELU_DSAVE if dsave else ops.ACT_QGELU
    wg, bf, c = fold
    out = torch.full((M, N), float("nan"), device="cuda", dtype=torch.bfloat16)
    d = torch.full((M, N), float("nan"), device="cuda", dtype=torch.bfloat16) if dsave else None
    check(_lib.vl_gemm_lnfold_bf16(_p(x), _p(wg), _p(bf), _p(c), _p(mean), _p(rstd), _p(out), _p(d), M, N, K, x.stride(0),
                                   wg.stride(0), out.stride(0), act, _stream()))
    # bounds: tests/test_hip_gemm_park.py::test_many_tiles_lnfold_variants (8e-3, GELU behind the fold), per block test_hip_lnfold.py (7.5e-3)
    ref = qgelu(pre).float()
    e = relerr(out, ref)
    worst = assert_blocks(out, ref, 7.5e-3, 256, 256, what="lnfold qgelu")
    print(f"lnfold dsave={dsave}: relerr {e:.2e}, worst block {worst:.2e}")
    assert bool(torch.isfinite(out).all()) and e < 8e-3, e
    if dsave:
        # out / out2 are functions of the kernel's own bf16 pre-activation: the folded kernel with act = none stores it
        p0 = torch.empty_like(out)
        check(_lib.vl_gemm_lnfold_bf16(_p(x), _p(wg), _p(bf), _p(c), _p(mean), _p(rstd), _p(p0), None, M, N, K, x.stride(0),
                                       wg.stride(0), out.stride(0), ops.ACT_NONE, _stream()))
        wy, wd = qgelu(p0), qgelu_grad(p0)
        assert float(((out.double() - wy).abs() - wy.abs() * 2.0 ** -8).max()) <= 1e-6
        assert float(((d.double() - wd).abs() - wd.abs() * 2.0 ** -8).max()) <= 1e-6
    # through ops.gemm_lnfold: this shape takes layernorm + gemm, with the same activation
    assert ops._fold_rows(x, out, N, K) == 0
    out2 = torch.full((M, N), float("nan"), device="cuda", dtype=torch.bfloat16)
    d2 = torch.full((M, N), float("nan"), device="cuda", dtype=torch.bfloat16) if dsave else None
    ops.gemm_lnfold(x, fold, mean, rstd, out2, w.bfloat16(), b, gamma, beta, torch.empty(M, K, device="cuda", dtype=torch.bfloat16),
                    act=act, out2=d2)
    assert relerr(out2, ref) < 8e-3 and (d2 is None or bool(torch.isfinite(d2).all()))


def test_qgelu_through_gemm_lnfold_with_folded_and_leftover_rows():
    """ops.gemm_lnfold where it does fold: 96 row tiles on the folded kernel, 40 leftover rows through layernorm + gemm."""
    M, N, K = 96 * 256 + 40, 512, 512
    ops, x, w, b, gamma, beta, mean, rstd, fold, pre = _lnfold_case(M, N, K)
    out = torch.full((M, N), float("nan"), device="cuda", dtype=torch.bfloat16)
    mm = ops._fold_rows(x, out, N, K)
    assert 0 < mm < M, mm
    d = torch.full((M, N), float("nan"), device="cuda", dtype=torch.bfloat16)
    hws = torch.empty(M - mm, K, device="cuda", dtype=torch.bfloat16)
    ops.gemm_lnfold(x, fold, mean, rstd, out, w.bfloat16(), b, gamma, beta, hws, act=ops.ACT_QGELU_DSAVE, out2=d)
    ref = qgelu(pre).float()
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(d).all())
    worst = assert_blocks(out, ref, 7.5e-3, 256, 256, extra=[("rows", mm, M)], what="gemm_lnfold qgelu")
    print(f"gemm_lnfold: relerr {relerr(out, ref):.2e}, worst block {worst:.2e}; derivative relerr {relerr(d, qgelu_grad(pre)):.2e}")
    assert relerr(out, ref) < 8e-3 and relerr(d, qgelu_grad(pre)) < 8e-3
    plain = torch.empty_like(out)
    ops.gemm_lnfold(x, fold, mean, rstd, plain, w.bfloat16(), b, gamma, beta, hws, act=ops.ACT_QGELU)
    assert relerr(plain, ref) < 8e-3


def test_qgelu_fp16_operands():
    """vl_gemm_f16 (the frozen text tower's GEMM; the OpenAI text tower is QuickGELU too): bound of tests/test_hip_f16.py."""
    ops = _ops()
    M, N, K = 768, 512, 512
    a, w, bias, acc = _operands(M, N, K, seed=5, dtype=torch.float16)
    out = torch.full((M, N), float("nan"), device="cuda", dtype=torch.float16)
    ops.gemm_f16(a, w, bias, out=out, act=ops.ACT_QGELU)
    ref = qgelu(acc).float()
    e = relerr(out, ref)
    worst = assert_blocks(out, ref, 6e-4, 256, 256, what="f16 qgelu")
    print(f"f16: relerr {e:.2e}, worst block {worst:.2e}")
    assert bool(torch.isfinite(out).all()) and e < 6e-4, e
    assert bool(((out.float() - ref).abs() <= ref.abs() * 2.0 ** -10 + 1e-3).all())
    with pytest.raises(RuntimeError):                                       # no derivative output on this entry
        ops.gemm_f16(a, w, bias, act=ops.ACT_QGELU_DSAVE)


@pytest.mark.parametrize("M,N,K", [(128, 128, 64), (130, 132, 68)])
def test_qgelu_fp32_engine_gemm(M, N, K):
    """vl_gemm_f32 / vl_gemm_f32_ex (expf and a true division) against fp64: the bound of tests/test_hip_f32.py's GELU case."""
    ops = _ops()
    a = rnd(M, K, seed=1).cuda(); w = rnd(N, K, seed=2, scale=SD_PRE * K ** -0.5).cuda(); bias = rnd(N, seed=3).cuda()
    acc = a.double() @ w.double().t() + bias.double()
    assert float(acc.min()) < -11 and float(acc.max()) > 11
    out = ops.gemm_f32(a, w, bias, act=ops.ACT_QGELU, out=torch.full((M, N), float("nan"), device="cuda"))
    e = relerr(out, qgelu(acc))
    print(f"f32 ({M}, {N}, {K}): relerr {e:.2e}, max abs {float((out.double() - qgelu(acc)).abs().max()):.2e}")
    assert bool(torch.isfinite(out).all()) and e < 2e-6, e
    res = rnd(M, N, seed=4).cuda()
    assert relerr(ops.gemm_f32(a, w, bias, res=res, act=ops.ACT_QGELU), qgelu(acc) + res.double()) < 2e-6
    # the epilogue form whose residual joins before the activation (one residual row per two output rows)
    rp = rnd((M + 1) // 2, N, seed=5).cuda()
    got = ops.gemm_f32_ex(a, w, bias, res=rp, act=ops.ACT_QGELU, res_div=2, res_pre=True)
    want = qgelu(acc + rp.double().repeat_interleave(2, 0)[:M])
    assert relerr(got, want) < 2e-6
    # every finite input: the saturated ends give x / -0, never NaN
    big = torch.tensor([[3.0e38, -3.0e38, 1e4, -1e4]], device="cuda").t().contiguous()      # [4, 1] pre-activations via a K = 4 GEMM
    eye = torch.zeros(4, 4, device="cuda"); eye[:, 0] = big[:, 0]
    one = torch.zeros(4, 4, device="cuda"); one[:, 0] = 1.0
    o = ops.gemm_f32(eye, one, None, act=ops.ACT_QGELU)
    assert bool(torch.isfinite(o).all()) and o[0, 0] == 3.0e38 and o[1, 0] == 0 and o[2, 0] == 1e4 and o[3, 0] == 0


def test_qgelu_finite_at_the_ends_of_bf16():
    """Largest finite bf16 magnitudes through the 16-bit epilogues: u / 1 at the positive end, -0 / 0 at the negative end."""
    ops = _ops()
    M, N, K = 256, 256, 512
    a = torch.zeros(M, K); a[:, 0] = 1.0
    w = torch.zeros(N, K)
    vals = torch.tensor([3.38e38, -3.38e38, 1e5, -1e5, 60.0, -60.0, 0.0, -0.0])
    w[:, 0] = vals.repeat(N // 8)
    a, w = a.bfloat16().cuda(), w.bfloat16().cuda()
    pre = w[:, 0].float()[None, :].expand(M, N)
    for cfg in (8, 1):
        d = torch.full((M, N), float("nan"), device="cuda", dtype=torch.bfloat16)
        y = ops.gemm(a, w, None, epi=ops.EPI_BF16, act=ops.ACT_QGELU_DSAVE, cfg=cfg, out2=d)
        y1 = ops.gemm(a, w, None, epi=ops.EPI_BF16, act=ops.ACT_QGELU, cfg=cfg)
        for t in (y, y1, d):
            assert bool(torch.isfinite(t).all()), cfg
        assert torch.equal(y.float(), torch.where(pre > 0, pre, torch.zeros_like(pre))) and torch.equal(y1, y)
        assert torch.equal(d.float(), torch.where(pre > 0, torch.ones_like(pre), torch.where(pre == 0, torch.full_like(pre, 0.5),
                                                                                           torch.zeros_like(pre))))


def test_qgelu_refusals_launch_nothing():
    ops = _ops()
    M, N, K = 256, 256, 512
    a, w, bias, acc = _operands(M, N, K, seed=9)
    nan = lambda: torch.full((M, N), float("nan"), device="cuda", dtype=torch.bfloat16)
    res = rnd(M, N, seed=1).bfloat16().cuda()
    cases = {
        "QGELU with EPI_RES_BF16": dict(epi=ops.EPI_RES_BF16, act=ops.ACT_QGELU, res=res),
        "QGELU_DSAVE with EPI_RES_BF16": dict(epi=ops.EPI_RES_BF16, act=ops.ACT_QGELU_DSAVE, res=res),
        "recompute form of EPI_DGELU with QGELU": dict(epi=ops.EPI_DGELU, act=ops.ACT_QGELU, res=res),
        "QGELU + out2 (store the pre-activation)": dict(epi=ops.EPI_BF16, act=ops.ACT_QGELU, out2=nan()),
    }
    for cfg in (-1, 8, 1):
        for what, kw in cases.items():
            out = nan()
            with pytest.raises(RuntimeError) as ei:
                ops.gemm(a, w, bias if kw["epi"] != ops.EPI_DGELU else None, out=out, cfg=cfg, **kw)
            assert "vl_gemm_bf16" in str(ei.value), (what, str(ei.value))
            torch.cuda.synchronize()
            assert bool(torch.isnan(out).all()), what                       # nothing ran
            if kw.get("out2") is not None:
                assert bool(torch.isnan(kw["out2"]).all()), what
        # QGELU_DSAVE without out2: the wrapper refuses it as it refuses the erf twin, the library refuses it by itself
        out = nan()
        for act in (ops.ACT_QGELU_DSAVE, ops.ACT_GELU_DSAVE):
            with pytest.raises(ValueError):
                ops.gemm(a, w, bias, out=out, cfg=cfg, epi=ops.EPI_BF16, act=act)
        from vitlens_hip.ops import _lib, _p, _stream
        rc = _lib.vl_gemm_bf16_ex(_p(a), _p(w), _p(bias), _p(out), None, None, M, N, K, a.stride(0), w.stride(0), out.stride(0), 1.0,
                                  ops.EPI_BF16, ops.ACT_QGELU_DSAVE, 1, cfg, _stream())
        assert rc != 0 and b"VL_ACT_QGELU_DSAVE needs out2" in _lib.vl_last_error()
        torch.cuda.synchronize()
        assert bool(torch.isnan(out).all())


# ---- tower level --------------------------------------------------------------------------------------------------------------
_CASE = {}


def _tiny():
    """tiny_depth.npz weights and inputs, the QuickGELU oracle's features and its autograd of the tri-modal step (once)."""
    if not _CASE:
        sd, ins, outs, grads, meta = split(load_npz("tiny_depth.npz"))
        tower, text, lens = specs_from_meta(meta)
        sdg = {k: (v.clone().requires_grad_(True) if (k.startswith("visual.") or k == "logit_scale") else v) for k, v in sd.items()}
        with quick_gelu_oracle():
            i = O.encode_image(sdg, ins["image"], tower)
            t = O.encode_text(sdg, ins["text"], text)
            v = O.encode_visual(sdg, ins["visual_x"], tower, lens)
            loss = O.tri_clip_loss(O.l2_normalize(i), O.l2_normalize(t), O.l2_normalize(v), sdg["logit_scale"].exp())
            loss.backward()
        with torch.no_grad():
            erf_i = O.encode_image(sd, ins["image"], tower)
        _CASE.update(sd=sd, ins=ins, meta=meta, tower=tower, text=text, lens=lens, image=i.detach(), textf=t.detach(),
                     visual=v.detach(), loss=float(loss), grads={k: p.grad for k, p in sdg.items() if p.requires_grad},
                     erf_image=erf_i, d_image=relerr(erf_i, i.detach()))
        assert _CASE["d_image"] > 1e-3                                     # the two activations give different towers (4e-3)
    return SimpleNamespace(**_CASE)


def _cfgs(c, quick_gelu=True):
    from vitlens_hip import engine as E
    tw, tx = c.tower, c.text
    tc = E.TowerCfg(width=tw.width, layers=tw.layers, heads=tw.heads, patch=tw.patch, image_size=tw.image_size,
                    embed_dim=tw.embed_dim, quick_gelu=quick_gelu)
    xc = E.TextCfg(context_length=tx.context_length, vocab_size=tx.vocab_size, width=tx.width, heads=tx.heads, layers=tx.layers,
                   embed_dim=tx.embed_dim, quick_gelu=quick_gelu)
    return E, tc, xc


def _cosm(a, b):
    n = lambda x: torch.nn.functional.normalize(x.float().cpu(), dim=-1)
    return n(a) @ n(b).t()


@pytest.mark.parametrize("res_dtype", [torch.float32, torch.bfloat16])
def test_quickgelu_image_and_text_towers(res_dtype):
    """The bounds of tests/test_hip_towers.py::test_tiny_golden_image_and_text, against the QuickGELU oracle."""
    c = _tiny()
    E, tc, xc = _cfgs(c)
    img = E.VitEngine(c.sd, "image.", tc, "cuda", res_dtype=res_dtype)
    f = img.encode_image(c.ins["image"].cuda())
    tol = 2e-2 if res_dtype == torch.float32 else 4e-2
    txt = E.TextEngine(c.sd, xc, "cuda", res_dtype=res_dtype)
    t = txt.encode_text(c.ins["text"].cuda())
    cm = float((_cosm(f, t) - _cosm(c.image, c.textf)).abs().max())
    print(f"{res_dtype}: image relerr {relerr(f, c.image):.2e}, text relerr {relerr(t, c.textf):.2e}, cosine matrix {cm:.2e}")
    assert relerr(f, c.image) < tol and relerr(t, c.textf) < tol
    assert cm < (5e-3 if res_dtype == torch.float32 else 8e-3)
    # flipping the flag changes the features: erf engines on the same weights give the erf oracle's tower, not this one
    E, tce, xce = _cfgs(c, quick_gelu=False)
    fe = E.VitEngine(c.sd, "image.", tce, "cuda", res_dtype=res_dtype).encode_image(c.ins["image"].cuda())
    te = E.TextEngine(c.sd, xce, "cuda", res_dtype=res_dtype).encode_text(c.ins["text"].cuda())
    print(f"erf engines against these: image {relerr(fe, f):.2e} (oracles: {c.d_image:.2e}), text {relerr(te, t):.2e}")
    # (the same kernels and rounding points either way: what separates the two runs is the activation, as far as it separates
    # the two oracles)
    assert relerr(fe, c.erf_image) < tol and relerr(fe, f) > 0.5 * c.d_image
    assert relerr(te, t) > 0.5 * c.d_image


@pytest.mark.parametrize("arith", ["bf16", "bf16x2"])
def test_quickgelu_text_engine_arithmetics(arith):
    c = _tiny()
    E, tc, xc = _cfgs(c)
    t = E.TextEngine(c.sd, xc, "cuda", arith=arith).encode_text(c.ins["text"].cuda())
    assert relerr(t, c.textf) < 2e-2, relerr(t, c.textf)


def test_quickgelu_text_engine_fp16_operands():
    """The fp16 text engine needs width % 256 == 0: two layers of width 512 (head dim 64), seeded, against the QuickGELU oracle;
    raw features 2e-2 and cosine matrix 1e-3, the bounds of the full-size erf towers in tests/test_hip_towers.py."""
    from vitlens_hip import engine as E
    spec = O.TextSpec(context_length=32, vocab_size=96, width=512, heads=8, layers=2, embed_dim=256)
    g = torch.Generator().manual_seed(5)
    sd = O.init_text(spec, g)
    txt = O.synth_text(4, g, ctx=32, vocab=96)
    with quick_gelu_oracle(), torch.no_grad():
        ref = O.encode_text(sd, txt, spec)
    erf = O.encode_text(sd, txt, spec)
    xc = E.TextCfg(context_length=32, vocab_size=96, width=512, heads=8, layers=2, embed_dim=256, quick_gelu=True)
    eng = E.TextEngine(sd, xc, "cuda")
    assert eng.arith == "f16"
    got = eng.encode_text(txt.cuda())
    cm = float((_cosm(got, got) - _cosm(ref, ref)).abs().max())
    print(f"f16 text tower: relerr {relerr(got, ref):.2e} (erf oracle {relerr(got, erf):.2e}), cosine matrix {cm:.2e}")
    assert relerr(got, ref) < 2e-2 and cm < 1e-3
    assert relerr(got, erf) > 0.5 * relerr(ref, erf)                      # the flag is not ignored (oracles: 1.1e-2 apart)


def test_quickgelu_depth_lens_forward_and_trainer_backward():
    """Depth Lens with an identity Perceiver: forward, and the trainer's backward against the QuickGELU oracle's autograd of the
    tri-modal loss; envelopes of tests/test_hip_train.py::test_depth_lens_forward_matches_golden /
    test_depth_tower_backward_vs_reference_grads."""
    from vitlens_hip import train as TR
    c = _tiny()
    E, tc, xc = _cfgs(c)
    le = E.LensEngine(c.sd, "visual.", tc, E.LensCfg(modality="depth", perceiver_identity=True), "cuda")
    f = le.encode(c.ins["visual_x"].cuda())
    assert relerr(f, c.visual) < 2e-2, relerr(f, c.visual)
    tr = TR.DepthLensTrainer(le, unlock_first_n=tc.layers)
    assert tr.tower.act_dsave == _ops().ACT_QGELU_DSAVE
    tr.tower.train_cls = tr.tower.train_pos = True
    feat = tr.forward(c.ins["visual_x"].cuda())
    assert relerr(feat, c.visual) < 2e-2
    v = c.visual.clone().requires_grad_(True)
    loss = O.tri_clip_loss(O.l2_normalize(c.image), O.l2_normalize(c.textf), O.l2_normalize(v), c.sd["logit_scale"].exp())
    assert abs(float(loss) - c.loss) < 1e-5
    loss.backward()
    tr.backward(v.grad.cuda())
    checked, worst = 0, ("", 0.0)
    for name, g in tr.grads.items():
        if name.endswith("conv1.weight_gemm"):
            ref = c.grads["visual.visual_adapter.conv1.weight"].reshape(g.shape[0], -1)
            got = g[:, :ref.shape[1]]
        else:
            ref, got = c.grads[name], g
        e = relerr(got, ref)
        worst = max(worst, (name, e), key=lambda p: p[1])
        assert e < 5e-2, (name, e)
        checked += 1
    print("worst gradient", worst)
    assert checked >= 2 * 12 + 4, checked


def test_quickgelu_fused_tri_modal_step():
    """One fused training step with quick_gelu in the cfgs it is handed: loss and every gradient against the QuickGELU oracle's
    autograd; envelopes of tests/test_hip_train.py::test_tri_modal_step_matches_reference_step."""
    from vitlens_hip import step as ST
    c = _tiny()
    E, tc, xc = _cfgs(c)
    st = ST.TriModalDepthStep(c.sd, tc, xc, "cuda", micro_batch=2, unlock_first_n=tc.layers, lr=1e-3)
    loss = st.forward_backward(c.ins["image"].cuda(), c.ins["text"].cuda(), c.ins["visual_x"].cuda())
    print("step loss", float(loss), "oracle", c.loss)
    assert abs(float(loss) - c.loss) < 2e-2, (float(loss), c.loss)
    n = 0
    for name, g in st.grads.items():
        if name == "logit_scale":
            ref = c.grads["logit_scale"].reshape(1)
        elif name.endswith("conv1.weight_gemm"):
            ref = c.grads["visual.visual_adapter.conv1.weight"].reshape(g.shape[0], -1); g = g[:, :ref.shape[1]]
        else:
            ref = c.grads[name]
        assert relerr(g, ref) < 6e-2, (name, relerr(g, ref))
        n += 1
    assert n == 12 * tc.layers + 3
    # the erf step on the same weights has another loss gradient: the flag is not ignored
    E, tce, xce = _cfgs(c, quick_gelu=False)
    se = ST.TriModalDepthStep(c.sd, tce, xce, "cuda", micro_batch=2, unlock_first_n=tc.layers, lr=1e-3)
    se.forward_backward(c.ins["image"].cuda(), c.ins["text"].cuda(), c.ins["visual_x"].cuda())
    k = "visual.transformer.resblocks.0.mlp.c_fc.weight"
    e_q, e_e = relerr(st.grads[k], c.grads[k]), relerr(se.grads[k], c.grads[k])
    print("c_fc gradient against the QuickGELU oracle: quick_gelu step", e_q, "erf step", e_e)
    assert e_e > e_q


def _api_model(c, precision="amp_bf16", **kw):
    import open_clip as oc
    with tempfile.TemporaryDirectory() as td:
        with open(os.path.join(td, "tiny-lens.json"), "w") as f:
            json.dump(c.meta["model_cfg"], f)
        oc.add_model_config(td)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            model = oc.tri_create_model("tiny-lens", None, precision=precision, device="cuda", output_dict=True,
                                        args=SimpleNamespace(**c.meta["args"]), **kw)
    model.load_state_dict(c.sd, strict=False)
    return model


def test_quickgelu_through_the_public_interface():
    """tri_create_model(force_quick_gelu=True): frozen image / text / depth towers in eval mode, the flag flipped, and a text
    tower that is not locked (TextTowerTrainer) against the oracle's autograd - the envelopes of tests/test_hip_api.py."""
    c = _tiny()
    model = _api_model(c, force_quick_gelu=True).eval()
    with torch.no_grad():
        fi = model.encode_image(c.ins["image"].cuda())
        ft = model.encode_text(c.ins["text"].cuda())
        fv = model.encode_visual(c.ins["visual_x"].cuda())
    assert relerr(fi, c.image) < 4e-2 and relerr(ft, c.textf) < 4e-2 and relerr(fv, c.visual) < 4e-2
    with torch.no_grad():
        ei = _api_model(c).eval().encode_image(c.ins["image"].cuda())
    assert relerr(ei, c.erf_image) < 4e-2 and relerr(ei, fi) > 0.5 * c.d_image
    # trainable text tower
    txt = c.ins["text"].cuda()
    r = torch.randn(txt.shape[0], c.text.embed_dim, generator=torch.Generator().manual_seed(3))
    model.train()
    f = model.encode_text(txt)
    assert f.requires_grad
    (f * r.cuda()).sum().backward()
    names = [n for n, p in model.named_parameters() if not n.startswith(("image.", "visual.")) and n != "logit_scale"]
    sdc = {k: v.clone().float().requires_grad_(k in names) for k, v in c.sd.items() if not k.startswith(("image.", "visual."))}
    with quick_gelu_oracle():
        ref = O.encode_text(sdc, c.ins["text"], c.text, normalize=False)
        (ref * r).sum().backward()
    assert relerr(f, ref) < 2e-2, relerr(f, ref)
    bad = {}
    for n in names:
        got, want = dict(model.named_parameters())[n].grad, sdc[n].grad
        if want is None or float(want.abs().max()) == 0.0:
            assert float(got.abs().max()) < 1e-6, n
            continue
        if relerr(got, want) > 6e-2:
            bad[n] = round(relerr(got, want), 4)
    assert not bad, bad


def test_quickgelu_precision_fp32_routes_to_the_f32_engines():
    """precision="fp32", eval mode: the fp32 engines with the flag, features within 1e-5 relative (tests/test_hip_f32.py)."""
    from vitlens_hip import f32 as F
    c = _tiny()
    model = _api_model(c, precision="fp32", force_quick_gelu=True).eval()
    with torch.no_grad():
        fi = model.encode_image(c.ins["image"].cuda())
        ft = model.encode_text(c.ins["text"].cuda())
        fv = model.encode_visual(c.ins["visual_x"].cuda())
    assert isinstance(model.image._engine_f32(), F.VitEngineF32) and isinstance(model._text(), F.TextEngineF32)
    assert model.image._engine_f32().cfg.quick_gelu and model._text().cfg.quick_gelu
    e = (relerr(fi, c.image), relerr(ft, c.textf), relerr(fv, c.visual))
    print("fp32 engines: image, text, depth relerr", e)
    assert max(e) < 1e-5, e
