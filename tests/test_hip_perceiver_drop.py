"""GPU: Perceiver dropout (csrc/vl_lens_drop.hip, the attention backward in csrc/vl_attn_bwd.hip) - the attention forward and
backward with the mask on the probabilities per (b, h, 32-row) block against float64 under the numpy mask of
tests/perceiver_drop_ref.py, the dropout backward at p = 0.0 against the p = 0 backward, the FeedForward row kernels exactly,
p = 0 as today's path bit for bit, a whole tiny Perceiver through PerceiverTrainer and through the drop-in model, and the
fused audio step under micro-batching and resume.

Tolerances of the attention kernels are not fixed numbers: each is 4x the worst block of a CPU emulation of the same arithmetic
against float64 on the same inputs (the rule of tests/test_hip_f32_lens.py, applied to bf16).  The figures are printed and, when
VITLENS_PERCEIVER_DROP_ERRORS names a file, written there (profiles/perceiver_dropout_errors.json is such a run)."""
import json
import os
import tempfile
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import attn_ref as A
import perceiver_drop_ref as R
import vitlens_oracle as O
from errloc import attn_block_relerr
from golden_util import load_npz, specs_from_meta, split

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
LN2 = 0.6931471805599453
ERRORS = {}


@pytest.fixture(scope="module", autouse=True)
def _write_errors():
    yield
    path = os.environ.get("VITLENS_PERCEIVER_DROP_ERRORS")
    if path:
        with open(path, "w") as f:
            json.dump(ERRORS, f, indent=1, sort_keys=True)


def _ops():
    from vitlens_hip import ops
    return ops


def relerr(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-300))


# ------------------------------------------------------------------------------------------------ attention, shared per case
_CASE = {}


def attn_case(name, p=None):
    """Inputs, mask, the float64 reference (forward and autograd) and the CPU emulations of one case (at another probability
    than its own if `p` is given) - computed once."""
    if (name, p) in _CASE:
        return _CASE[name, p]
    B, H, Lq, Lk, dh, p_case, seed = R.ATTN_CASES[name]
    key, p = (name, p), p_case if p is None else p
    q, k, v, qscale = A.make_scores("normal", B, H, Lq, Lk, dh, seed=seed)
    dO = torch.randn(B, H, Lq, dh, generator=torch.Generator().manual_seed(seed + 1000)).to(BF)
    keep = R.attn_keep(seed, R.ATTN_SAMPLE0, R.ATTN_SUB, p, B, H, Lq, Lk)
    mult = torch.from_numpy(keep).double() * float(R.scale32(p))
    q2 = A.q_rounded(q, qscale, BF).double()                    # the rounding the kernels apply as they load q
    # float64 reference with autograd; the gradient of the (not differentiable) rounding is the scale itself
    qd, kd, vd = (t.double().requires_grad_(True) for t in (q, k, v))
    s = ((qd * qscale + (q2 - q.double() * qscale)) @ kd.transpose(-1, -2)) * LN2          # natural-log units
    lse = torch.logsumexp(s, -1)
    P = torch.exp(s - lse.unsqueeze(-1))
    out = (P * mult) @ vd
    out.backward(dO.double())
    ref = dict(out=out.detach(), lse=lse.detach(), dq=qd.grad, dk=kd.grad, dv=vd.grad)
    # the emulation, forward: unnormalised probabilities, mask and scale in fp32, rounding to bf16, float64 product with V,
    # division by the FULL sum, the result stored as bf16
    with torch.no_grad():
        s2 = q2 @ k.double().transpose(-1, -2)                  # log2 units
        pu = torch.exp2(s2 - s2.amax(-1, keepdim=True))
        pt = (pu.float() * mult.float()).to(BF).double()
        emu_out = ((pt @ v.double()) / pu.sum(-1, keepdim=True)).to(BF)
        # backward: P~ and dS rounded to bf16, outputs stored as bf16 (dk through q2, as the kernel forms it)
        Pn = P.detach()
        Pt = (Pn.float() * mult.float()).to(BF).double()
        delta = (dO.double() * out.detach()).sum(-1, keepdim=True)
        dS = (Pn * ((dO.double() @ v.double().transpose(-1, -2)) * mult - delta)).to(BF).double()
        scale = dh ** -0.5
        emu = dict(out=emu_out, dv=(Pt.transpose(-1, -2) @ dO.double()).to(BF), dq=(scale * (dS @ k.double())).to(BF),
                   dk=(LN2 * (dS.transpose(-1, -2) @ q2)).to(BF))
    _CASE[key] = SimpleNamespace(B=B, H=H, Lq=Lq, Lk=Lk, dh=dh, p=p, seed=seed, q=q, k=k, v=v, dO=dO, qscale=qscale, ref=ref, emu=emu)
    return _CASE[key]


def _tol(c, what, L):
    worst, _ = attn_block_relerr(c.emu[what].double(), c.ref[what], c.B, c.H, L)
    return 4.0 * worst, worst


def _run_fwd(c, drop=True):
    ops = _ops()
    q, k, v = c.q.cuda(), c.k.cuda(), c.v.cuda()
    out = torch.full((c.B * c.Lq, c.H * c.dh), float("nan"), device="cuda", dtype=BF)
    lse = torch.full((c.B, c.H, c.Lq), float("nan"), device="cuda")
    if drop:
        ops.attn_fwd_drop(q, k, v, out, c.p, c.seed, R.ATTN_SAMPLE0, R.ATTN_SUB, lse=lse, qscale=c.qscale)
    else:
        ops.attn_fwd(q, k, v, out, lse=lse, qscale=c.qscale)
    return out, lse


@pytest.mark.parametrize("name", list(R.ATTN_CASES))
def test_attention_forward_with_dropout_per_block(name):
    c = attn_case(name)
    out, lse = _run_fwd(c)
    again, lse2 = _run_fwd(c)
    assert torch.isfinite(out.float()).all() and torch.isfinite(lse).all()
    assert torch.equal(out, again) and torch.equal(lse, lse2), "two launches differ"
    tol, emu = _tol(c, "out", c.Lq)
    got = out.cpu()
    kw, (b, h, r0, r1) = attn_block_relerr(got, c.ref["out"], c.B, c.H, c.Lq)
    print(f"fwd {name}: kernel worst block {kw:.3e} (b={b} h={h} queries {r0}:{r1}), emulation worst block {emu:.3e}, tol {tol:.3e}")
    ERRORS[f"attn_fwd/{name}"] = dict(kernel=kw, emulation=emu, tol=tol)
    assert kw <= tol, f"b={b} h={h} queries {r0}:{r1}: {kw:.3e} > {tol:.3e}"
    # the check sees one block scaled by 1 + 3 tol
    bad = got.clone().float().reshape(c.B, c.Lq, c.H, c.dh)
    bad[b, r0:r1, h] *= 1 + 3 * tol
    assert attn_block_relerr(bad.reshape(got.shape).to(BF), c.ref["out"], c.B, c.H, c.Lq)[0] > tol
    # lse: the p = 0 entry's on the same inputs, bit for bit (the mask sits behind the running sum), and the reference's
    out0, lse0 = _run_fwd(c, drop=False)
    assert torch.equal(lse, lse0)
    assert float((lse.cpu().double() - c.ref["lse"]).abs().max()) < 1e-4
    assert not torch.equal(out, out0)


@pytest.mark.parametrize("name", list(R.ATTN_CASES))
def test_attention_backward_with_dropout_per_block(name):
    ops = _ops()
    c = attn_case(name)
    out, lse = _run_fwd(c)
    q, k, v, dO = c.q.cuda(), c.k.cuda(), c.v.cuda(), c.dO.cuda()
    inner = c.H * c.dh
    o = ops.heads_view(out, c.B, c.Lq, c.H, c.dh)

    def run():
        dq = torch.full((c.B * c.Lq, inner), float("nan"), device="cuda", dtype=BF)
        dkv = torch.full((c.B * c.Lk, 2 * inner), float("nan"), device="cuda", dtype=BF)
        delta = torch.full((c.B, c.H, c.Lq), float("nan"), device="cuda")
        ops.attn_bwd_drop(q, k, v, dO, o, lse, delta, dq, dkv, dkv[:, inner:], inner, 2 * inner, c.p, c.seed, R.ATTN_SAMPLE0, R.ATTN_SUB)
        return dq, dkv
    dq, dkv = run()
    dq2, dkv2 = run()
    assert torch.equal(dq, dq2) and torch.equal(dkv, dkv2), "two launches differ"
    got = dict(dq=dq.cpu(), dk=dkv[:, :inner].cpu().contiguous(), dv=dkv[:, inner:].cpu().contiguous())
    for what, L, rows in (("dq", c.Lq, "queries"), ("dk", c.Lk, "keys"), ("dv", c.Lk, "keys")):
        assert torch.isfinite(got[what].float()).all(), what
        tol, emu = _tol(c, what, L)
        kw, (b, h, r0, r1) = attn_block_relerr(got[what], c.ref[what], c.B, c.H, L)
        print(f"bwd {name} {what}: kernel worst block {kw:.3e} (b={b} h={h} {rows} {r0}:{r1}), emulation worst block {emu:.3e}, tol {tol:.3e}")
        ERRORS[f"attn_bwd/{name}/{what}"] = dict(kernel=kw, emulation=emu, tol=tol)
        assert kw <= tol, f"{what} b={b} h={h} {rows} {r0}:{r1}: {kw:.3e} > {tol:.3e}"


@pytest.mark.parametrize("name", ["b", "c"])
def test_backward_dropout_entry_at_p0_is_the_two_kernel_backward(name):
    """One body for both entries (csrc/vl_attn_bwd.hip): at p = 0.0 the threshold is 0 and the scale 1, so every element is kept
    and the dropout instantiation computes what attn_bwd(fused=False) computes.  delta is the same code; dq: (dp - delta) P and
    P fma(dp, 1, -delta) round identically; dv: P * 1 = P - all three bit-equal.  dk sums the same dS, but -delta enters dP's
    accumulation in front of the products in one kernel and behind them in the other: the per-block rule against float64."""
    ops = _ops()
    c = attn_case(name, p=0.0)
    out, lse = _run_fwd(c, drop=False)
    q, k, v, dO = c.q.cuda(), c.k.cuda(), c.v.cuda(), c.dO.cuda()
    inner = c.H * c.dh
    o = ops.heads_view(out, c.B, c.Lq, c.H, c.dh)

    def run(drop):
        dq = torch.full((c.B * c.Lq, inner), float("nan"), device="cuda", dtype=BF)
        dkv = torch.full((c.B * c.Lk, 2 * inner), float("nan"), device="cuda", dtype=BF)
        delta = torch.full((c.B, c.H, c.Lq), float("nan"), device="cuda")
        args = (q, k, v, dO, o, lse, delta, dq, dkv, dkv[:, inner:], inner, 2 * inner)
        if drop:
            ops.attn_bwd_drop(*args, 0.0, c.seed, R.ATTN_SAMPLE0, R.ATTN_SUB)
        else:
            ops.attn_bwd(*args, fused=False)
        return delta, dq, dkv[:, :inner].contiguous(), dkv[:, inner:].contiguous()
    delta0, dq0, dk0, dv0 = run(False)
    delta1, dq1, dk1, dv1 = run(True)
    assert torch.isfinite(delta1).all() and torch.equal(delta1, delta0)
    assert torch.isfinite(dq1.float()).all() and torch.equal(dq1, dq0)
    assert torch.isfinite(dv1.float()).all() and torch.equal(dv1, dv0)
    tol, emu = _tol(c, "dk", c.Lk)
    for which, dk in (("p = 0 entry", dk0), ("dropout entry", dk1)):
        kw, (b, h, r0, r1) = attn_block_relerr(dk.cpu(), c.ref["dk"], c.B, c.H, c.Lk)
        print(f"bwd {name} at p = 0, dk of the {which}: worst block {kw:.3e} (b={b} h={h} keys {r0}:{r1}), emulation {emu:.3e}, tol {tol:.3e}")
        assert kw <= tol, f"dk ({which}) b={b} h={h} keys {r0}:{r1}: {kw:.3e} > {tol:.3e}"


def test_attention_entries_refuse_what_they_do_not_take():
    ops = _ops()
    q = torch.zeros(1, 1, 32, 48, device="cuda", dtype=BF)
    out = torch.zeros(32, 48, device="cuda", dtype=BF)
    with pytest.raises(RuntimeError, match="head dim"):
        ops.attn_fwd_drop(q, q, q, out, 0.1, 0, 0, 0)
    q = torch.zeros(1, 1, 32, 64, device="cuda", dtype=BF)
    out = torch.zeros(32, 64, device="cuda", dtype=BF)
    for bad in (1.0, -0.1, float("nan")):
        with pytest.raises(RuntimeError, match="probability"):
            ops.attn_fwd_drop(q, q, q, out, bad, 0, 0, 0)
    x = torch.zeros(4, 6, device="cuda")
    with pytest.raises(RuntimeError, match="multiple of 4"):
        ops.ff_drop_fwd(x, x, x.clone(), 2, 2, 0.1, 0, 0, 0)


# ------------------------------------------------------------------------------------------------ FeedForward rows
@pytest.mark.parametrize("name", list(R.FF_CASES))
def test_ff_row_kernels_exact(name):
    """x1 = x0 + y * (M / (1 - p)) and dy = bf16(dx1 * (M / (1 - p))): numpy float32 with the fp32 scale, bit for bit."""
    ops = _ops()
    B, n, D, p, seed = R.FF_CASES[name]
    g = torch.Generator().manual_seed(seed)
    y, x0, dx = (torch.randn(B * n, D, generator=g) for _ in range(3))
    sub = R.ATTN_SUB + 1
    mult = R.ff_keep(seed, R.ATTN_SAMPLE0, sub, p, B, n, D).astype(np.float32) * R.scale32(p)
    x1 = torch.full((B * n, D), float("nan"), device="cuda")
    ops.ff_drop_fwd(y.cuda(), x0.cuda(), x1, B, n, p, seed, R.ATTN_SAMPLE0, sub)
    want = x0.numpy() + y.numpy() * mult
    assert want.dtype == np.float32 and np.array_equal(x1.cpu().numpy(), want)
    dy = torch.full((B * n, D), float("nan"), device="cuda", dtype=BF)
    dyf = torch.full((B * n, D), float("nan"), device="cuda")
    ops.ff_drop_bwd(dx.cuda(), dy, B, n, p, seed, R.ATTN_SAMPLE0, sub, dy_f32=dyf)
    assert torch.equal(dy.cpu(), torch.from_numpy(dx.numpy() * mult).to(BF)) and np.array_equal(dyf.cpu().numpy(), dx.numpy() * mult)
    dy2 = torch.full_like(dy, float("nan"))
    ops.ff_drop_bwd(dx.cuda(), dy2, B, n, p, seed, R.ATTN_SAMPLE0, sub)          # the unrounded copy is optional
    assert torch.equal(dy2, dy)
    # in place on the residual stream, as the engine's single-stream workspace runs it
    xs = x0.cuda()
    ops.ff_drop_fwd(y.cuda(), xs, xs, B, n, p, seed, R.ATTN_SAMPLE0, sub)
    assert torch.equal(xs, x1)


# ------------------------------------------------------------------------------------------------ a whole tiny Perceiver
def _tiny():
    sd, ins, outs, grads, meta = split(load_npz("tiny_audio.npz"))
    tower, text, lens = specs_from_meta(meta)
    return sd, ins, meta, tower, text, lens


def _lens_cfg(lens, **kw):
    from vitlens_hip import engine as E
    return E.LensCfg(**{k: getattr(lens, k) for k in E.LensCfg.__dataclass_fields__ if hasattr(lens, k)}, **kw)


def _trainer(sd, lens, **kw):
    from vitlens_hip import engine as E, train as T
    pe = E.PerceiverEngine(sd, "visual.perceiver.", _lens_cfg(lens, **kw), "cuda")
    return pe, T.PerceiverTrainer(pe, "visual.perceiver.")


def _perceiver_inputs(lens, B=4, Tc=40, seed=11):
    g = torch.Generator().manual_seed(seed)
    data = torch.randn(B * Tc, lens.input_chan, generator=g).to(BF)
    dlat = torch.randn(B * lens.num_latents, lens.latent_dim, generator=g)
    return B, Tc, data, dlat


def _run_trainer(pt, data, dlat, B, drop):
    for g in pt.grads.values():
        g.zero_()
    lat = pt.forward(data.cuda(), B, drop).clone()
    ddata = pt.backward(dlat.cuda()).clone()
    return lat, ddata, {k: v.clone() for k, v in pt.reference_named_grads().items()}


def test_p0_is_todays_path_bit_for_bit():
    """No draw, and a draw with pa = pf = 0 routed through the same argument: outputs and every gradient bit-identical."""
    from vitlens_hip import engine as E
    sd, ins, meta, tower, text, lens = _tiny()
    B, Tc, data, dlat = _perceiver_inputs(lens)
    pe, pt = _trainer(sd, lens)
    a = _run_trainer(pt, data, dlat, B, None)
    b = _run_trainer(pt, data, dlat, B, E.LensDrop(5, R.sample0(1, 0, 0), 0.0, 0.0))
    assert pe.draw(5, 0) is None
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and a[2].keys() == b[2].keys()
    for k in a[2]:
        assert torch.equal(a[2][k], b[2][k]), k
    assert torch.equal(pe.forward(data.cuda(), B), a[0])               # and the engine's forward is the trainer's


def _reference_perceiver(sd, lens, data, dlat, B, Tc, masks, pa, pf):
    P = "visual.perceiver."
    sdd = {k: v.double().requires_grad_(True) for k, v in sd.items() if k.startswith(P)}
    x = data.double().reshape(B, Tc, -1).requires_grad_(True)
    lat = R.perceiver(sdd, P, x, lens, masks, pa, pf).reshape(B * lens.num_latents, -1)
    lat.backward(dlat.double())
    return lat.detach(), x.grad.reshape(B * Tc, -1), {k: v.grad for k, v in sdd.items()}


def test_tiny_perceiver_trainer_with_dropout_against_float64():
    """PerceiverTrainer at pa = pf = 0.1 against float64 autograd of the restatement under the same masks; every quantity within
    2x ITS OWN error at p = 0 (the unchanged path, measured here): dropout adds one fp32 scale and removes terms."""
    sd, ins, meta, tower, text, lens = _tiny()
    B, Tc, data, dlat = _perceiver_inputs(lens)
    pa = pf = 0.1
    pe0, pt0 = _trainer(sd, lens)
    lat0, dd0, g0 = _run_trainer(pt0, data, dlat, B, None)
    rl0, rd0, rg0 = _reference_perceiver(sd, lens, data.float(), dlat, B, Tc, None, 0.0, 0.0)
    pe, pt = _trainer(sd, lens, attn_dropout=pa, ff_dropout=pf)
    drop = pe.draw(R.TINY_SEED, R.sample0(0, 0, 0))
    lat, dd, g = _run_trainer(pt, data, dlat, B, drop)
    masks = R.perceiver_masks(R.TINY_SEED, R.sample0(0, 0, 0), pa, pf, B, Tc, lens)
    rl, rd, rg = _reference_perceiver(sd, lens, data.float(), dlat, B, Tc, masks, pa, pf)
    assert relerr(rl, rl0) > 5e-2                                       # the masks do something
    rows = {"latents_out": (relerr(lat, rl), relerr(lat0, rl0)), "ddata": (relerr(dd, rd), relerr(dd0, rd0))}
    assert g.keys() == g0.keys() and len(g) >= 40
    for k in g:
        rows[k] = (relerr(g[k], rg[k].reshape(g[k].shape)), relerr(g0[k], rg0[k].reshape(g0[k].shape)))
    over = {}
    for k, (e, e0) in rows.items():
        print(f"tiny Perceiver {k}: error with dropout {e:.3e}, at p = 0 {e0:.3e}, ratio {e / max(e0, 1e-30):.2f}")
        if e > 2 * e0:
            over[k] = (e, e0)
    ERRORS["tiny_trainer"] = {k: dict(dropout=e, p0=e0) for k, (e, e0) in rows.items()}
    assert not over, over
    # the engine (a train-mode forward without autograd) draws the same masks from the same numbers
    assert torch.equal(pe.forward(data.cuda(), B, drop), lat)
    # ... and a second forward / backward of the trainer redraws them: bit-identical
    lat2, dd2, g2 = _run_trainer(pt, data, dlat, B, drop)
    assert torch.equal(lat, lat2) and torch.equal(dd, dd2) and all(torch.equal(g[k], g2[k]) for k in g)


def _oc():
    import importlib
    import sys
    for k in [k for k in sys.modules if k == "open_clip" or k.startswith("open_clip.")]:
        if "vit-lens_amd" not in (getattr(sys.modules[k], "__file__", "") or ""):
            del sys.modules[k]
    return importlib.import_module("open_clip")


def _model(sd, meta, **over):
    oc = _oc()
    args = SimpleNamespace(**dict(meta["args"], **over))
    with tempfile.TemporaryDirectory() as td:
        with open(os.path.join(td, "tiny-lens.json"), "w") as f:
            json.dump(meta["model_cfg"], f)
        oc.add_model_config(td)
        model = oc.tri_create_model("tiny-lens", None, precision="fp32", device="cuda", output_dict=True, args=args)
    model.load_state_dict(sd, strict=False)
    model.lock_image_tower(); model.lock_text_tower()
    return model


def _reference_tower(sd, tower, lens, x, w, masks, pa, pf):
    P = "visual."
    sdd = {k: v.double().requires_grad_(v.is_floating_point()) for k, v in sd.items() if k.startswith(P)}
    tok, pos = O.audio_tokens(sdd, P, x.double(), lens)
    lat = R.perceiver(sdd, P + "perceiver.", tok + pos, lens, masks, pa, pf)
    f = O.vit_trunk(sdd, P, lat, tower, lens.use_orig_pos)
    (f * w.double()).sum().backward()
    return f.detach(), {k[len(P):]: v.grad for k, v in sdd.items() if v.grad is not None}


def test_drop_in_model_train_mode_with_dropout():
    """tri_create_model(args.perceiver_*_dropout = 0.1).train() -> encode_visual -> backward against float64 under the same
    masks (tolerance: 2x the same quantity's error at p = 0); eval() gives the p = 0 features bit for bit, two train-mode
    forwards differ, re-seeding and resetting the count reproduces the first bit for bit."""
    sd, ins, meta, tower, text, lens = _tiny()
    x = ins["visual_x"]
    B = x.shape[0]
    w = torch.randn(B, tower.embed_dim, generator=torch.Generator().manual_seed(3))
    pa = pf = 0.1

    def run(model):
        model.zero_grad()
        f = model.encode_visual(x.cuda())
        (f * w.cuda()).sum().backward()
        return f.detach().clone(), {k: p.grad.clone() for k, p in model.visual.named_parameters() if p.grad is not None}
    m0 = _model(sd, meta).train()
    f0, g0 = run(m0)
    rf0, rg0 = _reference_tower(sd, tower, lens, x, w, None, 0.0, 0.0)
    m = _model(sd, meta, perceiver_attn_dropout=pa, perceiver_ff_dropout=pf).train()
    assert (m.visual._cfgs()[1].attn_dropout, m.visual._cfgs()[1].ff_dropout) == (pa, pf)
    m.visual.set_drop_seed(R.TINY_SEED)
    f, g = run(m)
    ntok = (g["visual_adapter.pos_emb"].shape[0])
    masks = R.perceiver_masks(R.TINY_SEED, R.sample0(0, 0, 0), pa, pf, B, ntok, lens)
    rf, rg = _reference_tower(sd, tower, lens, x, w, masks, pa, pf)
    rows = {"features": (relerr(f, rf), relerr(f0, rf0))}
    for k in g:
        if k.startswith(("perceiver.", "visual_adapter.")):
            rows[k] = (relerr(g[k], rg[k].reshape(g[k].shape)), relerr(g0[k], rg0[k].reshape(g0[k].shape)))
    assert len(rows) >= 40
    over = {}
    for k, (e, e0) in rows.items():
        print(f"drop-in model {k}: error with dropout {e:.3e}, at p = 0 {e0:.3e}, ratio {e / max(e0, 1e-30):.2f}")
        if e > 2 * e0:
            over[k] = (e, e0)
    ERRORS["tiny_model"] = {k: dict(dropout=e, p0=e0) for k, (e, e0) in rows.items()}
    assert not over, over
    # train mode draws anew at every forward; the same seed and count repeat the sequence
    with torch.no_grad():
        a = m.encode_visual(x.cuda()).clone()              # a train-mode forward WITHOUT autograd drops too (count 1)
        b = m.encode_visual(x.cuda()).clone()              # (count 2)
        assert not torch.equal(a, b) and not torch.equal(a, f)
        m.visual.set_drop_seed(R.TINY_SEED, forwards=1)
        assert torch.equal(m.encode_visual(x.cuda()), a)
    m.visual.set_drop_seed(R.TINY_SEED)
    f2, g2 = run(m)
    assert torch.equal(f2, f) and all(torch.equal(g2[k], g[k]) for k in g)
    # eval never drops: the p = 0 model's features, bit for bit (bf16 operands on both sides)
    m.eval(); m0.eval()
    m.visual.arith_f32 = m0.visual.arith_f32 = False
    with torch.no_grad():
        assert torch.equal(m.encode_visual(x.cuda()), m0.encode_visual(x.cuda()))


# ------------------------------------------------------------------------------------------------ the fused point-cloud step
def test_pc_step_with_dropout_runs_redraws_and_resumes():
    """TriModalPCStep (PCLensTrainer with drop=) on the tiny point-cloud golden at pa = pf = 0.1, two micro-batches of 2, the
    backward's halves on two streams: finite loss and gradients that differ from the p = 0 step's, two step objects bit-identical
    (nothing but the numbers decides the masks), the next optimizer step draws anew, and a step resumed from (state_dict,
    optimizer_state_dict) continues bit-identically.  BatchNorm on its running statistics, so that a micro-batch is a sample's
    only context."""
    from vitlens_hip import engine as E, step as ST
    sd, ins, outs, grads, meta = split(load_npz("tiny_pc.npz"))
    tower, text, lens = specs_from_meta(meta)
    tc = E.TowerCfg(width=tower.width, layers=tower.layers, heads=tower.heads, patch=tower.patch, image_size=tower.image_size,
                    embed_dim=tower.embed_dim)
    xc = E.TextCfg(context_length=text.context_length, vocab_size=text.vocab_size, width=text.width, heads=text.heads,
                   layers=text.layers, embed_dim=text.embed_dim)
    lc = _lens_cfg(lens)
    img, txt, pts, start = ins["image"].cuda(), ins["text"].cuda(), ins["visual_x"].cuda(), ins["fps_start"].cuda()
    mk = lambda **kw: ST.TriModalPCStep(sd, tc, xc, lc, "cuda", micro_batch=2, lr=1e-3, bn_training=False, **kw)
    kw = dict(perceiver_attn_dropout=0.1, perceiver_ff_dropout=0.1, drop_seed=R.TINY_SEED)
    fb = lambda s: s.forward_backward(img, txt, pts, start)
    p0, a, b = mk(), mk(**kw), mk(**kw)
    l0, la, lb = fb(p0), fb(a), fb(b)
    assert a._lens_drop and not p0._lens_drop and a.lens_draw(2).sample0 == R.sample0(0, 0, 2)
    assert a.trainers[0].perc.drop == a.lens_draw(0) and a.trainers[1].perc.drop == a.lens_draw(2)
    assert torch.isfinite(la) and all(torch.isfinite(g).all() for g in a.grads.values())
    assert abs(float(la) - float(l0)) > 1e-4 and not torch.equal(a.flat_grad, p0.flat_grad)
    assert torch.equal(la, lb) and torch.equal(a.flat_grad, b.flat_grad)
    assert torch.equal(fb(a), la)                                   # no optimizer step between: the same draw
    a.optimizer_step(); b.optimizer_step()
    saved, saved_opt = a.state_dict(), a.optimizer_state_dict()
    rs = mk(**kw)
    rs.load_state_dict(saved); rs.load_optimizer_state_dict(saved_opt)
    assert rs.lens_draw(0) == a.lens_draw(0) and a.lens_draw(0).sample0 == R.sample0(1, 0, 0)
    l1, l1r = fb(a), fb(rs)
    assert torch.equal(l1, l1r) and torch.equal(a.flat_grad, rs.flat_grad)


# ------------------------------------------------------------------------------------------------ the fused audio step
def test_dual_audio_step_with_dropout_microbatches_and_resume():
    """DualAudioStep at pa = pf = 0.1: two micro-batches of 2 = one of 4 (a sample's masks follow its place in the per-GPU
    batch) - loss within 1e-5, the bound of the micro-batch comparison in tests/test_hip_patch_dropout.py, gradients within 1e-4
    (fp32 sums of the same per-sample products in another order; measured beside the p = 0 step's own figure) - and a step
    resumed from (state_dict, optimizer_state_dict) draws what the uninterrupted run draws: the next loss bit-identical."""
    from vitlens_hip import engine as E, step as ST
    sd, ins, meta, tower, text, lens = _tiny()
    tc = E.TowerCfg(width=tower.width, layers=tower.layers, heads=tower.heads, patch=tower.patch, image_size=tower.image_size,
                    embed_dim=tower.embed_dim)
    xc = E.TextCfg(context_length=text.context_length, vocab_size=text.vocab_size, width=text.width, heads=text.heads,
                   layers=text.layers, embed_dim=text.embed_dim)
    lc = _lens_cfg(lens)
    vis, txt = ins["visual_x"].cuda(), ins["text"].cuda()
    mk = lambda mb, **kw: ST.DualAudioStep(sd, tc, xc, lc, "cuda", micro_batch=mb, lr=1e-3, **kw)
    kw = dict(perceiver_attn_dropout=0.1, perceiver_ff_dropout=0.1, drop_seed=R.TINY_SEED)
    figures = {}
    for tag, k in (("p0", {}), ("dropout", kw)):
        s2, s4 = mk(2, **k), mk(4, **k)
        l2, l4 = s2.forward_backward(vis, txt), s4.forward_backward(vis, txt)
        worst = max(relerr(s2.grads[n], s4.grads[n]) for n in s4.grads if n.startswith("visual.perceiver."))
        figures[tag] = (abs(float(l2) - float(l4)), worst)
        print(f"DualAudioStep {tag}: |loss(2x2) - loss(1x4)| = {figures[tag][0]:.3e}, worst Lens gradient relative difference {worst:.3e}")
        if tag == "dropout":
            st, st4 = s2, s4
    ERRORS["dual_audio_microbatch"] = {k: dict(loss=a, grads=b) for k, (a, b) in figures.items()}
    assert figures["dropout"][0] < 1e-5 and figures["dropout"][1] < 1e-4, figures
    assert st._lens_drop and st.lens.lens.attn_dropout == 0.1 and st.lens_draw(2).sample0 == R.sample0(0, 0, 2)
    p0 = mk(2)
    assert not p0._lens_drop and abs(float(p0.forward_backward(vis, txt)) - float(st.forward_backward(vis, txt))) > 1e-4
    # resume
    st.optimizer_step()
    saved, saved_opt = st.state_dict(), st.optimizer_state_dict()
    rs = mk(2, **kw)
    rs.load_state_dict(saved); rs.load_optimizer_state_dict(saved_opt)
    assert st.opt.t == rs.opt.t == 1 and st.lens_draw(0) == rs.lens_draw(0) and st.lens_draw(0).sample0 == R.sample0(1, 0, 0)
    l_a, l_b = st.forward_backward(vis, txt), rs.forward_backward(vis, txt)
    assert torch.equal(l_a, l_b) and torch.equal(st.flat_grad, rs.flat_grad)
    # defaults: the step as it was
    a, b = mk(2), mk(2, perceiver_attn_dropout=0.0, perceiver_ff_dropout=0.0, drop_seed=5)
    assert torch.equal(a.step(vis, txt), b.step(vis, txt)) and torch.equal(a.flat_grad, b.flat_grad)
