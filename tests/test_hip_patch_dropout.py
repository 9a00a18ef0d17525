"""GPU: patch dropout (FLIP token masking) - the selection kernel, the gathered token assembly, the scatter of its backward,
the towers that run on K + 1 rows, the module path (same tokens as the reference) and the fused step.  The reference side is
tests/patchdrop_ref.py, pinned to the imported reference by tests/test_patch_dropout_host.py."""
import ctypes
import json
import os
import tempfile
import warnings
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import vitlens_oracle as O
import patchdrop_ref as PR
from golden_util import load_npz, seeded_like, specs_from_meta, split

pytestmark = pytest.mark.gpu


def relerr(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def _distinct_keys(B, T, seed):
    """A seeded permutation of arange(T) per sample, scaled to floats around zero: no ties."""
    g = torch.Generator().manual_seed(seed)
    return torch.stack([(torch.randperm(T, generator=g).float() - T / 2) * 0.37 for _ in range(B)])


def _check_inverse(keep, inv, T):
    assert torch.equal(inv.cpu().long(), PR.inverse(keep.cpu(), T))


# ---- 1. the selection, explicit keys -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,T,K", [(3, 16, 8), (2, 256, 128), (2, 256, 64), (2, 49, 12), (1, 10, 1), (2, 600, 599), (1, 4096, 1024)])
def test_patch_keep_is_topk(B, T, K):
    from vitlens_hip import ops
    keys = _distinct_keys(B, T, 11 + T)
    keep, inv = ops.patch_keep(keys.cuda(), K)
    assert keep.dtype == torch.int32 and inv.dtype == torch.int32 and keep.shape == (B, K) and inv.shape == (B, T)
    assert torch.equal(keep.cpu().long(), torch.topk(keys, K, dim=-1).indices)
    _check_inverse(keep, inv, T)


def test_patch_keep_ties_go_to_the_lower_index():
    from vitlens_hip import ops
    for B, T, K in ((2, 50, 12), (1, 300, 299)):
        keep, inv = ops.patch_keep(torch.full((B, T), 0.25).cuda(), K)
        assert torch.equal(keep.cpu().long(), torch.arange(K).expand(B, K))
        _check_inverse(keep, inv, T)
    # -0.0 and +0.0 are one value (as in torch.topk's comparison): still in index order
    z = torch.zeros(1, 8); z[0, ::2] = -0.0
    assert ops.patch_keep(z.cuda(), 5)[0].cpu().tolist() == [[0, 1, 2, 3, 4]]


def test_patch_keep_refuses_bad_shapes_with_a_status():
    from vitlens_hip import _lib, ops
    lib = _lib.load_library()
    buf = torch.full((8192,), -7, dtype=torch.int32, device="cuda")
    p = ctypes.c_void_p(buf.data_ptr())
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for B, T, K in ((1, 16, 0), (1, 16, 17), (1, 4097, 8), (0, 16, 8)):
        assert lib.vl_patch_keep(None, 0, 0, B, T, K, p, p, s) != 0, (B, T, K)
        assert b"vl_patch_keep" in lib.vl_last_error()
    torch.cuda.synchronize()
    assert bool((buf == -7).all())                                   # nothing was launched
    for T, K in ((16, 0), (16, 17), (4097, 8)):
        with pytest.raises(RuntimeError):
            ops.patch_keep(torch.zeros(1, T, device="cuda"), K)


# ---- 2. the selection, the kernel's own keys -----------------------------------------------------------------------------------
@pytest.mark.parametrize("B,T,K", [(5, 256, 128), (3, 50, 12)])
def test_patch_keep_philox_keys(B, T, K):
    from vitlens_hip import ops
    seed, s0 = 0x1234567890ABCDEF, 2 ** 32 - 2                       # the 32-bit carry of the counter is crossed at b = 2
    keep, inv = ops.patch_keep(None, K, B=B, T=T, seed=seed, sample0=s0, device="cuda")
    want = PR.philox_keep(seed, s0, B, T, K)
    assert np.array_equal(keep.cpu().numpy(), want)
    _check_inverse(keep, inv, T)
    again = ops.patch_keep(None, K, B=B, T=T, seed=seed, sample0=s0, device="cuda")
    assert torch.equal(again[0], keep) and torch.equal(again[1], inv)
    other = ops.patch_keep(None, K, B=B, T=T, seed=seed + 1, sample0=s0, device="cuda")[0]
    assert not torch.equal(other, keep)
    assert np.array_equal(other.cpu().numpy(), PR.philox_keep(seed + 1, s0, B, T, K))
    # sample b of a call at sample0 is sample 0 of a call at sample0 + b
    one = ops.patch_keep(None, K, B=1, T=T, seed=seed, sample0=s0 + 2, device="cuda")[0]
    assert torch.equal(one[0], keep[2])


# ---- 3. the gathered assembly is the dense one, row for row ---------------------------------------------------------------------
@pytest.mark.parametrize("B,T,K", [(3, 16, 5), (2, 256, 128)])
@pytest.mark.parametrize("D", [64, 1024])
@pytest.mark.parametrize("tok_dtype,out_dtype", [(torch.bfloat16, torch.bfloat16), (torch.bfloat16, torch.float32),
                                                 (torch.float32, torch.float32), (torch.float32, torch.bfloat16)])
@pytest.mark.parametrize("with_pos2", [False, True])
def test_assemble_keep_rows_are_the_dense_rows(B, T, K, D, tok_dtype, out_dtype, with_pos2):
    from vitlens_hip import ops
    g = torch.Generator().manual_seed(D + T + K)
    r = lambda *s: torch.randn(*s, generator=g).cuda()
    tok = r(B * T, D).to(tok_dtype)
    cls, pos, pos2, w, b = r(D), r(T + 1, D), (r(T, D) if with_pos2 else None), r(D), r(D)

    def run(keep):
        rows = B * (T + 1) if keep is None else B * (keep.shape[1] + 1)
        y = torch.full((rows, D), float("nan"), device="cuda", dtype=out_dtype)
        xpre = torch.full((rows, D), float("nan"), device="cuda")
        mean, rstd = torch.full((rows,), float("nan"), device="cuda"), torch.full((rows,), float("nan"), device="cuda")
        if keep is None:
            ops.assemble_ln_pre(tok, cls, pos, pos2, w, b, y, B, T, D, xpre=xpre, mean=mean, rstd=rstd)
        else:
            ops.assemble_ln_pre_keep(tok, keep, cls, pos, pos2, w, b, y, B, T, D, xpre=xpre, mean=mean, rstd=rstd)
        return y, xpre, mean, rstd
    dense = run(None)
    keep = ops.patch_keep(_distinct_keys(B, T, 5).cuda(), K)[0]
    rows = torch.cat([torch.zeros(B, 1, dtype=torch.long), 1 + keep.cpu().long()], dim=1) + torch.arange(B)[:, None] * (T + 1)
    rows = rows.reshape(-1).cuda()
    for got, want, name in zip(run(keep), dense, ("y", "xpre", "mean", "rstd")):
        assert not torch.isnan(got.float()).any(), name
        assert torch.equal(got, want[rows]), name
    # all tokens kept, in order: the dense call
    ident = torch.arange(T, dtype=torch.int32, device="cuda").expand(B, T).contiguous()
    for got, want, name in zip(run(ident), dense, ("y", "xpre", "mean", "rstd")):
        assert torch.equal(got, want), name
    # without the training outputs
    y = torch.empty(B * (K + 1), D, device="cuda", dtype=out_dtype)
    ops.assemble_ln_pre_keep(tok, keep, cls, pos, pos2, w, b, y, B, T, D)
    assert torch.equal(y, dense[0][rows])


# ---- 4. the scatter ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,T,K,D", [(3, 16, 5, 64), (2, 256, 64, 1024), (2, 10, 3, 7)])
def test_scatter_rows_keep(B, T, K, D):
    from vitlens_hip import ops
    g = torch.Generator().manual_seed(T + D)
    src = torch.randn(B * (K + 1), D, generator=g).cuda()
    keep, inv = ops.patch_keep(_distinct_keys(B, T, 6).cuda(), K)
    out = torch.full((B * T, D), float("nan"), device="cuda")
    got = ops.scatter_rows_keep(src, inv, K, out=out)
    want = torch.zeros(B, T, D)
    s = src.cpu().view(B, K + 1, D)
    want[torch.arange(B)[:, None], keep.cpu().long()] = s[:, 1:]
    assert got.data_ptr() == out.data_ptr() and torch.equal(got.cpu().view(B, T, D), want)
    dropped = inv.cpu() == 0
    assert int(dropped.sum()) == B * (T - K) and bool((got.cpu().view(B, T, D)[dropped] == 0).all())


# ---- 5. dropping equals a shorter tower, exactly ---------------------------------------------------------------------------------
@pytest.mark.parametrize("train_blocks,checkpoint", [((0,), False), ((), False), ((0,), True)])
def test_dropping_equals_a_shorter_tower(train_blocks, checkpoint):
    """ViT-L geometry, 2 blocks, one sample, 128 of 256 tokens kept, bf16 stream: the tower with `keep` against a tower on an
    engine whose position table and input tokens were gathered beforehand - the same kernels on the same rows, bit for bit.
    Block 1 is frozen, so the pruned last block runs (forward and backward) unless checkpoint=True recomputes it densely."""
    from vitlens_hip import engine as E, ops, train as TR
    spec = O.TowerSpec(layers=2)
    g = torch.Generator().manual_seed(3)
    sd = O.init_tower(spec, g, "visual.")
    T, K, D = 256, 128, 1024
    tok = (torch.randn(T, D, generator=g) * 0.5).bfloat16().cuda()
    dfeat = torch.randn(1, 768, generator=g).cuda()
    keep, inv = ops.patch_keep(_distinct_keys(1, T, 9).cuda(), K)
    kl = keep[0].cpu().long()
    kw = dict(train_blocks=train_blocks, train_cls=True, checkpoint=checkpoint)
    a = TR.TowerTrainer(E.VitEngine(sd, "visual.", E.TowerCfg(layers=2), "cuda", res_dtype=torch.bfloat16), **kw)
    fa = a.forward(tok, 1, keep=keep, inv=inv).clone()
    da = a.backward(dfeat).clone()
    sd2 = dict(sd)
    sd2["visual.positional_embedding"] = sd["visual.positional_embedding"][torch.cat([torch.zeros(1, dtype=torch.long), 1 + kl])]
    b = TR.TowerTrainer(E.VitEngine(sd2, "visual.", E.TowerCfg(layers=2), "cuda", res_dtype=torch.bfloat16), **kw)
    fb = b.forward(tok[kl.cuda()].contiguous(), 1).clone()
    db = b.backward(dfeat)
    assert a._pruned == b._pruned == (not checkpoint)               # (block 1 is frozen in every case: pruned unless recomputed)
    assert torch.equal(fa, fb)
    want = torch.zeros(T, D, device="cuda")
    want[kl.cuda()] = db
    assert da.shape == (T, D) and torch.equal(da, want)
    assert set(a.grads) == set(b.grads) and len(a.grads) == 12 * len(train_blocks) + 1
    for k in a.grads:
        assert torch.equal(a.grads[k], b.grads[k]), k


# ---- 6. against autograd through the oracle ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [128, 64])
def test_vitl_dropped_tower_vs_oracle_autograd(K):
    """The geometry of test_hip_train.test_vitl_block_backward_vs_oracle_autograd with tokens dropped: L = 129 and 65."""
    from vitlens_hip import engine as E, ops, train as TR
    spec = O.TowerSpec(layers=2)
    g = torch.Generator().manual_seed(3)
    sd = O.init_tower(spec, g, "visual.")
    tok = torch.randn(2, 256, 1024, generator=g) * 0.5
    dfeat = torch.randn(2, 768, generator=g)
    keep, inv = ops.patch_keep(_distinct_keys(2, 256, 4).cuda(), K)
    top = ("visual.class_embedding", "visual.positional_embedding")
    sdg = {k: v.clone().requires_grad_(k.startswith("visual.transformer.resblocks.0.") or k in top) for k, v in sd.items()}
    tk = tok.clone().requires_grad_(True)
    fr = PR.vit_trunk_keep(sdg, "visual.", tk, spec, keep.cpu())
    (fr * dfeat).sum().backward()
    eng = E.VitEngine(sd, "visual.", E.TowerCfg(layers=2), "cuda")
    tr = TR.TowerTrainer(eng, train_blocks=[0], train_cls=True, train_pos=True)
    feat = tr.forward(tok.reshape(-1, 1024).cuda().bfloat16(), 2, keep=keep, inv=inv)
    assert relerr(feat, fr.detach()) < 3e-2, relerr(feat, fr.detach())
    dtok = tr.backward(dfeat.cuda()).reshape(2, 256, 1024)
    assert relerr(dtok, tk.grad) < 3e-2, relerr(dtok, tk.grad)
    for name, gbuf in tr.grads.items():
        assert relerr(gbuf, sdg[name].grad) < 3e-2, (name, relerr(gbuf, sdg[name].grad))
    assert len(tr.grads) == 12 + 2
    dropped = inv.cpu() == 0
    assert bool((dtok.cpu()[dropped] == 0).all()) and float(dtok.cpu()[~dropped].abs().max()) > 0
    unkept = torch.cat([torch.zeros(1, dtype=torch.bool), dropped.all(dim=0)])
    gpos = tr.grads["visual.positional_embedding"].cpu()
    assert bool((gpos[unkept] == 0).all()) and (K == 128 or int(unkept.sum()) > 0)


# ---- 7. module level: the reference's tokens ------------------------------------------------------------------------------------
def _tiny_model(p):
    import open_clip as oc
    from test_patch_dropout_host import TINY, reference
    ref = reference()
    meta = split(load_npz("tiny_depth.npz"))[4]
    assert meta["model_cfg"] == TINY
    with tempfile.TemporaryDirectory() as td:
        with open(os.path.join(td, "tiny-patchdrop.json"), "w") as f:
            json.dump(TINY, f)
        oc.add_model_config(td)
        try:
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                model = oc.tri_create_model("tiny-patchdrop", None, precision="fp32", device="cuda", output_dict=True,
                                            args=SimpleNamespace(**meta["args"]), force_patch_dropout=p)
        finally:
            from open_clip import factory
            factory._CONFIG_PATHS.pop()
            factory._rescan()
    missing = model.load_state_dict(seeded_like(ref["stats"], 31), strict=False)
    assert not missing.missing_keys, missing.missing_keys
    return model, ref["cases"][repr(p)]


def test_module_keeps_the_tokens_the_reference_keeps():
    from test_patch_dropout_host import GRADS, SEED, inputs
    model, case = _tiny_model(0.5)
    image, depth, dfeat = (t.cuda() for t in inputs())
    model.train()
    named = dict(model.named_parameters())
    for tower, x, enc in (("visual", depth, model.encode_visual), ("image", image, model.encode_image)):
        rec = case[tower]
        torch.manual_seed(SEED)
        feat = enc(x)
        e = relerr(feat.detach(), torch.tensor(rec["features"]))
        print(tower, "train-mode features", e)
        assert e < 2e-2, (tower, e)                                        # test_hip_train.py's bound for the tiny towers
        (feat * dfeat).sum().backward()
        for k in GRADS[tower]:
            e = relerr(named[k].grad, torch.tensor(rec["grads"][k]))
            print(k, e)
            assert e < 5e-2, (k, e)                                          # test_hip_train.py's bound for the tiny gradients
        # the frozen tower of a training run (no-grad forward, train mode) drops the same tokens
        torch.manual_seed(SEED)
        with torch.no_grad():
            f2 = enc(x)
        assert relerr(f2, torch.tensor(rec["features"])) < 2e-2
        a, b = enc(x).detach(), enc(x).detach()                              # no re-seeding: other tokens
        assert not torch.equal(a, b)
    model.eval()
    with torch.no_grad():
        for tower, x, enc in (("visual", depth, model.encode_visual), ("image", image, model.encode_image)):
            f = enc(x)
            assert relerr(f, torch.tensor(case["eval"][tower])) < 2e-2 and torch.equal(f, enc(x))


# ---- 8. the fused step ----------------------------------------------------------------------------------------------------------
def _step_setup():
    from vitlens_hip import engine as E
    sd, ins, outs, grads, meta = split(load_npz("tiny_depth.npz"))
    tower, text, lens = specs_from_meta(meta)
    tc = E.TowerCfg(width=tower.width, layers=tower.layers, heads=tower.heads, patch=tower.patch, image_size=tower.image_size,
                    embed_dim=tower.embed_dim)
    xc = E.TextCfg(context_length=text.context_length, vocab_size=text.vocab_size, width=text.width, heads=text.heads,
                   layers=text.layers, embed_dim=text.embed_dim)
    return sd, ins, tower, text, tc, xc


def _kept(st, B):
    return [st.drop_indices(t, v, 0, B)[0].cpu() for t, v in ((0, st.lens.vit), (1, st.image))]


def test_fused_step_with_patch_dropout():
    from vitlens_hip import step as ST
    sd, ins, tower, text, tc, xc = _step_setup()
    img, txt, vis = ins["image"].cuda(), ins["text"].cuda(), ins["visual_x"].cuda()
    B, T, seed = 4, 16, 2024
    K = PR.keep_count(T, 0.5)
    mk = lambda mb, **kw: ST.TriModalDepthStep(sd, tc, xc, "cuda", micro_batch=mb, unlock_first_n=tc.layers, lr=1e-3, **kw)
    st = mk(2, patch_dropout=0.5, drop_seed=seed)
    loss = st.forward_backward(img, txt, vis)
    # the hand-assembled step: the oracle with the kept rows of both ViT towers, keep recomputed on the host
    kv = torch.from_numpy(PR.philox_keep(seed, PR.sample0(0, 0, 0, 0), B, T, K))
    ki = torch.from_numpy(PR.philox_keep(seed, PR.sample0(0, 0, 1, 0), B, T, K))
    got_v, got_i = _kept(st, B)
    assert torch.equal(got_v, kv) and torch.equal(got_i, ki) and not torch.equal(kv, ki)
    train = lambda k: k == "logit_scale" or k.startswith(("visual.transformer.resblocks.", "visual.visual_adapter."))
    sdg = {k: v.clone().float().requires_grad_(train(k)) for k, v in sd.items()}
    with torch.no_grad():
        fi = O.l2_normalize(PR.vit_trunk_keep(sdg, "image.", O.image_tokens(sdg, "image.", ins["image"], tower), tower, ki))
        ft = O.encode_text(sdg, ins["text"], text, normalize=True)
    tok, pos2 = O.depth_tokens(sdg, "visual.", ins["visual_x"], tower)
    fv = O.l2_normalize(PR.vit_trunk_keep(sdg, "visual.", tok, tower, kv, pos2=pos2))
    want = O.tri_clip_loss(fi, ft, fv, sdg["logit_scale"].exp())
    want.backward()
    print("loss", float(loss), "reference", float(want.detach()))
    assert abs(float(loss) - float(want)) < 2e-2, (float(loss), float(want))   # test_tri_modal_step_matches_reference_step's bounds
    n = 0
    for name, g in st.grads.items():
        if name.endswith("conv1.weight_gemm"):
            ref = sdg["visual.visual_adapter.conv1.weight"].grad.reshape(g.shape[0], -1); g = g[:, :ref.shape[1]]
        else:
            ref = sdg[name].grad.reshape(g.shape)
        assert relerr(g, ref) < 6e-2, (name, relerr(g, ref))
        n += 1
    assert n == 12 * tc.layers + 3
    # the kept set of a sample does not depend on the micro-batch size
    st4 = mk(4, patch_dropout=0.5, drop_seed=seed)
    loss4 = st4.forward_backward(img, txt, vis)
    assert all(torch.equal(a, b) for a, b in zip(_kept(st4, B), (kv, ki)))
    assert torch.equal(torch.cat([st.drop_indices(0, st.lens.vit, o, 2)[0] for o in (0, 2)]).cpu(), kv)
    assert abs(float(loss4) - float(loss)) < 1e-5, (float(loss4), float(loss))
    # the next step draws other sets; a restored step draws what the original would have
    st.optimizer_step()
    saved, saved_opt = st.state_dict(), st.optimizer_state_dict()
    nxt = _kept(st, B)
    assert st.opt.t == 1 and not torch.equal(nxt[0], kv) and not torch.equal(nxt[1], ki)
    assert torch.equal(nxt[0], torch.from_numpy(PR.philox_keep(seed, PR.sample0(1, 0, 0, 0), B, T, K)))
    rs = mk(2, patch_dropout=0.5, drop_seed=seed)
    rs.load_state_dict(saved); rs.load_optimizer_state_dict(saved_opt)
    assert all(torch.equal(a, b) for a, b in zip(_kept(rs, B), nxt))
    l_a, l_b = st.forward_backward(img, txt, vis), rs.forward_backward(img, txt, vis)
    assert torch.equal(l_a, l_b)
    assert torch.equal(st.flat_grad, rs.flat_grad)


def test_fused_step_without_patch_dropout_is_the_step_as_it_was():
    from vitlens_hip import step as ST
    sd, ins, tower, text, tc, xc = _step_setup()
    img, txt, vis = ins["image"].cuda(), ins["text"].cuda(), ins["visual_x"].cuda()
    mk = lambda **kw: ST.TriModalDepthStep(sd, tc, xc, "cuda", micro_batch=2, unlock_first_n=1, lr=1e-3, **kw)
    a, b = mk(), mk(patch_dropout=0.0, drop_seed=5)
    for _ in range(2):
        la, lb = a.step(img, txt, vis), b.step(img, txt, vis)
        assert torch.equal(la, lb) and torch.equal(a.flat_grad, b.flat_grad)
    for k in a.masters:
        assert torch.equal(a.masters[k], b.masters[k]), k
    c = mk(patch_dropout=0.5)
    assert not torch.equal(c.step(img, txt, vis), mk().step(img, txt, vis))
