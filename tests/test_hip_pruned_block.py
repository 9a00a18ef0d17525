"""The pruned last block of a class-token-pooled tower (engine.PRUNE_LAST_BLOCK; engine.run_blocks(..., pooled_only=True) ->
block_forward(cls_only=True) -> _cls_tail_forward in engine.Bf16Arith, from VitEngine.trunk and train.TowerTrainer): everything
behind the last block's in-projection runs on the B class rows only.

Same tree, switch on and off: features, dxpre and every gradient of the trainable block 0, each path measured against a float64
torch autograd evaluation (the oracle's vit_trunk) of the same bf16-rounded parameters.  Bounds: the ones test_hip_train.py
asserts for the full path on a bf16 residual stream (features 2e-2: test_depth_lens_forward_matches_golden; gradients 6e-2:
test_tri_modal_step_matches_reference_step[bfloat16]; whole-tensor relative error); and the pruned path may not be further
from float64 than the full path by more than one extra bf16 store, 2^-9 relative (round to nearest, 8 significand bits).
"""
import inspect

import pytest
import torch

BF16 = torch.bfloat16
TOL_FEAT, TOL_GRAD = 2e-2, 6e-2            # test_hip_train.py: features vs reference, gradients of a bf16 stream vs reference
ONE_BF16_STORE = 2.0 ** -9


# ------------------------------------------------------------------------------------------------ host: which path runs
def test_fallbacks_select_the_full_path():
    from vitlens_hip import engine as E, train as T
    ok = dict(layers=2, train_blocks=[0], checkpoint=False, causal=False, res_dtype=BF16, D=256, H=4, L=257)
    assert T.prunes_last_block(**ok)
    assert not T.prunes_last_block(**{**ok, "train_blocks": [0, 1]})          # a trainable last block
    assert not T.prunes_last_block(**{**ok, "checkpoint": True})              # recompute of that block
    assert not T.prunes_last_block(**{**ok, "D": 320})                        # head dim 80
    assert not T.prunes_last_block(**{**ok, "res_dtype": torch.float32})      # fp32 stream
    assert not T.prunes_last_block(**{**ok, "causal": True})                  # the text tower's mask
    assert not T.prunes_last_block(**{**ok, "L": 1025})                       # beyond the single-query kernels
    # a caller asking for tokens: run_blocks prunes only when told that the class rows are all that is read
    assert inspect.signature(E.run_blocks).parameters["pooled_only"].default is False
    assert E.prune_last_ok(256, 4, BF16, 257) and not E.prune_last_ok(256, 4, BF16, 257, pooled_only=False)
    keep = E.PRUNE_LAST_BLOCK
    try:
        E.PRUNE_LAST_BLOCK = False
        assert not T.prunes_last_block(**ok) and not E.prune_last_ok(256, 4, BF16, 257)
    finally:
        E.PRUNE_LAST_BLOCK = keep


# ------------------------------------------------------------------------------------------------ GPU
def relerr(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-300))


_CACHE = {}


def _problem(L):
    """Two blocks, D = 256, H = 4, B = 3: bf16-rounded parameters, inputs, and the float64 autograd reference (computed once)."""
    if L in _CACHE:
        return _CACHE[L]
    import vitlens_oracle as O
    B, D = 3, 256
    spec = O.TowerSpec(width=D, layers=2, heads=4, patch=14, image_size=224, embed_dim=128)
    g = torch.Generator().manual_seed(17)
    sd = {k: v.bfloat16().float() for k, v in O.init_tower(spec, g, "visual.").items()}
    sd["visual.positional_embedding"] = sd["visual.positional_embedding"][:L].contiguous()
    tok = (torch.randn(B, L - 1, D, generator=g) * 0.5).bfloat16().float()
    dfeat = torch.randn(B, 128, generator=g)
    p0 = "visual.transformer.resblocks.0."
    sdg = {k: v.double().requires_grad_(k.startswith(p0) or k == "visual.class_embedding") for k, v in sd.items()}
    tk = tok.double().requires_grad_(True)
    feat = O.vit_trunk(sdg, "visual.", tk, spec)
    (feat * dfeat.double()).sum().backward()
    ref = {"feat": feat.detach(), "dtok": tk.grad, "dcls": sdg["visual.class_embedding"].grad,
           "grads": {k: v.grad for k, v in sdg.items() if k.startswith(p0)}}
    _CACHE[L] = (sd, tok, dfeat, ref)
    return _CACHE[L]


def _run(L, prune, fold, nan_fill=False):
    """Engine features and trainer forward + backward with the two switches set; optionally with NaN in everything the pruned
    path must neither read nor leave unwritten."""
    from vitlens_hip import engine as E, train as T
    sd, tok, dfeat, _ = _problem(L)
    B, D = tok.shape[0], tok.shape[2]
    keep = E.PRUNE_LAST_BLOCK, E.LN_FOLD
    try:
        E.PRUNE_LAST_BLOCK, E.LN_FOLD = prune, fold
        eng = E.VitEngine(sd, "visual.", E.TowerCfg(width=D, layers=2, heads=4, embed_dim=128), "cuda", res_dtype=BF16)
        tr = T.TowerTrainer(eng, train_blocks=[0])
        t2 = tok.reshape(-1, D).cuda().bfloat16()
        nan = float("nan")
        if nan_fill:
            ws, S = eng.workspace(B, L), tr.saved(B, L)
            ws.a.fill_(nan); ws.hid.fill_(nan)
            for t in (S.X[3], S.X[4], S.a[1], S.u[1], S.hid, S.lse[1], S.dx, S.du, S.dOm, S.delta, S.dqkv):
                t.fill_(nan)
        f_inf = eng.trunk(t2, B).clone()
        feat = tr.forward(t2, B).clone()
        assert tr._pruned is bool(prune)
        if nan_fill:          # the forward wrote the class rows of the last block's slots and nothing else of them
            S = tr.saved(B, L)
            for X in (S.X[3], S.X[4]):
                rows = X.view(B, L, D)
                assert bool(torch.isfinite(rows[:, 0]).all()) and bool(torch.isnan(rows[:, 1:]).all())
            assert bool(torch.isnan(S.a[1]).all()) and bool(torch.isnan(S.u[1]).all())
        tr.backward(dfeat.cuda())
        out = {"f_inf": f_inf, "feat": feat, "dxpre": tr.dxpre.clone(), "grads": {k: v.clone() for k, v in tr.grads.items()}}
        torch.cuda.synchronize()
        return out
    finally:
        E.PRUNE_LAST_BLOCK, E.LN_FOLD = keep


def _errors(res, ref, B, L, D):
    dx = res["dxpre"].view(B, L, D)
    e = {"feat": relerr(res["feat"], ref["feat"]), "f_inf": relerr(res["f_inf"], ref["feat"]),
         "dtok": relerr(dx[:, 1:], ref["dtok"]), "dcls": relerr(dx[:, 0].sum(0), ref["dcls"])}
    for k, g in res["grads"].items():
        e[k.split("resblocks.0.")[1]] = relerr(g, ref["grads"][k])
    return e


@pytest.mark.gpu
@pytest.mark.parametrize("L,fold", [(257, True), (50, True), (257, False)])
def test_pruned_block_against_full_block_and_fp64(L, fold):
    """Measured on the MI355X (L = 257, folded; full / pruned): features 3.96e-3 / 4.00e-3, token gradient 6.31e-3 / 6.18e-3,
    block-0 gradients 3.7e-3 .. 6.8e-3 on both paths, the largest pruned-over-full excess 4.3e-4 (ln_1.bias); the failure
    message prints both columns."""
    sd, tok, dfeat, ref = _problem(L)
    B, D = tok.shape[0], tok.shape[2]
    full, pruned = _run(L, False, fold), _run(L, True, fold)
    assert set(full["grads"]) == set(pruned["grads"]) and len(full["grads"]) == 12
    for r in (full, pruned):
        assert all(bool(torch.isfinite(t).all()) for t in (r["feat"], r["f_inf"], r["dxpre"], *r["grads"].values()))
    ef, ep = _errors(full, ref, B, L, D), _errors(pruned, ref, B, L, D)
    table = "\n".join(f"  {k:28s} full {ef[k]:.3e}  pruned {ep[k]:.3e}" for k in ef)
    print(f"PRUNED L={L} fold={fold}\n{table}")
    for k in ef:
        bound = TOL_FEAT if k in ("feat", "f_inf") else TOL_GRAD
        assert ep[k] <= bound, f"{k}: pruned path off by {ep[k]:.3e} > {bound:.0e}\n{table}"
        assert ep[k] <= ef[k] + ONE_BF16_STORE, f"{k}: pruned {ep[k]:.3e} exceeds full {ef[k]:.3e} by more than one bf16 store\n{table}"
    # the two paths against each other: the same computation up to the rounding of the class rows
    assert relerr(pruned["feat"], full["feat"]) <= TOL_FEAT and relerr(pruned["dxpre"], full["dxpre"]) <= TOL_GRAD
    for k in full["grads"]:
        assert relerr(pruned["grads"][k], full["grads"][k]) <= TOL_GRAD, k


@pytest.mark.gpu
def test_pruned_block_reads_no_stale_rows():
    """NaN in the non-class rows of the last block's residual slots, in its big a / u / hid / lse slots and in the backward's
    full-size temporaries (the residual-gradient stream included: nothing zero-fills it any more): results finite and the
    same bits as without."""
    clean, dirty = _run(257, True, True), _run(257, True, True, nan_fill=True)
    for k in ("f_inf", "feat", "dxpre"):
        assert bool(torch.isfinite(dirty[k]).all()), k
        assert torch.equal(clean[k], dirty[k]), k
    for k, g in clean["grads"].items():
        assert bool(torch.isfinite(dirty["grads"][k]).all()) and torch.equal(g, dirty["grads"][k]), k
