"""GPU: the similarity-masked contrastive loss (`ClipLossSimMask`) on the HIP kernels - vl_ce_stats_masked / vl_ce_grad_masked
under `vitlens_hip.step.pair_forward / pair_backward`, the `open_clip.ClipLossSimMask` module and `DualAudioStep` - against
the float64 restatement of tests/simmask_ref.py (pinned to the reference's module by tests/test_simmask_host.py).

Inputs (simmask_ref.clustered): teacher features in near-duplicate clusters, independent students; before anything runs on
the GPU the conditions of simmask_ref.check_inputs are asserted in float64 at every shape: no off-diagonal similarity within
1e-3 of the threshold (the kernels' mask and the float64 mask are the same set), 5-50 % of the off-diagonal masked, every
64-row block with masked and kept elements.

Shapes sit at the kernels' edges: 4 rows per block, 64-lane column strides, 64-row column chunks, 256-column blocks, 32 x 32
gradient tiles with padded ldg / ldgt; rectangular with a label offset = the --local-loss geometry; row-blocked with a ragged
last block.  Tolerances are those of tests/test_hip_loss.py: the arithmetic is the same."""
import functools
import math
from types import SimpleNamespace

import pytest
import torch

import simmask_ref as SR
from golden_util import load_npz, specs_from_meta, split

pytestmark = pytest.mark.gpu

THRES = 0.8
SCALE = 14.285714
#        R,   C,   off, w_col, chunk_rows
WHOLE = [(70, 70, 0, 0.5, 0), (130, 300, 0, 0.5, 0), (257, 257, 0, 0.5, 0), (48, 144, 96, 0.0, 0), (48, 144, 0, 0.0, 0)]
BLOCKED = [(200, 200, 0, 0.5, 64), (48, 144, 48, 0.0, 32)]           # 200 = 3 x 64 + a ragged last block of 8


@functools.lru_cache(maxsize=None)
def _case(R, C, off, w_col, thres=THRES, scale=SCALE):
    """Inputs (CPU, f32) and the float64 reference of one case, computed once and shared; nothing mutates them."""
    t, s = SR.clustered(C, 1000 + C)
    x = t[off:off + R].contiguous()
    SR.check_inputs(x, t, THRES, off)
    keep = SR.keep_mask(x, t, thres, off)
    ref = SR.with_grads(lambda a, b, sc: SR.pair_loss(a, b, sc, keep, off, 0.5, w_col), x, s, scale)
    return x, s, t, keep, ref


def test_seeded_inputs_meet_the_conditions_at_every_shape():
    for R, C, off, _, chunk in WHOLE + BLOCKED:
        t, _ = SR.clustered(C, 1000 + C)
        frac = SR.check_inputs(t[off:off + R], t, THRES, off)
        assert 0.05 <= frac <= 0.5
    t, _ = SR.clustered(96, 1096)
    SR.check_inputs(t, t, THRES)


@pytest.fixture
def nan_outputs(monkeypatch):
    """Every buffer the ops allocate with torch.empty starts as NaN: an element a kernel fails to write shows."""
    real = torch.empty

    def empty(*a, **kw):
        out = real(*a, **kw)
        return out.fill_(float("nan")) if out.is_floating_point() else out
    monkeypatch.setattr(torch, "empty", empty)


def _run(x, y, t_rows, t_cols, scale, off, w_col, chunk, thres=THRES):
    from vitlens_hip import step as ST
    mask = None if thres is None else (t_rows, t_cols, thres)
    loss, ctx = ST.pair_forward(x, y, scale, off, 0.5, w_col, chunk_rows=chunk, mask=mask)
    assert (ctx[2] is None and ctx[9] == chunk) if chunk else ctx[2] is not None
    dx, dy, ds = ST.pair_backward(ctx)
    torch.cuda.synchronize()
    return loss, dx, dy, ds


def _rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / b.norm())


@pytest.mark.parametrize("R,C,off,w_col,chunk", WHOLE + BLOCKED)
def test_masked_pair_vs_float64_twice_bit_identical(R, C, off, w_col, chunk, nan_outputs):
    x, s, t, keep, (ref_loss, ref_dx, ref_dy, ref_ds) = _case(R, C, off, w_col)
    xc, yc, tc = x.cuda(), s.cuda(), t.cuda()
    a = _run(xc, yc, xc, tc, SCALE, off, w_col, chunk)
    b = _run(xc, yc, xc, tc, SCALE, off, w_col, chunk)
    loss, dx, dy, ds = a
    print("loss", float(loss), ref_loss, "dx", _rel(dx, ref_dx), "dy", _rel(dy, ref_dy), "dscale", float(ds), ref_ds)
    assert all(torch.isfinite(v).all() for v in a)
    assert abs(float(loss) - ref_loss) < 2e-4 * max(1.0, abs(ref_loss)), (float(loss), ref_loss)
    assert _rel(dx, ref_dx) < 4e-2 and _rel(dy, ref_dy) < 4e-2, (_rel(dx, ref_dx), _rel(dy, ref_dy))
    assert abs(float(ds) - ref_ds) < 2e-2 * max(1e-3, abs(ref_ds)) + 2e-5, (float(ds), ref_ds)
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    if chunk:                                                       # row-blocked against the whole matrix of the same kernels
        lw, dxw, dyw, dsw = _run(xc, yc, xc, tc, SCALE, off, w_col, 0)
        print("vs whole: loss", float(loss) - float(lw), "dx", _rel(dx, dxw), "dy", _rel(dy, dyw), "dscale", float(ds) - float(dsw))
        assert abs(float(loss) - float(lw)) < 2e-5 * max(1.0, abs(ref_loss))
        assert _rel(dx, dxw) < 1e-2 and _rel(dy, dyw) < 1e-2
        assert abs(float(ds) - float(dsw)) < 1e-2 * max(1e-3, abs(ref_ds)) + 2e-5
    # the unmasked loss of these inputs is another number: the comparison above can tell the two apart
    plain = SR.with_grads(lambda a_, b_, sc: SR.pair_loss(a_, b_, sc, torch.ones_like(keep), off, 0.5, w_col), x, s, SCALE)[0]
    assert abs(plain - ref_loss) > 10 * 2e-4 * max(1.0, abs(ref_loss))         # (a property of the inputs, known before the GPU runs)


@pytest.mark.parametrize("R,C,off,w_col,chunk", WHOLE + BLOCKED)
def test_nothing_masked_is_the_unmasked_path_bit_for_bit(R, C, off, w_col, chunk):
    x, s, t, _, _ = _case(R, C, off, w_col)
    xc, yc, tc = x.cuda(), s.cuda(), t.cuda()
    got = _run(xc, yc, xc, tc, SCALE, off, w_col, chunk, thres=2.0)
    want = _run(xc, yc, None, None, SCALE, off, w_col, chunk, thres=None)
    for u, v in zip(got, want):
        assert torch.equal(u, v)


@pytest.mark.parametrize("R,C,off,w_col,chunk", WHOLE + BLOCKED)
def test_everything_masked_is_logit_zero_not_minus_infinity(R, C, off, w_col, chunk):
    """thres = -2: every off-diagonal element is masked.  As logit 0 each still counts 1 in the denominators:
    row loss = mean_i[log(exp(L_ii) + (C - 1)) - L_ii], column loss the same with the R - 1 other rows of the column.
    A -inf implementation gives 0."""
    x, s, t, _, _ = _case(R, C, off, w_col)
    d = SCALE * (x.double() * s.double()[off:off + R]).sum(-1)
    want = 0.5 * float((torch.log(torch.exp(d) + (C - 1)) - d).mean()) + w_col * float((torch.log(torch.exp(d) + (R - 1)) - d).mean())
    loss, dx, dy, ds = _run(x.cuda(), s.cuda(), x.cuda(), t.cuda(), SCALE, off, w_col, chunk, thres=-2.0)
    print("loss", float(loss), want)
    assert want > 1.0 and abs(float(loss) - want) < 2e-4
    keep = torch.arange(C)[None, :] == (torch.arange(R)[:, None] + off)
    ref = SR.with_grads(lambda a, b, sc: SR.pair_loss(a, b, sc, keep, off, 0.5, w_col), x, s, SCALE)
    assert abs(ref[0] - want) < 1e-9
    assert _rel(dx, ref[1]) < 4e-2 and _rel(dy, ref[2]) < 4e-2
    assert abs(float(ds) - ref[3]) < 2e-2 * max(1e-3, abs(ref[3])) + 2e-5


@pytest.mark.parametrize("R,C,off,w_col,chunk", WHOLE)
def test_masked_gradient_elements_are_exactly_zero(R, C, off, w_col, chunk, nan_outputs):
    """G / GT straight from vl_ce_grad_masked at logit_scale 5 (moderate logits: no kept element underflows bf16): every
    masked element is exactly 0, every kept element is not, the pad columns [C, ldg) / [R, ldgt) are 0."""
    from vitlens_hip import ops
    x, s, t, keep, _ = _case(R, C, off, w_col)
    xc, yc, tc = x.cuda(), s.cuda(), t.cuda()
    logits = ops.logits_gemm(ops.split_bf16x3(xc, 0), ops.split_bf16x3(yc, 1), 5.0)
    sim = ops.logits_gemm(ops.split_bf16x3(xc, 0), ops.split_bf16x3(tc, 1), 1.0)
    assert float((sim.double().cpu() - x.double() @ t.double().t()).abs().max()) < 1e-4       # << the 1e-3 margin
    row_lse, col_lse, diag = ops.ce_stats(logits, off, want_cols=(w_col != 0.0), sim=sim, thres=THRES)
    from vitlens_hip.step import _label_columns_only
    col_lse = _label_columns_only(col_lse, off, R)                    # as pair_forward does: C > R leaves columns without a label
    dscale = torch.zeros(1, device="cuda")
    G, GT = ops.ce_grad(logits, row_lse, col_lse, off, 0.5, w_col, 5.0, dscale, sim=sim, thres=THRES)
    torch.cuda.synchronize()
    g, gt = G.float().cpu(), GT.float().cpu()
    assert torch.isfinite(g).all() and torch.isfinite(gt).all()
    assert torch.equal(g[:, :C] == 0, ~keep) and torch.equal(gt[:, :R] == 0, ~keep.t())
    assert not g[:, C:].any() and not gt[:, R:].any()
    assert torch.equal(g[:, :C], gt[:, :R].t())
    # d/dscale has no term from a masked element: sum over the KEPT elements of G * logits / scale, in float64 from the
    # kernel's own logits
    lm = logits.double().cpu() * keep
    hot = (torch.arange(C)[None, :] == (torch.arange(R)[:, None] + off)).double()
    g64 = 0.5 / R * (torch.exp(lm - torch.logsumexp(lm, 1, keepdim=True)) - hot)
    if w_col:
        labelled = ((torch.arange(C) >= off) & (torch.arange(C) < off + R)).double()[None, :]     # the column loss's own columns
        g64 = g64 + w_col / R * (torch.exp(lm - torch.logsumexp(lm, 0, keepdim=True)) - hot) * labelled
    want = float((g64 * lm).sum() / 5.0)
    assert _rel(g[:, :C], g64 * keep) < 1e-2                                                   # bf16 rounding of G
    assert abs(float(dscale) - want) < 2e-2 * max(1e-3, abs(want)) + 2e-5, (float(dscale), want)
    assert torch.equal(diag.cpu(), logits.cpu()[torch.arange(R), torch.arange(R) + off])      # diag is never masked


def test_ops_refuse_a_sim_that_does_not_match_the_logits():
    from vitlens_hip import ops
    logits = torch.zeros(8, 12, device="cuda")
    lse = torch.zeros(8, device="cuda")
    good = torch.zeros(8, 12, device="cuda")
    bad = [torch.zeros(8, 16, device="cuda"), torch.zeros(12, 8, device="cuda"), good.double(), good.bfloat16(), good.cpu(),
           torch.zeros(8, 24, device="cuda")[:, ::2], good.reshape(-1)]
    for sim in bad:
        with pytest.raises((ValueError, TypeError)):
            ops.ce_stats(logits, 0, sim=sim, thres=0.8)
        with pytest.raises((ValueError, TypeError)):
            ops.ce_grad(logits, lse, None, 0, 0.5, 0.0, 1.0, None, sim=sim, thres=0.8)
    with pytest.raises(ValueError):
        ops.ce_stats(logits, 0, sim=good)                            # sim without thres
    with pytest.raises(ValueError):
        ops.ce_stats(logits, 0, thres=0.8)                           # thres without sim
    ops.ce_stats(logits, 0, sim=torch.zeros(8, 16, device="cuda")[:, :12], thres=0.8)          # a row stride is fine


@pytest.mark.parametrize("chunk_rows", [0, 64])
def test_device_side_temperature_masks_the_same_set(chunk_rows):
    """`scale` as the 1-element log-temperature on the device: x is scaled by exp(logit_scale) before the logits GEMM, and
    the similarities must NOT come from that scaled copy (every |sim| would grow 14-fold and mask another set).  Bounds of
    test_hip_loss.test_device_side_temperature_equals_the_host_scalar_path."""
    x, s, t, keep, ref = _case(200, 200, 0, 0.5, THRES, float(math.exp(math.log(1 / 0.07))))
    xc, yc = x.cuda(), s.cuda()
    log_s = torch.tensor([math.log(1 / 0.07)], device="cuda")
    sc = float(log_s.exp())
    la, dxa, dya, dsa = _run(xc, yc, xc, xc, sc, 0, 0.5, chunk_rows)
    lb, dxb, dyb, dsb = _run(xc, yc, xc, xc, log_s, 0, 0.5, chunk_rows)
    assert abs(float(la) - ref[0]) < 2e-4 * max(1.0, abs(ref[0]))
    assert abs(float(la) - float(lb)) < 2e-5 * max(1.0, abs(float(la)))
    assert _rel(dxb, dxa) < 2e-3 and _rel(dyb, dya) < 2e-3, (_rel(dxb, dxa), _rel(dyb, dya))
    assert abs(float(dsb) - float(dsa) * sc) < 2e-3 * max(1.0, abs(float(dsa) * sc)), (float(dsb), float(dsa) * sc)


def test_local_loss_uses_one_similarity_block_per_rank():
    """`pair_loss_and_grads` as each of W = 3 ranks computes it under local_loss (peers constant: no collective is needed),
    either side as the teacher: the value is the reference's per-rank value, the ranks' mean is the gathered loss."""
    from vitlens_hip import step as ST
    W, b = 3, 16
    t, s = SR.clustered(W * b, 1048)
    SR.check_inputs(t, t, THRES)
    at, as_ = t.cuda(), s.cuda()
    glob = float(SR.loss_gathered(t.double(), s.double(), SCALE, THRES))
    tot = 0.0
    for r in range(W):
        sl = slice(r * b, (r + 1) * b)
        want = SR.with_grads(lambda a, c, sc: SR.loss_local(a, c, t.double(), s.double(), r, sc, THRES), t[sl], s[sl], SCALE)
        loss, dt, dst, ds = ST.pair_loss_and_grads(None, r, W, at[sl], as_[sl], at, as_, SCALE, local_loss=True, dist=True,
                                                   sim_teacher="x", sim_thres=THRES)
        assert abs(float(loss) - want[0]) < 2e-4 * max(1.0, abs(want[0])), (r, float(loss), want[0])
        assert abs(float(ds) - want[3]) < 2e-2 * max(1e-3, abs(want[3])) + 2e-5
        # the same pair with the sides swapped and the teacher named on the other side (the DualAudioStep orientation)
        loss2, dst2, dt2, ds2 = ST.pair_loss_and_grads(None, r, W, as_[sl], at[sl], as_, at, SCALE, local_loss=True, dist=True,
                                                       sim_teacher="y", sim_thres=THRES)
        assert abs(float(loss2) - float(loss)) < 2e-5 * max(1.0, abs(want[0]))
        assert _rel(dst2, dst) < 1e-2 and _rel(dt2, dt) < 1e-2
        tot += float(loss)
    assert abs(tot / W - glob) < 2e-4 * max(1.0, abs(glob))


# ---- module level -----------------------------------------------------------------------------------------------------------
def _oc():
    import importlib, sys
    for k in [k for k in sys.modules if k == "open_clip" or k.startswith("open_clip.")]:
        f = getattr(sys.modules[k], "__file__", "") or ""
        if "vit-lens_amd" not in f:
            del sys.modules[k]
    return importlib.import_module("open_clip")


@pytest.mark.parametrize("how", ["class", "create_loss", "chunk_rows"])
def test_module_forward_backward_vs_float64(how):
    oc = _oc()
    B = 96
    t, s = SR.clustered(B, 1096)
    SR.check_inputs(t, t, THRES)
    want = SR.with_grads(lambda a, b, sc: SR.loss_world1(a, b, sc, THRES), t, s, SCALE)
    if how == "create_loss":
        mod = oc.create_loss(SimpleNamespace(local_loss=False, gather_with_grad=False, rank=0, world_size=1, horovod=False, n_tower=3,
                                             use_dual_loss=True, contra_loss_type="sim_mask", sim_thres=THRES, model="ViT-B-32"))
        assert type(mod) is oc.ClipLossSimMask
    else:
        mod = oc.ClipLossSimMask(sim_thres=THRES, chunk_rows=32 if how == "chunk_rows" else None)
    x = t.cuda().requires_grad_(True); y = s.cuda().requires_grad_(True)
    ls = torch.tensor(SCALE, device="cuda", requires_grad=True)
    out = mod(x, y, ls, output_dict=True)
    assert list(out) == ["contrastive loss[with sim mask]"]
    loss = mod(x, y, ls)
    assert torch.equal(loss, out["contrastive loss[with sim mask]"])
    loss.backward()
    print("loss", float(loss), want[0], "dx", _rel(x.grad, want[1]), "dy", _rel(y.grad, want[2]), "dscale", float(ls.grad), want[3])
    assert abs(float(loss) - want[0]) < 2e-4 * max(1.0, abs(want[0]))
    assert _rel(x.grad, want[1]) < 4e-2 and _rel(y.grad, want[2]) < 4e-2        # the teacher's own gradient is the ordinary dx
    assert abs(float(ls.grad) - want[3]) < 2e-2 * max(1e-3, abs(want[3])) + 2e-5
    assert abs(float(oc.ClipLossGeneral()(x.detach(), y.detach(), ls.detach())) - want[0]) > 1e-2      # and it is not the plain loss


def test_teacher_side_module_vs_the_fused_steps_call():
    """The module takes (teacher, student); `DualAudioStep` calls `pair_loss_and_grads` with the visual (student) features in
    the x position and names the teacher: the same loss (the transposed logits through the same kernels: fp32 summation
    order) and the same gradients; naming the other side is another loss."""
    from vitlens_hip import step as ST
    oc = _oc()
    B = 96
    text, visual = SR.clustered(B, 1096)
    tx = text.cuda().requires_grad_(True); vx = visual.cuda().requires_grad_(True)
    ls = torch.tensor(SCALE, device="cuda", requires_grad=True)
    loss = oc.ClipLossSimMask(sim_thres=THRES)(tx, vx, ls)
    loss.backward()
    l2, dv, dt, ds = ST.pair_loss_and_grads(None, 0, 1, visual.cuda(), text.cuda(), visual.cuda(), text.cuda(), SCALE,
                                            sim_teacher="y", sim_thres=THRES)
    assert abs(float(l2) - float(loss)) < 2e-5 * max(1.0, abs(float(loss)))
    assert _rel(dv, vx.grad) < 1e-2 and _rel(dt, tx.grad) < 1e-2
    assert abs(float(ds) - float(ls.grad)) < 1e-2 * max(1e-3, abs(float(ls.grad))) + 2e-5
    wrong = ST.pair_loss_and_grads(None, 0, 1, visual.cuda(), text.cuda(), visual.cuda(), text.cuda(), SCALE,
                                   sim_teacher="x", sim_thres=THRES)[0]
    assert abs(float(wrong) - float(loss)) > 1e-2
    with pytest.raises(ValueError):
        ST.pair_loss_and_grads(None, 0, 1, visual.cuda(), text.cuda(), visual.cuda(), text.cuda(), SCALE, sim_teacher="text", sim_thres=0.8)
    with pytest.raises(ValueError):
        ST.pair_loss_and_grads(None, 0, 1, visual.cuda(), text.cuda(), visual.cuda(), text.cuda(), SCALE, sim_teacher="y")


# ---- step level -------------------------------------------------------------------------------------------------------------
def _tiny_audio():
    from vitlens_hip import engine as E
    sd, ins, outs, grads, meta = split(load_npz("tiny_audio.npz"))
    tower, text, lens = specs_from_meta(meta)
    tc = E.TowerCfg(width=tower.width, layers=tower.layers, heads=tower.heads, patch=tower.patch,
                    image_size=tower.image_size, embed_dim=tower.embed_dim)
    xc = E.TextCfg(context_length=text.context_length, vocab_size=text.vocab_size, width=text.width, heads=text.heads,
                   layers=text.layers, embed_dim=text.embed_dim)
    lc = E.LensCfg(**{k: getattr(lens, k) for k in E.LensCfg.__dataclass_fields__ if hasattr(lens, k)})
    txt = ins["text"].clone()
    txt[1] = txt[0]; txt[3] = txt[2]              # captions 0 = 1 and 2 = 3: text similarity 1.0 inside a pair, 0.63 across
    return sd, ins["visual_x"], txt, (tower, text, lens), (tc, xc, lc)


def test_dual_audio_step_sim_mask_vs_the_oracle_step():
    """One `DualAudioStep` step with contra_loss_type="sim_mask" (text = teacher, duplicated captions in the batch) against
    the oracle's dual step - its towers, torch autograd, the loss of simmask_ref, AdamW's first step written out.
      * loss: 3e-2, the bound of test_hip_train.test_dual_audio_step_runs_and_matches_reference_loss on this fixture;
      * updated parameters: AdamW's first step moves an element by lr * g / (|g| + eps) ~ lr * sign(g) (plus the same decay on
        both sides), so two updates differ by more than lr only where the gradient's sign differs, and there the
        gradient's error is at least |g_ref|: the elements whose update differs by more than lr carry at most (6e-2)^2 of
        the reference gradient's energy per tensor, 6e-2 being the suite's bound on this fixture's gradients
        (test_audio_lens_backward_vs_reference_grads); no element differs by more than 2 lr."""
    import vitlens_oracle as O
    from vitlens_hip import step as ST
    from vitlens_hip.train import AdamW
    sd, audio, txt, (tower, text, lens), (tc, xc, lc) = _tiny_audio()
    lr, eps, wd = 1e-3, 1e-6, 0.2
    st = ST.DualAudioStep(sd, tc, xc, lc, "cuda", micro_batch=2, lr=lr, eps=eps, weight_decay=wd, contra_loss_type="sim_mask",
                          sim_thres=THRES)
    decays = {}
    for name, m in st.masters.items():
        for k in ST._master_to_sd(name, m.detach(), st._base_sd, st.lens.lens):
            decays[k] = AdamW.decays(name, m)
    # the oracle's step
    ref_sd = {k: v.clone() for k, v in sd.items()}
    for k in decays:
        ref_sd[k] = sd[k].detach().float().clone().requires_grad_(True)
    ft = O.encode_text(ref_sd, txt, text, normalize=True)
    fv = O.encode_visual(ref_sd, audio, tower, lens, normalize=True)
    sim = ft.detach().double() @ ft.detach().double().t()
    offd = ~torch.eye(4, dtype=torch.bool)
    assert float((sim - THRES).abs()[offd].min()) > 1e-3 and int(((sim >= THRES) & offd).sum()) == 4
    ref_loss = SR.loss_world1(ft, fv, ref_sd["logit_scale"].exp(), THRES)
    ref_loss.backward()
    plain = float(O.clip_loss(ft.detach(), fv.detach(), ref_sd["logit_scale"].detach().exp()))
    assert abs(plain - float(ref_loss)) > 0.1                        # 10 x the bound below: the masked loss is another number
    loss = st.forward_backward(audio.cuda(), txt.cuda())
    print("loss", float(loss), float(ref_loss), "general", plain)
    assert abs(float(loss) - float(ref_loss)) < 3e-2, (float(loss), float(ref_loss))
    st.optimizer_step()
    got = st.state_dict()
    n = 0
    for k, dec in decays.items():
        p, g = ref_sd[k].detach(), ref_sd[k].grad
        assert g is not None, k
        want = p * (1.0 - lr * wd * float(dec)) - lr * g / (g.abs() + eps)
        diff = (got[k].float().cpu().reshape(want.shape) - want).abs()
        flipped = diff > lr
        energy = float((g[flipped] ** 2).sum()) / max(float((g ** 2).sum()), 1e-30)
        print(k, "max diff / lr", float(diff.max()) / lr, "flipped", int(flipped.sum()), "of", g.numel(), "energy", energy)
        assert float(diff.max()) <= 2 * lr * 1.001 + 1e-7, (k, float(diff.max()))
        assert energy <= 6e-2 ** 2, (k, energy)
        assert float((got[k].float().cpu().reshape(want.shape) - p).abs().max()) > 0, k          # it moved
        n += 1
    assert n >= 40, n


def test_dual_audio_step_general_is_the_step_without_the_argument():
    from vitlens_hip import step as ST
    sd, audio, txt, _, (tc, xc, lc) = _tiny_audio()
    runs = []
    for kw in ({}, dict(contra_loss_type="general", sim_thres=0.3)):
        st = ST.DualAudioStep(sd, tc, xc, lc, "cuda", micro_batch=2, lr=1e-3, **kw)
        l1 = st.forward_backward(audio.cuda(), txt.cuda())
        grads = {k: v.clone() for k, v in st.grads.items()}
        st.optimizer_step()
        l2 = st.step(audio.cuda(), txt.cuda())
        torch.cuda.synchronize()
        runs.append((l1, l2, grads, {k: v.clone() for k, v in st.masters.items()}))
    a, b = runs
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    for k in a[2]:
        assert torch.equal(a[2][k], b[2][k]), k
    for k in a[3]:
        assert torch.equal(a[3][k], b[3][k]), k
    with pytest.raises(NotImplementedError):
        ST.DualAudioStep(sd, tc, xc, lc, "cuda", micro_batch=2, contra_loss_type="label_mask")
