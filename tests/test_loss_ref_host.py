"""CPU: tests/loss_ref.py before any kernel is held to it.

  * the float64 references are pinned to float64 autograd of F.cross_entropy over rows and columns (square and --local-loss
    geometry), to simmask_ref.pair_loss with an all-ones mask, and to autograd of F.normalize, at 1e-12;
  * every input family is finite at every shape, and the float32 models of the kernels stay inside the derived bounds there
    (the worst ratio of every family is printed);
  * three planted arithmetic errors in the MODELS each exceed a bound, by a printed margin, and each is also run against the
    tolerances test_infonce_pieces has, at its four shapes;
  * every branch condition the GPU test's table names is met by at least one of its cases;
  * the figures the GPU test's 2 x model tolerances are twice of are recomputed here."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import loss_ref as LR
import simmask_ref as SR

F64 = torch.float64


def _t(a):
    return torch.from_numpy(np.asarray(a)).double()


def _ratio(err, bound):
    """Worst error / bound; a non-finite error counts as infinitely far out."""
    err = torch.as_tensor(err, dtype=F64)
    r = err / torch.as_tensor(bound, dtype=F64)
    return float("inf") if not bool(torch.isfinite(err).all()) else float(r.max())


# ---- the references -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R,C,off,w_col", [(70, 70, 0, 0.5), (48, 144, 96, 0.0), (48, 144, 96, 0.5), (5, 65, 0, 0.5)])
def test_references_are_float64_cross_entropy_and_its_autograd(R, C, off, w_col):
    t, s = SR.clustered(C, 1000 + C)
    x, y, scale = t[off:off + R].double(), s.double(), 14.2857
    sc = torch.tensor(scale, dtype=F64, requires_grad=True)
    A = (x @ y.t()).requires_grad_(True)
    lg = sc * A
    lab = torch.arange(R) + off
    want = 0.5 * F.cross_entropy(lg, lab)
    if w_col:
        want = want + w_col * F.cross_entropy(lg.t()[off:off + R], torch.arange(R))
    dA, dsc = torch.autograd.grad(want, (A, sc))
    want = want.detach()
    l = lg.detach()
    assert abs(float(LR.loss(l, off, 0.5, w_col)) - float(want)) < 1e-12
    ones = torch.ones(R, C, dtype=torch.bool)
    assert abs(float(LR.loss(l, off, 0.5, w_col, keep=ones)) - float(want)) < 1e-12
    assert abs(float(SR.pair_loss(x, y, scale, ones, off, 0.5, w_col)) - float(want)) < 1e-12
    G = LR.grad(l, off, 0.5, w_col)
    assert float((G * scale - dA).abs().max()) < 1e-12                   # dL/dA = scale dL/dlogits
    assert float((LR.grad(l, off, 0.5, w_col, keep=ones) - G).abs().max()) == 0.0
    assert abs(LR.dscale(G, l, scale) - float(dsc)) < 1e-12
    assert float((LR.row_lse(l) - torch.logsumexp(l, 1)).abs().max()) == 0.0
    assert float((LR.diag(l, off) - l[torch.arange(R), lab]).abs().max()) == 0.0
    st = LR.loss_from_stats(LR.row_lse(l), LR.col_lse(l) if w_col else None, LR.diag(l, off), R, C, off, 0.5, w_col)
    assert abs(float(st) - float(want)) < 1e-12


def test_masked_reference_is_simmask_pair_loss():
    R, C, off = 48, 144, 96
    t, s = SR.clustered(C, 1000 + C)
    x, y = t[off:off + R].double(), s.double()
    keep = SR.keep_mask(x, t, 0.8, off)
    assert 0 < int((~keep).sum())
    lg = 14.2857 * x @ y.t()
    want = SR.pair_loss(x, y, 14.2857, keep, off, 0.5, 0.5)
    assert abs(float(LR.loss(lg, off, 0.5, 0.5, keep=keep)) - float(want)) < 1e-12
    A = lg.clone().requires_grad_(True)
    (dA,) = torch.autograd.grad(SR.pair_loss(A, torch.eye(C, dtype=F64), 1.0, keep, off, 0.5, 0.5), A)
    assert float((LR.grad(lg, off, 0.5, 0.5, keep=keep) - dA).abs().max()) < 1e-12


def test_l2norm_bwd_reference_is_autograd_of_normalize():
    g = torch.Generator().manual_seed(3)
    x = torch.randn(5, 65, generator=g, dtype=F64)
    x[2] *= 1e-14                                                        # norm below eps: normalize divides by eps
    df = torch.randn(5, 65, generator=g, dtype=F64)
    xr = x.clone().requires_grad_(True)
    f = F.normalize(xr, dim=-1)
    (want,) = torch.autograd.grad((f * df).sum(), xr)
    got = LR.l2norm_bwd(f.detach(), df, x.norm(dim=-1))
    # the kernel's formula drops the derivative of max(norm, eps) in the eps branch, as F.normalize's backward does not: row 2
    # is compared with df / eps - f <f, df> / eps, which is what the formula says
    ok = torch.tensor([0, 1, 3, 4])
    assert float(((got - want)[ok].abs() / want[ok].abs().max()).max()) < 1e-12
    fd = f.detach()[2]
    assert float((got[2] - (df[2] - fd * (fd * df[2]).sum()) / 1e-12).abs().max()) == 0.0


def test_split_reference_bits_are_round_to_nearest_even():
    g = torch.Generator().manual_seed(4)
    x = torch.randn(37, 63, generator=g) * torch.logspace(-6, 6, 63)
    x[0, :4] = torch.tensor([1.00390625, 1.01171875, -1.00390625, 0.0])         # ties: to even, both directions
    def rne(v):
        b = v.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
        return (((b + 0x7FFF + ((b >> 16) & 1)) >> 16) & 0xFFFF).to(torch.int32)
    hi = rne(x)
    hif = (hi.to(torch.int64) << 16).to(torch.int32).view(torch.float32)
    lo = rne(x - hif)
    for pattern, parts in ((0, (hi, lo, hi)), (1, (hi, hi, lo))):
        got = LR.split_bf16x3(x, pattern).view(torch.int16).to(torch.int32) & 0xFFFF
        assert torch.equal(got, torch.cat(parts, dim=1))
    out = LR.split_bf16x3(x, 0).double()
    resid = (x.double() - out[:, :63] - out[:, 63:126]).abs()
    assert bool((resid <= 2.0 ** -17 * x.double().abs()).all())
    tr = LR.transpose_bf16(x, 40)
    assert torch.equal(tr[:, :37], x.t().bfloat16()) and float(tr[:, 37:].abs().max()) == 0.0


# ---- the models against the bounds, on every family at every shape ---------------------------------------------------------------
def model_ratios(family, R, C, off, guard=True, col_hot=True, drop=None):
    """{kernel: worst |model - reference| / bound} of one case, exactly as the GPU test forms the ratios of the kernels."""
    lg = LR.make_logits(family, R, C, off)
    assert bool(torch.isfinite(lg).all())
    rl, cl, dg = LR.row_lse(lg), LR.col_lse(lg), LR.diag(lg, off)
    assert bool(torch.isfinite(rl).all() and torch.isfinite(cl).all())
    out = {"row_lse": _ratio((_t(LR.row_lse_model(lg, guard=guard)) - rl).abs(), LR.lse_bound(lg, 1)),
           "col_lse": _ratio((_t(LR.col_lse_model(lg)) - cl).abs(), LR.lse_bound(lg, 0))}
    rl32, cl32 = rl.float(), LR.label_columns_only(cl, off, R).float()
    G = LR.grad(lg, off, 0.5, 0.5)
    delta, bound = LR.grad_bound(lg, off, rl32, cl32, 0.5, 0.5)
    gm = LR.grad_model(lg, off, rl32, cl32, 0.5, 0.5, col_hot=col_hot)
    out["g_f32"] = _ratio((_t(gm) - G).abs(), delta + 1e-300)
    out["G"] = _ratio((torch.from_numpy(gm).bfloat16().double() - G).abs(), bound)
    ldg, ldgt = (C + 63) // 64 * 64, (R + 63) // 64 * 64
    blocks = math.prod(LR.grad_grid(R, C, ldg, ldgt))
    want = 3.5 + LR.dscale(G, lg, 14.2857)
    ds = LR.dscale_model(gm, lg, 14.2857, 3.5, ldg, ldgt, drop=drop)
    out["dscale"] = _ratio(abs(float(ds) - want), LR.dscale_bound(G, lg, delta, 14.2857, 3.5, blocks))
    red = LR.ce_reduce_model(rl32, cl32, dg.float(), R, C, off, 0.5, 0.5, -2.75)
    want = -2.75 + float(LR.loss_from_stats(rl32, cl32, dg.float(), R, C, off, 0.5, 0.5))
    out["ce_reduce"] = _ratio(abs(float(red) - want), LR.ce_reduce_bound(rl32, cl32, dg.float(), R, C, off, 0.5, 0.5, -2.75))
    return out


@pytest.mark.parametrize("family", LR.FAMILIES)
def test_float32_models_stay_inside_the_bounds(family):
    worst = {}
    for R, C, off in LR.SHAPES:
        for k, v in model_ratios(family, R, C, off).items():
            if v > worst.get(k, (-1.0, None))[0]:
                worst[k] = (v, (R, C, off))
    for k, (v, shape) in worst.items():
        print(f"MODEL {family:10s} {k:9s} worst error / bound {v:.3f} at {shape}")
    assert all(v <= 1.0 for v, _ in worst.values()), worst


def test_sink_rows_sum_to_exactly_one_and_flat_rows_to_log_c():
    for fam in ("sink_first", "sink_last"):
        lg = LR.make_logits(fam, 65, 257)
        assert bool((torch.from_numpy(LR.row_lse_model(lg)) == 90.0).all())
    lg = LR.make_logits("flat", 130, 300)
    assert float((LR.row_lse(lg) - (3.25 + math.log(300))).abs().max()) < 1e-12


# ---- planted errors ----------------------------------------------------------------------------------------------------------
OLD_SHAPES = [(64, 64, 0), (100, 100, 0), (48, 192, 96), (1024, 1024, 0)]        # test_infonce_pieces


def _old_test_sees(R, C, off, guard=True, col_hot=True, drop=None):
    """test_infonce_pieces' own assertions (randn * 4 logits, fp32 autograd reference, loss 1e-4, G 5e-3 whole-tensor norm,
    dscale 1e-3) applied to the MODEL with a planted error; returns the names of the assertions that fail."""
    lg = (torch.randn(R, C, generator=torch.Generator().manual_seed(26)) * 4)
    square = R == C
    rl = torch.from_numpy(LR.row_lse_model(lg, guard=guard))
    cl = torch.from_numpy(LR.col_lse_model(lg)) if square else None
    dg = LR.diag(lg, off).float()
    l = lg.clone().requires_grad_(True)
    lab = torch.arange(R) + off
    ref = F.cross_entropy(l, lab) * 0.5
    if square:
        ref = ref + F.cross_entropy(l.t(), lab) * 0.5
    ref.backward()
    ref = ref.detach()
    failed = []
    loss = float(LR.ce_reduce_model(rl, cl, dg, R, C, off, 0.5, 0.5, 0.0))
    if not abs(loss - float(ref)) < 1e-4:
        failed.append("loss")
    gm = LR.grad_model(lg, off, rl, cl, 0.5, 0.5, col_hot=col_hot)
    G = torch.from_numpy(gm).bfloat16().float()
    if not float((G - l.grad).norm() / l.grad.norm()) < 5e-3:
        failed.append("G")
    ds = float(LR.dscale_model(gm, lg, 2.0, 0.0, (C + 63) // 64 * 64, (R + 63) // 64 * 64, drop=drop))
    ds_ref = float((l.grad * l.detach()).sum() / 2.0)
    if not abs(ds - ds_ref) < 1e-3 * max(1.0, abs(ds_ref)):
        failed.append("dscale")
    return failed


def test_planted_errors_exceed_the_bounds():
    """Three arithmetic changes to the models.  Each exceeds a derived bound on a case of the GPU test; which of them the old
    tolerances of test_infonce_pieces see, at its own four shapes:
      * butterfly without the -inf guards: NaN wherever two idle lanes meet (C < 32).  The old test never sees it: none of its
        shapes has C < 64, and with every lane busy the guards change no bit.
      * column term without its one-hot: every diagonal element of G is off by w_col / R.  The old test DOES see this one where it
        has a column term (its three square shapes, in G and in dscale): the diagonal carries most of G's norm.
      * one wave's partial of one (off-diagonal) block dropped from d/dscale: the old 1e-3 max(1, |ref|) sees it where a block is a large share
        of the matrix (64 x 64 is four blocks) and not at 1024 x 1024, where it is one of 1024 - the size at which the new
        bound, proportional to sum |g l|, is exceeded 178 times over."""
    assert all(v <= 1.0 for v in model_ratios("normal", 3, 5, 0).values())
    r = model_ratios("normal", 3, 5, 0, guard=False)["row_lse"]
    print(f"PLANTED unguarded -inf lane: row_lse error / bound = {r} at (3, 5) (NaN: 0 * exp(-inf + inf))")
    assert r > 1.0
    r = model_ratios("scale100", 130, 300, 0, col_hot=False)
    print(f"PLANTED column term without hot: G error / bound = {r['G']:.3e}, fp32 g error / delta = {r['g_f32']:.3e} at (130, 300)")
    assert r["G"] > 1.0 and r["g_f32"] > 1.0
    r = model_ratios("normal", 1040, 1040, 0, drop=(1, 3))["dscale"]
    print(f"PLANTED one wave's partial of block 1 dropped: dscale error / bound = {r:.3e} at (1040, 1040), 1 of 1156 blocks")
    assert r > 1.0
    seen = {}
    for R, C, off in OLD_SHAPES:
        assert _old_test_sees(R, C, off) == []
        seen[(R, C)] = {"guard": _old_test_sees(R, C, off, guard=False), "hot": _old_test_sees(R, C, off, col_hot=False),
                        "wave": _old_test_sees(R, C, off, drop=(1, 3))}
        print(f"PLANTED what test_infonce_pieces' tolerances see at ({R}, {C}): {seen[(R, C)]}")
    assert all(v["guard"] == [] for v in seen.values())
    assert all(v["hot"] == (["G", "dscale"] if R == C else []) for (R, C), v in seen.items())
    assert seen[(1024, 1024)]["wave"] == [] and seen[(64, 64)]["wave"] == ["dscale"]


# ---- coverage of the branch table ------------------------------------------------------------------------------------------------
def test_every_branch_condition_is_met_by_a_case():
    for cond, cases in LR.branch_conditions().items():
        print(f"BRANCH {cond}: {cases}")
        assert cases, cond
    for R, C, ldo, pad, shift, kernel in LR.TRANSPOSE_CASES:                  # the dispatch the table claims, for both dtypes
        for esize in (4, 2):
            assert ldo >= R
            assert LR.transpose_kernel(R, C, ldo, C + pad, shift * 4, 0) == kernel, (R, C, ldo, pad, shift, esize)
    for R, C, ldo in LR.COLSUM_CASES:
        assert LR.transpose_kernel(R, C, ldo, C + 8, 0, 0) == "tile64" and ldo >= R
    assert sorted((c[2] + 255) // 256 for c in LR.COLSUM_CASES) == [1, 8, 9, 11]
    assert set(LR.L2_DIMS) == {1, 63, 64, 65, 768} and set(LR.L2_ROWS) == {1, 4, 5, 9}


# ---- the figures behind the GPU test's 2 x model tolerances -----------------------------------------------------------------------
def test_feature_gradient_model_figures_are_the_ones_the_gpu_test_doubles():
    import test_hip_loss_kernels as T
    for R, C, off, w_col, chunk in LR.PAIR_CASES:
        x, y = T.pair_inputs(R, C, off)
        assert x.shape == (R, 64) and y.shape == (C, 64)
        for scale in (100.0, 14.2857):
            G = LR.grad(scale * x.double() @ y.double().t(), off, 0.5, w_col)
            dx, dy = scale * G @ y.double(), scale * G.t() @ x.double()
            mx, my = LR.dxdy_model(x, y, scale, off, 0.5, w_col)
            ex, ey = LR.worst_row(mx, dx), LR.worst_row(my, dy)
            px, py = T.MODEL_DXDY[(R, C, off, scale)]
            print(f"MODEL dx / dy worst row ({R}, {C}, {off}) scale {scale}: {ex:.3e} / {ey:.3e}   (pinned {px:.3e} / {py:.3e})")
            assert abs(ex / px - 1) < 0.01 and abs(ey / py - 1) < 0.01
