"""GPU: every kernel of csrc/vl_loss.hip against the float64 references of tests/loss_ref.py, element by element, up to logit
scale 100 - through ops.* on synthetic fp32 logits, and through step.pair_forward / pair_backward on clustered features.

Every check prints `MEASURED kernel | case | worst error / bound` before it asserts (1.000 = at the bound); the bounds are
loss_ref's, derived there and checked against float32 models of the kernels on the CPU (tests/test_loss_ref_host.py) - none
comes from what a kernel returns.  The logits are a [:, :C] view of a wider NaN-filled buffer; every output is written inside
a larger NaN-filled allocation whose surplus is compared bit for bit afterwards (outputs an ops.* entry allocates itself are
produced a second time through the C ABI into such an allocation and must be bit-equal to what ops.* returned, which is also
the second, bit-identical launch every case asks for).  Logits are finite throughout: a row of -inf only has no log-sum-exp
and is outside the kernels' domain.

Kernel branch -> covering case (loss_ref.branch_conditions lists them; the host test asserts each is non-empty):

  row_lse_kernel      idle lanes, both -inf guards of the butterfly     C = 1, 5, 63
                      a lane with a second element / many               C = 65 / 257, 300, 1040
                      a block with idle waves (R % 4 != 0)              R = 1, 3, 5, 65, 130, 257
                      every element a new maximum (a rescale per step)  ramp; none after the first: descend
                      diag = 0 for a label outside the columns          test_ce_stats_labels_outside_the_columns
  col_part_kernel     a ragged last 64-row chunk                        R = 65, 130, 257, 1040;  one chunk: R <= 64
                      a second 256-column block                         C = 257, 300, 1040
  col_comb_kernel     1, 2, 3, 5, 17 chunks                             R = 64, 65, 130, 257, 1040
  ce_reduce_kernel    R < 256, = 256, > 256; either term absent         test_ce_loss_accum
                      a label outside the columns is skipped            test_ce_loss_accum[5-...] (off = 3, C = 6)
  grad_kernel         G and GT, G only, GT only, each with d/dscale     test_ce_grad (all three in every case)
                      pad columns [C, ldg) / [R, ldgt) zero-filled      every shape but 64 x 64
                      +inf column statistics: the term is exactly 0     (130, 300), (48, 144, *); test_ce_grad_variants
                      row term absent / column term absent              test_ce_grad_variants
  part_finalize_kernel  more than 1024 partials (a second sweep)        1040 x 1040: 34 x 34 blocks, 34 x 33 for G / GT only
  l2norm_bwd_kernel   D < 64, = 64, > 64, 768; idle waves; norm < eps   test_l2_normalize_bwd
  split3_kernel       both patterns, odd D, past the first grid sweep   test_split_bf16x3
  transpose_bf16_kernel / transpose64_kernel, f32 and bf16 sources      test_transpose_to_bf16 (loss_ref.TRANSPOSE_CASES)
                      r0 >= ldo break; a partly stored 64-row tile      (300, 64, ldo 320); (300, 128, ldo 304)
  colws_finalize_kernel  nslab = 1, 8, 9, 11 (no full group; no tail; tail of 1 and of 3)      test_transpose_colsum

Measured on the MI355X (profiles/loss_kernels_ratios.txt has the table per kernel, family and shape): 271 cases in 4.1 s; worst
error / bound: row_lse 0.473, col_lse 0.570, G / GT 0.999 (the bf16 half ulp, reached), dscale 0.224, ce_loss_accum 0.106,
l2norm_bwd 0.617, split 0.998 (of 2^-17 |x|), colsum 0.018; pair loss and dscale below 0.01 of their worst-case tolerances."""
import functools
import math

import pytest
import torch

import errloc
import loss_ref as LR
import simmask_ref as SR
from test_hip_rows import bits, poisoned, still_poisoned

pytestmark = pytest.mark.gpu

F32, BF16, F64 = torch.float32, torch.bfloat16, torch.float64
GUARD = 64                      # poisoned elements (or rows) on either side of every output
W_ROW = W_COL = 0.5
SCALE = 14.2857                 # 1 / scale is inexact in fp32
DS_IN, LOSS_IN = 3.5, -2.75     # what the accumulators hold on entry

# ---- 2 x model tolerances: feature gradients of the pair level, per row ----------------------------------------------------------
# The model (loss_ref.dxdy_model, float64 with G and the transposed operand rounded to bf16 - what the two NT GEMMs consume) is
# this far from the exact gradients in its worst row; test_loss_ref_host.py recomputes the figures.  The factor 2 pays for what
# the model leaves out: G is rounded from an fp32 g that was formed from bf16x3 logits and fp32 statistics, the GEMM accumulates
# in fp32, and the row-blocked path rounds G after the block's re-weighting.  Measured on the MI355X beside each pair: the kernels
# reproduce the model to three digits (0.500 of the tolerance everywhere), the device log-scale runs (ln 100) included.
#             (R,   C, off, scale): (dx, dy)                                    measured on the MI355X, worst row (dx, dy)
MODEL_DXDY = {(70, 70, 0, 100.0): (3.347e-03, 4.826e-03),                     # 3.347e-03, 4.826e-03
              (70, 70, 0, 14.2857): (3.411e-03, 6.487e-03),                   # 3.411e-03, 6.487e-03
              (130, 300, 0, 100.0): (2.469e-03, 4.141e-03),                   # 2.469e-03, 4.141e-03
              (130, 300, 0, 14.2857): (3.040e-03, 3.569e-03),                 # 3.037e-03, 3.569e-03
              (48, 144, 96, 100.0): (3.292e-03, 3.035e-03),                   # 3.292e-03, 3.035e-03
              (48, 144, 96, 14.2857): (3.568e-03, 3.599e-03),                 # 3.568e-03, 3.599e-03
              (200, 200, 0, 100.0): (3.400e-03, 5.042e-03),                   # 3.400e-03, 5.042e-03 (row-blocked, chunk 64)
              (200, 200, 0, 14.2857): (4.213e-03, 5.919e-03)}                 # 4.213e-03, 5.919e-03 (row-blocked, chunk 64)


def _ops():
    from vitlens_hip import ops
    return ops


def measured(kernel, case, err, bound):
    """Worst error / bound over the elements; printed, then asserted <= 1 (a NaN fails)."""
    err, bound = torch.as_tensor(err, dtype=F64).cpu(), torch.as_tensor(bound, dtype=F64).cpu()
    r = float((err / bound).max()) if bool(torch.isfinite(err).all()) else float("nan")
    print(f"MEASURED {kernel} | {case} | " + (f"{r:.3f}" if r >= 1e-3 or r == 0 else f"{r:.1e}"))
    assert r <= 1.0, f"{kernel} {case}: worst error / bound = {r}"
    return r


def guarded(n, dtype=F32):
    """(buffer, view of n elements) with GUARD poisoned elements on either side."""
    buf = poisoned(n + 2 * GUARD, dtype=dtype)
    return buf, buf[GUARD:GUARD + n]


def guards_intact(buf, n, what):
    still_poisoned(buf[:GUARD], what + ": before"); still_poisoned(buf[GUARD + n:], what + ": behind")


def embed(t, pad=5, shift=0):
    """t [R, C] (CPU) as a view of a NaN-filled device buffer: row stride C + pad, a poisoned row before and behind, the view
    starting 4 * shift bytes into its row (shift = 0: 16-byte aligned whenever the row stride is)."""
    R, C = t.shape
    ld, skip = C + pad, shift * 4 // t.element_size()
    buf = poisoned((R + 2) * ld + skip, dtype=t.dtype)
    v = buf[ld + skip:ld + skip + R * ld].view(R, ld)[:, :C]
    v.copy_(t)
    return v


def same_bits(a, b):
    return a.shape == b.shape and bool((bits(a.contiguous()) == bits(b.contiguous())).all())


# ---- references, computed once per case and never mutated ------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def stats_case(family, R, C, off):
    lg = LR.make_logits(family, R, C, off)
    return dict(lg=lg, rl=LR.row_lse(lg), cl=LR.col_lse(lg), dg=LR.diag(lg, off), rb=LR.lse_bound(lg, 1), cb=LR.lse_bound(lg, 0))


@functools.lru_cache(maxsize=None)
def grad_case(family, R, C, off, w_row=W_ROW, w_col=W_COL, label_cols_only=True):
    """The statistics the kernel is GIVEN (the reference's, rounded to fp32; +inf outside the label columns) and G against them."""
    s = stats_case(family, R, C, off)
    rl32 = s["rl"].float() if w_row else None
    cl = LR.label_columns_only(s["cl"], off, R) if label_cols_only else s["cl"]
    cl32 = cl.float() if w_col else None
    G = LR.grad(s["lg"], off, w_row, w_col, label_cols_only=label_cols_only)
    delta, bound = LR.grad_bound(s["lg"], off, rl32, cl32, w_row, w_col)
    return dict(rl32=rl32, cl32=cl32, G=G, delta=delta, bound=bound)


def abi_stats(ops, lgv, off):
    """vl_ce_stats into guarded outputs (and a guarded workspace)."""
    from vitlens_hip._lib import check
    R, C = lgv.shape
    nws = 2 * ((R + 63) // 64) * C
    (rb, rl), (cb, cl), (db, dg), (wb, ws) = guarded(R), guarded(C), guarded(R), guarded(nws)
    check(ops._lib.vl_ce_stats(ops._p(lgv), lgv.stride(0), R, C, off, ops._p(rl), ops._p(cl), ops._p(dg), ops._p(ws), ops._stream()))
    torch.cuda.synchronize()
    for buf, n, what in ((rb, R, "row_lse"), (cb, C, "col_lse"), (db, R, "diag"), (wb, nws, "workspace")):
        guards_intact(buf, n, what)
    return rl, cl, dg


def abi_grad(ops, lgv, off, rl, cl, w_row, w_col, scale, ds_in):
    """vl_ce_grad (G and GT) into guarded outputs: G [R, ldg] and GT [C, ldgt] own their pad columns."""
    from vitlens_hip._lib import check
    R, C = lgv.shape
    ldg, ldgt = (C + 63) // 64 * 64, (R + 63) // 64 * 64
    nws = int(ops._lib.vl_ce_grad_ws_floats(R, C, ldg, ldgt))
    assert nws == math.prod(LR.grad_grid(R, C, ldg, ldgt))
    (gb, G), (tb, GT), (wb, ws), (sb, ds) = guarded(R * ldg, BF16), guarded(C * ldgt, BF16), guarded(nws), guarded(1)
    ds.fill_(ds_in)
    check(ops._lib.vl_ce_grad(ops._p(lgv), lgv.stride(0), R, C, off, ops._p(rl), ops._p(cl), float(w_row), float(w_col), ops._p(G), ldg,
                              ops._p(GT), ldgt, float(scale), ops._p(ds), ops._p(ws), ops._stream()))
    torch.cuda.synchronize()
    for buf, n, what in ((gb, R * ldg, "G"), (tb, C * ldgt, "GT"), (wb, nws, "workspace"), (sb, 1, "dscale")):
        guards_intact(buf, n, what)
    return G.view(R, ldg), GT.view(C, ldgt), ds


# ---- row / column statistics -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R,C,off", LR.SHAPES)
@pytest.mark.parametrize("family", LR.FAMILIES)
def test_ce_stats(family, R, C, off):
    ops = _ops()
    s = stats_case(family, R, C, off)
    lgv = embed(s["lg"])
    case = f"{family} {R}x{C}+{off}"
    rl, cl, dg = ops.ce_stats(lgv, off, want_cols=True)
    measured("row_lse", case, (rl.cpu().double() - s["rl"]).abs(), s["rb"])
    measured("col_lse", case, (cl.cpu().double() - s["cl"]).abs(), s["cb"])
    assert same_bits(dg.cpu(), s["dg"].float()), "diag is not the logits' diagonal bit for bit"
    rl2, cl2, dg2 = abi_stats(ops, lgv, off)
    assert same_bits(rl, rl2) and same_bits(cl, cl2) and same_bits(dg, dg2), "a second launch differs"
    rl3, none, dg3 = ops.ce_stats(lgv, off, want_cols=False)
    assert none is None and same_bits(rl, rl3) and same_bits(dg, dg3)


def test_ce_stats_labels_outside_the_columns():
    """label_off past the last column for some rows: diag is 0 there (and the statistics do not care)."""
    ops = _ops()
    lg = LR.make_logits("normal", 5, 6, 3)
    rl, cl, dg = ops.ce_stats(embed(lg), 3)
    want = LR.diag(lg, 3)
    assert bool((want[3:] == 0).all()) and bool((want[:3] != 0).all())
    assert same_bits(dg.cpu(), want.float())
    measured("row_lse", "normal 5x6+3", (rl.cpu().double() - LR.row_lse(lg)).abs(), LR.lse_bound(lg, 1))


# ---- the loss reduction ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("terms", ["both", "rows", "cols"])
@pytest.mark.parametrize("R,C,off", [(5, 6, 3)] + [(r, r + 7, 3) for r in LR.CE_REDUCE_ROWS[1:]])
def test_ce_loss_accum(R, C, off, terms):
    """ce_reduce_kernel from GIVEN fp32 statistics (the reference's, rounded), into an accumulator that holds LOSS_IN, against
    the float64 reduction of the same fp32 values."""
    ops = _ops()
    s = stats_case("normal", R, C, off)
    rl32, cl32, dg32 = s["rl"].float(), s["cl"].float(), s["dg"].float()
    rl = None if terms == "cols" else rl32
    cl = None if terms == "rows" else cl32
    want = LOSS_IN + float(LR.loss_from_stats(rl, cl, dg32, R, C, off, 0.5, 0.25))
    bound = LR.ce_reduce_bound(rl, cl, dg32, R, C, off, 0.5, 0.25, LOSS_IN)
    got = []
    for _ in range(2):
        buf, loss = guarded(1)
        loss.fill_(LOSS_IN)
        ops.ce_loss_accum(loss, None if rl is None else rl.cuda(), None if cl is None else cl.cuda(), dg32.cuda(), R, C, off, 0.5, 0.25)
        torch.cuda.synchronize()
        guards_intact(buf, 1, "loss")
        got.append(loss.clone())
    measured("ce_loss_accum", f"{terms} {R}x{C}+{off}", abs(float(got[0]) - want), bound)
    assert same_bits(got[0], got[1])


# ---- dL/dlogits and d/dscale -----------------------------------------------------------------------------------------------------
def check_grad(ops, case, lgv, lg, off, c, w_row, w_col, mode, scale=SCALE):
    """One launch of ops.ce_grad in `mode` against the case's references; returns (G, GT, dscale)."""
    R, C = lg.shape
    need_g, need_gt = mode != "gt_only", mode != "g_only"
    ldg, ldgt = (C + 63) // 64 * 64, (R + 63) // 64 * 64
    rl = None if c["rl32"] is None else c["rl32"].cuda()
    cl = None if c["cl32"] is None else c["cl32"].cuda()
    buf, ds = guarded(1)
    ds.fill_(DS_IN)
    G, GT = ops.ce_grad(lgv, rl, cl, off, w_row, w_col, scale, ds, need_g=need_g, need_gt=need_gt)
    torch.cuda.synchronize()
    guards_intact(buf, 1, "dscale")
    assert (G is None) == (not need_g) and (GT is None) == (not need_gt)
    zero = torch.zeros((), dtype=torch.int16, device="cuda")
    if need_g:
        assert G.shape == (R, ldg)
        measured("G", f"{case} {mode}", (G[:, :C].cpu().double() - c["G"]).abs(), c["bound"])
        assert bool((bits(G[:, C:].contiguous()) == zero).all()), "pad columns of G are not +0"
    if need_gt:
        assert GT.shape == (C, ldgt)
        measured("GT", f"{case} {mode}", (GT[:, :R].cpu().double() - c["G"].t()).abs(), c["bound"].t())
        assert bool((bits(GT[:, R:].contiguous()) == zero).all()), "pad columns of GT are not +0"
    blocks = math.prod(LR.grad_grid(R, C, ldg, ldgt, need_g, need_gt))
    want = DS_IN + LR.dscale(c["G"], lg, scale)
    measured("dscale", f"{case} {mode}", abs(float(ds) - want), LR.dscale_bound(c["G"], lg, c["delta"], scale, DS_IN, blocks))
    return G, GT, ds.clone()


@pytest.mark.parametrize("R,C,off", LR.SHAPES)
@pytest.mark.parametrize("family", LR.FAMILIES)
def test_ce_grad(family, R, C, off):
    """G, GT and d/dscale from the reference's statistics rounded to fp32 (+inf outside the label columns, as
    step._label_columns_only leaves them), in all three launch modes; the statistics kernels have test_ce_stats."""
    ops = _ops()
    lg = stats_case(family, R, C, off)["lg"]
    c = grad_case(family, R, C, off)
    lgv = embed(lg)
    case = f"{family} {R}x{C}+{off}"
    G, GT, ds = check_grad(ops, case, lgv, lg, off, c, W_ROW, W_COL, "both")
    assert same_bits(G[:, :C], GT[:, :R].t()), "G and GT^T differ"
    G1, _, ds1 = check_grad(ops, case, lgv, lg, off, c, W_ROW, W_COL, "g_only")
    _, GT2, ds2 = check_grad(ops, case, lgv, lg, off, c, W_ROW, W_COL, "gt_only")
    assert same_bits(G, G1) and same_bits(GT, GT2)
    G3, GT3, ds3 = abi_grad(ops, lgv, off, c["rl32"].cuda(), c["cl32"].cuda(), W_ROW, W_COL, SCALE, DS_IN)
    assert same_bits(G, G3) and same_bits(GT, GT3) and same_bits(ds, ds3), "a second launch differs"
    if C > R:                                              # a column that is no row's label: exactly the row term
        out = torch.ones(C, dtype=torch.bool)
        out[off:off + R] = False
        row_only = LR.grad(lg, off, W_ROW, 0.0)[:, out]
        measured("G", f"{case} row term only outside the label columns", (G[:, :C].cpu().double()[:, out] - row_only).abs(),
                 c["bound"][:, out])


#                        R,   C, off, w_row, w_col, label columns only
VARIANTS = [(130, 300, 0, 0.5, 0.0, True),                       # w_col = 0: col_lse = None
            (130, 300, 0, 0.0, 0.5, True),                       # the column term alone: +0 outside the label columns
            (48, 144, 96, 0.5, 0.5, False),                      # every column's statistic (before _label_columns_only)
            (48, 144, 96, 0.5 * 0.7 * 64 / 200, 0.5 * 0.7 * 64 / 200, True),   # weights w g f as the row-blocked backward passes
            (257, 257, 0, 0.3, 0.9, True)]


@pytest.mark.parametrize("family", ["scale100", "normal", "sink_last"])
@pytest.mark.parametrize("R,C,off,w_row,w_col,lab", VARIANTS)
def test_ce_grad_variants(family, R, C, off, w_row, w_col, lab):
    ops = _ops()
    lg = stats_case(family, R, C, off)["lg"]
    c = grad_case(family, R, C, off, w_row, w_col, lab)
    lgv = embed(lg)
    case = f"{family} {R}x{C}+{off} w=({w_row:.3g}, {w_col:.3g}){'' if lab else ' all columns'}"
    a = check_grad(ops, case, lgv, lg, off, c, w_row, w_col, "both", scale=100.0)
    b = check_grad(ops, case, lgv, lg, off, c, w_row, w_col, "both", scale=100.0)
    assert all(same_bits(u, v) for u, v in zip(a, b))
    assert same_bits(a[0][:, :C], a[1][:, :R].t())
    if not w_row and lab:
        out = torch.ones(C, dtype=torch.bool)
        out[off:off + R] = False
        assert bool((bits(a[0][:, :C][:, out.cuda()].contiguous()) == 0).all()), "+inf column statistic: the term is not +0"


def test_ce_grad_masked_elements():
    """The masked instantiation on the same bounds: a masked element is read as logit 0 and has G = 0."""
    ops = _ops()
    R, C, off = 130, 300, 0
    lg = LR.make_logits("scale100", R, C, off)
    t, _ = SR.clustered(C, 5000 + C)
    keep = SR.keep_mask(t[off:off + R], t, 0.8, off)
    assert 0.02 < float((~keep).float().mean()) < 0.6
    sim = torch.where(keep, 0.0, 1.0).cuda()
    lgv = embed(lg)
    rl, cl, dg = ops.ce_stats(lgv, off, sim=sim, thres=0.5)
    measured("row_lse", "masked scale100 130x300+0", (rl.cpu().double() - LR.row_lse(lg, keep)).abs(), LR.lse_bound(lg, 1, keep))
    measured("col_lse", "masked scale100 130x300+0", (cl.cpu().double() - LR.col_lse(lg, keep)).abs(), LR.lse_bound(lg, 0, keep))
    rl32 = LR.row_lse(lg, keep).float()
    cl32 = LR.label_columns_only(LR.col_lse(lg, keep), off, R).float()
    G = LR.grad(lg, off, 0.5, 0.5, keep=keep)
    delta, bound = LR.grad_bound(lg, off, rl32, cl32, 0.5, 0.5, keep=keep)
    ds = torch.full((1,), DS_IN, device="cuda")
    Gk, GTk = ops.ce_grad(lgv, rl32.cuda(), cl32.cuda(), off, 0.5, 0.5, SCALE, ds, sim=sim, thres=0.5)
    measured("G", "masked scale100 130x300+0", (Gk[:, :C].cpu().double() - G).abs(), bound)
    assert same_bits(Gk[:, :C], GTk[:, :R].t())
    assert bool((bits(Gk[:, :C].cpu().contiguous())[~keep] == 0).all())
    blocks = math.prod(LR.grad_grid(R, C, 320, 192))
    measured("dscale", "masked scale100 130x300+0", abs(float(ds) - DS_IN - LR.dscale(G, lg, SCALE, keep)),
             LR.dscale_bound(G, lg, delta, SCALE, DS_IN, blocks, keep))


# ---- F.normalize backward --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", LR.L2_DIMS)
@pytest.mark.parametrize("rows", LR.L2_ROWS)
def test_l2_normalize_bwd(rows, D):
    from vitlens_hip._lib import check
    ops = _ops()
    g = torch.Generator().manual_seed(100 * rows + D)
    x = torch.randn(rows, D, generator=g)
    if rows > 1:
        x[rows // 2] *= 1e-14                                         # one row whose norm is below eps: divided by eps
    nrm = x.norm(dim=-1)
    assert rows == 1 or float(nrm[rows // 2]) < 1e-12
    f = x / nrm.clamp_min(1e-12)[:, None]
    df = torch.randn(rows, D, generator=g)
    want, bound = LR.l2norm_bwd(f, df, nrm), LR.l2norm_bwd_bound(f, df, nrm)
    fc, dc, nc = f.cuda(), df.cuda(), nrm.cuda()
    dx = ops.l2_normalize_bwd(fc, dc, nc)
    measured("l2norm_bwd", f"{rows}x{D}", (dx.cpu().double() - want).abs(), bound + 1e-300)
    buf, out = guarded(rows * D)
    check(ops._lib.vl_l2_normalize_bwd(ops._p(fc), ops._p(dc), ops._p(nc), ops._p(out), rows, D, 1e-12, ops._stream()))
    torch.cuda.synchronize()
    guards_intact(buf, rows * D, "dx")
    assert same_bits(dx.view(-1), out)


# ---- the bf16x3 operand split ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", [0, 1])
@pytest.mark.parametrize("rows,D", [(9, 768), (5, 63), (1100, 1000)])          # 1100 x 1000 > 4096 x 256: a second grid sweep
def test_split_bf16x3(rows, D, pattern):
    from vitlens_hip._lib import check
    ops = _ops()
    g = torch.Generator().manual_seed(rows + D)
    x = torch.randn(rows, D, generator=g) * torch.logspace(-3, 3, D)
    x[0, :3] = torch.tensor([1.00390625, 1.01171875, -1.00390625])         # ties of the first rounding
    want = LR.split_bf16x3(x, pattern)
    xc = x.cuda()
    out = ops.split_bf16x3(xc, pattern)
    assert same_bits(out.cpu(), want), "hi / lo bits or layout"
    hi, lo = out[:, :D].cpu().double(), out[:, (D if pattern == 0 else 2 * D):][:, :D].cpu().double()
    measured("split_bf16x3", f"{rows}x{D} pattern {pattern}", (x.double() - hi - lo).abs(), 2.0 ** -17 * x.double().abs() + 1e-300)
    buf, o2 = guarded(rows * 3 * D, BF16)
    check(ops._lib.vl_split_bf16x3(ops._p(xc), ops._p(o2), rows, D, pattern, ops._stream()))
    torch.cuda.synchronize()
    guards_intact(buf, rows * 3 * D, "out")
    assert same_bits(out.view(-1), o2)


# ---- the transposes --------------------------------------------------------------------------------------------------------------
def guarded_rows(rows, ld, dtype=BF16):
    buf = poisoned(rows + 2, ld, dtype=dtype)
    return buf, buf[1:rows + 1]


@pytest.mark.parametrize("dt", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("R,C,ldo,pad,shift,kernel", LR.TRANSPOSE_CASES)
def test_transpose_to_bf16(R, C, ldo, pad, shift, kernel, dt):
    ops = _ops()
    x = (torch.randn(R, C, generator=torch.Generator().manual_seed(R + C)) * 3).to(dt)
    xv = embed(x, pad=pad, shift=shift)
    want = LR.transpose_bf16(x, ldo)
    for _ in range(2):
        buf, out = guarded_rows(C, ldo)
        assert LR.transpose_kernel(R, C, ldo, xv.stride(0), xv.data_ptr(), out.data_ptr()) == kernel
        got = ops.transpose_to_bf16(xv, ldo=ldo, out=out)
        torch.cuda.synchronize()
        assert got is out and same_bits(out.cpu(), want), "not x^T rounded to bf16 with +0 pad columns"
        still_poisoned(buf[0], "row before"); still_poisoned(buf[C + 1], "row behind")


@pytest.mark.parametrize("dt", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("R,C,ldo", LR.COLSUM_CASES)
def test_transpose_colsum(R, C, ldo, dt):
    ops = _ops()
    x = (torch.randn(R, C, generator=torch.Generator().manual_seed(R + C)) * 3 + 0.5).to(dt)
    xv = embed(x, pad=8)
    init = torch.linspace(-2.0, 3.0, C)
    want_t, want_s, bound = LR.transpose_bf16(x, ldo), LR.colsum(x, init, 0.5), LR.colsum_bound(x, init, 0.5)
    got = []
    for _ in range(2):
        buf, out = guarded_rows(C, ldo)
        cbuf, cs = guarded(C)
        cs.copy_(init)
        ops.transpose_colsum(xv, ldo, colsum_out=cs, scale=0.5, out=out)
        torch.cuda.synchronize()
        assert same_bits(out.cpu(), want_t)
        still_poisoned(buf[0], "row before"); still_poisoned(buf[C + 1], "row behind"); guards_intact(cbuf, C, "colsum")
        got.append(cs.clone())
    measured("transpose_colsum", f"{R}x{C} ldo {ldo} {'f32' if dt == F32 else 'bf16'}", (got[0].cpu().double() - want_s).abs(), bound)
    assert same_bits(got[0], got[1])


# ---- refusals ------------------------------------------------------------------------------------------------------------------
class _NoLaunch:
    """Stands in for the loaded library: any entry point that is reached fails the test."""
    def __getattr__(self, name):
        raise AssertionError(f"{name} was reached: the operands were not refused before the launch")


def test_operand_refusals_raise_before_a_launch_and_write_nothing(monkeypatch):
    ops = _ops()
    R, C = 6, 9
    lg = torch.randn(R, C, device="cuda")
    rl, cl, dg = ops.ce_stats(lg, 0)
    ds, loss = poisoned(1), poisoned(1)
    f, df, nrm = torch.randn(4, 8, device="cuda"), torch.randn(4, 8, device="cuda"), torch.ones(4, device="cuda")
    wide = torch.randn(4, 16, device="cuda")
    monkeypatch.setattr(ops, "_lib", _NoLaunch())
    bad_grad = [lambda: ops.ce_grad(lg.t().contiguous().t(), rl, cl, 0, 0.5, 0.5, 1.0, ds),        # column-major view
                lambda: ops.ce_grad(lg.double(), rl, cl, 0, 0.5, 0.5, 1.0, ds),
                lambda: ops.ce_grad(lg.bfloat16(), rl, cl, 0, 0.5, 0.5, 1.0, ds),
                lambda: ops.ce_grad(lg[0], rl, cl, 0, 0.5, 0.5, 1.0, ds),
                lambda: ops.ce_grad(lg, rl[:-1], cl, 0, 0.5, 0.5, 1.0, ds),
                lambda: ops.ce_grad(lg, rl, cl[:-1], 0, 0.5, 0.5, 1.0, ds),
                lambda: ops.ce_grad(lg, rl, cl.double(), 0, 0.5, 0.5, 1.0, ds),
                lambda: ops.ce_grad(lg, rl, cl, 0, 0.5, 0.5, 1.0, torch.zeros(2, device="cuda"))]
    bad_l2 = [lambda: ops.l2_normalize_bwd(wide[:, :8], df, nrm),                                  # strided f
              lambda: ops.l2_normalize_bwd(f, wide[:, :8], nrm),                                   # strided df
              lambda: ops.l2_normalize_bwd(f.bfloat16(), df, nrm),
              lambda: ops.l2_normalize_bwd(f, df.bfloat16(), nrm),
              lambda: ops.l2_normalize_bwd(f, df[:3], nrm),
              lambda: ops.l2_normalize_bwd(f, df, nrm[:3]),
              lambda: ops.l2_normalize_bwd(f, df, nrm.double()),
              lambda: ops.l2_normalize_bwd(f, df, torch.ones(8, device="cuda")[::2])]
    bad_loss = [lambda: ops.ce_loss_accum(loss, rl, cl, dg, R + 1, C, 0, 0.5, 0.5),                # R on trust
                lambda: ops.ce_loss_accum(loss, rl, cl, dg, R, C + 1, 0, 0.5, 0.5),                # Cc on trust
                lambda: ops.ce_loss_accum(loss, rl, cl, dg, 0, C, 0, 0.5, 0.5),
                lambda: ops.ce_loss_accum(loss, None, cl, dg[:-1], R, C, 0, 0.5, 0.5),
                lambda: ops.ce_loss_accum(loss, rl.double(), cl, dg, R, C, 0, 0.5, 0.5),
                lambda: ops.ce_loss_accum(torch.zeros(2, device="cuda"), rl, cl, dg, R, C, 0, 0.5, 0.5)]
    for i, call in enumerate(bad_grad + bad_l2 + bad_loss):
        with pytest.raises((ValueError, TypeError)):
            call()
    monkeypatch.undo()
    torch.cuda.synchronize()
    still_poisoned(ds, "dscale"); still_poisoned(loss, "loss")
    G, GT = ops.ce_grad(lg, rl, cl, 0, 0.5, 0.5, 1.0, torch.zeros(1, device="cuda"))               # and the good operands still pass
    assert bool(torch.isfinite(G.float()).all())


# ---- pair level: step.pair_forward / pair_backward ---------------------------------------------------------------------------------
def pair_inputs(R, C, off):
    """(x [R, 64], y [C, 64]) fp32 unit features: clustered teachers as the rows, independent students as the columns."""
    t, s = SR.clustered(C, 1000 + C)
    return t[off:off + R].contiguous(), s


def pair_scale(kind):
    """(what pair_forward is given - made on the device by the caller -, the temperature it amounts to, log-domain?)."""
    if kind == "f100":
        return 100.0, 100.0, False
    if kind == "f14":
        return 14.2857, 14.2857, False
    ls = torch.tensor([math.log(100.0)], dtype=F32)
    return ls, math.exp(float(ls.double())), True


@functools.lru_cache(maxsize=None)
def pair_case(R, C, off, w_col, kind):
    x, y = pair_inputs(R, C, off)
    _, s, dev = pair_scale(kind)
    lg = s * x.double() @ y.double().t()
    G = LR.grad(lg, off, 0.5, w_col)
    E = LR.logits_err_bound(x, y, s, dev)
    return dict(x=x, y=y, lg=lg, G=G, E=E, loss=float(LR.loss(lg, off, 0.5, w_col)), dx=s * G @ y.double(), dy=s * G.t() @ x.double(),
                ds=LR.dscale(G, lg, 1.0 if dev else s))


def pair_dscale_tol(c, off, w_col, div, launches, blocks):
    """Bound on the d/dscale accumulator of the pair level: loss_ref.dscale_bound (the kernels' own arithmetic, on exact logits
    and statistics) plus what the logits' error E and the statistics' error B (loss_ref.lse_bound) do to sum g l: l moves by E,
    every probability by a factor within exp(+-(2 max E + max B)), so
        |d(g l)| <= |g| E + (|l| + E) (exp(2 max E + max B) - 1) sum_terms w / R p.
    A row-blocked backward accumulates once per block: the accumulator's own rounding is counted per launch."""
    lg, G, E = c["lg"], c["G"], c["E"]
    R, C = lg.shape
    rl, cl = LR.row_lse(lg), LR.label_columns_only(LR.col_lse(lg), off, R)
    delta, _ = LR.grad_bound(lg, off, rl.float(), cl.float() if w_col else None, 0.5, w_col)
    tol = LR.dscale_bound(G, lg, delta, div, DS_IN, blocks)
    B = max(float(LR.lse_bound(lg, 1).max()), float(LR.lse_bound(lg, 0).max()))
    grow = math.expm1(2 * float(E.max()) + B)
    psum = sum(abs(w) / R * p for w, p, _, _, _ in LR.grad_terms(lg, off, rl, cl if w_col else None, 0.5, w_col))
    tol += float((G.abs() * E + (lg.abs() + E) * grow * psum).sum()) / div
    return tol + (launches - 1) * LR.U24 * (abs(DS_IN) + abs(DS_IN + c["ds"]))


def run_pair(c, kind, off, w_col, chunk, need_dx=True, need_dy=True):
    from vitlens_hip import step as ST
    scale, _, dev = pair_scale(kind)
    scale = scale.cuda() if dev else scale
    lbuf, loss_acc = guarded(1)
    dbuf, ds_acc = guarded(1)
    loss_acc.fill_(LOSS_IN); ds_acc.fill_(DS_IN)
    loss, ctx = ST.pair_forward(c["x"].cuda(), c["y"].cuda(), scale, off, 0.5, w_col, chunk_rows=chunk, loss_acc=loss_acc)
    assert (ctx[2] is None and ctx[9] == chunk) if chunk else ctx[2] is not None
    dx, dy, ds = ST.pair_backward(ctx, need_dx=need_dx, need_dy=need_dy, dscale_acc=ds_acc)
    torch.cuda.synchronize()
    assert loss is loss_acc and ds is ds_acc
    guards_intact(lbuf, 1, "loss accumulator"); guards_intact(dbuf, 1, "dscale accumulator")
    return loss.clone(), dx, dy, ds.clone()


def check_rows(kernel, case, out, ref, tol):
    worst, (r0, _, _, _) = errloc.block_relerr(out.cpu().double(), ref, 1, ref.shape[1])
    print(f"MEASURED {kernel} | {case} | worst row {r0}: {worst:.3e} (tolerance {tol:.2e}, {worst / tol:.3f} of it)")
    assert worst <= tol, f"{kernel} {case}: row {r0} has relative error {worst:.3e} > {tol:.2e}"


@pytest.mark.parametrize("kind", LR.SCALES)
@pytest.mark.parametrize("R,C,off,w_col,chunk", LR.PAIR_CASES)
def test_pair_vs_float64(R, C, off, w_col, chunk, kind):
    c = pair_case(R, C, off, w_col, kind)
    _, s, dev = pair_scale(kind)
    case = f"{R}x{C}+{off} chunk {chunk} {kind}"
    a = run_pair(c, kind, off, w_col, chunk)
    b = run_pair(c, kind, off, w_col, chunk)
    assert all(same_bits(u, v) for u, v in zip(a, b)), "a second run differs"
    loss, dx, dy, ds = a
    measured("pair loss", case, abs(float(loss) - LOSS_IN - c["loss"]), LR.pair_loss_tol(c["lg"], c["E"], off, 0.5, w_col, LOSS_IN))
    mx, my = MODEL_DXDY[(R, C, off, 100.0 if kind != "f14" else 14.2857)]
    check_rows("pair dx", case, dx, c["dx"], 2 * mx)
    check_rows("pair dy", case, dy, c["dy"], 2 * my)
    ldg, ldgt = (C + 63) // 64 * 64, (R + 63) // 64 * 64
    rows = [min(chunk, R - r0) for r0 in range(0, R, chunk)] if chunk else [R]
    blocks = lambda g, gt: sum(math.prod(LR.grad_grid(r, C, ldg, (r + 63) // 64 * 64, g, gt)) for r in rows)
    div = 1.0 if dev else s
    measured("pair dscale", case, abs(float(ds) - DS_IN - c["ds"]), pair_dscale_tol(c, off, w_col, div, len(rows), blocks(True, True)))
    _, none, dy1, ds1 = run_pair(c, kind, off, w_col, chunk, need_dx=False)
    assert none is None and same_bits(dy1, dy)
    measured("pair dscale", case + " dy only", abs(float(ds1) - DS_IN - c["ds"]), pair_dscale_tol(c, off, w_col, div, len(rows), blocks(False, True)))
    _, dx2, none, ds2 = run_pair(c, kind, off, w_col, chunk, need_dy=False)
    assert none is None and same_bits(dx2, dx)
    measured("pair dscale", case + " dx only", abs(float(ds2) - DS_IN - c["ds"]), pair_dscale_tol(c, off, w_col, div, len(rows), blocks(True, False)))
    if chunk:                                              # row-blocked against the whole matrix of the same kernels
        lw, dxw, dyw, dsw = run_pair(c, kind, off, w_col, 0)
        print(f"MEASURED blocked vs whole | {case} | loss {float(loss) - float(lw):.3e} dscale {float(ds) - float(dsw):.3e}")
        assert abs(float(loss) - float(lw)) < 2e-5 * max(1.0, abs(c["loss"]))                  # summation order
        check_rows("blocked vs whole dx", case, dx, dxw.cpu().double(), 1e-2)
        check_rows("blocked vs whole dy", case, dy, dyw.cpu().double(), 1e-2)
