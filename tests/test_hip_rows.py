"""GPU: the row-wise kernels (csrc/vl_rows.hip), the LayerNorm backward and the small elementwise kernels (csrc/vl_bwd.hip)
against the fp64 references of tests/rows_ref.py, on every dispatch branch: each register form (NCH) and the any-D form, every
dtype combination, strided and unaligned operands, the sparse residual gradient, the ill-conditioned-row branch of the row
statistics, and the elementwise kernels past their first grid sweep (4096 workgroups).

Every output buffer is poisoned with NaN first and is larger than what the kernel may touch; the surplus is compared bit for
bit afterwards.  fp32 outputs are compared per row (errloc blocks of 1 x D: one bad row cannot average away), statistics per
element, bf16 / fp16 outputs per element at their rounding.  Tolerances are derived next to where they are used, or are twice
the worst value measured on the MI355X (given beside them); every check prints its figure before it asserts."""
import math

import pytest
import torch

import errloc
import rows_ref

pytestmark = pytest.mark.gpu

NAN = float("nan")
F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
EPS24 = 2.0 ** -24                    # half an fp32 ulp, relative
HALF_ULP = {BF16: 2.0 ** -8, F16: 2.0 ** -11}      # |round(v) - v| <= HALF_ULP * |v| (normal range)
SWEEP = 4096 * 256                    # threads of one grid sweep of the elementwise kernels


def _ops():
    from vitlens_hip import ops
    return ops


def rnd(*shape, seed, scale=1.0, shift=0.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale + shift


def bits(t):
    return t.view({4: torch.int32, 2: torch.int16}[t.element_size()])


def poisoned(*shape, dtype=F32):
    return torch.full(shape, NAN, dtype=dtype, device="cuda")


def still_poisoned(t, what):
    """Every element of t (a part of a poisoned buffer no kernel may touch) holds the poison's bits."""
    want = bits(torch.full((1,), NAN, dtype=t.dtype, device=t.device))
    assert bool((bits(t.contiguous()) == want).all()), f"{what}: written outside the output"


def report(what, worst, tol):
    print(f"MEASURED {what}: {worst:.3e} (bound {tol:.2e})")
    assert worst <= tol, f"{what}: {worst:.3e} > {tol:.2e}"          # (a NaN fails this too)


def check_rows(out, ref, tol, what):
    """fp32 out [rows, D] against fp64 ref, every row a block of its own."""
    worst, (r0, _, _, _) = errloc.block_relerr(out, ref, 1, out.shape[1])
    print(f"MEASURED {what}: worst row {r0} relative error {worst:.3e} (bound {tol:.2e})")
    errloc.assert_blocks(out, ref, tol, 1, out.shape[1], what=what)


def check_rounded(out, ref, f32_tol, what):
    """A bf16 / fp16 out against fp64 ref, per element: out = round(v) of an fp32 v whose row is within f32_tol of ref's row
    (relative, 2-norm; hence every element within f32_tol * ||ref row||):  |out - ref| <= h |ref| + (1 + h) f32_tol ||row||."""
    h = HALF_ULP[out.dtype]
    bound = h * ref.abs() + (1 + h) * f32_tol * ref.norm(dim=-1, keepdim=True) + 1e-30
    report(what + " (fraction of the rounding bound)", float(((out.double() - ref).abs() / bound).max()), 1.0)


def check_out(out, ref, f32_tol, what):
    if out.dtype == F32:
        check_rows(out, ref, f32_tol, what)
    else:
        check_rounded(out, ref, f32_tol, what)


def stat_bounds(D):
    """Worst-case rounding count of the two-pass statistics, in units of 2^-24: a lane adds D/64 values, the wave reduction 6
    more, 1/D and the product 2; the squares add the rounding of d = x - mean (twice) and of the fma.  D/64 + 12 covers the
    mean (relative to mean|x|) and, halved by the root plus rsqrtf's 2 ulp and the eps addition, rstd (relative)."""
    return (D / 64 + 12) * EPS24


def check_stats(mean, rstd, x, what, eps=1e-5):
    mu, rs = rows_ref.row_stats(x, eps)
    b = stat_bounds(x.shape[-1])
    report(what + " mean / (bound * mean|x|)", float(((mean.double() - mu).abs() / (b * x.double().abs().mean(-1) + 1e-30)).max()), 1.0)
    report(what + " rstd relative", float((rstd.double() / rs - 1).abs().max()), b)


# Twice the worst per-row relative error measured on the MI355X against fp64, over every case of this file:
TOL_LN_FWD = 1.9e-7       # measured 9.39e-8 (D = 72, 5 rows, bf16 -> fp32); D = 2048: 9.30e-8; gather / pooling 7.5e-8
TOL_ASSEMBLE = 2.2e-7     # measured 1.10e-7 (B = 3, T = 4, D = 256, fp32 tokens, pos2): the assembly's two additions on top
TOL_LN_BWD = 1.6e-7       # measured 7.93e-8 (sparse, L = 257, D = 72, fp32 stream); dense forms 5.7e-8


def ln_params(D, seed):
    return (1 + rnd(D, seed=seed, scale=0.1)).cuda(), rnd(D, seed=seed + 1, scale=0.1).cuda()


def rows_like_activations(rows, D, seed, dtype):
    """Rows with offsets and scales of their own, as a residual stream has them."""
    x = rnd(rows, D, seed=seed) * (0.5 + 2 * rnd(rows, 1, seed=seed + 1).abs()) + rnd(rows, 1, seed=seed + 2)
    return x.to(dtype)


# ------------------------------------------------------------------------------------------------ LayerNorm forward
def _ln_forward(rows, D, in_dt, out_dt, xs=None, ys=None, x_off=0, y_off=0, stats=True, what=""):
    """ops.layernorm on x [rows, D] inside a [rows, xs] buffer (x_off elements into its allocation), out inside a poisoned
    [rows + 1, ys] buffer (y_off elements in)."""
    ops = _ops()
    xs, ys = xs or D, ys or D
    x = rows_like_activations(rows, D, 100 + D + rows, in_dt)
    xbuf = torch.zeros(rows * xs + x_off + 8, dtype=in_dt)
    xv = xbuf[x_off:x_off + rows * xs].view(rows, xs)
    xv[:, :D] = x
    xbuf = xbuf.cuda()
    xg = xbuf[x_off:x_off + rows * xs].view(rows, xs)
    w, b = ln_params(D, 7)
    ybuf = poisoned((rows + 1) * ys + y_off + 8, dtype=out_dt)
    y = ybuf[y_off:y_off + (rows + 1) * ys].view(rows + 1, ys)
    mean, rstd = (poisoned(rows + 1), poisoned(rows + 1)) if stats else (None, None)
    ops.layernorm(xg, w, b, y[:, :D], rows, D, x_row_stride=xs, mean=mean, rstd=rstd)
    ref, _, _ = rows_ref.layernorm_fwd(xg[:, :D], w, b)
    check_out(y[:rows, :D], ref, TOL_LN_FWD, f"layernorm {what} D={D} rows={rows}")
    still_poisoned(y[rows], "row past the last")
    still_poisoned(ybuf[:y_off], "before the output"); still_poisoned(ybuf[y_off + (rows + 1) * ys:], "behind the output")
    if ys > D:
        still_poisoned(y[:, D:], "columns between the rows")
    if stats:
        check_stats(mean[:rows], rstd[:rows], xg[:, :D], f"layernorm {what} D={D} rows={rows}")
        still_poisoned(mean[rows:], "mean"); still_poisoned(rstd[rows:], "rstd")


@pytest.mark.parametrize("rows", [1, 5])
@pytest.mark.parametrize("D", [256, 1280, 2048, 1536, 1664, 72])
def test_layernorm_forward_every_form(D, rows):
    """ln_rows_kernel: NCH 1, 5, 8 (D = 256, 1280, 2048), the `default:` arm of the switch (1536 = 6 chunks: any-D form), a D
    that is no multiple of 256 (1664, ViT-bigG) and fewer than two sweeps of the wave (72); one wave, and a second workgroup of
    one wave (5 rows).  bf16 -> fp32 with mean / rstd, and fp32 -> bf16.    Measured worst row, fp32 out: 9.4e-8 (D = 72)."""
    _ln_forward(rows, D, BF16, F32, what="bf16->f32")
    _ln_forward(rows, D, F32, BF16, stats=False, what="f32->bf16")


@pytest.mark.parametrize("D", [256, 72])
@pytest.mark.parametrize("in_dt,out_dt", [(F32, F32), (F32, BF16), (F32, F16), (BF16, F32), (BF16, BF16)])
def test_layernorm_forward_dtype_pairs(D, in_dt, out_dt):
    """The five (input, output) pairs ln_dispatch has kernels for, register form (256) and any-D form (72)."""
    _ln_forward(5, D, in_dt, out_dt, what=f"{in_dt}->{out_dt}")


@pytest.mark.parametrize("in_dt", [F32, BF16])
def test_layernorm_forward_strides_and_unaligned_bases(in_dt):
    """D = 256: rows D + 4 apart keep the register form (16-byte accesses on strided rows); D + 2 apart, or a base address one
    element into the allocation, must take the any-D form (ln_launch's alignment predicate) - and all must be right.  The same
    for the output's stride and base."""
    for xs, ys, xo, yo in [(260, 256, 0, 0), (258, 256, 0, 0), (256, 260, 0, 0), (256, 258, 0, 0), (260, 264, 0, 0),
                           (256, 256, 1, 0), (256, 256, 0, 1), (260, 260, 1, 1)]:
        for out_dt in (F32, BF16):
            _ln_forward(5, 256, in_dt, out_dt, xs=xs, ys=ys, x_off=xo, y_off=yo, what=f"xs={xs} ys={ys} x+{xo} y+{yo} {in_dt}->{out_dt}")


@pytest.mark.parametrize("D", [256, 72])
def test_layernorm_forward_row_index_and_row_mul_bf16(D):
    """The EOT gather (source row = r * row_mul + row_index[r]) and the class-token pooling (x_row_stride = L * D) on a bf16
    residual stream."""
    ops = _ops()
    B, L = 5, 9
    x = rows_like_activations(B * L, D, 31, BF16).cuda()
    w, b = ln_params(D, 9)
    idx = torch.tensor([3, 0, 8, 5, 1], device="cuda")
    y = poisoned(B + 1, D)
    mean, rstd = poisoned(B + 1), poisoned(B + 1)
    ops.layernorm(x, w, b, y, B, D, x_row_stride=D, row_index=idx, row_mul=L, mean=mean, rstd=rstd)
    src = x.view(B, L, D)[torch.arange(B, device="cuda"), idx]
    check_rows(y[:B], rows_ref.layernorm_fwd(src, w, b)[0], TOL_LN_FWD, f"gather D={D}")
    check_stats(mean[:B], rstd[:B], src, f"gather D={D}")
    still_poisoned(y[B], "row past the last")
    y = poisoned(B + 1, D)
    ops.layernorm(x, w, b, y, B, D, x_row_stride=L * D)
    check_rows(y[:B], rows_ref.layernorm_fwd(x.view(B, L, D)[:, 0], w, b)[0], TOL_LN_FWD, f"pooling D={D}")
    still_poisoned(y[B], "row past the last")


@pytest.mark.parametrize("tok_dt", [BF16, F32])
@pytest.mark.parametrize("D", [256, 1280, 72])
@pytest.mark.parametrize("B,T", [(1, 1), (3, 4)])
def test_assemble_ln_pre_saves_what_the_backward_reads(B, T, D, tok_dt):
    """assemble_ln_pre (ln_rows_kernel MODE 1; NCH 1, 5 and the any-D form), pos2 present and absent: `xpre` bit-equal to the
    fp32 sum in the kernel's order (token + pos) + pos2, `mean` / `rstd` / `out` against fp64 on the exact assembled rows."""
    ops = _ops()
    R = B * (T + 1)
    tok = rnd(B, T, D, seed=40 + D).to(tok_dt).cuda()
    cls, pos, pos2 = rnd(D, seed=41).cuda(), rnd(T + 1, D, seed=42).cuda(), rnd(T, D, seed=43).cuda()
    w, b = ln_params(D, 44)
    for p2 in (None, pos2):
        for out_dt in (F32, BF16):
            y, xpre = poisoned(R + 1, D, dtype=out_dt), poisoned(R + 1, D)
            mean, rstd = poisoned(R + 1), poisoned(R + 1)
            ops.assemble_ln_pre(tok, cls, pos, p2, w, b, y, B, T, D, xpre=xpre, mean=mean, rstd=rstd)
            what = f"assemble B={B} T={T} D={D} {tok_dt} pos2={p2 is not None} -> {out_dt}"
            assert torch.equal(bits(xpre[:R]), bits(rows_ref.assemble_f32(tok, cls, pos, p2))), what + ": xpre"
            exact = rows_ref.assemble(tok, cls, pos, p2)
            check_out(y[:R], rows_ref.layernorm_fwd(exact, w, b)[0], TOL_ASSEMBLE, what)
            b_st = stat_bounds(D) + 2 * EPS24
            mu, rs = rows_ref.row_stats(exact)
            report(what + " mean", float(((mean[:R].double() - mu).abs() / (b_st * exact.abs().mean(-1))).max()), 1.0)
            report(what + " rstd", float((rstd[:R].double() / rs - 1).abs().max()), b_st)
            for t, name in ((y, "out"), (xpre, "xpre"), (mean, "mean"), (rstd, "rstd")):
                still_poisoned(t[R:], name)


# ------------------------------------------------------------------------------------------------ row statistics
def _row_stats_case(D, rows, m_main, planted=False):
    ops = _ops()
    x = rows_like_activations(rows, D, 50 + D, BF16)
    where = {}
    if planted:
        far, near, const = rows_ref.ill_conditioned_rows(D)
        where = {"far": slice(7, 11), "near": slice(100, 104), "const": slice(258, 259)}
        x[where["far"]], x[where["near"]], x[where["const"]] = far, near, const
        assert where["const"].stop <= m_main
    x = x.cuda()
    part = rows_ref.slice_partials(x) if m_main else None
    mean, rstd = poisoned(rows + 3), poisoned(rows + 3)
    ops.ln_row_stats(part, x, m_main, mean, rstd)
    mu, rs = rows_ref.row_stats(x)
    what = f"ln_row_stats D={D} m_main={m_main}"
    # the bounds of test_residual_gemm_leaves_the_row_statistics_of_what_it_stores
    report(what + " mean", float((mean[:rows].double() - mu).abs().max()), 2e-5 * (1 + float(mu.abs().max())))
    report(what + " rstd relative", float((rstd[:rows].double() / rs - 1).abs().max()), 2e-4)
    still_poisoned(mean[rows:], "mean"); still_poisoned(rstd[rows:], "rstd")
    return mean, rstd, mu, rs, where


@pytest.mark.parametrize("m_main", [0, 260, 259])
@pytest.mark.parametrize("D", [512, 768, 1280, 1536, 2048])
def test_ln_row_stats_every_form(D, m_main):
    """row_stats_kernel: the register form with nc = 1, 3, 4 (D = 512, 1536, 2048) and the any-D form (768, 1280) on the
    leftover rows; main rows from per-slice partial sums built here.  300 rows; m_main = 260 crosses the 256-row workgroup of
    the first branch and leaves 40 = 10 x 4 rows, 259 leaves a short last workgroup, 0 = every row from the rows themselves."""
    _row_stats_case(D, 300, m_main)


def test_ln_row_stats_ill_conditioned_rows_take_the_two_pass_branch():
    """D = 1024 (register form nc = 2), among the main rows: four rows at offset 1000, sigma 4 - `var < 1e-3 * ex2` holds, and
    the one-pass formula on these very partial sums is off by 1.4e-3 in rstd (7 x the bound; fp32 emulation in
    tests/test_rows_ref_host.py), so the fallback is what passes; four rows at offset 40, sigma 1.5 - not taken, one-pass error
    2.6e-5; one constant row - variance exactly 0."""
    mean, rstd, mu, rs, where = _row_stats_case(1024, 300, 260, planted=True)
    for name, s in where.items():
        report(f"planted '{name}' rows rstd relative", float((rstd[s].double() / rs[s] - 1).abs().max()), 2e-4)
    assert float(rstd[where["const"]]) == pytest.approx(1e-5 ** -0.5, rel=1e-6) and float(mean[where["const"]]) == 3.140625


@pytest.mark.parametrize("D", [512, 768])
@pytest.mark.parametrize("layout", ["aligned", "stride D + 2"])
def test_ln_row_stats_h_left(D, layout):
    """The LayerNorm output of the consuming GEMM's leftover rows from the same launch (h_row0 > m_main): 16-byte stores into
    an aligned buffer, the two-byte-store fallback for a view whose row stride is D + 2 (register form, D = 512), the any-D
    form (768).  Nothing before row h_row0 or behind the last row is written."""
    ops = _ops()
    rows, m_main, h_row0 = 300, 256, 272
    x = rows_like_activations(rows, D, 60 + D, BF16).cuda()
    w, b = ln_params(D, 61)
    ys = D if layout == "aligned" else D + 2
    guard = 3
    hbuf = poisoned(rows - h_row0 + 2 * guard, ys, dtype=BF16)
    h_left = hbuf[guard:guard + rows - h_row0, :D]
    assert (h_left.data_ptr() % 16 == 0) == (layout == "aligned")
    mean, rstd = poisoned(rows), poisoned(rows)
    ops.ln_row_stats(rows_ref.slice_partials(x), x, m_main, mean, rstd, ln_w=w, ln_b=b, h_left=h_left, h_row0=h_row0)
    ref = rows_ref.layernorm_fwd(x[h_row0:], w, b)[0]
    check_rounded(h_left, ref, TOL_LN_FWD, f"h_left D={D} {layout}")
    still_poisoned(hbuf[:guard], "rows before h_row0"); still_poisoned(hbuf[guard + rows - h_row0:], "rows behind the last")
    if ys > D:
        still_poisoned(hbuf[:, D:], "columns between the rows")
    mu, rs = rows_ref.row_stats(x)
    report("mean", float((mean.double() - mu).abs().max()), 2e-5 * (1 + float(mu.abs().max())))
    report("rstd relative", float((rstd.double() / rs - 1).abs().max()), 2e-4)


# ------------------------------------------------------------------------------------------------ LayerNorm backward
def _ln_backward(rows, D, dy_dt, x_dt, g_dt, dres="dense", want_dx=True, want_dxb=False, xs=None, dys=None, dxs=None, what=""):
    """ops.layernorm_bwd on operands inside wider buffers (row strides xs, dys, dxs); dres: 'dense', 'inplace' (dres is dx) or
    None.  Outputs poisoned, one row and the columns behind D in surplus."""
    ops = _ops()
    xs, dys, dxs = xs or D, dys or D, dxs or D
    xf = torch.zeros(rows, xs, dtype=x_dt); xf[:, :D] = rows_like_activations(rows, D, 70 + D + rows, x_dt)
    dyf = torch.zeros(rows, dys, dtype=dy_dt); dyf[:, :D] = rnd(rows, D, seed=71 + D).to(dy_dt)
    xf, dyf = xf.cuda(), dyf.cuda()
    x, dy = xf[:, :D], dyf[:, :D]
    w, _ = ln_params(D, 72)
    mu, rs = rows_ref.row_stats(x)
    mean, rstd = mu.float(), rs.float()                       # what a forward saved: the reference reads the same fp32 values
    dres_vals = rnd(rows, D, seed=73 + D).to(g_dt).cuda() if dres else None
    dx = dxb = dres_t = None
    if want_dx or dres == "inplace":
        dx = poisoned(rows + 1, dxs, dtype=g_dt)
    if dres == "inplace":
        dx[:rows, :D] = dres_vals
        dres_t = dx
    elif dres == "dense":
        dres_t = torch.zeros(rows, dxs, dtype=g_dt, device="cuda"); dres_t[:, :D] = dres_vals
    if want_dxb:
        dxb = poisoned(rows + 1, dxs, dtype=BF16)
    ops.layernorm_bwd(dyf, xf, mean, rstd, w, rows, D, dres=dres_t, dx=dx, dx_bf16=dxb, x_row_stride=xs, dy_row_stride=dys,
                      dx_row_stride=dxs)
    ref = rows_ref.layernorm_bwd(dy, x, mean, rstd, w, dres_vals)
    what = f"layernorm_bwd {what} D={D} rows={rows} ({dy_dt}, {x_dt}, {g_dt}) dres={dres}"
    for out, name in ((dx, "dx"), (dxb, "dx_bf16")):
        if out is None:
            continue
        check_out(out[:rows, :D], ref, TOL_LN_BWD, f"{what} {name}")
        still_poisoned(out[rows], name + ": row past the last")
        if dxs > D:
            still_poisoned(out[:, D:], name + ": columns between the rows")
    return dx


@pytest.mark.parametrize("D", [256, 72])
@pytest.mark.parametrize("g_dt", [F32, BF16])
@pytest.mark.parametrize("x_dt", [F32, BF16])
@pytest.mark.parametrize("dy_dt", [F32, BF16])
def test_layernorm_bwd_every_dtype_combination(dy_dt, x_dt, g_dt, D):
    """ln_bwd_kernel: the eight (dy, x, gradient-stream) combinations in the register form (D = 256, NCH 1) and the any-D form
    (72), 5 rows = a second workgroup of one wave.    Measured worst row, fp32 stream: 5.7e-8."""
    _ln_backward(5, D, dy_dt, x_dt, g_dt)


@pytest.mark.parametrize("rows", [1, 5, 6])
@pytest.mark.parametrize("D", [256, 512, 768, 1024, 1280, 24])
@pytest.mark.parametrize("dts", [(BF16, BF16, BF16), (BF16, F32, F32)])
def test_layernorm_bwd_every_form(dts, D, rows):
    """NCH 1, 2, 3, 4 (D = 256 ... 1024) and the any-D form (1280: ViT-H, no register form; 24: fewer than one sweep of the
    wave), rows in {1, 5, 6}, on the two combinations the trainers use."""
    _ln_backward(rows, D, *dts)


@pytest.mark.parametrize("D", [256, 72])
@pytest.mark.parametrize("g_dt", [F32, BF16])
def test_layernorm_bwd_call_forms(D, g_dt):
    """In place (dres is dx), dx_bf16 together with dx and alone, no dres."""
    _ln_backward(5, D, BF16, BF16, g_dt, dres="inplace", what="in place")
    _ln_backward(5, D, BF16, BF16, g_dt, dres="dense", want_dxb=True, what="dx + dx_bf16")
    _ln_backward(5, D, BF16, BF16, g_dt, dres=None, what="no dres")
    if g_dt == F32:
        _ln_backward(5, D, BF16, BF16, F32, dres=None, want_dx=False, want_dxb=True, what="dx_bf16 alone")
        _ln_backward(5, D, BF16, BF16, F32, dres="dense", want_dx=False, want_dxb=True, what="dx_bf16 alone, dres")


@pytest.mark.parametrize("D", [256, 72])
@pytest.mark.parametrize("dts", [(BF16, BF16, BF16), (BF16, F32, F32), (F32, BF16, F32)])
def test_layernorm_bwd_strides(dts, D):
    """x_row_stride = 3 * D (the pooled-row call of train.py: x is every L-th row of the stream), dy / dx strides D + 8
    (points.py's column windows), and a stride of D + 2 on each operand in turn: at D = 256 that must take the any-D form
    (rows no longer on 8 / 16-byte boundaries) and be right."""
    _ln_backward(5, D, *dts, xs=3 * D, what="xs=3D")
    _ln_backward(5, D, *dts, dys=D + 8, dxs=D + 8, want_dxb=True, what="dys=dxs=D+8")
    _ln_backward(5, D, *dts, xs=D + 2, what="xs=D+2")
    _ln_backward(5, D, *dts, dys=D + 2, what="dys=D+2")
    _ln_backward(5, D, *dts, dxs=D + 2, want_dxb=True, what="dxs=D+2")


def _sparse_case(B, L, D, g_dt, rows=None, dres_stride=None, dx_off=0):
    ops = _ops()
    rows = rows or B * L
    dres_stride = dres_stride or D + 4
    x = rows_like_activations(rows, D, 80 + D, BF16).cuda()
    dy = rnd(rows, D, seed=81 + D).bfloat16().cuda()
    w, _ = ln_params(D, 82)
    mu, rs = rows_ref.row_stats(x)
    mean, rstd = mu.float(), rs.float()
    wide = rnd(B, dres_stride, seed=83, shift=3.0).to(g_dt).cuda()      # |dres| ~ 3: adding it to a row that has none would show
    dres = wide[:, :D]
    buf = poisoned((rows + 1) * D + dx_off + 8, dtype=g_dt)
    dx = buf[dx_off:dx_off + (rows + 1) * D].view(rows + 1, D)
    ops.layernorm_bwd_sparse_res(dy, x, mean, rstd, w, rows, D, dres, L, dx)
    what = f"sparse B={B} L={L} D={D} rows={rows} {g_dt} dres stride {dres_stride} dx+{dx_off}"
    check_out(dx[:rows], rows_ref.layernorm_bwd_sparse(dy, x, mean, rstd, w, dres, L), TOL_LN_BWD, what)
    still_poisoned(dx[rows], "row past the last"); still_poisoned(buf[:dx_off], "before dx"); still_poisoned(buf[dx_off + (rows + 1) * D:], "behind dx")
    # the rows without a residual gradient: the same kernel, the same order, nothing added - the bits of the dense call without dres
    plain = poisoned(rows, D, dtype=g_dt)
    ops.layernorm_bwd(dy, x, mean, rstd, w, rows, D, dx=plain)
    if dx_off == 0 and dres_stride % 4 == 0:                       # (same form on both sides; the any-D form adds in another order)
        none = torch.arange(rows, device="cuda") % L != 0
        assert torch.equal(bits(dx[:rows][none]), bits(plain[none])), what + ": rows without a residual gradient"
    return dx[:rows], plain


@pytest.mark.parametrize("g_dt", [F32, BF16])
@pytest.mark.parametrize("D", [256, 72])
@pytest.mark.parametrize("B,L", [(3, 5), (2, 257)])
def test_layernorm_bwd_sparse_res(B, L, D, g_dt):
    """dres_every > 1: row i * L adds row i of dres - a column window of a wider buffer, row stride D + 4 - every other row
    adds nothing and is bit-equal to the dense call without dres.  A dense form that added dres to every row would be off by
    |dres| ~ 3 on those rows, a relative error of order 1 (bound 1.6e-7; measured 7.9e-8).  rows = B * L - 2: the last sample is cut short."""
    _sparse_case(B, L, D, g_dt)
    _sparse_case(B, L, D, g_dt, rows=B * L - 2)


@pytest.mark.parametrize("g_dt", [F32, BF16])
def test_layernorm_bwd_sparse_res_unaligned_operands_take_the_any_d_form(g_dt):
    """D = 256 with a dres whose row stride is D + 1, and with a dx that starts one element into its allocation: neither is on
    8 / 16-byte boundaries, ln_bwd_launch's predicate must send both to the any-D form, and the results are right."""
    _sparse_case(3, 5, 256, g_dt, dres_stride=257)
    _sparse_case(3, 5, 256, g_dt, dx_off=1)
    _sparse_case(3, 5, 256, g_dt, dres_stride=257, dx_off=1, rows=13)


# ------------------------------------------------------------------------------------------------ elementwise kernels
def f32_from_bits(words):
    return torch.tensor([w - 2 ** 32 if w >= 2 ** 31 else w for w in words], dtype=torch.int32).view(F32)


def test_cast_bf16_rounding_cases_bit_exact():
    """cast_f32_bf16_kernel against torch's cast on a built set: exact ties on both sides of even, one fp32 ulp either side of
    a tie, +-0, +-inf, the largest finite fp32 (-> inf), NaN (stays NaN); with and without out=."""
    ops = _ops()
    pos = [0x3F808000, 0x3F818000, 0x3F807FFF, 0x3F808001, 0x3F817FFF, 0x3F818001, 0x00000000, 0x7F800000, 0x7F7FFFFF,
           0x3F800000, 0x7F7F8000, 0x7F7F7FFF, 0x00808000, 0x00800000]
    x = f32_from_bits(pos + [p | 0x80000000 for p in pos]).cuda()
    want = x.bfloat16()
    got = ops.cast_bf16(x)
    assert got.dtype == BF16 and torch.equal(bits(got), bits(want)), (bits(got).tolist(), bits(want).tolist())
    assert bits(want)[0] == 0x3F80 and bits(want)[1] == 0x3F82 and bool(torch.isinf(want[8]))      # ties to even; overflow to inf
    out = poisoned(x.numel() + 3, dtype=BF16)
    assert ops.cast_bf16(x, out=out).data_ptr() == out.data_ptr()
    assert torch.equal(bits(out[:x.numel()]), bits(want))
    still_poisoned(out[x.numel():], "behind the output")
    nan = f32_from_bits([0x7FC00000, 0xFFC00000, 0x7F800001, 0x7FFFFFFF]).cuda()
    assert bool(torch.isnan(ops.cast_bf16(nan)).all())


def test_cast_bf16_subnormal_inputs():
    """fp32 subnormals: torch's cast (round to nearest even into a bf16 subnormal, or up to the smallest normal) or a zero of
    the same sign (a flushed denormal).  Which one is recorded in the output; on the MI355X: torch's cast."""
    ops = _ops()
    pos = [0x00000001, 0x00008000, 0x00018000, 0x00010000, 0x007FFFFF, 0x007F8000, 0x00400000]
    x = f32_from_bits(pos + [p | 0x80000000 for p in pos]).cuda()
    got, want = bits(ops.cast_bf16(x)), bits(x.bfloat16())
    zero = bits(torch.zeros_like(x).copysign(x).bfloat16())
    print("MEASURED cast_bf16 subnormals:", "torch's cast" if torch.equal(got, want) else "flushed to zero" if torch.equal(got, zero) else "mixed")
    assert bool(((got == want) | (got == zero)).all()), (got.tolist(), want.tolist())


def test_cast_bf16_past_the_first_sweep():
    """n = 4096 * 256 + 77: the grid-stride loop wraps once and leaves a tail of 77."""
    ops = _ops()
    n = SWEEP + 77
    x = (rnd(n, seed=90) * torch.exp(4 * rnd(n, seed=91))).cuda()
    out = poisoned(n + 5, dtype=BF16)
    ops.cast_bf16(x, out=out)
    assert torch.equal(bits(out[:n]), bits(x.bfloat16()))
    still_poisoned(out[n:], "behind the output")


@pytest.mark.parametrize("x_dt,y_dt", [(F32, F32), (F32, BF16), (BF16, F32), (BF16, BF16)])
@pytest.mark.parametrize("rows", [16, 14566])
def test_add_rows_bit_exact(rows, x_dt, y_dt):
    """y[r] = x[r] + table[r % T], T = 5, D = 72: rows = 3 T + 1 (the table wraps, a partial last period), and
    rows = 14566 (= 1 mod T; rows * D > 2^20: past the first sweep).  One fp32 addition and one cast: bit-equal to torch's."""
    ops = _ops()
    T, D = 5, 72
    x = rnd(rows, D, seed=92).to(x_dt).cuda(); table = rnd(T, D, seed=93).cuda()
    assert rows % T == 1 and (rows == 16 or rows * D > SWEEP)
    out = poisoned(rows + 1, D, dtype=y_dt)
    ops.add_rows(x, table, out, rows, T, D)
    want = (x.float().view(-1, D) + table.repeat((rows + T - 1) // T, 1)[:rows]).to(y_dt)
    assert torch.equal(bits(out[:rows]), bits(want))
    still_poisoned(out[rows], "row past the last")


@pytest.mark.parametrize("alpha", [1.0, -0.37])
def test_axpy_is_one_fma(alpha):
    """y += alpha * x, n = 2^20 + 77 (wraps, tail of 77).  The kernel is one fmaf: correctly rounded, so
    |out - exact| <= 2^-24 |exact| + 2^-149 with exact = fp64(fp32(alpha)) * x + y."""
    ops = _ops()
    n = SWEEP + 77
    x, y0 = rnd(n, seed=94).cuda(), rnd(n, seed=95).cuda()
    buf = poisoned(n + 3); buf[:n] = y0
    y = buf[:n]
    ops.axpy(y, x, alpha)
    exact = float(torch.tensor(alpha, dtype=F32).double()) * x.double() + y0.double()
    excess = ((y.double() - exact).abs() - (EPS24 * exact.abs() + 2.0 ** -149)).max()
    report(f"axpy alpha={alpha}: worst |err| - bound", float(excess), 0.0)
    still_poisoned(buf[n:], "behind y")


# scale_exp: expected size (1.5 |ls| + 4) * 2^-24 relative - the product ls * log2(e) rounded in front of the hardware
# exponential (an absolute error of |ls| * 1.44 * 2^-24 in the exponent, relative after it), its 1 ulp, and two multiplications.
# Twice the worst relative error measured on the MI355X against fp64, per log_scale (measured: 0, 1.33e-7, 1.98e-7, 1.79e-7;
# log_scale = 0 is exact: exp(0) = 1 and both values of mul are powers of two).
SCALE_EXP_TOL = {0.0: 0.0, math.log(1 / 0.07): 2.7e-7, math.log(100.0): 4.0e-7, -3.0: 3.6e-7}


@pytest.mark.parametrize("mul", [1.0, 0.5])
@pytest.mark.parametrize("ls", sorted(SCALE_EXP_TOL))
def test_scale_exp(ls, mul):
    """out = x * exp(*log_scale) * mul against fp64, out of place and in place (step.py: out=t), n = 2^20 + 77.
    Measured worst relative error: ls = 0: 0 (exact), ln(1/0.07): 1.33e-7, ln 100: 1.98e-7, -3: 1.79e-7; expected size
    (1.5 |ls| + 4) 2^-24 = 2.4e-7, 4.8e-7, 6.5e-7, 5.1e-7."""
    ops = _ops()
    n = SWEEP + 77
    x = rnd(n, seed=96).cuda()
    lst = torch.tensor([ls], device="cuda")
    exact = x.double() * math.exp(float(lst.double())) * mul
    expected = (1.5 * abs(ls) + 4) * EPS24
    out = poisoned(n + 3)
    assert ops.scale_exp(x, lst, out=out[:n], mul=mul).data_ptr() == out.data_ptr()
    worst = float(((out[:n].double() - exact).abs() / exact.abs().clamp_min(1e-300)).max())
    print(f"scale_exp ls={ls:.4f}: expected size {expected:.2e}")
    report(f"scale_exp ls={ls:.4f} mul={mul} relative", worst, SCALE_EXP_TOL[ls])
    still_poisoned(out[n:], "behind out")
    t = x.clone()
    ops.scale_exp(t, lst, out=t, mul=mul)
    assert torch.equal(bits(t), bits(out[:n]))                   # in place: the same numbers
    fresh = ops.scale_exp(x, lst, mul=mul)
    assert torch.equal(bits(fresh), bits(out[:n]))


def test_clamp_scalar_keeps_nan():
    """logit_scale.clamp_(0, ln 100): below, inside, above, both bounds exactly, +-inf, and NaN - which stays NaN as
    torch.clamp_ keeps it (fminf(fmaxf(NaN, lo), hi) would return lo = 0.0: a diverged run must look diverged)."""
    ops = _ops()
    lo, hi = 0.0, math.log(100.0)
    hi32 = float(torch.tensor(hi, dtype=F32))
    for v in (-1.5, 2.6593, 7.0, lo, hi32, float("inf"), float("-inf"), NAN, -0.0):
        p = torch.tensor([v, 123.0], device="cuda")
        ops.clamp_scalar(p, lo, hi)
        want = torch.tensor([v], dtype=F32).clamp_(lo, hi)
        got = p.cpu()
        if math.isnan(v):
            assert math.isnan(float(got[0])), f"NaN came out as {float(got[0])}"
        else:
            assert float(got[0]) == float(want[0]), (v, float(got[0]), float(want[0]))
        assert float(got[1]) == 123.0


@pytest.mark.parametrize("D", [72, 256])
@pytest.mark.parametrize("form", ["class token", "tokens", "all rows"])
def test_batch_rowsum_call_forms(form, D):
    """out[t] += sum_b x[b * stride + off + t] in the three forms of train.py - (B, 1, D, L, 0) the class-token row,
    (B, T, D, T + 1, 1) the token rows, (B, L, D, L, 0) every row - B = 7, L = 5, accumulating into a non-zero out.
    Bound (a sequential fp32 sum of B + 1 terms): |err| <= (B + 1) 2^-24 (sum_b |x_b| + |out0|) per element."""
    B, L = 7, 5
    T, stride, off = {"class token": (1, L, 0), "tokens": (L - 1, L, 1), "all rows": (L, L, 0)}[form]
    _batch_rowsum_case(B, T, D, stride, off, B * L)


def test_batch_rowsum_past_the_first_sweep():
    """T * D = 4100 * 256 > 2^20 with B = 2: the grid-stride loop wraps."""
    assert 4100 * 256 > SWEEP
    _batch_rowsum_case(2, 4100, 256, 4101, 1, 2 * 4101)


def _batch_rowsum_case(B, T, D, stride, off, xrows):
    ops = _ops()
    x = rnd(xrows, D, seed=97).cuda()
    out0 = rnd(T, D, seed=98).cuda()
    buf = poisoned(T + 1, D); buf[:T] = out0
    ops.batch_rowsum(x, buf, B, T, D, stride, off)
    exact = rows_ref.batch_rowsum(x, out0, B, T, D, stride, off)
    bound = (B + 1) * EPS24 * rows_ref.batch_rowsum_abs(x, out0, B, T, D, stride, off)
    report(f"batch_rowsum B={B} T={T} D={D}: worst |err| / bound", float(((buf[:T].double() - exact).abs() / bound).max()), 1.0)
    still_poisoned(buf[T], "row past the last")


def test_im2col_f32_bit_exact():
    """im2col_kernel<float>: the two cases of test_im2col_token_order_exact and a non-square one (C = 3, 20 x 33, kernel 4 x 6,
    stride 3 x 5, Kp = 80): bit-equal to unfold, zero pad columns."""
    ops = _ops()
    unfold = torch.nn.functional.unfold
    x = (torch.arange(2 * 3 * 28 * 28) % 200 - 100).float().reshape(2, 3, 28, 28)
    cols, gh, gw = ops.im2col_f32(x.cuda(), 14, 14, 14, 14, 640)
    assert cols.dtype == F32 and tuple(cols.shape) == (2 * gh * gw, 640)
    assert torch.equal(cols[:, :588].cpu(), unfold(x, (14, 14), stride=14).transpose(1, 2).reshape(2 * gh * gw, -1))
    assert float(cols[:, 588:].abs().max()) == 0.0
    xs = (torch.arange(2 * 33 * 24) % 120 - 60).float().reshape(2, 33, 24)
    cols, gh, gw = ops.im2col_f32(xs.unsqueeze(1).cuda(), 8, 8, 5, 5, 64, transpose_hw=True)
    assert (gh, gw) == (4, 6)
    assert torch.equal(cols.cpu(), unfold(xs.unsqueeze(1).transpose(2, 3), (8, 8), stride=5).transpose(1, 2).reshape(-1, 64))
    x = rnd(2, 3, 20, 33, seed=99)                                  # random fp32: a copy must keep every bit
    cols, gh, gw = ops.im2col_f32(x.cuda(), 4, 6, 3, 5, 80)
    assert (gh, gw) == (6, 6)
    ref = unfold(x, (4, 6), stride=(3, 5)).transpose(1, 2).reshape(2 * 36, 72)
    assert torch.equal(bits(cols[:, :72].cpu()), bits(ref)) and float(cols[:, 72:].abs().max()) == 0.0


def _gelu_checks(out, ref, first_sweep, wg, what):
    """Per element: the bound of test_gelu_erf_accuracy (half a bf16 ulp + 1e-6); per block (errloc), the part past the first
    sweep split into its whole workgroups and its ragged last one.  Block bound: every element within 2^-8 |ref| + 1e-6, so a
    block's relative 2-norm error is below 2^-8 + 1e-6 sqrt(n_blk) / ||ref_blk|| < 4e-3 on these inputs."""
    n = out.numel()
    report(what + ": worst |err| - (half ulp + 1e-6)", float(((out.double() - ref).abs() - (ref.abs() * 2.0 ** -8 + 1e-6)).max()), 0.0)
    tail0 = first_sweep + (n - first_sweep) // wg * wg
    extra = [("cols", first_sweep, tail0), ("cols", tail0, n)]
    worst, (_, _, c0, c1) = errloc.block_relerr(out[None], ref[None], 1, 1 << 20, extra=extra)
    print(f"MEASURED {what}: worst block cols {c0}:{c1} {worst:.3e}")
    errloc.assert_blocks(out[None], ref[None], 4e-3, 1, 1 << 20, extra=extra, what=what)


def test_gelu_bf16_past_the_first_sweep():
    """gelu_kernel (8 values per thread): n = 4096 * 256 * 8 + 8 * 300 - one wrapped sweep of 300 threads, a whole workgroup
    and a ragged one of 44 - inputs spread over [-8, 8]; n % 8 != 0 is refused."""
    ops = _ops()
    n = SWEEP * 8 + 8 * 300
    u = (torch.rand(n, generator=torch.Generator().manual_seed(5)) * 16 - 8).bfloat16().cuda()
    out = poisoned(n + 8, dtype=BF16)
    ops.gelu_bf16(u, out[:n])
    _gelu_checks(out[:n], torch.nn.functional.gelu(u.double()), SWEEP * 8, 256 * 8, "gelu_bf16")
    still_poisoned(out[n:], "behind the output")
    with pytest.raises(RuntimeError, match="multiple of 8"):
        ops.gelu_bf16(u[:n - 4], out[:n - 4])


def test_geglu_bf16_past_the_first_sweep():
    """geglu_kernel (4 outputs per thread): 1031 x 4072 outputs = 4096 * 256 * 4 + 3928 - a wrapped sweep of 982 threads, three
    whole workgroups and a ragged one; h holds interleaved (a, gate) pairs; n_out % 4 != 0 is refused."""
    ops = _ops()
    rows, n_out = 1031, 4072
    assert rows * n_out > SWEEP * 4
    h = (torch.rand(rows, 2 * n_out, generator=torch.Generator().manual_seed(6)) * 16 - 8).bfloat16().cuda()
    out = poisoned(rows + 1, n_out, dtype=BF16)
    ops.geglu_bf16(h, out[:rows])
    ref = h.double()[:, 0::2] * torch.nn.functional.gelu(h.double()[:, 1::2])
    # the product a * gelu(gate): gelu's 1e-6 absolute error times |a| <= 8 (and its bf16 rounding: 8.1e-6), one fp32 rounding
    o, r = out[:rows].reshape(-1), ref.reshape(-1)
    report("geglu_bf16: worst |err| - (half ulp + 8.1e-6)",
           float(((o.double() - r).abs() - (r.abs() * (2.0 ** -8 + 2.0 ** -23) + 8.1e-6)).max()), 0.0)
    tail0 = SWEEP * 4 + (o.numel() - SWEEP * 4) // 1024 * 1024
    errloc.assert_blocks(o[None], r[None], 4e-3, 1, 1 << 20, extra=[("cols", SWEEP * 4, tail0), ("cols", tail0, o.numel())], what="geglu_bf16")
    still_poisoned(out[rows], "row past the last")
    with pytest.raises(RuntimeError, match="multiple of 4"):
        ops.geglu_bf16(h[:, :2 * 4070], out[:rows, :4070])


# ------------------------------------------------------------------------------------------------ text_embed, l2_normalize
def test_text_embed_clamps_ids_bf16():
    """ids below 0 and >= vocab are clamped into the table; D = 72 (two sweeps of the wave, the second partial), bf16 output:
    one fp32 addition and one cast, bit-equal to torch's."""
    ops = _ops()
    V, D, B, L = 50, 72, 3, 7
    emb, pos = rnd(V, D, seed=22).cuda(), rnd(L, D, seed=23).cuda()
    ids = torch.randint(0, V, (B, L), generator=torch.Generator().manual_seed(1))
    ids[0, 0], ids[1, 3], ids[2, 6], ids[2, 0] = -1, V, V + 1000, -(2 ** 40)
    ids = ids.cuda()
    for dt in (BF16, F32):
        out = poisoned(B * L + 1, D, dtype=dt)
        ops.text_embed(ids, emb, pos, out)
        want = (emb[ids.clamp(0, V - 1)] + pos).reshape(-1, D).to(dt)
        assert torch.equal(bits(out[:B * L]), bits(want))
        still_poisoned(out[B * L], "row past the last")


@pytest.mark.parametrize("D", [24, 1280])
def test_l2_normalize_zero_row(D):
    """An all-zero row: output 0, norm 0, nothing NaN (the eps floor of F.normalize); the other rows against fp64.  Bound: the
    norm is the root of D fma's (D/64 + 8 roundings, halved), then a reciprocal, a maximum and a product: (D/128 + 8) 2^-24."""
    ops = _ops()
    rows = 6
    x = rnd(rows, D, seed=24 + D)
    x[2] = 0.0
    x = x.cuda()
    y, yb, nrm = poisoned(rows + 1, D), poisoned(rows + 1, D, dtype=BF16), poisoned(rows + 1)
    ops.l2_normalize(x, out=y, out_bf16=yb, norms=nrm)
    assert float(y[2].abs().max()) == 0.0 and float(yb[2].float().abs().max()) == 0.0 and float(nrm[2]) == 0.0
    assert bool(torch.isfinite(y[:rows]).all()) and bool(torch.isfinite(nrm[:rows]).all())
    ref = torch.nn.functional.normalize(x.double(), dim=-1)
    tol = (D / 128 + 8) * EPS24
    report(f"l2_normalize D={D} relative", float(((y[:rows].double() - ref).abs() / ref.abs().clamp_min(1e-300))[x != 0].max()), tol)
    report(f"l2_normalize D={D} norms relative", float((nrm[:rows].double() / x.double().norm(dim=-1).clamp_min(1e-300) - 1).abs()[[0, 1, 3, 4, 5]].max()), tol)
    assert torch.equal(bits(yb[:rows]), bits(y[:rows].bfloat16()))
    for t in (y, yb, nrm):
        still_poisoned(t[rows:], "past the last row")
