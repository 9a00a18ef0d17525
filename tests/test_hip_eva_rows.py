"""GPU: the row-wise kernels at the EVA ViT-g geometry - `assemble_tokens` ([cls ; tokens] + pos with no LayerNorm behind it,
csrc/vl_rows.hip) and the D = 1408 register forms of the LayerNorm forward and backward (five 256-element chunks and a half
chunk in lanes 0-31; csrc/vl_rows.hip, csrc/vl_bwd.hip) - against the fp64 references of tests/rows_ref.py.

The helpers, the poisoned surplus and the bounds are those of tests/test_hip_rows.py (TOL_LN_FWD, TOL_LN_BWD, stat_bounds,
check_out): nothing here is wider, on any row - the rows of `rows_ref.ill_conditioned_rows` (offset 1000 with sigma 4, offset
40 with sigma 1.5, one constant row) planted among 258 ordinary ones included.  The register form holds TOL_LN_FWD on them
because it takes the mean of the deviations off again (csrc/vl_rows.hip); a form that subtracts a rounded fp32 mean and stops
cannot: at offset 1000 half an fp32 ulp of the mean is 3e-5, 7.6e-6 of sigma, and the first GPU run of this file measured
2.3e-7 on an ORDINARY row with |mean| = 4.1 sigma.  The backward reads the saved mean and forms x - mean exactly on such rows
(Sterbenz), so it holds TOL_LN_BWD as it is.

One bound is derived here because that file has no case of the kind: `assemble_tokens` is two fp32 additions,
(token + pos) + pos2, each within 2^-24 of its own result, so every element is within 2 * 2^-24 * (|token| + |pos| + |pos2|)
of the fp64 sum (one addition less without pos2); a bf16 output adds half a bf16 ulp of that value.  The fp32 result is also
compared bit for bit with the same two additions done by torch."""
import pytest
import torch

import rows_ref
from test_hip_rows import (BF16, EPS24, F16, F32, HALF_ULP, TOL_LN_BWD, TOL_LN_FWD, _ops, bits, check_out, check_stats, ln_params,
                           poisoned, report, rnd, rows_like_activations, stat_bounds, still_poisoned)

pytestmark = pytest.mark.gpu

D_EVA = 1408


# ------------------------------------------------------------------------------------------------ assemble_tokens
def _assemble_case(B, T, D, tok_dt, out_dt, with_pos2, tok_off=0, out_off=0, pos_off=0):
    """ops.assemble_tokens with the tokens, the output and the position table `*_off` elements into their allocations."""
    ops = _ops()
    R = B * (T + 1)
    tbuf = torch.zeros(B * T * D + tok_off + 8, dtype=tok_dt)
    tbuf[tok_off:tok_off + B * T * D] = rnd(B * T * D, seed=140 + D).to(tok_dt)
    tok = tbuf.cuda()[tok_off:tok_off + B * T * D].view(B, T, D)
    cls = rnd(D, seed=141).cuda()
    pbuf = torch.zeros((T + 1) * D + pos_off + 8); pbuf[pos_off:pos_off + (T + 1) * D] = rnd((T + 1) * D, seed=142)
    pos = pbuf.cuda()[pos_off:pos_off + (T + 1) * D].view(T + 1, D)
    pos2 = rnd(T, D, seed=143).cuda() if with_pos2 else None
    ybuf = poisoned((R + 1) * D + out_off + 8, dtype=out_dt)
    y = ybuf[out_off:out_off + (R + 1) * D].view(R + 1, D)
    xpre = poisoned(R + 1, D)
    ops.assemble_tokens(tok, cls, pos, pos2, y[:R], B, T, D, xpre=xpre[:R])
    what = f"assemble_tokens B={B} T={T} D={D} {tok_dt} -> {out_dt} pos2={with_pos2} offsets tok+{tok_off} out+{out_off} pos+{pos_off}"
    ref = rows_ref.assemble(tok, cls, pos, pos2)
    mag = rows_ref.assemble(tok.abs(), cls.abs(), pos.abs(), None if pos2 is None else pos2.abs())
    b32 = (2 if with_pos2 else 1) * EPS24 * mag + 1e-300
    report(what + " xpre |err| / bound", float(((xpre[:R].double() - ref).abs() / b32).max()), 1.0)
    if out_dt == F32:
        report(what + " |err| / bound", float(((y[:R].double() - ref).abs() / b32).max()), 1.0)
    else:
        h = HALF_ULP[out_dt]
        report(what + " |err| / bound", float(((y[:R].double() - ref).abs() / (h * (ref.abs() + b32) + b32)).max()), 1.0)
    same = rows_ref.assemble_f32(tok, cls, pos, pos2)
    assert torch.equal(bits(xpre[:R]), bits(same)), what + ": xpre is not (token + pos) + pos2 in fp32"
    assert torch.equal(bits(y[:R]), bits(same.to(out_dt))), what + ": out is not the rounded fp32 sum"
    still_poisoned(y[R], "row past the last"); still_poisoned(xpre[R], "xpre: row past the last")
    still_poisoned(ybuf[:out_off], "before the output"); still_poisoned(ybuf[out_off + (R + 1) * D:], "behind the output")


@pytest.mark.parametrize("tok_dt", [BF16, F32])
@pytest.mark.parametrize("B,T,D", [(2, 16, 1408), (3, 5, 176), (2, 16, 1024)])
def test_assemble_tokens(B, T, D, tok_dt):
    """The 8 / 16-byte form at D = 1408 (5.5 sweeps of the wave), 176 (less than one sweep: lanes 44-63 idle) and 1024; f32 and
    bf16 output, with and without pos2; 34 / 18 rows = a partial last workgroup."""
    for out_dt in (F32, BF16):
        for with_pos2 in (False, True):
            _assemble_case(B, T, D, tok_dt, out_dt, with_pos2)


@pytest.mark.parametrize("which", ["tokens", "out", "pos"])
def test_assemble_tokens_misaligned_base_takes_the_generic_form(which):
    """D = 1408 with the tokens, the output or the position table one element into its allocation: no row of that operand is
    on an 8 / 16-byte boundary, the launch must pick the one-element form, and the result is the same."""
    off = {"tokens": (1, 0, 0), "out": (0, 1, 0), "pos": (0, 0, 1)}[which]
    for tok_dt, out_dt in ((BF16, BF16), (F32, F32), (BF16, F32)):
        _assemble_case(2, 16, D_EVA, tok_dt, out_dt, True, *off)


def test_assemble_tokens_refusals():
    ops = _ops()
    D = 176
    tok, cls, pos = torch.zeros(2, 3, D, device="cuda"), torch.zeros(D, device="cuda"), torch.zeros(4, D, device="cuda")
    with pytest.raises(ValueError, match="f32 or bf16"):
        ops.assemble_tokens(tok.half(), cls, pos, None, torch.zeros(8, D, device="cuda"), 2, 3, D)
    with pytest.raises(ValueError, match="do not fit"):
        ops.assemble_tokens(tok, cls, pos[:3], None, torch.zeros(8, D, device="cuda"), 2, 3, D)


# ------------------------------------------------------------------------------------------------ LayerNorm at D = 1408
def planted_rows(rows, D, dtype):
    """rows_like_activations with rows_ref.ill_conditioned_rows (resized to D) planted from row 8 on when there is room:
    returns (x, index tensor of the planted rows)."""
    x = rows_like_activations(rows, D, 100 + D + rows, dtype)
    if rows < 32:
        return x, torch.zeros(0, dtype=torch.long)
    far, near, const = rows_ref.ill_conditioned_rows(D)
    x[8:12], x[20:24], x[30:31] = far.to(dtype), near.to(dtype), const.to(dtype)
    return x, torch.tensor(list(range(8, 12)) + list(range(20, 24)) + [30])


def _ln_forward_1408(rows, in_dt, out_dt, eps, xs=None, ys=None, x_off=0, y_off=0, D=D_EVA, what=""):
    ops = _ops()
    xs, ys = xs or D, ys or D
    x, planted = planted_rows(rows, D, in_dt)
    xbuf = torch.zeros(rows * xs + x_off + 8, dtype=in_dt)
    xbuf[x_off:x_off + rows * xs].view(rows, xs)[:, :D] = x
    xbuf = xbuf.cuda()
    xg = xbuf[x_off:x_off + rows * xs].view(rows, xs)
    w, b = ln_params(D, 7)
    ybuf = poisoned((rows + 1) * ys + y_off + 8, dtype=out_dt)
    y = ybuf[y_off:y_off + (rows + 1) * ys].view(rows + 1, ys)
    mean, rstd = poisoned(rows + 1), poisoned(rows + 1)
    ops.layernorm(xg, w, b, y[:, :D], rows, D, x_row_stride=xs, mean=mean, rstd=rstd, eps=eps)
    what = f"layernorm {what} D={D} rows={rows} eps={eps:g} {in_dt}->{out_dt}"
    ref, mu, rs = rows_ref.layernorm_fwd(xg[:, :D], w, b, eps)
    check_out(y[:rows, :D], ref, TOL_LN_FWD, what)
    check_stats(mean[:rows], rstd[:rows], xg[:, :D], what, eps=eps)
    still_poisoned(y[rows], "row past the last")
    still_poisoned(ybuf[:y_off], "before the output"); still_poisoned(ybuf[y_off + (rows + 1) * ys:], "behind the output")
    if ys > D:
        still_poisoned(y[:, D:], "columns between the rows")
    still_poisoned(mean[rows:], "mean"); still_poisoned(rstd[rows:], "rstd")
    return y[:rows, :D], rstd[:rows], planted


@pytest.mark.parametrize("eps", [1e-6, 1e-5])
@pytest.mark.parametrize("rows", [1, 4, 7, 258])
def test_layernorm_forward_1408(rows, eps):
    """ln_rows_kernel<5, ..., HALF>: one wave, one full workgroup, a second workgroup of three waves, and 258 rows (a last
    workgroup of two waves) with the ill-conditioned rows planted; the five dtype pairs; both eps values."""
    for in_dt, out_dt in [(F32, F32), (F32, BF16), (F32, F16), (BF16, F32), (BF16, BF16)]:
        _ln_forward_1408(rows, in_dt, out_dt, eps)


def test_layernorm_forward_1408_reads_eps():
    """The constant row (variance exactly 0) has rstd = eps^-1/2: 1000 at 1e-6, 316.2 at 1e-5 - a kernel that dropped its eps
    argument fails check_stats' rstd bound (3.4e-6 relative) by five orders of magnitude on one of the two."""
    for eps in (1e-6, 1e-5):
        _, rstd, planted = _ln_forward_1408(258, BF16, F32, eps)
        assert float(rstd[planted[-1]]) == pytest.approx(eps ** -0.5, rel=stat_bounds(D_EVA))


@pytest.mark.parametrize("in_dt", [F32, BF16])
def test_layernorm_forward_1408_strides_and_unaligned_bases(in_dt):
    """Rows D + 4 / D + 8 apart keep the register form; D + 2 apart, or a base one element into the allocation, must take the
    any-D form (ln_launch's alignment predicate) - all must be right, and nothing outside the rows is written."""
    for xs, ys, xo, yo in [(1412, 1408, 0, 0), (1408, 1416, 0, 0), (1412, 1416, 0, 0), (1410, 1408, 0, 0), (1408, 1410, 0, 0),
                           (1408, 1408, 1, 0), (1408, 1408, 0, 1), (1412, 1412, 1, 1)]:
        for out_dt in (F32, BF16):
            _ln_forward_1408(7, in_dt, out_dt, 1e-6, xs=xs, ys=ys, x_off=xo, y_off=yo, what=f"xs={xs} ys={ys} x+{xo} y+{yo}")


def test_layernorm_forward_1408_row_index_and_pooling():
    """The class-token pooling (x_row_stride = L * D) and the row gather on a bf16 stream of width 1408."""
    ops = _ops()
    B, L, D = 5, 9, D_EVA
    x = rows_like_activations(B * L, D, 31, BF16).cuda()
    w, b = ln_params(D, 9)
    idx = torch.tensor([3, 0, 8, 5, 1], device="cuda")
    y, mean, rstd = poisoned(B + 1, D), poisoned(B + 1), poisoned(B + 1)
    ops.layernorm(x, w, b, y, B, D, x_row_stride=D, row_index=idx, row_mul=L, mean=mean, rstd=rstd, eps=1e-6)
    src = x.view(B, L, D)[torch.arange(B, device="cuda"), idx]
    check_out(y[:B], rows_ref.layernorm_fwd(src, w, b, 1e-6)[0], TOL_LN_FWD, "gather D=1408")
    check_stats(mean[:B], rstd[:B], src, "gather D=1408", eps=1e-6)
    still_poisoned(y[B], "row past the last")
    y = poisoned(B + 1, D)
    ops.layernorm(x, w, b, y, B, D, x_row_stride=L * D, eps=1e-6)
    check_out(y[:B], rows_ref.layernorm_fwd(x.view(B, L, D)[:, 0], w, b, 1e-6)[0], TOL_LN_FWD, "pooling D=1408")
    still_poisoned(y[B], "row past the last")


def _ln_backward_1408(rows, dy_dt, x_dt, g_dt, eps, dres="dense", want_dxb=False, xs=None, dys=None, dxs=None, dx_off=0, D=D_EVA,
                      what=""):
    ops = _ops()
    xs, dys, dxs = xs or D, dys or D, dxs or D
    xf = torch.zeros(rows, xs, dtype=x_dt); xf[:, :D] = planted_rows(rows, D, x_dt)[0]
    dyf = torch.zeros(rows, dys, dtype=dy_dt); dyf[:, :D] = rnd(rows, D, seed=71 + D).to(dy_dt)
    xf, dyf = xf.cuda(), dyf.cuda()
    x, dy = xf[:, :D], dyf[:, :D]
    w, _ = ln_params(D, 72)
    mu, rs = rows_ref.row_stats(x, eps)
    mean, rstd = mu.float(), rs.float()                       # what a forward saved: the reference reads the same fp32 values
    dres_vals = rnd(rows, D, seed=73 + D).to(g_dt).cuda() if dres else None
    buf = poisoned((rows + 1) * dxs + dx_off + 8, dtype=g_dt)
    dx = buf[dx_off:dx_off + (rows + 1) * dxs].view(rows + 1, dxs)
    dres_t = None
    if dres == "inplace":
        dx[:rows, :D] = dres_vals
        dres_t = dx
    elif dres == "dense":
        dres_t = torch.zeros(rows, dxs, dtype=g_dt, device="cuda"); dres_t[:, :D] = dres_vals
    dxb = poisoned(rows + 1, dxs, dtype=BF16) if want_dxb and dx_off == 0 else None
    ops.layernorm_bwd(dyf, xf, mean, rstd, w, rows, D, dres=dres_t, dx=dx, dx_bf16=dxb, x_row_stride=xs, dy_row_stride=dys,
                      dx_row_stride=dxs)
    ref = rows_ref.layernorm_bwd(dy, x, mean, rstd, w, dres_vals)
    what = f"layernorm_bwd {what} D={D} rows={rows} eps={eps:g} ({dy_dt}, {x_dt}, {g_dt}) dres={dres}"
    for out, name in ((dx, "dx"), (dxb, "dx_bf16")):
        if out is None:
            continue
        check_out(out[:rows, :D], ref, TOL_LN_BWD, f"{what} {name}")
        still_poisoned(out[rows], name + ": row past the last")
        if dxs > D:
            still_poisoned(out[:, D:], name + ": columns between the rows")
    still_poisoned(buf[:dx_off], "before dx")


@pytest.mark.parametrize("eps", [1e-6, 1e-5])
@pytest.mark.parametrize("rows", [1, 4, 7, 258])
def test_layernorm_bwd_1408(rows, eps):
    """ln_bwd_kernel<5, ..., HALF>: the eight (dy, x, gradient-stream) combinations at the four row counts, the statistics of
    either eps, the ill-conditioned rows planted at 258 rows."""
    for dy_dt in (F32, BF16):
        for x_dt in (F32, BF16):
            for g_dt in (F32, BF16):
                _ln_backward_1408(rows, dy_dt, x_dt, g_dt, eps)


@pytest.mark.parametrize("g_dt", [F32, BF16])
def test_layernorm_bwd_1408_call_forms_strides_and_unaligned_operands(g_dt):
    """In place, dx + dx_bf16, no dres; x_row_stride = 3 D (the pooled-row call), strides D + 8 (register form), a stride of
    D + 2 on each operand in turn and a dx one element into its allocation (any-D form)."""
    dts = (BF16, BF16, g_dt)
    _ln_backward_1408(7, *dts, 1e-6, dres="inplace", what="in place")
    _ln_backward_1408(7, *dts, 1e-6, dres="dense", want_dxb=True, what="dx + dx_bf16")
    _ln_backward_1408(7, *dts, 1e-6, dres=None, what="no dres")
    _ln_backward_1408(7, *dts, 1e-6, xs=3 * D_EVA, what="xs=3D")
    _ln_backward_1408(7, *dts, 1e-6, dys=D_EVA + 8, dxs=D_EVA + 8, want_dxb=True, what="dys=dxs=D+8")
    _ln_backward_1408(7, *dts, 1e-6, xs=D_EVA + 2, what="xs=D+2")
    _ln_backward_1408(7, *dts, 1e-6, dys=D_EVA + 2, what="dys=D+2")
    _ln_backward_1408(7, *dts, 1e-6, dxs=D_EVA + 2, want_dxb=True, what="dxs=D+2")
    _ln_backward_1408(7, *dts, 1e-6, dx_off=1, what="dx+1")


@pytest.mark.parametrize("g_dt", [F32, BF16])
def test_layernorm_bwd_1408_sparse_res(g_dt):
    """dres_every = 257 at width 1408 (the class-token rows behind a pruned last block): row i * 257 adds row i of a dres whose
    row stride is D + 4, every other row is bit-equal to the dense call without dres; a dres stride of D + 1 takes the any-D form."""
    ops = _ops()
    B, L, D = 2, 257, D_EVA
    rows = B * L - 2
    x = rows_like_activations(rows, D, 80 + D, BF16).cuda()
    dy = rnd(rows, D, seed=81 + D).bfloat16().cuda()
    w, _ = ln_params(D, 82)
    mu, rs = rows_ref.row_stats(x, 1e-6)
    mean, rstd = mu.float(), rs.float()
    for stride in (D + 4, D + 1):
        dres = rnd(B, stride, seed=83, shift=3.0).to(g_dt).cuda()[:, :D]
        dx = poisoned(rows + 1, D, dtype=g_dt)
        ops.layernorm_bwd_sparse_res(dy, x, mean, rstd, w, rows, D, dres, L, dx)
        what = f"sparse D=1408 {g_dt} dres stride {stride}"
        check_out(dx[:rows], rows_ref.layernorm_bwd_sparse(dy, x, mean, rstd, w, dres, L), TOL_LN_BWD, what)
        still_poisoned(dx[rows], "row past the last")
        if stride % 4 == 0:
            plain = poisoned(rows, D, dtype=g_dt)
            ops.layernorm_bwd(dy, x, mean, rstd, w, rows, D, dx=plain)
            none = torch.arange(rows, device="cuda") % L != 0
            assert torch.equal(bits(dx[:rows][none]), bits(plain[none])), what + ": rows without a residual gradient"
