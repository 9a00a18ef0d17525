"""Single-query attention (vl_attn_fwd_q1 / vl_attn_bwd_q1 through ops.attn_fwd_q1 / ops.attn_bwd_q1) against float64 on the
kernels' own bf16 operands, per (b, h) block, and against the dense kernels' row.

Operands are the column blocks of one packed [tokens, 3*width] matrix, as the towers hold them.  The measures and the bounds are
the dense kernels' own: the forward's attn_fwd_ref / TOL_OUT / lse tolerance of test_hip_attn_fwd.py, the backward's
_attn_bwd_reference and the one-query-against-many-keys bound TOL_BLK_CROSS of test_hip_train.py (its dense counterpart for
self-attention of the bench geometry: TOL_BLK_BENCH).  Agreement with the dense kernels is asked within the sum of both bounds.
"""
import pytest
import torch

import attn_ref as A

BF16 = torch.bfloat16
# (B, H, L, query row): bench geometry; several batches / heads; a single key; L no multiple of any lane count; the upper
# bound of the kernels; a query row that is not row 0
CASES = [(1, 1, 257, 0), (2, 3, 257, 0), (2, 2, 1, 0), (1, 2, 50, 0), (1, 1, 1024, 0), (2, 3, 257, 256)]


def test_binding_signatures_match_the_header_parameter_counts():
    """Host: the ctypes tables of the two entries (and of the sparse-residual LayerNorm backward) have one type per parameter
    of the header's declaration."""
    import os
    import re
    from vitlens_hip import _lib
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "vitlens_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in ("vl_attn_fwd_q1", "vl_attn_bwd_q1", "vl_layernorm_bwd_sres"):
        params = re.search(name + r"\s*\(([^;]*?)\)\s*;", hdr, flags=re.S).group(1)
        assert len(params.split(",")) == len(_lib.SIGNATURES[name]), name


def _inputs(B, H, L, seed):
    from vitlens_hip import ops
    g = torch.Generator().manual_seed(seed)
    inner = H * 64
    qkv = torch.randn(B * L, 3 * inner, generator=g).bfloat16().cuda()
    q, k, v = (ops.heads_view(qkv, B, L, H, 64, i * inner) for i in range(3))
    dO = torch.randn(B, inner, generator=g).bfloat16().cuda()
    return q, k, v, dO, 64 ** -0.5 * ops.LOG2E, 64 ** -0.5


def _fwd(q, k, v, qrow, qscale):
    from vitlens_hip import ops
    B, H, L, _ = q.shape
    out = torch.full((B, H * 64), float("nan"), dtype=BF16, device="cuda")
    lse = torch.full((B, H), float("nan"), device="cuda")
    ops.attn_fwd_q1(q, k, v, out, lse=lse, qrow=qrow, qscale=qscale)
    return out, lse


def _rows4(x, B, H):
    """[B, H*64] -> [B, H, 1, 64]"""
    return x.reshape(B, H, 1, 64)


@pytest.mark.gpu
@pytest.mark.parametrize("B,H,L,qrow", CASES)
def test_attn_fwd_q1_vs_fp64_and_dense_row(B, H, L, qrow):
    import test_hip_attn_fwd as F
    from errloc import attn_block_relerr
    from vitlens_hip import ops
    q, k, v, _, qscale, _ = _inputs(B, H, L, seed=1000 * L + qrow + H)
    out, lse = _fwd(q, k, v, qrow, qscale)
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(lse).all())
    out2, lse2 = _fwd(q, k, v, qrow, qscale)
    assert torch.equal(out.view(torch.int16), out2.view(torch.int16)) and torch.equal(lse, lse2), "a second launch differs"
    ref, ref_lse = A.attn_fwd_ref(q, k, v, qscale, False, BF16)
    ref, ref_lse = ref[:, :, qrow:qrow + 1], ref_lse[:, :, qrow]
    tol = F.TOL_OUT[BF16]
    blk, (wb, wh, _, _) = attn_block_relerr(_rows4(out, B, H), ref, B, H, 1, tile=1)
    lse_err = float((lse.double() - ref_lse).abs().max())
    lse_tol = max(F.LSE_FACTOR * F.MODEL_LSE[(BF16, "normal")], F._ulps(float(ref_lse.abs().max())))
    # the dense kernel's row
    dense = torch.empty(B * L, H * 64, dtype=BF16, device="cuda")
    dlse = torch.empty(B, H, L, device="cuda")
    ops.attn_fwd(q, k, v, dense, lse=dlse, qscale=qscale)
    drow = dense.view(B, L, H * 64)[:, qrow]
    dblk, _ = attn_block_relerr(_rows4(out, B, H), _rows4(drow, B, H).double(), B, H, 1, tile=1)
    dlse_err = float((lse - dlse[:, :, qrow]).abs().max())
    print(f"ATTNQ1 fwd blk {blk:.3e} tol {tol:.2e} lse {lse_err:.3e} tol {lse_tol:.2e} vs dense {dblk:.3e} lse {dlse_err:.3e}")
    assert blk <= tol, f"out: b={wb} h={wh} has relative error {blk:.3e} > {tol:.1e}"
    assert lse_err <= lse_tol, (lse_err, lse_tol)
    assert dblk <= 2 * tol and dlse_err <= 2 * lse_tol, (dblk, dlse_err)


@pytest.mark.gpu
@pytest.mark.parametrize("B,H,L,qrow", CASES)
def test_attn_bwd_q1_vs_fp64_and_dense(B, H, L, qrow):
    import test_hip_train as T
    from errloc import assert_attn_blocks, attn_block_relerr
    from vitlens_hip import ops
    inner = H * 64
    q, k, v, dO, qscale, scale = _inputs(B, H, L, seed=1000 * L + qrow + H)
    o, lse = _fwd(q, k, v, qrow, qscale)
    dqkv = torch.full((B * L, 3 * inner), float("nan"), dtype=BF16, device="cuda")
    ops.attn_bwd_q1(q, k, v, dO, o, lse, dqkv, dqkv[:, inner:], dqkv[:, 2 * inner:], 3 * inner, 3 * inner, qrow=qrow)
    assert bool(torch.isfinite(dqkv).all()), "a gradient row was left unwritten or is not finite"
    dq, dk, dv = dqkv[:, :inner], dqkv[:, inner:2 * inner], dqkv[:, 2 * inner:]
    # every other token's dQ row is exactly zero
    other = torch.ones(B, L, dtype=torch.bool, device="cuda")
    other[:, qrow] = False
    assert float(dq.reshape(B, L, inner)[other].float().abs().max()) == 0.0 if L > 1 else True
    # float64 reference: the dense backward's, with dO (and the forward's o) on the query row only
    dO_full = torch.zeros(B, H, L, 64, dtype=BF16, device="cuda")
    dO_full[:, :, qrow] = dO.view(B, H, 64)
    o_full = torch.zeros(B * L, inner, dtype=BF16, device="cuda")
    o_full.view(B, L, inner)[:, qrow] = o
    _, rq, rk, rv = T._attn_bwd_reference(q, k, v, dO_full, qscale, scale, False, o_full)
    tol = T.TOL_BLK_CROSS
    dq_row = _rows4(dq.reshape(B, L, inner)[:, qrow], B, H)
    dv_max = float(dv.float().abs().max())
    errs = {}
    if float(rq.abs().max()) < 1e-9:            # a single key: dS = P (dP - delta) = 0 in exact arithmetic
        assert float(dq.float().abs().max()) <= 1e-2 * dv_max and float(dk.float().abs().max()) <= 1e-2 * dv_max
    else:
        errs["dq"], _ = attn_block_relerr(dq_row, rq[:, :, qrow:qrow + 1], B, H, 1, tile=1)
        errs["dk"] = assert_attn_blocks(dk, rk, tol, B, H, L, "keys", what="dk")
        errs["dk_last"], _ = attn_block_relerr(_rows4(dk.reshape(B, L, inner)[:, L - 1], B, H), rk[:, :, L - 1:], B, H, 1, tile=1)
    errs["dv"] = assert_attn_blocks(dv, rv, tol, B, H, L, "keys", what="dv")
    errs["dv_last"], _ = attn_block_relerr(_rows4(dv.reshape(B, L, inner)[:, L - 1], B, H), rv[:, :, L - 1:], B, H, 1, tile=1)
    # the dense backward on the same (one-row) dO, its own forward's o and lse
    dense_o = torch.empty(B * L, inner, dtype=BF16, device="cuda")
    dense_lse = torch.empty(B, H, L, device="cuda")
    ops.attn_fwd(q, k, v, dense_o, lse=dense_lse, qscale=qscale)
    dO_tok = dO_full.permute(0, 2, 1, 3).reshape(B * L, inner).contiguous()
    dd = torch.full((B * L, 3 * inner), float("nan"), dtype=BF16, device="cuda")
    ops.attn_bwd(q, k, v, ops.heads_view(dO_tok, B, L, H, 64), ops.heads_view(dense_o, B, L, H, 64), dense_lse,
                 torch.empty(B, H, L, device="cuda"), dd, dd[:, inner:], dd[:, 2 * inner:], 3 * inner, 3 * inner)
    both = tol + T.TOL_BLK_BENCH
    heads = lambda t: t.reshape(B, L, H, 64).permute(0, 2, 1, 3).double()
    dense_errs = {}
    for name, a, b in (("dq", dq, dd[:, :inner]), ("dk", dk, dd[:, inner:2 * inner]), ("dv", dv, dd[:, 2 * inner:])):
        if float(b.float().abs().max()) < 1e-2 * dv_max and name != "dv":
            continue                                       # (the single key: both are rounding noise around zero)
        dense_errs[name] = assert_attn_blocks(a, heads(b), both, B, H, L, "rows", what=name + " vs dense")
    print("ATTNQ1 bwd " + " ".join(f"{k} {e:.3e}" for k, e in errs.items()) + f" tol {tol:.1e} | vs dense "
          + " ".join(f"{k} {e:.3e}" for k, e in dense_errs.items()) + f" tol {both:.1e}")
    for name, e in errs.items():
        assert e <= tol, (name, e, tol)


@pytest.mark.gpu
def test_q1_entries_refuse_what_they_do_not_take():
    from vitlens_hip import ops
    hv = lambda L, dh, H=2: ops.heads_view(torch.zeros(2 * L, 3 * H * dh, dtype=BF16, device="cuda"), 2, L, H, dh)
    out = torch.full((2, 128), float("nan"), dtype=BF16, device="cuda")
    for view, qrow in ((hv(1025, 64), 0), (hv(50, 64), 50), (hv(50, 64), -1)):
        with pytest.raises(RuntimeError):
            ops.attn_fwd_q1(view, view, view, out, qrow=qrow)
    with pytest.raises((RuntimeError, ValueError)):
        v80 = hv(50, 80)
        ops.attn_fwd_q1(v80, v80, v80, torch.empty(2, 160, dtype=BF16, device="cuda"))
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()), "a refused call wrote to out"
