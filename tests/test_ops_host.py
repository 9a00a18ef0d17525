"""CPU: host-side decisions of `vitlens_hip.ops` that need no GPU - the k-slice choice of the token-major weight-gradient GEMM
(`tn_splits`) against the preconditions its C entry point enforces (vl_gemm.hip: every slice >= 4 steps of 64 tokens), and
the library symbols `weight_grad` enqueues on each of its routes (recorded on CPU tensors, tests/launch_trace.py)."""
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "vit-lens_amd"))


def _c_side_accepts(nk, splits):
    ln = (nk + splits - 1) // splits
    eff = (nk + ln - 1) // ln
    return ln >= 4 and nk - (eff - 1) * ln >= 4 and eff <= splits


def test_tn_split_choice_is_accepted_by_the_kernel_and_fills_the_chip():
    from vitlens_hip.ops import tn_splits
    # the C3 micro-batch (257 * 256 tokens = 1028 steps): c_fc / c_proj 64 tiles, in_proj 48, out_proj 16
    assert tn_splits(1028, 64) == 4 and tn_splits(1028, 48) == 4 and tn_splits(1028, 16) == 16
    assert tn_splits(1028, 256) == 1                       # enough tiles: no split
    assert tn_splits(64, 16) == 0                          # 16 tiles would need 16 slices of 4 steps: below the 16-step floor
    assert tn_splits(20, 1024) == 1 and tn_splits(15, 1024) == 0
    for nk in range(1, 1400, 7):
        for tiles in (1, 3, 12, 16, 48, 64, 100, 192, 256, 1024):
            s = tn_splits(nk, tiles)
            if s:
                assert s in (1, 2, 4, 8, 16) and tiles * s >= 192 and nk // s >= 16
                assert _c_side_accepts(nk, s), (nk, tiles, s)
                smaller = [q for q in (1, 2, 4, 8, 16) if q < s and tiles * q >= 192 and nk // q >= 16 and _c_side_accepts(nk, q)]
                assert not smaller, (nk, tiles, s, smaller)


def _weight_grad_launches(R, M, N, dy_dtype, narrow, bias=True):
    import torch
    from launch_trace import recording
    from vitlens_hip import ops
    dy = torch.empty(R, M, dtype=dy_dtype); x = torch.empty(R, N, dtype=torch.bfloat16)
    g = torch.empty(M, N); gb = torch.empty(M) if bias else None
    with recording() as trace:
        assert ops.weight_grad(dy, x, g, bias_grad=gb, narrow=narrow) is g
    return trace


TN, NT_SPLITK, NT_GEMM = "vl_gemm_tn_splitk_accum_f32", "vl_gemm_splitk_accum_f32", "vl_gemm_bf16_ex"
FUSED, TRANSPOSE, COLSUM = "vl_transpose_colsum_bf16", "vl_transpose_to_bf16", "vl_colsum"


@pytest.mark.parametrize("route,R,M,N,narrow,want", [
    ("whole tiles", 4096, 1024, 3072, False, [TN, COLSUM]),
    ("whole tiles", 4096, 1024, 3072, True, [TN, COLSUM]),
    ("narrow, padded path", 4096, 64, 1024, True, [TN, COLSUM]),
    ("narrow, narrow=False", 4096, 64, 1024, False, [FUSED, TRANSPOSE, NT_SPLITK]),
    ("few work items", 4096, 1024, 1024, False, [FUSED, TRANSPOSE, NT_SPLITK]),      # 16 tiles x 4 slices < 192: refused by gemm_dw_tn
    ("few work items, narrow=True", 4096, 1024, 1024, True, [TN, COLSUM]),           # gemm_dw_tn_any: few_tiles_ok slices
    ("rows % 64 != 0, fused transpose", 771, 256, 512, True, [FUSED, TRANSPOSE, NT_GEMM]),
    ("rows % 64 != 0, fused transpose", 771, 256, 512, False, [FUSED, TRANSPOSE, NT_GEMM]),
    ("rows < 256: separate transpose and colsum", 200, 256, 512, True, [TRANSPOSE, COLSUM, TRANSPOSE, NT_GEMM]),
])
def test_weight_grad_routes(route, R, M, N, narrow, want):
    """The library symbols `ops.weight_grad` enqueues for bf16 operands, route by route (recorded on CPU tensors)."""
    import torch
    from launch_trace import symbols
    trace = _weight_grad_launches(R, M, N, torch.bfloat16, narrow)
    assert symbols(trace) == want, route
    if want[0] == TN:
        name, args = trace[0]
        Mp, Np = (M + 255) // 256 * 256, (N + 255) // 256 * 256
        assert args[3:6] == (Mp, Np, R), route                       # whole 256-column tiles, the token count as given
        assert args[1].t.shape[1] == Np and args[0].t.shape[1] == Mp
    if want[0] == FUSED:
        assert trace[0][1][7] is not None                            # the fused transpose receives the bias gradient


@pytest.mark.parametrize("R,M,N", [(4096, 1024, 3072), (4096, 64, 1024), (4096, 1024, 1024), (771, 256, 512), (200, 256, 512)])
@pytest.mark.parametrize("narrow", [True, False])
def test_weight_grad_fp32_dy_takes_the_transposing_path_and_sums_dy_as_given(R, M, N, narrow):
    """An fp32 dy never fits the token-major kernel.  Its bias gradient is the column sums of the fp32 values on every route
    and at every row count: `vl_colsum` on dy itself, and the transpose (fused where the shape fits, R >= 256) gets no
    column-sum destination - it would sum the bf16-rounded copies."""
    import torch
    from launch_trace import symbols
    trace = _weight_grad_launches(R, M, N, torch.float32, narrow)
    names = symbols(trace)
    assert TN not in names and names[0] == COLSUM and names.count(COLSUM) == 1
    assert trace[0][1][1] == 0 and trace[0][1][0].t.dtype == torch.float32          # VL_F32 operand: dy as given
    assert names[1] in (FUSED, TRANSPOSE) and names[2] == TRANSPOSE and names[3] in (NT_SPLITK, NT_GEMM) and len(names) == 4
    assert names[1] == (FUSED if R >= 256 else TRANSPOSE)
    if names[1] == FUSED:
        assert trace[1][1][7] is None
    # without a bias gradient: no column sum at all
    assert COLSUM not in symbols(_weight_grad_launches(R, M, N, torch.float32, narrow, bias=False))
