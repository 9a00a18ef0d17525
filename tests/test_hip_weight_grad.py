"""GPU: `ops.weight_grad` on every route (tests/test_ops_host.py names the library symbols of each): g += dy^T x and
bias_grad += the column sums of dy, accumulated into buffers that already hold values, against fp64 on the operands as given.
Bounds: those of tests/test_hip_gemm_tn.py - 2e-6 on the whole gradient, 5e-7 per 64 x 64 block, 1e-5 on the bias gradient."""
import pytest
import torch

from errloc import assert_blocks, block_relerr

pytestmark = pytest.mark.gpu


def relerr(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / (b.norm() + 1e-30))


def _case(R, M, N, dy_dtype, narrow, seed):
    from vitlens_hip import ops
    g = torch.Generator().manual_seed(seed)
    dy = torch.randn(R, M, generator=g).to(dy_dtype).cuda()
    x = torch.randn(R, N, generator=g).bfloat16().cuda()
    g0 = torch.randn(M, N, generator=g).cuda()
    b0 = torch.randn(M, generator=g).cuda()
    got_g, got_b = g0.clone(), b0.clone()
    assert ops.weight_grad(dy, x, got_g, bias_grad=got_b, narrow=narrow) is got_g
    ref_g = g0.double() + dy.bfloat16().double().t() @ x.double()      # the product is bf16 x bf16 on every route
    ref_b = b0.double() + dy.double().sum(0)                           # the bias gradient: dy AS GIVEN
    what = f"weight_grad R={R} {M}x{N} {dy_dtype} narrow={narrow}"
    worst, blk = block_relerr(got_g, ref_g, 64, 64)
    print(f"MEASURED {what}: g whole {relerr(got_g, ref_g):.3e}, worst 64x64 block {worst:.3e} at {blk}, bias {relerr(got_b, ref_b):.3e}")
    assert relerr(got_g, ref_g) < 2e-6, what
    assert_blocks(got_g, ref_g, 5e-7, 64, 64, what=what)
    assert relerr(got_b, ref_b) < 1e-5, what
    assert_blocks(got_b[None], ref_b[None], 1e-5, 1, 64, what=what + " bias gradient")
    # a second call adds exactly the same numbers
    again_g, again_b = g0.clone(), b0.clone()
    ops.weight_grad(dy, x, again_g, bias_grad=again_b, narrow=narrow)
    assert torch.equal(got_g, again_g) and torch.equal(got_b, again_b), what + ": not reproducible"
    # without a bias gradient: the same product
    only_g = g0.clone()
    ops.weight_grad(dy, x, only_g, narrow=narrow)
    assert torch.equal(only_g, got_g), what + ": the product depends on the bias gradient"


@pytest.mark.parametrize("R,M,N,narrow", [
    (4096, 1024, 3072, False),     # whole tiles: the token-major kernel, then colsum
    (4096, 64, 1024, True),        # narrow: the zero-padded path
    (4096, 64, 1024, False),       # narrow with narrow=False: the transposing path, fused transpose + column sums
    (4096, 1024, 1024, False),     # few work items: refused by the token-major kernel, the transposing path
    (4096, 1024, 1024, True),      # the same through gemm_dw_tn_any's few-tile slices
    (771, 256, 512, True),         # rows not a multiple of 64: fused transpose (R >= 256), token axis padded to 832
    (200, 256, 512, True),         # below 256 rows: separate transpose and colsum
])
def test_weight_grad_bf16_operands_every_route(R, M, N, narrow):
    _case(R, M, N, torch.bfloat16, narrow, R + M + N)


@pytest.mark.parametrize("R", [200, 771, 4096])
def test_weight_grad_fp32_dy_sums_dy_as_given_at_every_row_count(R):
    """An fp32 dy with a bias gradient: the column sums of the fp32 values, not of the bf16 copies the transpose writes, below
    and above the fused transpose's 256-row threshold alike.  Sums of the bf16-rounded values differ from these by ~1e-3
    relative (2^-9 per term), a hundred times the 1e-5 bound."""
    _case(R, 256, 512, torch.float32, True, R)
    dy = torch.randn(R, 256, generator=torch.Generator().manual_seed(R))
    rounded = dy.bfloat16().double().sum(0)
    assert relerr(rounded, dy.double().sum(0)) > 1e-4              # the reference tells the two apart
