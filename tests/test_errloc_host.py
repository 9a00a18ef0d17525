"""CPU: the per-block comparison helpers (tests/errloc.py) at the shapes the GPU tests use them on.  Seeded data, bf16
rounding of the output plus fp32 summation-order noise must pass at every block size; each mutation below must pass the
whole-tensor check its GPU test keeps (which is the gap) and fail the per-block check, naming the block it is in."""
import pytest
import torch

from errloc import FLOOR, assert_attn_blocks, assert_blocks, attn_block_relerr, block_relerr


def relerr(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def _noisy(ref, seed):
    """What a correct bf16 kernel returns: the fp32 value with summation-order noise (a few fp32 ulps), rounded to bf16."""
    g = torch.Generator().manual_seed(seed)
    return (ref * (1 + 4 * 2.0 ** -24 * torch.randn(ref.shape, generator=g))).bfloat16()


def _gauss(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


ATTN_TOL, GEMM_TOL = 9e-3, 5e-3        # the per-block tolerances of the attention backward and persistent GEMM tests


@pytest.mark.parametrize("rows,cols", [(256, 256), (32, 64), (1, 1024), (1, 1), (2048, 768)])
def test_bf16_noise_passes_at_every_block_size(rows, cols):
    M = 2048 if rows == 2048 else 256 * 40
    ref = _gauss(M, 1024, seed=rows + cols)
    worst = assert_blocks(_noisy(ref, 1), ref, 4e-3 if rows * cols >= 2048 else 8e-3, rows, cols)
    assert worst > 0


@pytest.mark.parametrize("B,H,L,dh", [(2, 4, 257, 64), (1, 2, 50, 64)])
def test_bf16_noise_passes_attention_blocks(B, H, L, dh):
    ref = _gauss(B * L, H * dh, seed=L)
    assert attn_block_relerr(_noisy(ref, 2), ref, B, H, L)[0] < 1e-2
    heads = ref.view(B, L, H, dh).permute(0, 2, 1, 3).contiguous()            # heads layout against token-major: same
    assert attn_block_relerr(_noisy(ref, 2), heads, B, H, L) == attn_block_relerr(_noisy(ref, 2), ref, B, H, L)


def test_bf16_noise_passes_on_a_row_sample_of_the_bench_gemm():
    """(65 792, 1024) = 257 x 256 rows: the first and last 8192 rows (the remainder launch's rows a range of their own)."""
    M = 257 * 256
    ref = _gauss(16384, 1024, seed=3)
    assert_blocks(_noisy(ref, 3), ref, 4e-3, 256, 256, extra=[("rows", 16384 - (M - 256 * 256), 16384)])


def test_near_zero_blocks_are_measured_against_their_fair_share():
    ref = torch.relu(_gauss(1024, 1024, seed=4))
    ref[:256, :256] = 1e-6 * _gauss(256, 256, seed=5)             # a block that is ~0 in the reference
    out = _noisy(ref, 4).float()
    out[:256, :256] += 1e-4                                      # absolute noise there: far below the rest's scale
    assert_blocks(out, ref, 8e-3, 256, 256)
    with pytest.raises(AssertionError, match="rows 0:256, cols 0:256"):
        assert_blocks(out, ref, 8e-3, 256, 256, floor=0.0)       # without the floor it would flake


def test_mutation_lone_row_of_dk():
    """Row 256 of dK scaled by 1.3 in every (b, h) at (2, 4, 257, 64)."""
    B, H, L, dh = 2, 4, 257, 64
    ref = _gauss(B * L, H * dh, seed=6)
    out = _noisy(ref, 6).float()
    out.view(B, L, H, dh)[:, 256] *= 1.3
    assert relerr(out, ref) < 2e-2                               # test_hip_train.py's whole-tensor check passes
    with pytest.raises(AssertionError, match=r"dk: b=\d h=\d keys 256:257 "):
        assert_attn_blocks(out, ref, ATTN_TOL, B, H, L, "keys", what="dk")


def test_mutation_one_gemm_tile():
    """One 256x256 tile scaled by 1.05 at M = 256 x 40, N = 4096."""
    ref = _gauss(256 * 40, 4096, seed=7)
    out = _noisy(ref, 7).float()
    out[256 * 23:256 * 24, 768:1024] *= 1.05
    assert relerr(out, ref) < 4e-3                               # test_hip_gemm_park.py's whole-tensor check passes
    with pytest.raises(AssertionError, match="rows 5888:6144, cols 768:1024 "):
        assert_blocks(out, ref, GEMM_TOL, 256, 256)


def test_mutation_ragged_tile_shifted_by_one_row():
    """The last ragged tile (rows 32:50) of one (b, h) at L = 50 written one row down (row r gets row r - 1): detectable as
    long as neighbouring rows differ - here rows that vary slowly along the sequence, as gradients of nearby tokens do."""
    B, H, L, dh = 1, 2, 50, 64
    t = torch.arange(L, dtype=torch.float32)[:, None]
    base = _gauss(B, H, 1, dh, seed=8) + torch.sin(t / 16.0 + _gauss(B, H, 1, dh, seed=9))
    ref = (base + 0.01 * _gauss(B, H, L, dh, seed=10)).permute(0, 2, 1, 3).reshape(B * L, H * dh)
    out = _noisy(ref, 8).float()
    v = out.view(B, L, H, dh)
    v[0, 33:50, 1] = v[0, 32:49, 1].clone()
    assert relerr(out, ref) < 2e-2
    with pytest.raises(AssertionError, match="b=0 h=1 queries 32:50 "):
        assert_attn_blocks(out, ref, ATTN_TOL, B, H, L, "queries")


def test_mutation_two_heads_swapped():
    """Heads 1 and 2 of batch 1 swapped at (2, 4, 257, 64), heads that share most of their signal (a common component,
    as heads looking at the same tokens have)."""
    B, H, L, dh = 2, 4, 257, 64
    ref = (_gauss(B, 1, L, dh, seed=11) + 0.02 * _gauss(B, H, L, dh, seed=12)).permute(0, 2, 1, 3).reshape(B * L, H * dh)
    out = _noisy(ref, 11).float()
    v = out.view(B, L, H, dh)
    v[1, :, [1, 2]] = v[1, :, [2, 1]].clone()
    assert relerr(out, ref) < 2e-2
    with pytest.raises(AssertionError, match=r"b=1 h=[12] rows \d+:\d+ "):
        assert_attn_blocks(out, ref, ATTN_TOL, B, H, L)


def test_mutation_leftover_rows_take_the_neighbouring_bias():
    """M = 256 x 64 + 8, N = 1024: the 8 leftover rows (a launch of their own) add bias[c + 1] instead of bias[c]."""
    M, N = 256 * 64 + 8, 1024
    acc = _gauss(M, N, seed=13)
    bias = 0.05 * _gauss(N, seed=14)
    ref = acc + bias
    out = _noisy(ref, 13).float()
    out[M - 8:] += torch.roll(bias, -1) - bias
    assert relerr(out, ref) < 4e-3
    with pytest.raises(AssertionError, match=rf"rows {M - 8}:{M}, cols \d+:\d+ "):
        assert_blocks(out, ref, GEMM_TOL, 256, 256, extra=[("rows", M - 8, M)])


def test_worst_block_is_reported_with_its_coordinates():
    ref = _gauss(600, 300, seed=15)
    out = ref.clone()
    out[513, 299] += 1.0
    worst, blk = block_relerr(out, ref, 256, 128, extra=[("rows", 512, 520)])
    assert blk == (512, 520, 256, 300) and abs(worst - 1 / float(ref[512:520, 256:300].norm())) < 1e-6
    out[7, 0] = float("nan")
    assert block_relerr(out, ref, 256, 128)[1] == (0, 256, 0, 128)
    assert FLOOR > 0
