"""CPU: the fp64 references of tests/rows_ref.py against independent statements of the same operations - fp64 autograd of
torch.nn.functional.layer_norm for the backward, the dense form on a zero-filled residual gradient for the sparse one, plain
loops for the assembly and the batch sum - and the fp32 emulation of the one-pass variance that shows which of the rows
test_hip_rows.py builds take the ill-conditioned-row branch of row_stats_kernel, and what a kernel without it would return."""
import math

import pytest
import torch

import rows_ref


def rnd(*shape, seed=0, scale=1.0, dtype=torch.float64):
    return (torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64) * scale).to(dtype)


@pytest.mark.parametrize("rows,D", [(1, 24), (5, 72), (6, 256)])
def test_forward_reference_is_torch_layer_norm(rows, D):
    x = rnd(rows, D, seed=1, scale=3) + 1
    w, b = 1 + rnd(D, seed=2, scale=0.1), rnd(D, seed=3, scale=0.1)
    y, mean, rstd = rows_ref.layernorm_fwd(x, w, b)
    assert torch.allclose(y, torch.nn.functional.layer_norm(x, (D,), w, b, 1e-5), rtol=1e-12, atol=1e-12)
    assert torch.allclose(mean, x.mean(-1), rtol=1e-13, atol=1e-13)
    assert torch.allclose(rstd, (x.var(-1, unbiased=False) + 1e-5).rsqrt(), rtol=1e-12)
    m2, r2 = rows_ref.row_stats(x)
    assert torch.equal(m2, mean) and torch.equal(r2, rstd)


@pytest.mark.parametrize("rows,D", [(1, 24), (5, 72), (6, 256)])
@pytest.mark.parametrize("with_dres", [False, True])
def test_backward_reference_is_autograd_of_layer_norm(rows, D, with_dres):
    x = (rnd(rows, D, seed=4, scale=2) + 0.5).requires_grad_(True)
    w, b = 1 + rnd(D, seed=5, scale=0.2), rnd(D, seed=6, scale=0.1)
    dy = rnd(rows, D, seed=7)
    dres = rnd(rows, D, seed=8) if with_dres else None
    torch.nn.functional.layer_norm(x, (D,), w, b, 1e-5).backward(dy)
    _, mean, rstd = rows_ref.layernorm_fwd(x.detach(), w, b)
    got = rows_ref.layernorm_bwd(dy, x.detach(), mean, rstd, w, dres)
    want = x.grad if dres is None else x.grad + dres
    assert float((got - want).abs().max()) < 1e-12 * (1 + float(want.abs().max()))


def test_backward_reference_converts_low_precision_operands_exactly():
    rows, D = 3, 72
    x, dy = rnd(rows, D, seed=9, dtype=torch.bfloat16), rnd(rows, D, seed=10, dtype=torch.bfloat16)
    w = 1 + rnd(D, seed=11, scale=0.2, dtype=torch.float32)
    _, mean, rstd = rows_ref.layernorm_fwd(x, w, torch.zeros(D))
    a = rows_ref.layernorm_bwd(dy, x, mean.float(), rstd.float(), w)
    b = rows_ref.layernorm_bwd(dy.double(), x.double(), mean.float().double(), rstd.float().double(), w.double())
    assert a.dtype == torch.float64 and torch.equal(a, b)


@pytest.mark.parametrize("B,L,rows", [(3, 5, 15), (2, 257, 514), (3, 5, 13)])
def test_sparse_backward_is_the_dense_one_on_a_zero_filled_residual(B, L, rows):
    """rows = B * L - 2: the last sample is cut short, its first row still has a residual gradient."""
    D = 24
    x, dy = rnd(rows, D, seed=12), rnd(rows, D, seed=13)
    w = 1 + rnd(D, seed=14, scale=0.2)
    _, mean, rstd = rows_ref.layernorm_fwd(x, w, torch.zeros(D, dtype=torch.float64))
    small = rnd(B, D, seed=15)
    dense = torch.zeros(B * L, D, dtype=torch.float64)
    dense[::L] = small
    want = rows_ref.layernorm_bwd(dy, x, mean, rstd, w, dense[:rows])
    got = rows_ref.layernorm_bwd_sparse(dy, x, mean, rstd, w, small, L)
    assert torch.equal(got, want)
    # the reference tells the two apart: a dense form that added a residual gradient to EVERY row would be off by |dres|
    every = rows_ref.layernorm_bwd(dy, x, mean, rstd, w, small.repeat_interleave(L, 0)[:rows])
    assert float((every - got).abs().max()) > 1.0


def test_assembly_references_agree_and_follow_the_row_layout():
    B, T, D = 3, 4, 24
    tok = rnd(B, T, D, seed=16, dtype=torch.bfloat16)
    cls, pos, pos2 = (rnd(D, seed=17, dtype=torch.float32), rnd(T + 1, D, seed=18, dtype=torch.float32),
                      rnd(T, D, seed=19, dtype=torch.float32))
    for p2 in (None, pos2):
        ref = rows_ref.assemble(tok, cls, pos, p2)
        for b in range(B):
            for l in range(T + 1):
                want = cls.double() + pos[0].double() if l == 0 else (
                    tok[b, l - 1].double() + pos[l].double() + (0 if p2 is None else p2[l - 1].double()))
                assert torch.equal(ref[b * (T + 1) + l], want)
        f32 = rows_ref.assemble_f32(tok, cls, pos, p2)
        assert f32.dtype == torch.float32
        # two fp32 additions of O(1) values: within two roundings of the exact sum
        assert float((f32.double() - ref).abs().max()) <= 2 * 2.0 ** -24 * float(ref.abs().max() + 4)


@pytest.mark.parametrize("B,T,D,stride,off", [(7, 1, 24, 5, 0), (7, 4, 24, 5, 1), (7, 5, 24, 5, 0)])
def test_batch_rowsum_reference_is_a_plain_loop(B, T, D, stride, off):
    x = rnd(B * stride, D, seed=20, dtype=torch.float32)
    out0 = rnd(T, D, seed=21, dtype=torch.float32)
    want = out0.double().clone()
    for b in range(B):
        for t in range(T):
            want[t] += x[b * stride + off + t].double()
    assert torch.allclose(rows_ref.batch_rowsum(x, out0, B, T, D, stride, off), want, rtol=1e-14, atol=1e-14)
    assert bool((rows_ref.batch_rowsum_abs(x, out0, B, T, D, stride, off) >= want.abs() - 1e-12).all())


def test_the_planted_rows_reach_the_ill_conditioned_branch_and_would_fail_without_it():
    """The figures the GPU test rests on: at offset 1000 / sigma 4 every row meets `var < 1e-3 * ex2` and the one-pass rstd
    misses the 2e-4 bound many times over (so a kernel without the fallback fails the test); at offset 40 / sigma 1.5 the
    branch is not taken and the one-pass result is inside the bound (so the test does not demand the fallback there)."""
    far, near, const = rows_ref.ill_conditioned_rows()
    _, rstd, taken = rows_ref.one_pass_fp32(far)
    _, want = rows_ref.row_stats(far)
    err_far = float((rstd.double() / want - 1).abs().max())
    print("per row:", [f"{float(e):.2e}" for e in (rstd.double() / want - 1).abs()])
    assert bool(taken.all()) and err_far > 5 * 2e-4, err_far
    _, rstd, taken = rows_ref.one_pass_fp32(near)
    _, want = rows_ref.row_stats(near)
    err_near = float((rstd.double() / want - 1).abs().max())
    assert not bool(taken.any()) and err_near < 2e-4, err_near
    _, _, taken = rows_ref.one_pass_fp32(const)
    assert bool(taken.all())                  # variance 0: the fallback's two-pass sum returns exactly rsqrt(eps)
    _, want = rows_ref.row_stats(const)
    assert abs(float(want) - 1e-5 ** -0.5) < 1e-9 * 1e-5 ** -0.5
    print(f"one-pass rstd error: offset 1000 sigma 4: {err_far:.2e}; offset 40 sigma 1.5: {err_near:.2e}")


def test_nan_clamp_reference():
    """torch.clamp_ keeps a NaN (C's fminf(fmaxf(NaN, lo), hi) returns lo = 0.0: the difference test_hip_rows.py's clamp test
    sees); infinities go to the bounds."""
    t = torch.tensor([float("nan"), float("inf"), float("-inf")])
    t.clamp_(0.0, math.log(100.0))
    assert math.isnan(float(t[0])) and float(t[1]) == pytest.approx(math.log(100.0)) and float(t[2]) == 0.0
