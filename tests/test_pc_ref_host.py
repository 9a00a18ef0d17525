"""CPU: the float64 references of tests/pc_ref.py against torch's own BatchNorm + autograd and torch.max(dim), at small
shapes with the edges the GPU tests (tests/test_hip_pc_kernels.py) rely on: ties, NaN and all -inf groups, SyncBatchNorm
ranks of one row; and the per-block check at the block geometry of those tests fails on an output with one block scaled."""
import pytest
import torch

import pc_ref as ref
from errloc import assert_blocks

F = torch.nn.functional
D = torch.float64


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _x(R, C, seed):
    g = _gen(seed)
    return (torch.randn(R, C, generator=g) * 0.7 + 3 * torch.randn(C, generator=g)).bfloat16()


def _params(C, seed):
    g = _gen(seed)
    return (1 + 0.1 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g),
            1 + 0.2 * torch.rand(C, generator=g))


def _close(a, b, tol=1e-12):
    a, b = a.double(), b.double()
    assert float((a - b).norm()) <= tol * max(float(b.norm()), 1e-300), float((a - b).norm() / b.norm())


@pytest.mark.parametrize("train", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("relu", [True, False], ids=["relu", "plain"])
def test_bn_reference_equals_torch_batch_norm_and_autograd(train, relu):
    R, C = 53, 24
    x = _x(R, C, seed=1)
    dy = torch.randn(R, C, generator=_gen(2)).bfloat16()
    gamma, beta, rm0, rv0 = _params(C, seed=3)
    xr = x.to(D).requires_grad_(True); g = gamma.to(D).requires_grad_(True); b = beta.to(D).requires_grad_(True)
    rm, rv = rm0.to(D), rv0.to(D)
    y = F.batch_norm(xr, rm, rv, g, b, training=train, momentum=0.1, eps=1e-5)
    if relu:
        y = torch.relu(y)
    y.backward(dy.to(D))
    if train:
        mean, var = ref.bn_stats(x)
        _close(mean, x.to(D).mean(0)); _close(var, x.to(D).var(0, unbiased=False))
        rm64, rv64 = ref.bn_running(rm0, rv0, mean, var, R, 0.1)
        _close(rm64, rm); _close(rv64, rv)
    else:
        mean, var = rm0, rv0
    _close(ref.bn_apply(x, mean, var, gamma, beta, 1e-5, relu), y.detach())
    dx, dg, db = ref.bn_bwd(dy, x, mean, var, gamma, beta, 1e-5, relu, train)
    _close(dx, xr.grad); _close(dg, g.grad); _close(db, b.grad)
    # the gate given explicitly (the forward's output > 0) is the gate derived from the forward
    gate = y.detach() > 0
    dx2, dg2, db2 = ref.bn_bwd(dy, x, mean, var, gamma, beta, 1e-5, relu, train, gate if relu else None)
    assert torch.equal(dx2, dx) and torch.equal(dg2, dg) and torch.equal(db2, db)


def test_syncbn_reference_ranks_equal_the_concatenated_batch():
    """Per-rank (mean, M2, count), Chan merge in rank order, summed backward sums and the per-rank elementwise pass with
    the global count equal the one-batch reference; one rank holds a single row."""
    R, C = 97, 16
    x = _x(R, C, seed=4)
    dy = torch.randn(R, C, generator=_gen(5)).bfloat16()
    gamma, beta, _, _ = _params(C, seed=6)
    cuts = [0, 1, 40, 41, R]
    parts = [slice(cuts[i], cuts[i + 1]) for i in range(len(cuts) - 1)]
    locs = [ref.bn_local(x[p]) for p in parts]
    assert [n for _, _, n in locs] == [1, 39, 1, 56] and float(locs[0][1].abs().max()) == 0.0
    mean, var, m2, n = ref.chan_merge(locs)
    m64, v64 = ref.bn_stats(x)
    assert n == R
    _close(mean, m64); _close(var, v64); _close(m2, v64 * R)
    sums = [ref.bn_bwd_sums(dy[p], x[p], mean, var, gamma, beta, 1e-5, True) for p in parts]
    s1, s2 = sum(s[0] for s in sums), sum(s[1] for s in sums)
    dx = torch.cat([ref.bn_bwd_apply(dy[p], x[p], mean, var, gamma, beta, s1, s2, R, 1e-5, True) for p in parts])
    dx1, dg1, db1 = ref.bn_bwd(dy, x, mean, var, gamma, beta, 1e-5, True, True)
    _close(dx, dx1); _close(s2, dg1); _close(s1, db1)


def _group_input(G, M, C, seed):
    g = _gen(seed)
    x = torch.randn(G * M, C, generator=g).bfloat16()
    v = x.view(G, M, C)
    if M > 1:
        v[0, 1] = v[0, M - 1] = v[0].amax(0) + 1                     # tie at the max: row 1 must win
        v[1, :] = v[1, 0]                                            # every row equal: row 0
    v[2] = -float("inf")                                             # all -inf: index 0
    v[3, M - 1, 0] = float("nan")                                    # a NaN wins
    v[4, M // 2, :] = float("nan"); v[4, M - 1, :] = float("nan")    # the first NaN wins
    v[5, 0, 1] = float("inf"); v[5, M - 1, 1] = float("nan")         # NaN beats +inf
    return x


@pytest.mark.parametrize("M", [1, 2, 7, 33])
def test_group_max_reference_equals_torch_max(M):
    G, C = 9, 6
    x = _group_input(G, M, C, seed=7)
    vals, idx = ref.group_max(x, M)
    tv, ti = x.to(D).view(G, M, C).max(dim=1)
    assert torch.equal(vals.isnan(), tv.isnan())
    assert torch.equal(vals.nan_to_num(), tv.nan_to_num()) and torch.equal(idx, ti)
    assert bool(vals[3, 0].isnan()) and int(idx[3, 0]) == M - 1
    assert int(idx[4, 2]) == M // 2 and bool(vals[2].eq(-float("inf")).all()) and bool(idx[2].eq(0).all())
    if M > 1:
        assert int(idx[0, 3]) == 1 and int(idx[1, 3]) == 0
    # backward: dg at the arg-max rows (+ base), as autograd routes torch.max(dim)
    dg = torch.randn(G, C, generator=_gen(8)).bfloat16()
    base = torch.randn(G * M, C, generator=_gen(9)).bfloat16()
    xr = x.to(D).view(G, M, C).requires_grad_(True)
    xr.max(dim=1).values.backward(dg.to(D))
    assert torch.equal(ref.group_max_bwd(idx, dg, M), xr.grad.view(G * M, C))
    assert torch.equal(ref.group_max_bwd(idx, dg, M, base), xr.grad.view(G * M, C) + base.to(D))
    y = _x(G * M, C, seed=10)
    _close(ref.group_sum(y, M), y.to(D).view(G, M, C).sum(1), 0)


def test_pad3_reference():
    c = torch.randn(5, 3, generator=_gen(11))
    p = ref.pad3(c, 8)
    assert torch.equal(p[:, :3], c.to(D)) and bool((p[:, 3:] == 0).all())


def test_bf16_ulp_and_ulp_distance():
    v = torch.tensor([1.0, 1.5, 2.0, 3.0, -0.75, 2.0 ** -130, 0.0], dtype=D)
    assert ref.bf16_ulp(v).tolist() == [2.0 ** -7, 2.0 ** -7, 2.0 ** -6, 2.0 ** -6, 2.0 ** -8, 2.0 ** -133, 2.0 ** -133]
    r = torch.tensor([1.0, 3.0, float("nan"), float("-inf"), 2.0], dtype=D)
    assert ref.within_bf16_ulps(torch.tensor([1.0078125, 3.0, float("nan"), float("-inf"), 2.0]), r)[0] == 0
    n, i, u = ref.within_bf16_ulps(torch.tensor([1.0, 3.0, 1.0, float("-inf"), 2.0 + 2 ** -5]), r)
    assert n == 2 and i == 2 and u == float("inf")
    n, i, u = ref.within_bf16_ulps(torch.tensor([1.0, 3.0, float("nan"), float("-inf"), 2.0 + 2 ** -5]), r)
    assert n == 1 and i == 4 and u == pytest.approx(2.0)


def test_bn_geometry_matches_the_wrappers():
    assert [ref.bn_nchunk(R) for R in (1, 127, 128, 65535, 65536, 2 ** 21)] == [1, 1, 2, 1023, 1024, 1024]
    assert ref.bn_chunk_rows(2 ** 21) == 2048 and ref.bn_chunk_rows(1024 * 128 + 37) == 129
    assert ref.bn_apply_period(2 ** 21, 512) == 16384 and ref.bn_apply_period(2 ** 21, 128) == 65536
    assert ref.bn_apply_period(70001, 384) == ref.bn_chunk_rows(70001) == 69


@pytest.mark.parametrize("R,C,rows,tol", [(16384 * 2 + 5, 512, 16384, 3.5e-3), (65536 + 3, 128, 65536, 4e-3),
                                          (70001, 384, 69, 4e-3), (1, 512, 1, 1.8e-7), (1, 256, 1, 7e-8)])
def test_errloc_at_the_bn_geometry_fails_on_one_block_scaled(R, C, rows, tol):
    """bf16 rounding of the output passes the per-block check at the GPU tests' geometry (sweeps of the capped grid x 128
    columns; one row for the per-column statistics); scaling one block of a later sweep by 1 + 4 tol passes the
    whole-tensor check but fails the per-block one, at that block."""
    g = _gen(R)
    ref64 = (torch.randn(R, C, generator=g) * 0.7).to(D)
    out = ref64.float() if tol < 1e-4 else ref64.bfloat16()
    assert_blocks(out, ref64, tol, rows, 128)
    r0 = (R - 1) // rows * rows
    bad = out.clone()
    bad[r0:r0 + rows, C - 128:C] *= 1 + 4 * tol
    whole = float((bad.to(D) - ref64).norm() / ref64.norm())
    if R > rows:
        assert whole < tol
    with pytest.raises(AssertionError, match=f"block rows {r0}:{min(R, r0 + rows)}, cols {C - 128}:{C} "):
        assert_blocks(bad, ref64, tol, rows, 128)
