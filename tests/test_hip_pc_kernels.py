"""GPU: the point-cloud tokenizer's non-GEMM kernels (csrc/vl_bn.hip; group_max and pad3 in csrc/vl_points.hip) against
the float64 references of tests/pc_ref.py, at the C5 benchmark geometry (128 clouds x 512 groups x 32 points: 2 097 152
rows, 65 536 groups) and at every dispatch branch of the wrappers in vitlens_hip.ops.

Each BatchNorm output is checked whole-tensor and per block (tests/errloc.py), with blocks that follow the kernel's own
work split: 128 columns for the per-column statistics and parameter gradients, 4 096 * rpb rows (one sweep of the capped
grid of the column-stationary apply kernels, which then walk down the rows) x 128 columns for the apply passes.  Each
per-block check is shown to fail on the kernel's own output with one block scaled.  Every buffer the wrappers allocate is
filled with NaN first, so a row or column a kernel skips shows up.  The group kernels and pad3 are checked exactly.
"""
import math

import pytest
import torch

import pc_ref as ref
from errloc import assert_blocks

pytestmark = pytest.mark.gpu

NAN_FILL = {torch.float32: float("nan"), torch.bfloat16: float("nan"), torch.float64: float("nan"), torch.int32: -1}
C5_ROWS, C5_GROUPS, C5_M = 128 * 512 * 32, 128 * 512, 32
EPS = 1e-5

# Per-block tolerances: about twice the worst block measured on the MI355X over the cases below (noted beside each).
TOL_MEAN = 7e-8        # mean of bn_stats / bn_stats_local / bn_stats_merge, measured 3.4e-8
TOL_VAR = 1.8e-7       # var and M2, measured 8.7e-8 (1.4e-7 with row 0 at 1 000 sigma)
TOL_RUN = 1.5e-7       # running mean / var, measured 7.1e-8
TOL_Y = 3.5e-3         # bn_apply, bf16 out, measured 1.75e-3
TOL_DX = 4e-3          # bn_bwd / bn_bwd_apply dx, bf16 out, measured 2.1e-3
TOL_DPARAM = 7e-7      # dgamma / dbeta accumulated into non-zero f32 buffers, measured 3.6e-7


class _NaNAllocs:
    """Stands in for the torch module inside vitlens_hip.ops: every empty / empty_like the wrappers allocate (outputs and
    workspaces) comes back filled with NaN (-1 for int32), so output a kernel never writes shows up."""

    def __getattr__(self, name):
        return getattr(torch, name)

    @staticmethod
    def _fill(t):
        return t.fill_(NAN_FILL[t.dtype])

    def empty(self, *a, **k):
        return self._fill(torch.empty(*a, **k))

    def empty_like(self, *a, **k):
        return self._fill(torch.empty_like(*a, **k))


@pytest.fixture
def ops(monkeypatch):
    from vitlens_hip import ops as o
    monkeypatch.setattr(o, "torch", _NaNAllocs())
    return o


def _g(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def _randn(*shape, seed):
    return torch.randn(*shape, generator=_g(seed), device="cuda")


def _x(R, C, seed, ld=None):
    """bf16 [R, C] (a view of [R, ld] when ld > C) whose columns have |mean| >> std: mean ~ 3 N(0,1), std 0.7."""
    buf = torch.empty(R, ld or C, device="cuda", dtype=torch.bfloat16)
    x = buf[:, :C]
    x.copy_(_randn(R, C, seed=seed).mul_(0.7).add_(3 * _randn(C, seed=seed + 1000)))
    return x


def _params(C, seed):
    gamma = 1 + 0.1 * _randn(C, seed=seed)
    beta = 0.1 * _randn(C, seed=seed + 1)
    rm = 0.1 * _randn(C, seed=seed + 2)
    rv = 1 + 0.2 * torch.rand(C, generator=_g(seed + 3), device="cuda")
    return gamma, beta, rm, rv


def relerr(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


MEASURED = {}


def _blocks(out, ref64, tol, rows, cols, what):
    """assert_blocks, then the same check on the kernel's output with its last block scaled by 1 + 4 tol must fail and
    name that block: the check can see an error confined to one block of this geometry."""
    if out.dim() == 1:
        out, ref64 = out[None], ref64[None]
    worst = assert_blocks(out, ref64, tol, rows, cols, what=what)
    MEASURED[what] = max(MEASURED.get(what, 0.0), worst)
    print(f"measured {what}: {worst:.3e} (tol {tol:.1e})")
    M, N = out.shape
    r0, c0 = (M - 1) // rows * rows, (N - 1) // cols * cols
    bad = out.clone()
    bad[r0:r0 + rows, c0:c0 + cols] *= 1 + 4 * tol
    with pytest.raises(AssertionError, match=f"block rows {r0}:{min(M, r0 + rows)}, cols {c0}:{min(N, c0 + cols)} "):
        assert_blocks(bad, ref64, tol, rows, cols, what=what)
    return worst


# ------------------------------------------------------------------------------------------------ BatchNorm, one rank
BN_CASES = [
    # R, C, train, relu, ld
    pytest.param(C5_ROWS, 512, True, True, None, id="c5-C512-train-relu"),
    pytest.param(C5_ROWS, 128, True, False, None, id="c5-C128-train"),
    pytest.param(C5_ROWS, 128, False, True, None, id="c5-C128-eval-relu"),
    pytest.param(3001, 24, True, True, None, id="elem-C24"),
    pytest.param(70001, 384, True, True, None, id="elem-C384-cap"),        # pnsa encoder_dims 384; chunks past R stay empty
    pytest.param(20011, 4096, False, True, None, id="elem-C4096-eval"),
    pytest.param(4096 * 4 - 1, 512, True, True, None, id="walk-minus1"),
    pytest.param(4096 * 4 + 1, 512, True, True, None, id="walk-plus1"),
    pytest.param(100, 128, True, True, None, id="one-chunk"),
    pytest.param(1024 * 128 + 37, 256, True, True, None, id="chunk-cap-ragged"),
    pytest.param(40000, 128, True, True, 136, id="strided"),
]


@pytest.mark.parametrize("R,C,train,relu,ld", BN_CASES)
def test_bn_stats_apply_bwd_vs_fp64(ops, R, C, train, relu, ld):
    assert ops._bn_chunks(R) == ref.bn_nchunk(R)
    x = _x(R, C, seed=1, ld=ld)
    dy = _x(R, C, seed=2, ld=ld).sub_(3 * _randn(C, seed=1002).bfloat16())     # ~ N(0, 0.7)
    gamma, beta, rm0, rv0 = _params(C, seed=3)
    rows = ref.bn_apply_period(R, C)
    if train:
        rm, rv = rm0.clone(), rv0.clone()
        mean, var = ops.bn_stats(x, rm, rv, 0.1)
        m64, v64 = ref.bn_stats(x)
        rm64, rv64 = ref.bn_running(rm0, rv0, m64, v64, R)
        _blocks(mean, m64, TOL_MEAN, 1, 128, "bn_stats mean")
        _blocks(var, v64, TOL_VAR, 1, 128, "bn_stats var")
        _blocks(rm, rm64, TOL_RUN, 1, 128, "running_mean")
        _blocks(rv, rv64, TOL_RUN, 1, 128, "running_var")
        mean2, var2 = ops.bn_stats(x)
        assert torch.equal(mean2, mean) and torch.equal(var2, var), "bn_stats: two launches differ"
        del m64, v64
    else:
        mean, var = rm0, rv0
    # forward
    out = None
    if ld:
        obuf = torch.full((R, ld), -7.0, device="cuda", dtype=torch.bfloat16)
        out = obuf[:, :C]
    y = ops.bn_apply(x, mean, var, gamma, beta, EPS, relu, out=out)
    y64 = ref.bn_apply(x, mean, var, gamma, beta, EPS, relu)
    assert relerr(y, y64) < TOL_Y
    _blocks(y, y64, TOL_Y, rows, 128, "bn_apply y")
    del y64
    if ld:
        assert bool((obuf[:, C:] == -7.0).all()), "bn_apply wrote into the columns between rows"
    # backward: dgamma / dbeta accumulate into non-zero buffers of their own size
    gate = y > 0 if relu else None
    dx64, dg64, db64 = ref.bn_bwd(dy, x, mean, var, gamma, beta, EPS, relu, train, gate)
    dg0 = math.sqrt(R) * _randn(C, seed=5); db0 = math.sqrt(R) * _randn(C, seed=6)
    dg, db = dg0.clone(), db0.clone()
    dx = ops.bn_bwd(dy, x, mean, var, gamma, beta, dg, db, EPS, relu, train)
    assert relerr(dx, dx64) < TOL_DX
    _blocks(dx, dx64, TOL_DX, rows, 128, "bn_bwd dx")
    _blocks(dg, dg64 + dg0, TOL_DPARAM, 1, 128, "bn_bwd dgamma")
    _blocks(db, db64 + db0, TOL_DPARAM, 1, 128, "bn_bwd dbeta")
    dg2, db2 = dg0.clone(), db0.clone()
    dx2 = ops.bn_bwd(dy, x, mean, var, gamma, beta, dg2, db2, EPS, relu, train)
    assert torch.equal(dx2, dx) and torch.equal(dg2, dg) and torch.equal(db2, db), "bn_bwd: two launches differ"
    del dx2
    if ld:
        # a strided dx: the C ABI takes its row stride; the columns between rows stay untouched
        n = ref.bn_nchunk(R)
        ws = torch.full(((n + 1) * 2 * C,), float("nan"), device="cuda")
        dbuf = torch.full((R, ld), -7.0, device="cuda", dtype=torch.bfloat16)
        dg3, db3 = dg0.clone(), db0.clone()
        ops.check(ops._lib.vl_bn_bwd(ops._p(dy), dy.stride(0), ops._p(x), x.stride(0), ops._p(mean), ops._p(var),
                                 ops._p(gamma), ops._p(beta), EPS, int(relu), int(train), ops._p(ws), n, ops._p(dg3),
                                 ops._p(db3), ops._p(dbuf), ld, R, C, ops._stream()))
        assert torch.equal(dbuf[:, :C], dx) and torch.equal(dg3, dg), "bn_bwd: a strided dx differs from a dense one"
        assert bool((dbuf[:, C:] == -7.0).all()), "bn_bwd wrote into the columns between rows"
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ SyncBatchNorm split
def test_syncbn_split_at_c5_equals_fp64_and_one_rank(ops):
    """Uneven "ranks" of the C5 batch, one of them a single row: stats_local -> merge and bwd_reduce -> (sum over ranks) ->
    bwd_apply against the float64 reference on the concatenated batch and against the one-rank kernels."""
    R, C = C5_ROWS, 256
    cuts = [0, 1, 700001, 1500000, R]
    x = _x(R, C, seed=11)
    dy = _x(R, C, seed=12).sub_(3 * _randn(C, seed=1012).bfloat16())
    gamma, beta, rm0, rv0 = _params(C, seed=13)
    parts = [slice(cuts[i], cuts[i + 1]) for i in range(len(cuts) - 1)]
    locs = [ops.bn_stats_local(x[p]) for p in parts]
    for p, loc in zip(parts, locs):
        m64, m2, n = ref.bn_local(x[p])
        assert loc[2 * C:].view(torch.int32).item() == n
        _blocks(loc[:C], m64, TOL_MEAN, 1, 128, "bn_stats_local mean")
        if n > 1:
            _blocks(loc[C:2 * C], m2, TOL_VAR, 1, 128, "bn_stats_local M2")
        else:
            assert bool((loc[C:2 * C] == 0).all())
    rm, rv = rm0.clone(), rv0.clone()
    mean, var, total = ops.bn_stats_merge(torch.stack(locs), rm, rv, 0.1)
    assert int(total) == R
    m64, v64 = ref.bn_stats(x)
    cm, cv, _, cn = ref.chan_merge([ref.bn_local(x[p]) for p in parts])
    assert cn == R and relerr(cm, m64) < 1e-14 and relerr(cv, v64) < 1e-12
    rm64, rv64 = ref.bn_running(rm0, rv0, m64, v64, R)
    _blocks(mean, m64, TOL_MEAN, 1, 128, "bn_stats_merge mean")
    _blocks(var, v64, TOL_VAR, 1, 128, "bn_stats_merge var")
    _blocks(rm, rm64, TOL_RUN, 1, 128, "merge running_mean")
    _blocks(rv, rv64, TOL_RUN, 1, 128, "merge running_var")
    fm, fv = ops.bn_stats(x)
    assert relerr(mean, fm) < TOL_MEAN and relerr(var, fv) < TOL_VAR
    del m64, v64
    y = ops.bn_apply(x, mean, var, gamma, beta, EPS, True)
    gate = y > 0
    del y
    dgs = [torch.zeros(C, device="cuda") for _ in parts]; dbs = [torch.zeros(C, device="cuda") for _ in parts]
    sums = [ops.bn_bwd_reduce(dy[p], x[p], mean, var, gamma, beta, dgs[i], dbs[i], EPS, True) for i, p in enumerate(parts)]
    tot = torch.stack(sums).sum(0)
    dx = torch.cat([ops.bn_bwd_apply(dy[p], x[p], mean, var, gamma, beta, tot, total, EPS, True) for p in parts])
    dx64, dg64, db64 = ref.bn_bwd(dy, x, mean, var, gamma, beta, EPS, True, True, gate)
    assert relerr(dx, dx64) < TOL_DX
    _blocks(dx, dx64, TOL_DX, ref.bn_apply_period(R, C), 128, "syncbn dx")
    _blocks(sum(dgs), dg64, TOL_DPARAM, 1, 128, "syncbn dgamma")
    _blocks(sum(dbs), db64, TOL_DPARAM, 1, 128, "syncbn dbeta")
    del dx64
    dg1, db1 = torch.zeros(C, device="cuda"), torch.zeros(C, device="cuda")
    dx1 = ops.bn_bwd(dy, x, mean, var, gamma, beta, dg1, db1, EPS, True, True)
    assert relerr(dx, dx1) < TOL_DX and relerr(sum(dgs), dg1) < TOL_DPARAM and relerr(sum(dbs), db1) < TOL_DPARAM
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ the ReLU gate
@pytest.mark.parametrize("C", [4096, 512], ids=["elem-C4096", "rows-C512"])
def test_relu_gate_of_backward_equals_forward(ops, C):
    """Eval mode with beta chosen so that a bf16 value x* lands on each column's threshold: the backward must pass a
    gradient exactly where the forward's output is positive (the gate of the function the forward computed), in the
    thread-per-element and the column-stationary kernels alike, and bn_bwd_reduce's sum of dy' must count those rows."""
    R = 8192
    mean = 3 * _randn(C, seed=21)
    var = 0.25 + torch.rand(C, generator=_g(22), device="cuda")
    gamma = 1 + 0.3 * _randn(C, seed=23)
    xs = (mean + 0.7 * _randn(C, seed=24)).bfloat16().float()                 # x*, one per column
    s = (gamma / (var + EPS).sqrt()).float()
    beta = -((xs - mean) * s)                                                  # fl32(fl32(x* - mean) * fl32(gamma / sqrt))
    x = _x(R, C, seed=25)
    x[::2] = xs.bfloat16()                                                     # x* in half the rows
    h = ops.bn_apply(x, mean, var, gamma, beta, EPS, True)
    dy = torch.ones(R, C, device="cuda", dtype=torch.bfloat16)
    dx = ops.bn_bwd(dy, x, mean, var, gamma, beta, torch.zeros(C, device="cuda"), torch.zeros(C, device="cuda"), EPS,
                    True, False)
    fwd, bwd = h > 0, dx != 0
    bad = (fwd != bwd).nonzero()
    assert bad.numel() == 0, (f"{bad.shape[0]} elements where the backward's gate differs from the forward's, first at "
                              f"row {int(bad[0, 0])}, column {int(bad[0, 1])}: forward {float(h[tuple(bad[0])])}, "
                              f"backward dx {float(dx[tuple(bad[0])])}")
    sums = ops.bn_bwd_reduce(dy, x, mean, var, gamma, beta, torch.zeros(C, device="cuda"), torch.zeros(C, device="cuda"),
                             EPS, True)
    cnt = fwd.sum(0).float()
    bad = (sums[:C] != cnt).nonzero()
    assert bad.numel() == 0, (f"bn_bwd_reduce: sum dy' differs from the forward's count of positive outputs in {bad.numel()}"
                              f" columns, first column {int(bad[0, 0])}: {float(sums[bad[0, 0]])} vs {float(cnt[bad[0, 0]])}")
    # the SyncBatchNorm elementwise pass gates the same way
    total = torch.tensor([R], device="cuda", dtype=torch.int32)
    dxs = ops.bn_bwd_apply(dy, x, mean, var, gamma, beta, torch.zeros(2 * C, device="cuda"), total, EPS, True)
    assert torch.equal(dxs != 0, fwd), "bn_bwd_apply: the gate differs from the forward's"


# ------------------------------------------------------------------------------------------------ outlier in row 0
@pytest.mark.parametrize("k", [10, 100, 1000])
def test_bn_stats_with_outlier_row0_at_c5(ops, k):
    """Row 0 k standard deviations from its column's mean: the statistics must stay within the tolerance the ordinary
    case needs, on the one-rank and the per-rank (SyncBatchNorm) paths."""
    R, C = C5_ROWS, 128
    x = _x(R, C, seed=31)
    x[0] = (x[0].float() + k * 0.7).bfloat16()
    m64, v64 = ref.bn_stats(x)
    mean, var = ops.bn_stats(x)
    _blocks(mean, m64, TOL_MEAN, 1, 128, f"outlier {k} sigma: mean")
    _blocks(var, v64, TOL_VAR, 1, 128, f"outlier {k} sigma: var")
    loc = ops.bn_stats_local(x)
    _, m2, _ = ref.bn_local(x)
    _blocks(loc[C:2 * C], m2, TOL_VAR, 1, 128, f"outlier {k} sigma: local M2")


# ------------------------------------------------------------------------------------------------ group kernels
def _group_input(G, M, C, seed, edges=True):
    x = _x(G * M, C, seed=seed).sub_(3 * _randn(C, seed=seed + 1000).bfloat16())
    if edges and G >= 8:
        v = x.view(G, M, C)
        if M > 1:
            top = v.amax(1) + 1
            v[1, M - 1] = top[1]; v[1, M // 2] = top[1]                        # a tie at the max: row M//2 must win
            v[2, :] = v[2, 0]                                                  # every row equal: row 0 wins
            v[4, M - 1] = v[4, 0]                                              # duplicated bf16 rows
        v[3] = -float("inf")                                                   # all -inf: max -inf at row 0
        v[5, M - 1, 0] = float("nan")                                          # one NaN, in the last row
        v[6, M // 2, : C // 2] = float("nan")                                  # NaN in two rows: the first one wins
        v[6, M - 1, :] = float("nan")
        v[7, 0, 1] = float("inf"); v[7, M - 1, 1] = float("nan")               # NaN beats +inf
    return x


GROUP_CASES = [
    pytest.param(C5_GROUPS, C5_M, 256, id="c5-C256"),
    pytest.param(999, 1, 96, id="M1"),
    pytest.param(1001, 33, 96, id="M33"),
]


@pytest.mark.parametrize("G,M,C", GROUP_CASES)
def test_group_max_exact(ops, G, M, C):
    x = _group_input(G, M, C, seed=41)
    vals, _ = ref.group_max(x, M)
    for dt in (torch.bfloat16, torch.float32):
        got = ops.group_max(x, M, dt)
        bad = ~((got.double() == vals) | (got.isnan() & vals.isnan()))
        assert not bool(bad.any()), (f"group_max ({dt}): {int(bad.sum())} values differ from amax, first at group "
                                     f"{int(bad.nonzero()[0, 0])}, column {int(bad.nonzero()[0, 1])}")
        assert torch.equal(ops.group_max(x, M, dt).view(torch.int16 if dt == torch.bfloat16 else torch.int32),
                           got.view(torch.int16 if dt == torch.bfloat16 else torch.int32)), "group_max: two launches differ"


@pytest.mark.parametrize("G,M,C", GROUP_CASES)
@pytest.mark.parametrize("with_base", [False, True], ids=["no-base", "base"])
def test_group_max_bwd_exact(ops, G, M, C, with_base):
    f = _group_input(G, M, C, seed=51)
    dg = _randn(G, C, seed=52).bfloat16()
    base = _randn(G * M, C, seed=53).bfloat16() if with_base else None
    _, idx = ref.group_max(f, M)
    got = ops.group_max_bwd(f, dg, M, base)
    arg = torch.zeros(G, M, C, dtype=torch.bool, device="cuda").scatter_(1, idx.view(G, 1, C), True).view(G * M, C)
    want_off = base if with_base else torch.zeros_like(got)
    off = arg.logical_not() & (got.view(torch.int16) != want_off.view(torch.int16))
    assert not bool(off.any()), (f"group_max_bwd: {int(off.sum())} elements outside the arg-max rows differ from base, "
                                 f"first at row {int(off.nonzero()[0, 0])}, column {int(off.nonzero()[0, 1])}")
    r64 = ref.group_max_bwd(idx, dg, M, base)
    slack = (r64.abs() + dg.double().abs().repeat_interleave(M, 0)) * 2.0 ** -24       # fp32 base + dg
    n, i, u = ref.within_bf16_ulps(got[arg], r64[arg], slack[arg])
    assert n == 0, f"group_max_bwd: {n} arg-max elements beyond one bf16 ulp of base + dg, worst {u:.2f} ulps"
    # the routing itself: dg lands on the arg-max row (NaN wins, first maximum wins a tie)
    if G >= 8 and M > 1:
        assert int(idx[1, 0]) == M // 2 and int(idx[2, 0]) == 0 and int(idx[3, 0]) == 0 and int(idx[5, 0]) == M - 1
    assert torch.equal(ops.group_max_bwd(f, dg, M, base).view(torch.int16), got.view(torch.int16)), \
        "group_max_bwd: two launches differ"


@pytest.mark.parametrize("G,M,C", [pytest.param(C5_GROUPS, C5_M, 512, id="c5-C512"),
                                   pytest.param(999, 1, 96, id="M1"), pytest.param(1001, 33, 96, id="M33")])
def test_group_sum_within_one_ulp(ops, G, M, C):
    x = _group_input(G, M, C, seed=61, edges=False)
    got = ops.group_sum(x, M)
    r64 = ref.group_sum(x, M)
    slack = x.double().abs().view(G, M, C).sum(1) * (M * 2.0 ** -24)             # fp32 accumulation over M rows
    n, i, u = ref.within_bf16_ulps(got, r64, slack)
    assert n == 0, f"group_sum: {n} sums beyond one bf16 ulp, worst at group {i // C}, column {i % C}: {u:.2f} ulps"
    assert torch.equal(ops.group_sum(x, M).view(torch.int16), got.view(torch.int16)), "group_sum: two launches differ"


def test_pad3_exact(ops):
    R, Kp = 65536, 64
    c = _randn(R, 3, seed=71)
    got = ops.pad3(c, Kp)
    assert torch.equal(got[:, :3], c.bfloat16()) and bool((got[:, 3:] == 0).all())
    assert got.shape == (R, Kp)
