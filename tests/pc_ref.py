"""float64 references of the point-cloud tokenizer's non-GEMM kernels (csrc/vl_bn.hip, group_max / pad3 in
csrc/vl_points.hip).  Every function computes in float64 on the device its inputs live on, so the references of the C5-size
operands ([2 097 152, 512]) are computed on the GPU.  tests/test_pc_ref_host.py pins them against torch's BatchNorm +
autograd and torch.max(dim) on the CPU.

BatchNorm1d normalises the columns of x [R, C] over its rows.  `gate` is the ReLU gate of the fused forward (bool [R, C]):
pass the forward's own output > 0 to measure a backward against the function the forward computed, or leave it None to
derive it from the float64 forward.
"""
import torch

F64 = torch.float64


def _d(t):
    return None if t is None else t.to(F64)


# ---- BatchNorm1d --------------------------------------------------------------------------------------------------------
def bn_stats(x):
    """Batch statistics: (mean, biased var) [C]."""
    x = _d(x)
    mean = x.mean(0)
    return mean, (x - mean).square_().mean(0)


def bn_running(running_mean, running_var, mean, var, R, momentum=0.1):
    """nn.BatchNorm1d's running-stat update: the unbiased variance goes into running_var."""
    unb = var * (R / (R - 1)) if R > 1 else var
    return ((1 - momentum) * _d(running_mean) + momentum * _d(mean),
            (1 - momentum) * _d(running_var) + momentum * _d(unb))


def bn_apply(x, mean, var, gamma, beta, eps=1e-5, relu=False):
    y = (_d(x) - _d(mean)) * (_d(gamma) / (_d(var) + eps).sqrt()) + _d(beta)
    return y.clamp_min_(0) if relu else y


def _dprime(dy, x, mean, var, gamma, beta, eps, relu, gate):
    d = _d(dy).clone()
    if relu:
        if gate is None:
            gate = bn_apply(x, mean, var, gamma, beta, eps) > 0
        d.mul_(gate)
    return d


def bn_bwd_sums(dy, x, mean, var, gamma, beta, eps=1e-5, relu=False, gate=None):
    """(sum dy', sum dy' * xhat) [C] each, dy' = dy * gate: dbeta and dgamma, and what SyncBatchNorm all-reduces."""
    d = _dprime(dy, x, mean, var, gamma, beta, eps, relu, gate)
    xh = (_d(x) - _d(mean)) / (_d(var) + eps).sqrt()
    s1 = d.sum(0)
    s2 = d.mul_(xh).sum(0)
    return s1, s2


def bn_bwd_apply(dy, x, mean, var, gamma, beta, s1, s2, n, eps=1e-5, relu=False, train=True, gate=None):
    """dx from the column sums (s1, s2) of bn_bwd_sums over a batch of n rows (n > R for a SyncBatchNorm rank)."""
    d = _dprime(dy, x, mean, var, gamma, beta, eps, relu, gate)
    rs = 1.0 / (_d(var) + eps).sqrt()
    if train:
        xh = (_d(x) - _d(mean)) * rs
        d.sub_(_d(s1) / n).sub_(xh.mul_(_d(s2) / n))
    return d.mul_(_d(gamma) * rs)


def bn_bwd(dy, x, mean, var, gamma, beta, eps=1e-5, relu=False, train=True, gate=None):
    """Backward of [relu](BatchNorm1d(x)) given mean / var: (dx, dgamma, dbeta).  train: mean and var are x's own batch
    statistics and get gradients; eval: they are constants (running statistics)."""
    s1, s2 = bn_bwd_sums(dy, x, mean, var, gamma, beta, eps, relu, gate)
    dx = bn_bwd_apply(dy, x, mean, var, gamma, beta, s1, s2, x.shape[0], eps, relu, train, gate)
    return dx, s2, s1


# ---- SyncBatchNorm split ------------------------------------------------------------------------------------------------
def bn_local(x):
    """One rank's share: (mean [C], M2 = sum (x - mean)^2 [C], row count)."""
    x = _d(x)
    mean = x.mean(0)
    return mean, (x - mean).square_().sum(0), x.shape[0]


def chan_merge(parts):
    """Chan et al. pairwise merge of [(mean, M2, count), ...] in list order -> (mean, biased var, M2, count)."""
    n, mu, m2 = 0, None, None
    for mk, m2k, nk in parts:
        mk, m2k = _d(mk), _d(m2k)
        if mu is None:
            n, mu, m2 = nk, mk.clone(), m2k.clone()
            continue
        d, nn = mk - mu, n + nk
        mu = mu + d * (nk / nn)
        m2 = m2 + m2k + d * d * (n * nk / nn)
        n = nn
    return mu, m2 / n, m2, n


# ---- group max / sum ------------------------------------------------------------------------------------------------------
def group_max(x, M):
    """Max over each run of M rows of x [G*M, C], with torch.max(dim)'s semantics: the first maximum wins a tie, a NaN
    wins and propagates (the first NaN is the arg-max), an all -inf group gives index 0.  -> (values f64 [G, C],
    indices int64 [G, C])."""
    v = _d(x).view(-1, M, x.shape[1])
    nan = v.isnan()
    has_nan = nan.any(1)
    amax = v.amax(1)                                    # NaN in a group makes its amax NaN
    hit = torch.where(has_nan[:, None], nan, v == amax[:, None])
    del v, nan
    return amax, hit.to(torch.uint8).argmax(1)          # argmax: the first of the maxima


def group_max_bwd(idx, dg, M, base=None):
    """Backward of group_max: dg [G, C] scattered to the arg-max row of each group, plus base [G*M, C] when given."""
    G, C = dg.shape
    out = torch.zeros(G, M, C, dtype=F64, device=dg.device) if base is None else _d(base).view(G, M, C).clone()
    out.scatter_add_(1, idx.view(G, 1, C), _d(dg).view(G, 1, C))
    return out.view(G * M, C)


def group_sum(x, M):
    return _d(x).view(-1, M, x.shape[1]).sum(1)


def pad3(c, Kp=64):
    """Centres [R, 3] -> [R, Kp] zero padded."""
    c = _d(c).reshape(-1, 3)
    out = torch.zeros(c.shape[0], Kp, dtype=F64, device=c.device)
    out[:, :3] = c
    return out


# ---- comparison helpers -----------------------------------------------------------------------------------------------
def bf16_ulp(v):
    """The spacing of bf16 numbers at |v| (f64), the subnormal spacing below the smallest normal."""
    v = _d(v).abs()
    _, e = torch.frexp(v.clamp_min(2.0 ** -126))
    return torch.ldexp(torch.ones_like(v), (e - 8).to(torch.int32))


def within_bf16_ulps(out, ref, slack=None, ulps=1.0):
    """Elements of the bf16 out farther than `ulps` bf16 ulps (+ slack, an f64 bound of the kernel's own fp32 rounding)
    from the f64 ref: (count, index of the worst, its distance in ulps).  NaN in out or ref counts as a miss unless both
    are NaN; equal infinities match."""
    o, r = _d(out), _d(ref)
    same = (o == r) | (o.isnan() & r.isnan())
    lim = bf16_ulp(r) * ulps + (0 if slack is None else slack)
    dist = torch.where(same, torch.zeros_like(o), (o - r).abs().nan_to_num(nan=float("inf")))
    over = dist > lim
    q = torch.where(same, torch.zeros_like(o), dist / lim)
    i = int(q.reshape(-1).argmax())
    return int(over.sum()), i, float(q.reshape(-1)[i]) * ulps


# ---- the kernels' work split (csrc/vl_bn.hip): the block geometry of the per-block checks -------------------------------
def bn_nchunk(R):
    """Row chunks of the statistics / backward partials (vitlens_hip.ops._bn_chunks)."""
    return max(1, min(1024, R // 64))


def bn_chunk_rows(R):
    n = bn_nchunk(R)
    return -(-R // n)


def bn_apply_period(R, C):
    """Rows one sweep of an apply pass covers: 4 096 blocks x rpb rows for the column-stationary kernels (C/8 a divisor
    of 256), whose blocks then walk down the rows; the thread-per-element kernels have no sweep, so their blocks are the
    statistics' row chunks."""
    tpr = C // 8
    return 4096 * (256 // tpr) if 256 % tpr == 0 else bn_chunk_rows(R)
