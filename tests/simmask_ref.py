"""Similarity-masked contrastive loss (`ClipLossSimMask`): a float64 restatement, and the seeded inputs of its tests.

The loss (x = TEACHER features, y = student features, s = temperature, all rank-major gathers written all_*):

    sim  = all_x @ all_x^T                      teacher similarities, from the features as given (no temperature)
    M    = not (sim >= thres)  or  eye          KEPT elements; a NaN similarity is kept; global indices
    L    = s * x @ y^T
    loss = (CE(L * M, rows) + CE((L * M)^T, rows)) / 2

The mask MULTIPLIES the logits: a masked element is logit 0.0 in both softmaxes, not -inf.  No gradient flows through M.

keep_mask       M for a block of teacher rows against teacher columns.
pair_loss       the building block every branch reduces to: w_row * CE over the rows of (L * M) + w_col * CE over its columns,
                row r's label being column r + label_off, for any R x C block.  The kernels' tests call it directly.
loss_world1     world_size == 1.
loss_gathered   world_size > 1, local_loss off: the world-1 loss of the gathered features.
loss_local      world_size > 1, local_loss on, as rank `rank` computes it: b rows of each direction, the x direction masked by
                M[rank*b : (rank+1)*b, :] and the y direction by M^T[rank*b : (rank+1)*b, :].
with_grads      value and gradients (torch autograd, float64) of any of the above.
clustered       seeded teacher features in near-duplicate clusters, and independent students.
check_inputs    the conditions the GPU tests require of such inputs (asserted in float64, before anything runs on a GPU).
"""
import torch
import torch.nn.functional as F


def keep_mask(t_rows, t_cols, thres, label_off=0):
    """bool [R, C]: element (r, c) is kept when c == r + label_off or not (t_rows[r] . t_cols[c] >= thres)."""
    sim = t_rows.detach().double() @ t_cols.detach().double().t()
    R, C = sim.shape
    eye = torch.arange(C)[None, :] == (torch.arange(R)[:, None] + label_off)
    return torch.logical_or(torch.logical_not(sim >= thres), eye)


def pair_loss(x, y, scale, keep, label_off=0, w_row=0.5, w_col=0.5):
    """x [R, E], y [C, E] (float64, may require grad), scale a float64 scalar (tensor or float), keep bool [R, C]."""
    logits = (scale * x @ y.t()) * keep.to(x.dtype)
    R = x.shape[0]
    labels = torch.arange(R) + label_off
    diag = logits[torch.arange(R), labels]
    loss = w_row * (torch.logsumexp(logits, dim=1) - diag).mean()
    if w_col:
        loss = loss + w_col * (torch.logsumexp(logits, dim=0)[labels] - diag).mean()
    return loss


def loss_world1(x, y, scale, thres):
    keep = keep_mask(x, x, thres)
    lx = (scale * x @ y.t()) * keep.to(x.dtype)
    ly = (scale * y @ x.t()) * keep.t().to(x.dtype)
    labels = torch.arange(x.shape[0])
    return (F.cross_entropy(lx, labels) + F.cross_entropy(ly, labels)) / 2


def loss_gathered(all_x, all_y, scale, thres):
    keep = keep_mask(all_x, all_x, thres)
    lx = (scale * all_x @ all_y.t()) * keep.to(all_x.dtype)
    labels = torch.arange(all_x.shape[0])
    return (F.cross_entropy(lx, labels) + F.cross_entropy(lx.t(), labels)) / 2


def loss_local(x, y, all_x, all_y, rank, scale, thres):
    b = x.shape[0]
    keep = keep_mask(all_x, all_x, thres)
    lx = (scale * x @ all_y.t()) * keep[rank * b:(rank + 1) * b].to(x.dtype)
    ly = (scale * y @ all_x.t()) * keep.t()[rank * b:(rank + 1) * b].to(x.dtype)
    labels = torch.arange(b) + rank * b
    return (F.cross_entropy(lx, labels) + F.cross_entropy(ly, labels)) / 2


def with_grads(fn, x, y, scale):
    """fn(x, y, scale) -> loss on float64 leaves; returns (loss, dx, dy, dscale) as float64 tensors / floats."""
    x = x.detach().double().clone().requires_grad_(True)
    y = y.detach().double().clone().requires_grad_(True)
    s = torch.tensor(float(scale), dtype=torch.float64, requires_grad=True)
    loss = fn(x, y, s)
    loss.backward()
    return float(loss.detach()), x.grad, y.grad, float(s.grad)


# ---- inputs -----------------------------------------------------------------------------------------------------------------
DIM = 64
NOISE = 0.037          # members = unit(centre + NOISE * N(0, I_64)): two members of one centre have cosine ~ 1 / (1 + 64 NOISE^2) = 0.92
CENTRES = 12           # unit centres a cluster may sit at


def clustered(n, seed, dim=DIM):
    """(teacher [n, dim], student [n, dim]) float32 unit vectors.  Teacher: clusters of 2-6 members, each a unit centre plus
    small noise, order shuffled.  The centre of a cluster is one of CENTRES random unit vectors, so that clusters which meet
    at a centre mask each other too: independent centres would mask (mean cluster size - 1) / n of a row, 1.2 % at n = 300,
    below the 5 % the tests ask for.  Students: independent unit vectors."""
    g = torch.Generator().manual_seed(seed)
    centres = F.normalize(torch.randn(CENTRES, dim, generator=g, dtype=torch.float64), dim=-1)
    rows = []
    while len(rows) < n:
        c = centres[int(torch.randint(0, CENTRES, (1,), generator=g))]
        for _ in range(int(torch.randint(2, 7, (1,), generator=g))):
            rows.append(F.normalize(c + NOISE * torch.randn(dim, generator=g, dtype=torch.float64), dim=-1))
    t = torch.stack(rows[:n])[torch.randperm(n, generator=g)]
    s = F.normalize(torch.randn(n, dim, generator=g, dtype=torch.float64), dim=-1)
    return t.float(), s.float()


def check_inputs(t_rows, t_cols, thres, label_off=0, margin=1e-3, lo=0.05, hi=0.50, block=64):
    """The conditions on a teacher block [R, dim] x [C, dim]; returns the masked fraction of the off-diagonal elements.
      * no off-diagonal |sim - thres| < margin (1e-3 is > 100x the 2^-17 error of the similarity GEMM: the kernels' mask
        and the float64 mask are the same set);
      * between `lo` and `hi` of the off-diagonal elements are masked;
      * every `block`-row block holds masked and kept off-diagonal elements."""
    sim = t_rows.double() @ t_cols.double().t()
    R, C = sim.shape
    off = ~(torch.arange(C)[None, :] == (torch.arange(R)[:, None] + label_off))
    assert float((sim - thres).abs()[off].min()) >= margin, float((sim - thres).abs()[off].min())
    masked = (sim >= thres) & off
    frac = float(masked.sum()) / float(off.sum())
    assert lo <= frac <= hi, frac
    for r0 in range(0, R, block):
        m, o = masked[r0:r0 + block], off[r0:r0 + block]
        assert bool(m.any()) and bool((o & ~m).any()), r0
    return frac
