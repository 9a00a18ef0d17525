"""The linear probe restated on tensors: Dropout -> BatchNorm1d(affine=False, eps=1e-6) -> Linear, nn.CrossEntropyLoss(), its
gradients, and LARS (You, Gitman, Ginsburg: "Large batch training of convolutional networks", in the MoCo v3 form the
reference ships: no weight decay and no trust ratio on tensors of one dimension).  Every function computes in the dtype it is
given: float64 is the yardstick of the GPU tests, float32 gives "the same computation in torch fp32 on the CPU" whose error
against float64 sizes their limit.  tests/test_linprobe_host.py pins this file to the imported reference."""
import numpy as np
import torch

import philox_ref

EPS = 1e-6            # nn.BatchNorm1d(lp_input_dim, affine=False, eps=1e-6)
BN_MOMENTUM = 0.1     # nn.BatchNorm1d's default


def dropout(x, keep, p):
    """nn.Dropout(p) in train mode with the mask given: kept elements times 1 / (1 - p), dropped ones 0."""
    if keep is None or p == 0.0:
        return x
    return x * keep.to(x.dtype) * (1.0 / (1.0 - p))


def philox_keep(seed, sample0, B, D, p):
    """The mask vl_lp_bn_fwd draws itself: element (b, d) is DROPPED when word d & 3 of Philox4x32-10 with counter
    (d >> 2, lo32(sample0 + b), hi32(sample0 + b), 0) and key (lo32(seed), hi32(seed)) is below floor(p 2^32)."""
    thr = np.uint64(int(float(np.float32(p)) * 4294967296.0))
    s = (np.uint64(sample0) + np.arange(B, dtype=np.uint64))[:, None]
    g = np.arange(D // 4, dtype=np.uint64)[None, :]
    z = np.zeros((B, D // 4), dtype=np.uint64)
    w = philox_ref.philox4x32_10(g + z, (s & philox_ref.M32) + z, (s >> np.uint64(32)) + z, z, seed & 0xFFFFFFFF, seed >> 32)
    words = np.stack(w, axis=-1).reshape(B, D)
    return torch.from_numpy(words >= thr)


def bn_train(x, running_mean, running_var, momentum=BN_MOMENTUM, eps=EPS):
    """Batch statistics: -> xhat, mean, biased var, new running_mean, new running_var (the unbiased variance goes there)."""
    B = x.shape[0]
    mean = x.mean(0)
    var = ((x - mean) ** 2).mean(0)
    xhat = (x - mean) / torch.sqrt(var + eps)
    rm = (1 - momentum) * running_mean + momentum * mean
    rv = (1 - momentum) * running_var + momentum * var * B / (B - 1)
    return xhat, mean, var, rm, rv


def bn_eval(x, running_mean, running_var, eps=EPS):
    return (x - running_mean) / torch.sqrt(running_var + eps)


def ce(logits, target, gscale=1.0):
    """nn.CrossEntropyLoss() (mean) -> loss, G = gscale (softmax - onehot) / B, dbias = G's column sums."""
    B, C = logits.shape
    lse = torch.logsumexp(logits, dim=1)
    loss = (lse - logits.gather(1, target[:, None])[:, 0]).mean()
    G = torch.exp(logits - lse[:, None])
    G[torch.arange(B), target] -= 1.0
    G = G * (gscale / B)
    return loss, G, G.sum(0)


def clip_coef(sumsq, max_norm, grad_scale=1.0):
    """torch.nn.utils.clip_grad_norm_'s coefficient for the gradient grad_scale * g, |g|^2 = sumsq; 1 without a max_norm."""
    if max_norm is None or not max_norm > 0:
        return 1.0
    return min(1.0, max_norm / (grad_scale * float(sumsq) ** 0.5 + 1e-6))


def lars_step(slots, lr, momentum=0.9, trust=1e-3, grad_scale=1.0, max_norm=None, decay_bias=False):
    """LARS.step on slots = dicts of p, g, mu (tensors of one dtype), wd, adapt -> new (p, mu) per slot; inputs untouched.
    decay_bias: the WRONG rule (weight decay on every tensor), for the test that tells the two apart."""
    sumsq = sum(float((s["g"].double() ** 2).sum()) for s in slots)
    c = grad_scale * clip_coef(sumsq, max_norm, grad_scale)
    out = []
    for s in slots:
        p, mu = s["p"], s["mu"]
        dp = s["g"] * c
        if s["adapt"]:
            dp = dp + s["wd"] * p
            pn, dn = torch.linalg.vector_norm(p), torch.linalg.vector_norm(dp)
            q = trust * pn / dn if (pn > 0 and dn > 0) else 1.0
            dp = dp * q
        elif decay_bias:
            dp = dp + s["wd"] * p
        mu = momentum * mu + dp
        out.append((p - lr * mu, mu))
    return out


def rank(logits, target):
    """rank_b = #{c: logits[b,c] > logits[b,t]} + #{c < t: logits[b,c] == logits[b,t]} (a NaN compares false)."""
    v = logits.gather(1, target[:, None])
    c = torch.arange(logits.shape[1])[None, :]
    return ((logits > v) | ((logits == v) & (c < target[:, None]))).sum(1)


class Head:
    """The probe head and its optimizer state in one dtype: forward, backward and LARS as ProbeHead runs them."""

    def __init__(self, weight, bias, dtype=torch.float64, p=0.0, wd=0.0, momentum=0.9, trust=1e-3, decay_bias=False):
        self.dt = dtype
        self.w, self.b = weight.to(dtype).clone(), bias.to(dtype).clone()
        D = weight.shape[1]
        self.rm, self.rv = torch.zeros(D, dtype=dtype), torch.ones(D, dtype=dtype)
        self.mu_w, self.mu_b = torch.zeros_like(self.w), torch.zeros_like(self.b)
        self.p, self.wd, self.momentum, self.trust, self.decay_bias = p, wd, momentum, trust, decay_bias

    def forward(self, feat, train, keep=None):
        x = feat.to(self.dt)
        if train:
            self.xd = dropout(x, keep, self.p)
            self.xhat, self.mean, self.var, self.rm, self.rv = bn_train(self.xd, self.rm, self.rv)
        else:
            self.xhat = bn_eval(x, self.rm, self.rv)
        self.logits = self.xhat @ self.w.t() + self.b
        return self.logits

    def backward(self, target):
        self.loss, self.G, self.db = ce(self.logits, target)
        self.dw = self.G.t() @ self.xhat
        return self.loss

    def step(self, lr, grad_scale=1.0, max_norm=None):
        slots = [dict(p=self.w, g=self.dw, mu=self.mu_w, wd=self.wd, adapt=True),
                 dict(p=self.b, g=self.db, mu=self.mu_b, wd=self.wd, adapt=False)]
        (self.w, self.mu_w), (self.b, self.mu_b) = lars_step(slots, lr, self.momentum, self.trust, grad_scale, max_norm,
                                                             decay_bias=self.decay_bias)


def case_inputs(index, B, C, steps=4, image_size=32):
    """The batches of recorded case `index`: (x [steps, B, 3, S, S], target int64 [steps, B]) from one seeded generator."""
    g = torch.Generator().manual_seed(610 + index)
    x = torch.randn(steps, B, 3, image_size, image_size, generator=g)
    target = torch.randint(0, C, (steps, B), generator=g)
    target[:, 0], target[:, 1] = 0, C - 1
    return x, target
