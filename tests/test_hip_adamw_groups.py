"""GPU: vl_adamw_multi_step_groups - the multi-tensor AdamW launch with a learning-rate scale per tensor and tensors that are
exempt from gradient clipping (the OpenShape recipe's optimizer: `backbone.transformer` at 0.1 x lr, the logit scale outside
clip_grad_norm_'s parameter list).

The table: tensors of 1, 3, 2047, 2048, 2049 and 4096 + 5 elements, in that order (repeated), so that the 2048-element tiles
straddle tensors with different settings; 1, 7 and 130 slots; lr_scale in {1, 0.1}, weight_decay in {0, 0.2}; the exempt tensor
first, in the middle and last.  Every operand is a view into a larger NaN-filled allocation, some 16-byte aligned (the kernel's
vector path) and some not (its scalar path).

Bound against float64: the one tests/test_hip_grad_clip.py (test_adamw_multi_matches_torch_clip_and_adamw) uses for the same
quantities against its float64 run - relative error of parameters, first and second moments below 1e-5 per tensor.  The norm:
within 4 ulp of float32 of the float64 norm, as there."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

ULP = 2.0 ** -23
SIZES = (1, 3, 2047, 2048, 2049, 4096 + 5)
KW = dict(lr=1e-2, beta1=0.9, beta2=0.98, eps=1e-6)
WD = 0.2
NAN = float("nan")


def relerr(a, b):          # (tests/test_hip_grad_clip.py: relerr)
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


class Arena:
    """Tensors of `sizes` as views into one NaN-filled device allocation, with NaN gaps between them; every third view starts
    off the 16-byte grid."""

    def __init__(self, sizes):
        off, self.spans = 8, []
        for i, n in enumerate(sizes):
            start = (off + 3) // 4 * 4 + (1 if i % 3 == 1 else 0)
            self.spans.append((start, n))
            off = start + n + 5
        self.buf = torch.full((off + 8,), NAN, device="cuda")
        self.views = [self.buf[s:s + n] for s, n in self.spans]
        self.outside = torch.ones(off + 8, dtype=torch.bool)
        for s, n in self.spans:
            self.outside[s:s + n] = False

    def fill(self, tensors):
        for v, t in zip(self.views, tensors):
            v.copy_(t)

    def untouched_outside(self):
        return bool(torch.isnan(self.buf.cpu()[self.outside]).all())


class Table:
    """A slot table over four arenas, its per-slot settings, and the launches."""

    def __init__(self, nslots, seed, exempt=None, uniform=False):
        from vitlens_hip import train as TR
        self.sizes = [SIZES[i % len(SIZES)] for i in range(nslots)]
        self.gen = torch.Generator().manual_seed(seed)
        self.p0 = [torch.randn(n, generator=self.gen) for n in self.sizes]
        self.P, self.G, self.M, self.V = (Arena(self.sizes) for _ in range(4))
        self.P.fill(self.p0)
        self.M.fill([torch.zeros(n) for n in self.sizes]); self.V.fill([torch.zeros(n) for n in self.sizes])
        self.lr_scale = [1.0 if uniform else (1.0, 0.1)[i % 2] for i in range(nslots)]
        self.wd = [(0.0, WD)[(i // 2) % 2] for i in range(nslots)]
        self.exempt = None if exempt is None else {"first": 0, "middle": nslots // 2, "last": nslots - 1}[exempt]
        rows = [(self.P.views[i].data_ptr(), self.G.views[i].data_ptr(), self.M.views[i].data_ptr(), self.V.views[i].data_ptr(),
                 self.sizes[i], self.wd[i]) for i in range(nslots)]
        self.slots = TR.pack_adamw_slots(rows).cuda()
        self.groups_host = TR.pack_adamw_groups([(self.lr_scale[i], i == self.exempt) for i in range(nslots)])
        self.groups = self.groups_host.cuda()
        self.norm = torch.zeros((), device="cuda")
        self.t = 0

    def clipped(self):
        return [i for i in range(len(self.sizes)) if i != self.exempt]

    def new_grads(self, scale):
        gr = [torch.randn(n, generator=self.gen) * scale for n in self.sizes]
        self.G.fill(gr)
        return gr

    def sumsq(self, grads):
        """The squared norm of the clipped set: one vl_sumsq_f32 call over their gradients laid out contiguously."""
        from vitlens_hip import ops
        idx = self.clipped()
        flat = torch.cat([grads[i] for i in idx]).cuda() if idx else torch.zeros(0, device="cuda")
        return ops.grad_sumsq(flat)

    def step_groups(self, grads, grad_scale, max_norm):
        from vitlens_hip import ops
        self.t += 1
        ops.adamw_multi_step_groups(self.slots, self.groups, self.groups_host, len(self.sizes), KW["lr"], KW["beta1"], KW["beta2"],
                                    KW["eps"], self.t, grad_scale, max_norm, self.sumsq(grads), self.norm)

    def step_plain(self, grads, grad_scale, max_norm):
        from vitlens_hip import ops
        self.t += 1
        ops.adamw_multi(self.slots, len(self.sizes), KW["lr"], KW["beta1"], KW["beta2"], KW["eps"], self.t, grad_scale, max_norm,
                        self.sumsq(grads), self.norm)

    def assert_nothing_outside(self, grads):
        torch.cuda.synchronize()
        for name, a in (("p", self.P), ("g", self.G), ("m", self.M), ("v", self.V)):
            assert a.untouched_outside(), (name, "written outside the tensors")
        for i, g in enumerate(grads):
            assert torch.equal(self.G.views[i].cpu(), g), (i, "the gradient changed")


def ref64_optimizer(params, groups, lr, betas, eps):
    """torch.optim.AdamW over float64 `params` {name: tensor} with one torch parameter group per tensor: `groups`
    {name: (lr_scale, weight_decay)}.  (Also the reference of tests/test_hip_openshape_step.py.)"""
    return torch.optim.AdamW([{"params": [p], "lr": lr * groups[k][0], "weight_decay": groups[k][1]} for k, p in params.items()],
                             lr=lr, betas=betas, eps=eps)


class Ref64:
    """torch.optim.AdamW in float64 with the table's groups and torch.nn.utils.clip_grad_norm_ over the non-exempt tensors only."""

    def __init__(self, tb):
        self.tb = tb
        self.p = [p.double().requires_grad_(True) for p in tb.p0]
        self.opt = ref64_optimizer(dict(enumerate(self.p)), {i: (tb.lr_scale[i], tb.wd[i]) for i in range(len(self.p))},
                                   KW["lr"], (KW["beta1"], KW["beta2"]), KW["eps"])

    def step(self, grads, grad_scale, max_norm):
        for p, g in zip(self.p, grads):
            p.grad = g.double() * grad_scale
        clipped = [self.p[i] for i in self.tb.clipped()]
        total = float(torch.nn.utils.clip_grad_norm_(clipped, max_norm, norm_type=2.0)) if clipped else 0.0
        self.opt.step()
        return total

    def moments(self, i):
        st = self.opt.state[self.p[i]]
        return st["exp_avg"], st["exp_avg_sq"]


# ------------------------------------------------------------------------------------------------ (a)
@pytest.mark.parametrize("nslots", [1, 7, 130])
def test_ones_and_no_exempt_tensor_are_the_plain_entry_bit_for_bit(nslots):
    a, b = Table(nslots, 21, uniform=True), Table(nslots, 21, uniform=True)
    for it in range(3):
        # step 0 clips (norms of hundreds against 1.0), step 2 does not
        scale = (1.0, 1.0, 1e-4)[it]
        ga, gb = a.new_grads(scale), b.new_grads(scale)
        assert all(torch.equal(x, y) for x, y in zip(ga, gb))
        a.step_groups(ga, 0.5, 1.0)
        b.step_plain(gb, 0.5, 1.0)
    torch.cuda.synchronize()
    assert torch.equal(a.norm.view(torch.int32), b.norm.view(torch.int32))
    for i in range(nslots):
        for name, x, y in (("p", a.P, b.P), ("m", a.M, b.M), ("v", a.V, b.V)):
            assert torch.equal(x.views[i].view(torch.int32), y.views[i].view(torch.int32)), (i, name)
        assert not torch.equal(a.P.views[i].cpu(), a.p0[i]), (i, "did not move")
    a.assert_nothing_outside(ga)


# ------------------------------------------------------------------------------------------------ (b), (d), (e)
@pytest.mark.parametrize("grad", ["clipping", "inside"])
@pytest.mark.parametrize("exempt", ["first", "middle", "last"])
@pytest.mark.parametrize("nslots", [1, 7, 130])
def test_groups_against_float64_adamw_with_partial_clipping(nslots, exempt, grad):
    """Three steps.  `clipping`: unit-variance gradients, norms of tens to hundreds against max_norm 1: the coefficient is far
    below 1.  `inside`: gradients of 1e-4, norms below 0.05: the coefficient is 1."""
    tb = Table(nslots, 33, exempt=exempt)
    ref = Ref64(tb)
    scale, grad_scale, max_norm = (1.0 if grad == "clipping" else 1e-4), 0.5, 1.0
    for it in range(3):
        grads = tb.new_grads(scale)
        total = ref.step(grads, grad_scale, max_norm)
        tb.step_groups(grads, grad_scale, max_norm)
        # (d) the norm that comes back is the clipped set's, not the table's
        n_set = math.sqrt(sum(float(grads[i].double().pow(2).sum()) for i in tb.clipped())) * grad_scale
        n_all = math.sqrt(sum(float(g.double().pow(2).sum()) for g in grads)) * grad_scale
        got = float(tb.norm)
        assert abs(total - n_set) <= 1e-12 * max(n_set, 1e-300)
        assert abs(got - n_set) <= 4 * ULP * n_set, (got, n_set)
        if nslots > 1:
            assert (n_set > max_norm) == (grad == "clipping")
            # (a one-element exempt tensor moves the table's norm by less than the bound above: nothing to tell apart there)
            separable = abs(n_all - n_set) > 16 * ULP * n_all
            assert separable or tb.sizes[tb.exempt] == 1
            assert not separable or abs(got - n_all) > 4 * ULP * n_all, "the exempt tensor is in the norm"
    tb.assert_nothing_outside(grads)          # (e)
    worst = {"p": 0.0, "m": 0.0, "v": 0.0}
    for i in range(nslots):
        m64, v64 = ref.moments(i)
        e = {"p": relerr(tb.P.views[i], ref.p[i].detach()), "m": relerr(tb.M.views[i], m64), "v": relerr(tb.V.views[i], v64)}
        for k in e:
            worst[k] = max(worst[k], e[k])
        assert e["p"] < 1e-5 and e["m"] < 1e-5 and e["v"] < 1e-5, (i, tb.sizes[i], tb.lr_scale[i], tb.wd[i], i == tb.exempt, e)
    print(f"adamw groups {nslots} slots exempt {exempt} {grad}: worst rel err p {worst['p']:.3e} m {worst['m']:.3e} v {worst['v']:.3e}")
    # the settings are felt: a 0.1 x tensor moved about a tenth as far as a 1 x tensor (slots 4 and 5: 2049 and 4101 elements, no
    # decay, scales 1 and 0.1)
    if nslots >= 7:
        big = [i for i in range(nslots) if tb.sizes[i] >= 2047 and tb.wd[i] == 0.0]
        assert {tb.lr_scale[i] for i in big} == {1.0, 0.1}
        for i in big:
            moved = float((tb.P.views[i].cpu() - tb.p0[i]).abs().mean())
            want = 3 * KW["lr"] * tb.lr_scale[i]          # three Adam steps of about lr * lr_scale each
            assert 0.3 * want < moved < 1.5 * want, (i, tb.lr_scale[i], moved, want)


# ------------------------------------------------------------------------------------------------ (c)
@pytest.mark.parametrize("exempt", ["first", "middle", "last"])
@pytest.mark.parametrize("nslots", [7, 130])
def test_exempt_tensor_is_updated_as_in_a_table_of_its_own_without_clipping(nslots, exempt):
    from vitlens_hip import ops, train as TR
    tb = Table(nslots, 44, exempt=exempt)
    i = tb.exempt
    n, ls, wd = tb.sizes[i], tb.lr_scale[i], tb.wd[i]
    alone = [torch.full((n + 16,), NAN, device="cuda") for _ in range(4)]
    p, g, m, v = (t[4:4 + n] for t in alone) if tb.P.spans[i][0] % 4 == 0 else (t[5:5 + n] for t in alone)
    p.copy_(tb.p0[i]); m.zero_(); v.zero_()
    solo = [t.clone() for t in (p, m, v)]          # the per-tensor kernel's copy, for a scale of 1
    slots = TR.pack_adamw_slots([(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), n, wd)]).cuda()
    gh = TR.pack_adamw_groups([(ls, True)])
    gd = gh.cuda()
    for it in range(3):
        grads = tb.new_grads(1.0)
        tb.step_groups(grads, 0.5, 1.0)          # the table clips hard (coefficient about 1e-2)
        g.copy_(grads[i])
        # the lone table: exempt as well, and handed a squared norm that would clip everything to nothing
        ops.adamw_multi_step_groups(slots, gd, gh, 1, KW["lr"], KW["beta1"], KW["beta2"], KW["eps"], it + 1, 0.5, 1.0,
                                    torch.full((1,), 1e30, device="cuda"))
        if ls == 1.0:
            ops.adamw_step(solo[0], g, solo[1], solo[2], KW["lr"], KW["beta1"], KW["beta2"], KW["eps"], wd, it + 1, 0.5)
    torch.cuda.synchronize()
    for name, mine, lone in (("p", tb.P, p), ("m", tb.M, m), ("v", tb.V, v)):
        assert torch.equal(mine.views[i].view(torch.int32), lone.view(torch.int32)), (name, "the exempt tensor felt the table")
    if ls == 1.0:
        for name, lone, s in (("p", p, solo[0]), ("m", m, solo[1]), ("v", v, solo[2])):
            assert torch.equal(lone.view(torch.int32), s.view(torch.int32)), (name, "differs from vl_adamw_step")
    assert not torch.equal(p.cpu(), tb.p0[i])


# ------------------------------------------------------------------------------------------------ (f)
@pytest.mark.parametrize("bad", [float("nan"), float("inf"), -float("inf"), -0.5])
def test_bad_lr_scale_is_refused_and_nothing_is_written(bad):
    import ctypes as C
    from vitlens_hip import _lib, ops, train as TR
    tb = Table(7, 55, exempt="middle")
    grads = tb.new_grads(1.0)
    sumsq = tb.sumsq(grads)
    rows = [(tb.lr_scale[i], i == tb.exempt) for i in range(7)]
    rows[5] = (bad, False)
    gh = TR.pack_adamw_groups(rows)
    gd = gh.cuda()
    with pytest.raises(RuntimeError, match="lr_scale"):
        ops.adamw_multi_step_groups(tb.slots, gd, gh, 7, KW["lr"], KW["beta1"], KW["beta2"], KW["eps"], 1, 1.0, 1.0, sumsq, tb.norm)
    lib = _lib.load_library()
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    args = (C.c_void_p(tb.slots.data_ptr()), C.c_void_p(gd.data_ptr()), C.c_void_p(gh.data_ptr()))
    tail = (KW["lr"], KW["beta1"], KW["beta2"], KW["eps"], 1, 1.0, 1.0, C.c_void_p(sumsq.data_ptr()), None, s)
    assert lib.vl_adamw_multi_step_groups(*args, 7, *tail) != 0
    good = C.c_void_p(tb.groups_host.data_ptr())
    assert lib.vl_adamw_multi_step_groups(args[0], args[1], None, 7, *tail) != 0               # no host copy to check
    assert lib.vl_adamw_multi_step_groups(args[0], args[1], good, 1025, *tail) != 0
    assert lib.vl_adamw_multi_step_groups(args[0], args[1], good, 7, KW["lr"], 0.9, 0.98, 1e-6, 0, 1.0, 1.0, tail[7], None, s) != 0
    assert lib.vl_adamw_multi_step_groups(args[0], args[1], good, 7, KW["lr"], 0.9, 0.98, 1e-6, 1, 1.0, 0.0, tail[7], None, s) != 0
    with pytest.raises(ValueError):
        TR.AdamW({"w": torch.zeros(4, device="cuda")}, lr_scale={"w": bad})
    with pytest.raises(ValueError):
        TR.AdamW({"w": torch.zeros(4, device="cuda")}, no_clip=["missing"])
    torch.cuda.synchronize()
    for i in range(7):
        assert torch.equal(tb.P.views[i].cpu(), tb.p0[i]), (i, "written")
        assert not bool(tb.M.views[i].any()) and not bool(tb.V.views[i].any()), i
    assert float(tb.norm) == 0.0
    tb.assert_nothing_outside(grads)


# ------------------------------------------------------------------------------------------------ the Python optimizer
def test_python_adamw_takes_the_groups_and_existing_callers_change_nothing():
    """`AdamW(lr_scale=, no_clip=, decay=)`: the clipped step against float64 (bound: as above); without the new arguments the
    optimizer takes the launch it always took (no group table is built)."""
    from vitlens_hip import ops, train as TR
    g = torch.Generator().manual_seed(66)
    shapes = {"logit_scale": (), "trunk.w": (33, 65), "trunk.ln.bias": (65,), "lens.w_il": (40, 52), "lens.norm.weight": (52,)}
    p0 = {k: torch.randn(s, generator=g) for k, s in shapes.items()}
    mine = {k: v.clone().cuda() for k, v in p0.items()}
    lr_scale = {"trunk.w": 0.1, "trunk.ln.bias": 0.1}
    decay = {"lens.w_il": True, "lens.norm.weight": False}
    opt = TR.AdamW(mine, lr=1e-2, betas=(0.9, 0.98), eps=1e-6, weight_decay=0.2, lr_scale=lr_scale, no_clip=["logit_scale"], decay=decay)
    plain = TR.AdamW({k: v.clone() for k, v in mine.items()}, lr=1e-2)
    assert opt._grouped and not plain._grouped
    ref = {k: v.double().requires_grad_(True) for k, v in p0.items()}
    dec = lambda k: decay.get(k, TR.AdamW.decays(k, p0[k]))
    topt = torch.optim.AdamW([{"params": [ref[k]], "lr": 1e-2 * lr_scale.get(k, 1.0), "weight_decay": 0.2 if dec(k) else 0.0} for k in ref],
                             lr=1e-2, betas=(0.9, 0.98), eps=1e-6)
    # the flat buffer of a step: the exempt tensor first, the clipped set one contiguous range behind it
    al = lambda n: (n + 3) // 4 * 4
    flat = torch.zeros(sum(al(v.numel()) for v in p0.values()), device="cuda")
    views, off = {}, 0
    for k, v in p0.items():
        views[k] = flat[off:off + v.numel()].view(v.shape); off += al(v.numel())
    for it in range(3):
        grads = {k: torch.randn(shapes[k], generator=g) for k in p0}
        for k in ref:
            ref[k].grad = grads[k].double()
            views[k].copy_(grads[k])
        total = float(torch.nn.utils.clip_grad_norm_([ref[k] for k in ref if k != "logit_scale"], 1.0))
        topt.step()
        opt.step(views, max_norm=1.0, sumsq=ops.grad_sumsq(flat[4:]))
        assert abs(float(opt.last_grad_norm) - total) <= 4 * ULP * total
    for k in ref:
        st = topt.state[ref[k]]
        e = (relerr(mine[k], ref[k].detach()), relerr(opt.m[k], st["exp_avg"]), relerr(opt.v[k], st["exp_avg_sq"]))
        assert max(e) < 1e-5, (k, e)
    # without `sumsq` the optimizer reduces the clipped tensors itself: the same set
    again = TR.AdamW({k: v.clone().cuda() for k, v in p0.items()}, lr=1e-2, lr_scale=lr_scale, no_clip=["logit_scale"], decay=decay)
    again.step(views, max_norm=1.0)
    assert abs(float(again.last_grad_norm) - total) <= 4 * ULP * total
    # the unclipped per-tensor loop scales the learning rate too
    loop = TR.AdamW({k: v.clone().cuda() for k, v in p0.items()}, lr=1e-2, lr_scale=lr_scale, decay=decay)
    loop.step(views)
    one = TR.AdamW({k: v.clone().cuda() for k, v in p0.items()}, lr=1e-2, lr_scale=lr_scale, no_clip=["logit_scale"], decay=decay)
    one.step(views, max_norm=1e30)
    for k in p0:
        assert torch.equal(loop.params[k], one.params[k]), k
