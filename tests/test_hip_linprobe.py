"""GPU: the linear probe's kernels (csrc/vl_linprobe.hip), ProbeHead / LinearProbeStep and the module path.

Every fp32 kernel output is compared with tests/linprobe_ref.py in fp64.  The limit per tensor is

    max-abs error <= max(4 x the error of the same computation in torch fp32 on the CPU against fp64, 1e-5 max|ref|)

(4: another summation order; 1e-5: the project's fp32 criterion).  Operands sit inside larger, NaN-filled allocations, so a
read or a write outside them shows.  The measured errors are collected in ERRORS (written out when VITLENS_LINPROBE_ERRORS
names a file: profiles/linprobe_errors.json is such a run)."""
import json
import math
import os
import struct
import tempfile
import warnings
from types import SimpleNamespace

import pytest
import torch

import linprobe_ref as LR
from golden_util import load_npz, seeded_like, split

pytestmark = pytest.mark.gpu

DEV = "cuda"
NAN = float("nan")
PAD = 64                     # guard elements on either side of an operand (256 bytes: alignment is kept)
ERRORS = {}


@pytest.fixture(scope="module", autouse=True)
def _write_errors():
    yield
    path = os.environ.get("VITLENS_LINPROBE_ERRORS")
    if path:
        with open(path, "w") as f:
            json.dump(ERRORS, f, indent=1, sort_keys=True)


def ops():
    from vitlens_hip import ops as o
    return o


class Guarded:
    """A [rows, cols] operand at row stride ld inside a larger allocation filled with `fill`; intact() says whether everything
    outside the operand still holds the fill."""

    def __init__(self, rows, cols, ld=None, dtype=torch.float32, fill=NAN, src=None):
        ld = cols if ld is None else ld
        self.rows, self.cols, self.ld, self.fill = rows, cols, ld, fill
        self.buf = torch.full((2 * PAD + rows * ld,), fill, dtype=dtype, device=DEV)
        self.full = self.buf[PAD:PAD + rows * ld].view(rows, ld)
        self.t = self.full[:, :cols]
        if src is not None:
            self.t.copy_(src.to(DEV))

    def _is_fill(self, x):
        return x.isnan() if (self.fill != self.fill) else (x == self.fill)

    def intact(self):
        n = self.rows * self.ld
        ok = bool(self._is_fill(self.buf[:PAD]).all()) and bool(self._is_fill(self.buf[PAD + n:]).all())
        return ok and bool(self._is_fill(self.full[:, self.cols:]).all())


def vec(n, dtype=torch.float32, fill=NAN, src=None):
    g = Guarded(1, n, dtype=dtype, fill=fill, src=None if src is None else src.reshape(1, -1))
    g.v = g.t[0]
    return g


def check(name, got, ref64, ref32):
    """got (device or CPU tensor) against the fp64 reference at the limit of the module docstring; records the figures."""
    got, ref64 = got.detach().double().cpu(), ref64.double()
    err = float((got - ref64).abs().max()) if got.numel() else 0.0
    base = float((ref32.double() - ref64).abs().max()) if got.numel() else 0.0
    top = float(ref64.abs().max()) if got.numel() else 0.0
    limit = max(4.0 * base, 1e-5 * top)
    ERRORS[name] = {"err": err, "torch_fp32_err": base, "max_abs_ref": top, "limit": limit}
    print(f"{name}: err {err:.3e}  torch-fp32 err {base:.3e}  max|ref| {top:.3e}  limit {limit:.3e}")
    assert got.shape == ref64.shape, (name, got.shape, ref64.shape)
    assert err <= limit, (name, err, limit)


# ---- vl_lp_bn_fwd -------------------------------------------------------------------------------------------------------
BN_SHAPES = ((2, 64), (6, 64), (67, 200), (257, 1024))


def bn_input(B, D, seed=0):
    """LayerNorm-like rows; the first half of the columns sits at a mean of 100 x its spread (E[x^2] - mean^2 loses them)."""
    g = torch.Generator().manual_seed(1000 + B * 7 + D + seed)
    x = torch.randn(B, D, generator=g)
    x[:, :D // 2] = x[:, :D // 2] * 0.3 + 30.0
    return x


@pytest.mark.parametrize("mode", ("mask", "p0", "eval"))
@pytest.mark.parametrize("B,D", BN_SHAPES)
def test_lp_bn_fwd(B, D, mode):
    o = ops()
    x = bn_input(B, D)
    g = torch.Generator().manual_seed(B + D)
    p = 0.25 if mode == "mask" else 0.0
    keep = (torch.rand(B, D, generator=g) >= p) if mode == "mask" else None
    rm0, rv0 = torch.randn(D, generator=g) * 0.1, torch.rand(D, generator=g) + 0.5
    ldt = LR_pad4(B) + 4
    gx = Guarded(B, D, ld=D + 4, src=x)
    gh, gt = Guarded(B, D, ld=D + 8), Guarded(D, ldt)
    gm, gv = vec(D), vec(D)
    grm, grv = vec(D, src=rm0), vec(D, src=rv0)
    gk = Guarded(B, D, dtype=torch.uint8, fill=1, src=keep) if keep is not None else None
    train = mode != "eval"
    tag = f"bn/{mode}/B{B}_D{D}/"
    for call in range(2 if train else 1):
        o.lp_bn_fwd(gx.t, grm.v, grv.v, train, p=p, keep=None if gk is None else gk.t, xhat=gh.t,
                    xhatT=gt.t if train else None, mean=gm.v if train else None, var=gv.v if train else None)
    torch.cuda.synchronize()
    for G in (gx, gh, gm, gv, grm, grv):
        assert G.intact()
    assert torch.equal(gx.t.cpu(), x)
    refs = {}
    for dt in (torch.float64, torch.float32):
        xd = LR.dropout(x.to(dt), keep, p)
        if train:
            rm, rv = rm0.to(dt), rv0.to(dt)
            for call in range(2):
                xhat, mean, var, rm, rv = LR.bn_train(xd, rm, rv)
            refs[dt] = dict(xhat=xhat, mean=mean, var=var, running_mean=rm, running_var=rv)
        else:
            refs[dt] = dict(xhat=LR.bn_eval(x.to(dt), rm0.to(dt), rv0.to(dt)))
    got = dict(xhat=gh.t, mean=gm.v, var=gv.v, running_mean=grm.v, running_var=grv.v)
    for k in refs[torch.float64]:
        check(tag + k, got[k], refs[torch.float64][k], refs[torch.float32][k])
    if train:
        assert gt.intact()
        assert torch.equal(gt.t[:, :B], gh.t.t())                                # the transpose, bit for bit
        assert bool((gt.t[:, B:] == 0).all())                                    # zeros behind column B
    else:
        assert torch.equal(grm.v.cpu(), rm0) and torch.equal(grv.v.cpu(), rv0)      # eval touches no statistic
        assert bool(gm.v.isnan().all()) and bool(gt.full.isnan().all())


def LR_pad4(n):
    return (n + 3) // 4 * 4


def _own_mask(o, x, p, seed, sample0):
    """The mask of the kernel's own draw, read off its output: with positive inputs the dropped elements of a column share its
    smallest normalised value."""
    B, D = x.shape
    rm, rv = torch.zeros(D, device=DEV), torch.ones(D, device=DEV)
    xhat = o.lp_bn_fwd(x, rm, rv, True, p=p, seed=seed, sample0=sample0)
    return xhat > xhat.min(dim=0, keepdim=True).values


def test_lp_bn_fwd_own_philox_draw():
    o = ops()
    B, D, p = 257, 1024, 0.25
    x = (1.0 + torch.rand(B, D, generator=torch.Generator().manual_seed(5))).to(DEV)
    seed, s0 = 0x1234567887654321, (1 << 40) + 17
    m = _own_mask(o, x, p, seed, s0)
    frac = float(m.double().mean())
    print("kept fraction", frac)
    assert abs(frac - 0.75) <= 5.1e-3                                             # 6 sigma, sigma = sqrt(.25 * .75 / 263168)
    assert torch.equal(m, _own_mask(o, x, p, seed, s0))                           # the same seed and sample0: the same mask
    assert torch.equal(m.cpu(), LR.philox_keep(seed, s0, B, D, p))                # and it is the documented generator
    part = _own_mask(o, x[100:].contiguous(), p, seed, s0 + 100)                  # a piece of the batch draws its own rows
    assert torch.equal(part, m[100:])
    other = _own_mask(o, x, p, seed + 1, s0)
    assert float((other != m).double().mean()) > 0.3


def test_lp_bn_fwd_refusals():
    o = ops()
    from vitlens_hip import _lib
    lib = _lib.load_library()
    x = torch.randn(4, 8, device=DEV)
    rm, rv, out = torch.zeros(8, device=DEV), torch.ones(8, device=DEV), torch.full((4, 8), NAN, device=DEV)
    P = lambda t: None if t is None else t.data_ptr()
    def call(B=4, D=8, p=0.0, train=1, ldx=8, ldh=8, xhatT=None, ldt=0, rmean=rm):
        return lib.vl_lp_bn_fwd(P(x), ldx, None, p, 0, 0, train, P(rmean), P(rv), 0.1, 1e-6, P(out), ldh, P(xhatT), ldt, None, None,
                                B, D, None)
    assert call(B=1) != 0 and b"B >= 2" in lib.vl_last_error()
    assert call(D=6) != 0 and b"multiple of 4" in lib.vl_last_error()
    assert call(p=1.0) != 0 and b"[0, 1)" in lib.vl_last_error()
    assert call(ldx=6) != 0
    assert call(train=0, rmean=None) != 0 and b"running" in lib.vl_last_error()
    assert call(xhatT=out, ldt=6) != 0 and b"ldt" in lib.vl_last_error()
    torch.cuda.synchronize()
    assert bool(out.isnan().all())                                               # refused without a launch
    with pytest.raises(ValueError):
        o.lp_bn_fwd(x[:1], rm, rv, True)
    with pytest.raises(RuntimeError):
        o.lp_bn_fwd(x.cpu(), rm.cpu(), rv.cpu(), True)                             # no CPU path


# ---- vl_ce_label ----------------------------------------------------------------------------------------------------------
def ce_case(B, C, big=False):
    g = torch.Generator().manual_seed(B * 1000 + C)
    logits = torch.randn(B, C, generator=g) * (30.0 if big else 3.0)
    if big:
        logits.clamp_(-80.0, 80.0)
        logits[0, 0], logits[1, C - 1] = 80.0, -80.0
    target = torch.randint(0, C, (B,), generator=g)
    target[0], target[1] = 0, C - 1
    return logits, target


def run_ce(o, logits, target, gscale=1.0):
    B, C = logits.shape
    gl = Guarded(B, C, ld=C + 3, src=logits)
    gg, ggt = Guarded(B, C, ld=C + 5), Guarded(C, LR_pad4(B) + 4)
    gdb, gloss = vec(C), vec(1)
    tg = vec(B, dtype=torch.int64, fill=-7, src=target)
    o.ce_label(gl.t, tg.v, gscale=gscale, loss=gloss.v, G=gg.t, GT=ggt.t, dbias=gdb.v)
    torch.cuda.synchronize()
    return gl, gg, ggt, gdb, gloss, tg


@pytest.mark.parametrize("B", (2, 67, 257))
@pytest.mark.parametrize("C", (1, 2, 7, 64, 65, 1000, 1030))
def test_ce_label(B, C):
    o = ops()
    big = (B, C) == (67, 1000)                                                    # the case with logits in +-80
    logits, target = ce_case(B, C, big)
    gscale = 0.5 if C == 7 else 1.0
    gl, gg, ggt, gdb, gloss, tg = run_ce(o, logits, target, gscale)
    for G in (gl, gg, ggt, gdb, gloss, tg):
        assert G.intact()
    r64, r32 = LR.ce(logits.double(), target, gscale), LR.ce(logits.clone(), target, gscale)
    tag = f"ce/B{B}_C{C}{'_pm80' if big else ''}/"
    check(tag + "loss", gloss.v, r64[0].reshape(1), r32[0].reshape(1))
    check(tag + "G", gg.t, r64[1], r32[1])
    check(tag + "dbias", gdb.v, r64[2], r32[2])
    assert torch.equal(ggt.t[:, :B], gg.t.t()) and bool((ggt.t[:, B:] == 0).all())
    again = run_ce(o, logits, target, gscale)                                     # fixed-order sums: bit-equal on a repeat
    for a, b in zip((gg, ggt, gdb, gloss), again[1:5]):
        assert torch.equal(a.t, b.t)
    lo = o.ce_label(gl.t, tg.v)[0]                                                # the loss alone: the same bits
    assert torch.equal(lo, gloss.v)


def test_ce_label_bad_targets_give_nan_rows_only():
    o = ops()
    B, C = 67, 7
    logits, target = ce_case(B, C)
    target[5], target[40] = -1, C
    gl, gg, ggt, gdb, gloss, tg = run_ce(o, logits, target)
    for G in (gl, gg, ggt, gdb, gloss, tg):
        assert G.intact()                                                         # the guard bands are untouched
    nan_rows = gg.t.isnan().all(dim=1).cpu()
    assert nan_rows.nonzero().flatten().tolist() == [5, 40]
    assert not bool(gg.t.isnan().any(dim=1).cpu()[~nan_rows].any())
    assert bool(gloss.v.isnan().all()) and bool(gdb.v.isnan().all())
    good = torch.ones(B, dtype=torch.bool); good[5] = good[40] = False
    ref = LR.ce(logits[good].double(), target[good])[1] * (good.sum().item() / B)
    assert float((gg.t.cpu()[good].double() - ref).abs().max()) <= 1e-5 * float(ref.abs().max())


def test_ce_label_refusals():
    from vitlens_hip import _lib
    lib = _lib.load_library()
    logits, target = torch.randn(4, 7, device=DEV), torch.zeros(4, dtype=torch.int64, device=DEV)
    loss, ws = torch.full((1,), NAN, device=DEV), torch.empty(64, device=DEV)
    P = lambda t: None if t is None else t.data_ptr()
    assert lib.vl_ce_label_ws_floats(67, 7) == 2 * 67 + 2 * 7
    assert lib.vl_ce_label(P(logits), 7, P(target), 4, 0, 1.0, P(loss), None, 0, None, 0, None, P(ws), None) != 0
    assert lib.vl_ce_label(P(logits), 6, P(target), 4, 7, 1.0, P(loss), None, 0, None, 0, None, P(ws), None) != 0
    assert b"ld" in lib.vl_last_error()
    assert lib.vl_ce_label(P(logits), 7, P(target), 4, 7, 1.0, P(loss), None, 0, P(logits), 6, None, P(ws), None) != 0
    assert b"ldgt" in lib.vl_last_error()
    assert lib.vl_ce_label(P(logits), 7, P(target), 4, 7, 1.0, P(loss), None, 0, None, 0, None, None, None) != 0
    assert b"workspace" in lib.vl_last_error()
    torch.cuda.synchronize()
    assert bool(loss.isnan().all())


# ---- vl_lars_multi_step ---------------------------------------------------------------------------------------------------
def lars_table(shapes, seed, zero_weight=None, zero_grad=None):
    g = torch.Generator().manual_seed(seed)
    slots = []
    for i, (shape, adapt) in enumerate(shapes):
        n = 1
        for s in shape:
            n *= s
        p = torch.randn(n, generator=g) * 0.05
        if zero_weight == i:
            p.zero_()
        slots.append(dict(p=p, mu=torch.zeros(n), adapt=adapt, shape=shape, zero_grad=zero_grad == i))
    return slots


def lars_grads(slots, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.zeros_like(s["p"]) if s["zero_grad"] else torch.randn(s["p"].numel(), generator=g) * 0.02 for s in slots]


LARS_TABLES = {
    "2x64": [((2, 64), True), ((2,), False)],
    "7x64": [((7, 64), True), ((7,), False)],
    "1000x1024": [((1000, 1024), True), ((1000,), False)],
    "crossing": [((3, 1000), True), ((2053,), True), ((2049,), False), ((5,), False)],     # sizes that cross the 2048-element tile
}


def fp32_round(x):
    return struct.unpack("f", struct.pack("f", x))[0]


def fp32_clip(sumsq, max_norm, gscale):
    """min(1, max_norm / (grad_scale sqrt(sumsq) + 1e-6)) with fp32 operands and every operation correctly rounded to fp32.
    Each one is the IEEE fp64 operation rounded once more: for a square root, a quotient, a product and a sum of fp32 values
    that second rounding changes nothing (53 >= 2 x 24 + 2 bits).  A host library's vectorised fp32 sqrt need not be correctly
    rounded; math.sqrt is.  (The grad_scale of these cases is a power of two: its product is exact, so a fused multiply-add
    and a separate multiply and add give the same denominator.)"""
    root = fp32_round(math.sqrt(fp32_round(sumsq)))
    den = fp32_round(fp32_round(fp32_round(gscale) * root) + fp32_round(1e-6))
    return min(1.0, fp32_round(fp32_round(max_norm) / den))


# every table plain and with max_norm + grad_scale; the two q = 1 branches on the small tables
LARS_CASES = [(t, v) for t in LARS_TABLES for v in ("plain", "clip_scale")] + [(t, v) for t in ("2x64", "7x64", "crossing")
                                                                                 for v in ("zero_weight", "zero_grad")]


@pytest.mark.parametrize("table,variant", LARS_CASES)
def test_lars_multi_step(table, variant):
    o = ops()
    shapes = LARS_TABLES[table]
    wd = 0.0 if variant == "zero_grad" else 1e-4
    max_norm, gscale = (0.05, 0.5) if variant == "clip_scale" else (None, 1.0)
    lr, mom, trust = 0.1, 0.9, 1e-3
    slots = lars_table(shapes, 7, zero_weight=0 if variant == "zero_weight" else None, zero_grad=0 if variant == "zero_grad" else None)
    dev = [dict(p=vec(s["p"].numel(), src=s["p"]), g=vec(s["p"].numel()), mu=vec(s["p"].numel(), src=s["mu"])) for s in slots]
    packed = o.pack_lars_slots([(d["p"].v, d["g"].v, d["mu"].v, wd, s["adapt"]) for d, s in zip(dev, slots)]).to(DEV)
    total = sum(s["p"].numel() for s in slots)
    ws = torch.empty(o.lars_ws_floats(total, len(slots)) // 2 + 1, dtype=torch.float64, device=DEV)
    st = {dt: [dict(p=s["p"].to(dt), mu=s["mu"].to(dt), wd=wd, adapt=s["adapt"]) for s in slots] for dt in (torch.float64, torch.float32)}
    for step in range(3):                                                         # three steps: the momentum is exercised
        grads = lars_grads(slots, 100 + step)
        flat = torch.cat(grads).to(DEV)
        for d, gr in zip(dev, grads):
            d["g"].v.copy_(gr.to(DEV))
        sumsq = o.grad_sumsq(flat) if max_norm else None
        before = [(d["p"].v.cpu().clone(), d["mu"].v.cpu().clone()) for d in dev]
        o.lars_multi_step(packed, len(slots), lr, mom, trust, gscale, max_norm, sumsq, ws=ws)
        torch.cuda.synchronize()
        for dt, ss in st.items():
            for s, gr in zip(ss, grads):
                s["g"] = gr.to(dt)
            for s, (p, mu) in zip(ss, LR.lars_step(ss, lr, mom, trust, gscale, max_norm)):
                s["p"], s["mu"] = p, mu
        for i, (d, s) in enumerate(zip(dev, slots)):
            assert d["p"].intact() and d["g"].intact() and d["mu"].intact()
            tag = f"lars/{table}/{variant}/step{step}/slot{i}/"
            check(tag + "p", d["p"].v, st[torch.float64][i]["p"], st[torch.float32][i]["p"])
            check(tag + "mu", d["mu"].v, st[torch.float64][i]["mu"], st[torch.float32][i]["mu"])
            if not s["adapt"]:
                # a bias: mu = m mu + g', p -= lr mu with every operation rounded to fp32 on its own - bit for bit
                g1 = grads[i] * gscale
                if max_norm:
                    g1 = g1 * fp32_clip(float(sumsq.cpu()), max_norm, gscale)
                mu = torch.add(torch.mul(before[i][1], mom), g1)
                p = torch.sub(before[i][0], torch.mul(mu, lr))
                assert torch.equal(d["mu"].v.cpu(), mu) and torch.equal(d["p"].v.cpu(), p), tag
        if variant == "zero_weight" and step == 0:
            # |p| = 0: q = 1, the first step is p = -lr g exactly (wd p = 0, mu = g)
            assert torch.equal(dev[0]["p"].v.cpu(), torch.sub(torch.zeros_like(grads[0]), torch.mul(grads[0], lr)))
        if variant == "zero_grad":
            assert torch.equal(dev[0]["p"].v.cpu(), slots[0]["p"])                # |dp| = 0 with wd = 0: q = 1, nothing moves
    again_p = [d["p"].v.clone() for d in dev]
    assert all(torch.isfinite(p).all() for p in again_p)


def test_lars_refusals_and_short_workspace():
    o = ops()
    from vitlens_hip import _lib
    lib = _lib.load_library()
    p, g, mu = (torch.ones(5000, device=DEV) for _ in range(3))
    packed = o.pack_lars_slots([(p, g, mu, 0.0, True)]).to(DEV)
    ws = torch.empty(8, dtype=torch.float64, device=DEV)
    P = lambda t: None if t is None else t.data_ptr()
    assert lib.vl_lars_multi_step(P(packed), 2000, 0.1, 0.9, 1e-3, 1.0, 0.0, None, P(ws), 16, None) != 0
    assert lib.vl_lars_multi_step(P(packed), 1, 0.1, 0.9, 1e-3, 1.0, 1.0, None, P(ws), 16, None) != 0 and b"sumsq" in lib.vl_last_error()
    assert lib.vl_lars_multi_step(P(packed), 1, 0.1, 0.9, 1e-3, 1.0, 0.0, None, None, 0, None) != 0 and b"workspace" in lib.vl_last_error()
    torch.cuda.synchronize()
    assert bool((p == 1).all()) and bool((mu == 1).all())
    assert lib.vl_lars_ws_floats(5000, 1) == 4 * (5000 // 2048 + 1)
    with pytest.raises(ValueError):
        o.pack_lars_slots([(p, g[:10], mu, 0.0, True)])


# ---- vl_topk_hits ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", (2, 5, 7, 1000))
def test_topk_hits_distinct_logits(C):
    o = ops()
    B = 67
    ks = (1, 5) if C >= 5 else (1, 2)
    g = torch.Generator().manual_seed(C)
    logits = torch.stack([torch.randperm(C, generator=g).float() * 0.37 - 3.0 for _ in range(B)])
    target = torch.randint(0, C, (B,), generator=g)
    target[0], target[1] = 0, C - 1
    gl = Guarded(B, C, ld=C + 3, src=logits)
    gc = Guarded(B, 2, dtype=torch.uint8, fill=0xAB)
    gh = vec(2, dtype=torch.int32, fill=-5)
    gh.v.zero_()
    tg = target.to(DEV)
    o.topk_hits(gl.t, tg, ks, hits=gh.v, correct=gc.t)
    torch.cuda.synchronize()
    assert gl.intact() and gc.intact() and gh.intact()
    top = logits.topk(max(ks), dim=1).indices
    want = torch.stack([(top[:, :k] == target[:, None]).any(dim=1) for k in ks], dim=1)
    assert torch.equal(gc.t.cpu().bool(), want)
    assert gh.v.tolist() == want.sum(0).tolist()
    o.topk_hits(gl.t, tg, ks, hits=gh.v)                                          # the counters accumulate
    assert gh.v.tolist() == (2 * want.sum(0)).tolist()
    assert torch.equal(want, torch.stack([LR.rank(logits, target) < k for k in ks], dim=1))


def test_topk_hits_ties_nan_and_bad_targets():
    o = ops()
    B, C = 67, 7
    g = torch.Generator().manual_seed(3)
    logits = torch.randint(0, 3, (B, C), generator=g).float()                    # three levels: ties everywhere
    target = torch.randint(0, C, (B,), generator=g)
    logits[4] = NAN                                                               # a NaN row: nothing is greater, rank 0
    logits[9, 2] = NAN
    hits, correct = o.topk_hits(logits.to(DEV), target.to(DEV), (1, 3), need_correct=True)
    r = LR.rank(logits, target)
    want = torch.stack([r < 1, r < 3], dim=1)
    assert int(r[4]) == 0
    assert torch.equal(correct.cpu().bool(), want) and hits.tolist() == want.sum(0).tolist()
    bad = target.clone(); bad[0], bad[1] = -1, C
    hits2, correct2 = o.topk_hits(logits.to(DEV), bad.to(DEV), (1, 3), need_correct=True)
    want[0] = want[1] = False
    assert torch.equal(correct2.cpu().bool(), want) and hits2.tolist() == want.sum(0).tolist()


# ---- ProbeHead ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", (64, 1024))
def test_probe_head_three_steps(D):
    from vitlens_hip.linprobe import ProbeHead
    C, B, p, wd, lr = 7, 37, 0.25, 1e-4, 0.1
    g = torch.Generator().manual_seed(D)
    w0, b0 = torch.randn(C, D, generator=g) * 0.01, torch.randn(C, generator=g) * 0.01
    head = ProbeHead(D, C, DEV, dropout=p, weight=w0, bias=b0, weight_decay=wd)
    refs = {dt: LR.Head(w0, b0, dt, p=p, wd=wd) for dt in (torch.float64, torch.float32)}
    for step in range(3):
        feat = bn_input(B, D, seed=step)
        keep = torch.rand(B, D, generator=g) >= p
        target = torch.randint(0, C, (B,), generator=g)
        max_norm = 0.01 if step == 1 else None
        logits = head.forward(feat.to(DEV), True, keep=keep.to(DEV))
        head.backward(logits, target.to(DEV))
        got = dict(logits=logits.clone(), loss=head.loss.clone(), dw=head.dw.clone(), db=head.db.clone())
        head.optimizer_step(lr, max_norm=max_norm)
        for r in refs.values():
            r.forward(feat, True, keep); r.backward(target); r.step(lr, max_norm=max_norm)
        got.update(weight=head.weight, bias=head.bias, running_mean=head.running_mean, running_var=head.running_var)
        r64, r32 = refs[torch.float64], refs[torch.float32]
        for k, a64, a32 in (("logits", r64.logits, r32.logits), ("loss", r64.loss.reshape(1), r32.loss.reshape(1)), ("dw", r64.dw, r32.dw),
                            ("db", r64.db, r32.db), ("weight", r64.w, r32.w), ("bias", r64.b, r32.b), ("running_mean", r64.rm, r32.rm),
                            ("running_var", r64.rv, r32.rv)):
            check(f"head/D{D}/step{step}/{k}", got[k], a64, a32)
    sd = head.state_dict()
    assert tuple(sd) == ("lp_head.1.running_mean", "lp_head.1.running_var", "lp_head.1.num_batches_tracked", "lp_head.2.weight",
                         "lp_head.2.bias") and int(sd["lp_head.1.num_batches_tracked"]) == 3
    other = ProbeHead(D, C, DEV)
    other.load_state_dict(sd)
    feat = bn_input(B, D, seed=9).to(DEV)
    assert torch.equal(other.forward(feat, False), head.forward(feat, False))
    hits = head.hits(head.logits, target.to(DEV))
    assert hits.tolist() == [int((LR.rank(head.logits.cpu(), target) < k).sum()) for k in (1, 5)]


# ---- LinearProbeStep and the module path on the tiny tactile config -------------------------------------------------------
def _host():
    import test_linprobe_host as H
    return H


@pytest.fixture()
def tiny_config():
    import open_clip as oc
    H = _host()
    with tempfile.TemporaryDirectory() as td:
        with open(os.path.join(td, "zz-tiny-linprobe.json"), "w") as f:
            json.dump(H.TINY, f)
        oc.add_model_config(td)
        try:
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                yield
        finally:
            from open_clip import factory
            factory._CONFIG_PATHS.pop()
            factory._rescan()


def _probe_model(ci, **kw):
    """Our ViTLensLP of recorded case ci with the recorded weights, locked, on the GPU."""
    from open_clip.linprobe_model import ViTLensLP
    H = _host()
    proj, drop, C, B, wd = H.CASES[ci]
    model = ViTLensLP(H._args(lp_enable_vit_proj=proj, lp_dropout_rate=drop, lp_num_classes=C, **kw))
    model.load_state_dict(seeded_like(H.reference()["cases"][ci]["stats"], H.SEED + ci))
    model.lp_lock_parameters()
    return model.to(DEV)


def _check_head_against_own_features(tag, head, feat, target, got_logits, got_loss, w0, b0, wd, lr):
    refs = {dt: LR.Head(w0, b0, dt, wd=wd) for dt in (torch.float64, torch.float32)}
    for r in refs.values():
        r.forward(feat, True); r.backward(target); r.step(lr)
    r64, r32 = refs[torch.float64], refs[torch.float32]
    check(tag + "logits", got_logits, r64.logits, r32.logits)
    check(tag + "loss", got_loss, r64.loss.reshape(1), r32.loss.reshape(1))
    check(tag + "weight", head.weight, r64.w, r32.w)
    check(tag + "bias", head.bias, r64.b, r32.b)
    check(tag + "running_mean", head.running_mean, r64.rm, r32.rm)
    check(tag + "running_var", head.running_var, r64.rv, r32.rv)


@pytest.mark.parametrize("ci", (0, 1))
def test_linear_probe_step_tiny_tactile(tiny_config, ci):
    """(1) its pooled features against the recorded reference ones at the image tower's tolerance of tests/test_hip_towers.py
    (relative L2 < 2e-2: bf16 GEMM operands); (2) logits, loss and the updated head against linprobe_ref on ITS OWN features."""
    from vitlens_hip.linprobe import LinearProbeStep
    H = _host()
    proj, drop, C, B, wd = H.CASES[ci]
    rec = H.reference()["cases"][ci]
    model = _probe_model(ci)
    sd = seeded_like(rec["stats"], H.SEED + ci)
    w0, b0 = sd["lp_head.2.weight"], sd["lp_head.2.bias"]
    st = LinearProbeStep(model.backbone, C, H.LR0, weight_decay=wd, enable_vit_proj=proj, weight=w0, bias=b0)
    x, target = LR.case_inputs(ci, B, C, H.STEPS)
    loss = st.step(x[0].to(DEV), target[0].to(DEV))
    feat = st.feat                                                               # the features that step ran on
    want = torch.tensor(rec["steps"][0]["pooled"])
    e = float((feat.cpu() - want).norm() / want.norm())
    print("pooled features relative L2 error", e)
    assert feat.shape == want.shape and e < 2e-2, e
    _check_head_against_own_features(f"step/tactile_case{ci}/", st.head, feat.cpu(), target[0], st.head.logits, loss, w0, b0, wd, H.LR0)
    print("loss", float(loss), "reference", rec["steps"][0]["loss"])
    hits = st.evaluate(x[1].to(DEV), target[1].to(DEV))
    ev = st.head.logits.cpu()
    assert hits.tolist() == [int((LR.rank(ev, target[1]) < k).sum()) for k in (1, 5)]


class _ListData:
    """What linprobe_train_one_epoch and test_linprob_single take: a loader over a list of batches."""

    def __init__(self, batches, labels):
        self.batches = batches
        self.num_batches, self.num_samples = len(batches), sum(len(b["label"]) for b in batches)
        self.dataloader, self.dataset = self, SimpleNamespace(idx2label=labels, label2idx={v: k for k, v in enumerate(labels)}, split="val")

    def set_epoch(self, epoch):
        self.epoch = epoch

    def __iter__(self):
        return iter(self.batches)

    def __len__(self):
        return len(self.batches)


@pytest.mark.parametrize("ci", (0, 2))
def test_module_path_gives_the_bits_of_linear_probe_step(tiny_config, ci):
    """ViTLensLP + LARS + linprobe_train_one_epoch on a two-batch loader against LinearProbeStep on the same batches: the same
    kernels on the same operands, so the same head bit for bit (case 2 has dropout: the same seed draws the same masks)."""
    from open_clip.linprobe_model import LabelCrossEntropyLoss
    from training.optimizer import LARS
    from training.train import linprobe_train_one_epoch
    from training.zero_shot import test_linprob_single
    from vitlens_hip.linprobe import LinearProbeStep
    H = _host()
    proj, drop, C, B, wd = H.CASES[ci]
    x, target = LR.case_inputs(ci, B, C, H.STEPS)
    batches = [{"tactile": x[s], "label": target[s]} for s in range(2)]
    args = SimpleNamespace(device=DEV, accum_freq=1, skip_scheduler=False, v_key="tactile", grad_clip_norm=None, rank=0, world_size=1,
                           batch_size=B, log_every_n_steps=1, precision="fp32", distributed=False)
    model = _probe_model(ci, seed=5)
    opt = LARS(model.lp_head.parameters(), lr=0.0, weight_decay=wd)
    lrs = []
    def scheduler(step):
        opt.param_groups[0]["lr"] = H.LR0 * (1 + step)
        lrs.append(opt.param_groups[0]["lr"])
    data = {"train": _ListData(batches, list(range(C)))}
    linprobe_train_one_epoch(model, data, LabelCrossEntropyLoss(), 0, opt, None, scheduler, None, args)
    assert lrs == [H.LR0, 2 * H.LR0]
    assert all(p.grad is None for n, p in model.named_parameters() if not n.startswith("lp_head.2."))

    twin = _probe_model(ci)
    sd = twin.state_dict()
    st = LinearProbeStep(twin.backbone, C, H.LR0, weight_decay=wd, dropout=drop, enable_vit_proj=proj, drop_seed=5,
                         weight=sd["lp_head.2.weight"], bias=sd["lp_head.2.bias"])
    for s in range(2):
        st.step(x[s].to(DEV), target[s].to(DEV), lr=H.LR0 * (1 + s))
    got, want = model.state_dict(), st.state_dict()
    for k in want:
        assert torch.equal(got[k].cpu(), want[k].cpu()), k
    assert torch.equal(opt.state[model.lp_head[2].weight]["mu"], st.head.mu_w)
    assert torch.equal(opt.state[model.lp_head[2].bias]["mu"], st.head.mu_b)
    # nn.CrossEntropyLoss works too (its gradient goes through the transpose and the column sum behind it): same head to fp32
    other = _probe_model(ci, seed=5)
    opt2 = LARS(other.lp_head.parameters(), lr=H.LR0, weight_decay=wd)
    args.skip_scheduler = True
    linprobe_train_one_epoch(other, data, torch.nn.CrossEntropyLoss(), 0, opt2, None, None, None, args)
    st2 = LinearProbeStep(_probe_model(ci).backbone, C, H.LR0, weight_decay=wd, dropout=drop, enable_vit_proj=proj, drop_seed=5,
                          weight=sd["lp_head.2.weight"], bias=sd["lp_head.2.bias"])
    for s in range(2):
        st2.step(x[s].to(DEV), target[s].to(DEV))
    w = st2.head.weight
    assert float((other.lp_head[2].weight.detach() - w).abs().max()) <= 1e-5 * float(w.abs().max())
    # evaluation: the counts of vl_topk_hits
    test = _ListData([{"tactile": x[s], "label": target[s] if s else target[s].tolist()} for s in range(2, 4)], list(range(C)))
    out = test_linprob_single(test, model, None, args=args)
    hits = sum(st.evaluate(x[s].to(DEV), target[s].to(DEV)) for s in range(2, 4)).tolist()
    assert out == {"acc1": 100.0 * hits[0] / (2 * B), "acc5": 100.0 * hits[1] / (2 * B)}
    assert set(test_linprob_single(_ListData(test.batches, [0, 1]), model, None, args=args)) == {"acc1"}


@pytest.mark.parametrize("modality", ("depth", "audio"))
def test_other_modalities_forward_and_step(modality):
    """A v_key other than tactile: the depth Lens (identity Perceiver) and the audio Lens (Perceiver) as backbones, with the
    projection kept so that the pooled feature is the golden `visual_raw` (tests/test_hip_api.py's 3e-2 for these towers)."""
    import open_clip as oc
    from open_clip.linprobe_model import LabelCrossEntropyLoss, ViTLensLP
    from training.optimizer import LARS
    sd, ins, outs, grads, meta = split(load_npz(f"tiny_{modality}.npz"))
    C, lr = 5, 0.1
    a = dict(meta["args"], model="zz-tiny-lens", pretrained=None, precision="fp32", force_quick_gelu=False, force_custom_text=False,
             force_image_size=None, pretrained_image=False, cache_dir=None, lp_enable_vit_proj=True, lp_dropout_rate=0.0,
             lp_num_classes=C)
    with tempfile.TemporaryDirectory() as td:
        with open(os.path.join(td, "zz-tiny-lens.json"), "w") as f:
            json.dump(meta["model_cfg"], f)
        oc.add_model_config(td)
        try:
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                model = ViTLensLP(SimpleNamespace(**a))
        finally:
            from open_clip import factory
            factory._CONFIG_PATHS.pop()
            factory._rescan()
    missing = model.backbone.load_state_dict({k[len("visual."):]: v for k, v in sd.items() if k.startswith("visual.")}, strict=False)
    assert not missing.missing_keys and not missing.unexpected_keys
    model.lp_lock_parameters()
    model.to(DEV).train()
    x = ins["visual_x"].to(DEV)
    target = torch.tensor([0, C - 1, 2, 2], device=DEV)
    w0, b0 = model.lp_head[2].weight.detach().cpu().clone(), model.lp_head[2].bias.detach().cpu().clone()
    seen = {}
    model.backbone.register_forward_hook(lambda m, i, o: seen.update(feat=o.detach().float().clone()))
    opt = LARS(model.lp_head.parameters(), lr=lr)
    logits = model(x)
    feat = seen["feat"]                                                          # the features the head ran on
    e = float((feat.cpu() - outs["visual_raw"]).norm() / outs["visual_raw"].norm())
    print(modality, "pooled feature relative L2 error", e)
    assert e < 3e-2
    loss = LabelCrossEntropyLoss()(logits, target)
    loss.backward()
    opt.step()
    torch.cuda.synchronize()
    head = SimpleNamespace(weight=model.lp_head[2].weight.detach(), bias=model.lp_head[2].bias.detach(),
                           running_mean=model.lp_head[1].running_mean, running_var=model.lp_head[1].running_var)
    _check_head_against_own_features(f"step/{modality}/", head, feat.cpu(), target.cpu(), logits.detach(), loss.detach().reshape(1),
                                     w0, b0, 0.0, lr)
    assert int(model.lp_head[1].num_batches_tracked) == 1
