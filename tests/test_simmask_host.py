"""CPU: the similarity-masked contrastive loss (`ClipLossSimMask`, --contra_loss_type sim_mask).

1. tests/simmask_ref.py, the float64 restatement the GPU tests compare against, is pinned to the imported reference's own
   `ClipLossSimMask` (world 1, B = 24, E = 16, thres 0.8, logit_scale 20; loss, dx, dy, d/dlogit_scale stored under
   tests/golden/reference/), and its three branches agree with each other: the mean over ranks of the `local_loss` values is
   the gathered global value.
2. The public interface: `create_loss` returns the module for dual + sim_mask and refuses tri + sim_mask and label_mask; the
   epoch drivers' `_refuse` lets sim_mask through; constructor and `forward` signatures equal the recorded reference ones.
The kernels' side: tests/test_hip_loss_simmask.py."""
import inspect
import os
from types import SimpleNamespace

import pytest
import torch

import simmask_ref as SR
from golden_util import reference_run

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, E, THRES, SCALE, SEED = 24, 16, 0.8, 20.0, 41

_REF = r'''
import inspect, json, sys, torch
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[2])
import ref_loader
ref_loader.load()
from open_clip.loss import ClipLossSimMask
import simmask_ref as SR
B, E, thres, scale, seed = int(sys.argv[3]), int(sys.argv[4]), float(sys.argv[5]), float(sys.argv[6]), int(sys.argv[7])
t, s = SR.clustered(B, seed, dim=E)
x = t.clone().requires_grad_(True); y = s.clone().requires_grad_(True)
ls = torch.tensor(scale, requires_grad=True)
mod = ClipLossSimMask(sim_thres=thres)
loss = mod(x, y, ls)
loss.backward()
sim = (x.detach() @ x.detach().t())
masked = int(((sim >= thres) & ~torch.eye(B, dtype=torch.bool)).sum())
sig = lambda f: [[p.name, None if p.default is inspect.Parameter.empty else repr(p.default), str(p.kind)]
                 for p in inspect.signature(f).parameters.values()]
d = mod(x.detach(), y.detach(), ls.detach(), output_dict=True)
print("JSON" + json.dumps({"loss": float(loss), "dx": x.grad.tolist(), "dy": y.grad.tolist(), "dscale": float(ls.grad),
                           "masked": masked, "keys": list(d), "init": sig(ClipLossSimMask.__init__),
                           "forward": sig(ClipLossSimMask.forward)}))
'''


def _ref():
    return reference_run("test_simmask_host.reference_sim_mask_loss", _REF,
                         [os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests"), str(B), str(E), str(THRES), str(SCALE), str(SEED)])


def test_restatement_matches_the_reference_module():
    ref = _ref()
    t, s = SR.clustered(B, SEED, dim=E)
    frac = SR.check_inputs(t, t, THRES)
    assert ref["masked"] == round(frac * B * (B - 1)) and ref["masked"] > 0
    loss, dx, dy, ds = SR.with_grads(lambda x, y, sc: SR.loss_world1(x, y, sc, THRES), t, s, SCALE)
    rel = lambda a, b: float((a - b).norm() / b.norm())
    want_dx, want_dy = torch.tensor(ref["dx"], dtype=torch.float64), torch.tensor(ref["dy"], dtype=torch.float64)
    print("loss", loss, ref["loss"], "dx", rel(dx, want_dx), "dy", rel(dy, want_dy), "dscale", ds, ref["dscale"])
    assert abs(loss - ref["loss"]) <= 1e-5 * abs(ref["loss"])
    assert rel(dx, want_dx) <= 1e-5 and rel(dy, want_dy) <= 1e-5
    assert abs(ds - ref["dscale"]) <= 1e-5 * abs(ref["dscale"])
    # the generic building block the kernels' tests use is the same function
    keep = SR.keep_mask(t, t, THRES)
    l2, dx2, dy2, ds2 = SR.with_grads(lambda x, y, sc: SR.pair_loss(x, y, sc, keep), t, s, SCALE)
    assert abs(l2 - loss) < 1e-12 and rel(dx2, dx) < 1e-12 and rel(dy2, dy) < 1e-12 and abs(ds2 - ds) < 1e-12 * max(1.0, abs(ds))
    # and a -inf mask would be another loss
    lg = (SCALE * t.double() @ s.double().t()).masked_fill(~keep, float("-inf"))
    lab = torch.arange(B)
    neg_inf = float((torch.nn.functional.cross_entropy(lg, lab) + torch.nn.functional.cross_entropy(lg.t(), lab)) / 2)
    assert abs(neg_inf - ref["loss"]) > 1e-3 * abs(ref["loss"])


def test_mean_of_local_losses_is_the_gathered_loss():
    W, b = 3, 16
    t, s = SR.clustered(W * b, 43)
    SR.check_inputs(t, t, THRES)
    ax, ay = t.double(), s.double()
    glob = float(SR.loss_gathered(ax, ay, SCALE, THRES))
    loc = [float(SR.loss_local(ax[r * b:(r + 1) * b], ay[r * b:(r + 1) * b], ax, ay, r, SCALE, THRES)) for r in range(W)]
    assert abs(sum(loc) / W - glob) < 1e-12 * abs(glob), (loc, glob)
    assert abs(glob - float(SR.loss_world1(ax, ay, SCALE, THRES))) < 1e-12 * abs(glob)
    assert max(loc) - min(loc) > 1e-6                      # the ranks' values differ: the identity is about their mean
    # each local value is two row losses of the building block with ONE similarity block per rank
    for r in range(W):
        keep = SR.keep_mask(ax[r * b:(r + 1) * b], ax, THRES, label_off=r * b)
        two = (SR.pair_loss(ax[r * b:(r + 1) * b], ay, SCALE, keep, r * b, 0.5, 0.0)
               + SR.pair_loss(ay[r * b:(r + 1) * b], ax, SCALE, keep, r * b, 0.5, 0.0))
        assert abs(float(two) - loc[r]) < 1e-12 * abs(loc[r])


def _args(**kw):
    base = dict(local_loss=False, gather_with_grad=False, rank=0, world_size=1, horovod=False, model="ViT-B-32", n_tower=3,
                use_dual_loss=True, contra_loss_type="sim_mask", sim_thres=0.73, distill=False)
    base.update(kw)
    return SimpleNamespace(**base)


def test_create_loss_builds_sim_mask_for_the_dual_loss_only(caplog):
    import logging
    import open_clip as oc
    with caplog.at_level(logging.INFO):
        loss = oc.create_loss(_args(local_loss=True, rank=2, world_size=4))
    assert type(loss) is oc.ClipLossSimMask and loss.sim_thres == 0.73
    assert (loss.local_loss, loss.rank, loss.world_size, loss.cache_labels) == (True, 2, 4, True)
    assert "[Loss class]: ClipLossSimMask" in caplog.text
    with pytest.raises(NotImplementedError) as ei:
        oc.create_loss(_args(use_dual_loss=False))
    assert "ClipLoss" in str(ei.value)                     # says what the reference does there
    for dual in (True, False):
        with pytest.raises(NotImplementedError):
            oc.create_loss(_args(contra_loss_type="label_mask", use_dual_loss=dual))
    assert type(oc.create_loss(_args(contra_loss_type="general"))) is oc.ClipLossGeneral


def test_epoch_drivers_let_sim_mask_through():
    from training import train as T
    T._refuse(SimpleNamespace(contra_loss_type="sim_mask"))
    T._refuse(SimpleNamespace(contra_loss_type="general"))
    with pytest.raises(NotImplementedError):
        T._refuse(SimpleNamespace(contra_loss_type="label_mask"))


def test_signatures_equal_the_reference():
    """Names, order and defaults; the product may only append optional parameters (`chunk_rows`)."""
    ref = _ref()
    import open_clip as oc
    assert ref["keys"] == ["contrastive loss[with sim mask]"]
    sig = lambda f: [[p.name, None if p.default is inspect.Parameter.empty else repr(p.default), str(p.kind)]
                     for p in inspect.signature(f).parameters.values()]
    assert sig(oc.ClipLossSimMask.forward) == ref["forward"]
    mine = sig(oc.ClipLossSimMask.__init__)
    assert mine[:len(ref["init"])] == ref["init"]
    assert mine[len(ref["init"]):] == [["chunk_rows", "None", "POSITIONAL_OR_KEYWORD"]]
    with pytest.raises(RuntimeError):                      # no CPU implementation of the loss math
        oc.ClipLossSimMask()(torch.eye(4), torch.eye(4), torch.tensor(10.0))


# ---- the loss core's bookkeeping on a torch stand-in for the HIP ops -------------------------------------------------------------
def _masked_ops():
    """tests/test_pair_chunks_host.py's stand-in, its CE ops taking `sim` / `thres` as the masked entry points do."""
    import test_pair_chunks_host as P
    o = P._ops()
    plain_stats, plain_grad = o.ce_stats, o.ce_grad

    def kept(logits, label_off, sim, thres):
        R, C = logits.shape
        assert sim.shape == logits.shape
        eye = torch.arange(C)[None, :] == (torch.arange(R)[:, None] + label_off)
        return torch.logical_or(torch.logical_not(sim >= thres), eye)

    def ce_stats(logits, label_off=0, want_cols=True, sim=None, thres=None):
        if sim is None:
            return plain_stats(logits, label_off, want_cols)
        return plain_stats(logits * kept(logits, label_off, sim, thres), label_off, want_cols)

    def ce_grad(logits, row_lse, col_lse, label_off, w_row, w_col, logit_scale, dscale, need_g=True, need_gt=True, sim=None, thres=None):
        if sim is None:
            return plain_grad(logits, row_lse, col_lse, label_off, w_row, w_col, logit_scale, dscale, need_g, need_gt)
        k = kept(logits, label_off, sim, thres)
        ds = torch.zeros_like(dscale)
        G, _ = plain_grad(logits * k, row_lse, col_lse, label_off, w_row, w_col, logit_scale, ds, True, False)
        G = G * k
        dscale += (G * logits).sum() / logit_scale
        return (G if need_g else None), (G.t().contiguous() if need_gt else None)
    o.ce_stats, o.ce_grad = ce_stats, ce_grad
    return o


@pytest.mark.parametrize("R,C,off,w_col", [(37, 37, 0, 0.5), (16, 48, 32, 0.0), (16, 48, 0, 0.0), (20, 48, 8, 0.5)])
def test_pair_core_with_a_mask_row_blocks_and_device_temperature(R, C, off, w_col, monkeypatch):
    """pair_forward / pair_backward with a mask on the stand-in ops: every block size gives simmask_ref's loss and gradients
    (the similarity block of a row block sits next to its logits block, forward and backward), and the device-temperature
    mode - x scaled by exp(logit_scale) before the logits GEMM - masks the same set: the similarities are those of the
    un-scaled teacher features."""
    from vitlens_hip import step as ST
    monkeypatch.setattr(ST, "ops", _masked_ops())
    t, s = SR.clustered(C, 50 + C)
    x = t[off:off + R].contiguous()
    keep = SR.keep_mask(x, t, THRES, off)
    assert bool((~keep).any())
    want = SR.with_grads(lambda a, b, sc: SR.pair_loss(a, b, sc, keep, off, 0.5, w_col), x, s, SCALE)
    rel = lambda a, b: float((a.double() - b).norm() / b.norm())
    for rb in (0, 1, 5, R - 1):
        for scale in (SCALE, torch.tensor([SCALE]).log()):
            loss, ctx = ST.pair_forward(x, s, scale, off, 0.5, w_col, chunk_rows=rb, mask=(x, t, THRES))
            dx, dy, ds = ST.pair_backward(ctx)
            assert abs(float(loss) - want[0]) < 1e-5 * abs(want[0]), (rb, float(loss), want[0])
            assert rel(dx, want[1]) < 1e-4 and rel(dy, want[2]) < 1e-4, rb
            ds_want = want[3] * (SCALE if torch.is_tensor(scale) else 1.0)             # d/d(log-scale) in device mode
            assert abs(float(ds) - ds_want) < 1e-4 * max(1.0, abs(ds_want)), (rb, float(ds), ds_want)
    with pytest.raises(ValueError):
        ST.pair_forward(x, s, SCALE, off, 0.5, w_col, mask=(x[:-1], t, THRES))
    # the plain loss on the same geometry: with C > R and a column loss, the columns that are no row's label get no column
    # gradient (they are in no term of the loss)
    ones = torch.ones_like(keep)
    want = SR.with_grads(lambda a, b, sc: SR.pair_loss(a, b, sc, ones, off, 0.5, w_col), x, s, SCALE)
    for rb in (0, 5):
        loss, ctx = ST.pair_forward(x, s, SCALE, off, 0.5, w_col, chunk_rows=rb)
        dx, dy, ds = ST.pair_backward(ctx)
        assert abs(float(loss) - want[0]) < 1e-5 * abs(want[0]) and rel(dx, want[1]) < 1e-4 and rel(dy, want[2]) < 1e-4
        assert abs(float(ds) - want[3]) < 1e-4 * max(1.0, abs(want[3]))


@pytest.mark.parametrize("teacher", ["x", "y"])
def test_pair_loss_and_grads_names_the_teacher_side(teacher, monkeypatch):
    """World 1, gathered, and local_loss as each of 3 ranks computes it (peers constant), with the teacher in either argument
    position: simmask_ref's branches, value and gradients."""
    from vitlens_hip import step as ST
    monkeypatch.setattr(ST, "ops", _masked_ops())
    W, b = 3, 8
    t, s = SR.clustered(W * b, 77)
    assert bool((~SR.keep_mask(t, t, THRES)).any())
    rel = lambda a, b_: float((a.double() - b_).norm() / b_.norm())
    order = (lambda te, st: (te, st)) if teacher == "x" else (lambda te, st: (st, te))
    kw = dict(sim_teacher=teacher, sim_thres=THRES)
    want = SR.with_grads(lambda a, c, sc: SR.loss_world1(a, c, sc, THRES), t, s, SCALE)
    loss, d0, d1, ds = ST.pair_loss_and_grads(None, 0, 1, *order(t, s), *order(t, s), SCALE, **kw)
    dt, dst = order(d0, d1)
    assert abs(float(loss) - want[0]) < 1e-5 * want[0] and rel(dt, want[1]) < 1e-4 and rel(dst, want[2]) < 1e-4
    assert abs(float(ds) - want[3]) < 1e-4 * max(1.0, abs(want[3]))
    plain = float(ST.pair_loss_and_grads(None, 0, 1, *order(t, s), *order(t, s), SCALE)[0])
    assert abs(plain - want[0]) > 1e-2                                   # without the arguments: today's loss
    for r in range(W):
        sl = slice(r * b, (r + 1) * b)
        want = SR.with_grads(lambda a, c, sc: SR.loss_local(a, c, t.double(), s.double(), r, sc, THRES), t[sl], s[sl], SCALE)
        loss, d0, d1, ds = ST.pair_loss_and_grads(None, r, W, *order(t[sl], s[sl]), *order(t, s), SCALE, local_loss=True, dist=True, **kw)
        dt, dst = order(d0, d1)
        assert abs(float(loss) - want[0]) < 1e-5 * want[0], (r, float(loss), want[0])
        assert rel(dt, want[1]) < 1e-4 and rel(dst, want[2]) < 1e-4, r
        assert abs(float(ds) - want[3]) < 1e-4 * max(1.0, abs(want[3]))
