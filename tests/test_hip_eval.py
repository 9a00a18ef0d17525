"""GPU: the evaluation kernels (csrc/vl_eval.hip) against the fp64 / integer restatements of tests/eval_ref.py.  Counts are
compared exactly, average precisions within 1e-12.  Operands and outputs sit inside larger allocations whose surroundings are
checked afterwards, so a read of the padding (NaN) or a write outside an output shows."""
import numpy as np
import pytest
import torch

import eval_ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 64


def ops():
    from vitlens_hip import ops as o
    return o


class Boxed:
    """A tensor of `shape` (row stride ld for 2-D) inside a larger allocation filled with `fill`."""

    def __init__(self, shape, dtype, fill, ld=None, src=None):
        rows, cols = (shape[0], shape[1]) if len(shape) == 2 else (1, shape[0])
        ld = cols if ld is None else ld
        self.fill, self.rows, self.cols, self.ld = fill, rows, cols, ld
        self.buf = torch.full((2 * GUARD + rows * ld,), fill, dtype=dtype, device=DEV)
        full = self.buf[GUARD:GUARD + rows * ld].view(rows, ld)
        self.t = full[:, :cols] if len(shape) == 2 else full[0, :cols]
        self.full = full
        if src is not None:
            self.t.copy_(torch.as_tensor(src).to(DEV))

    def intact(self):
        same = (lambda x: x.isnan()) if self.fill != self.fill else (lambda x: x == self.fill)
        return bool(same(self.buf[:GUARD]).all() and same(self.buf[-GUARD:]).all() and same(self.full[:, self.cols:]).all())


def _logits(B, C, seed):
    """Values on a grid of eighths: ties within and between groups at every size."""
    rng = np.random.default_rng(seed)
    return (np.round(rng.standard_normal((B, C)) * 8) / 8).astype(np.float32), rng.integers(0, C, B)


def _maps(C):
    fold3 = np.arange(C, dtype=np.int32)
    fold3[[0, C // 2, C - 1]] = C - 1                    # (C = 2: both classes)
    return {"identity": None, "fold3": fold3, "all": np.full(C, 100, np.int32)}


def _run_hits(o, logits, target, ks, cmap, ld_extra=3):
    B, C = logits.shape
    gl = Boxed((B, C), torch.float32, float("nan"), ld=C + ld_extra, src=logits)
    hits, per_class, pred = Boxed((2,), torch.int32, -7), Boxed((3, C), torch.int32, -7), Boxed((B,), torch.int32, -7)
    hits.t.zero_(); per_class.t.zero_()
    cm = None if cmap is None else torch.from_numpy(cmap).to(DEV)
    tg = torch.as_tensor(target, dtype=torch.int64).to(DEV)
    per = per_class.full.view(3, C)
    o.eval_hits(gl.t, tg, ks, class_map=cm, hits=hits.t, per_class=per, pred=pred.t)
    torch.cuda.synchronize()
    assert gl.intact() and hits.intact() and per_class.intact() and pred.intact()
    return hits, per, pred, (gl, tg, cm)


@pytest.mark.parametrize("C", (2, 5, 40, 527, 1203))
@pytest.mark.parametrize("B", (1, 63, 257))
def test_eval_hits_equals_the_restatement(B, C):
    o = ops()
    logits, target = _logits(B, C, seed=1000 * B + C)
    for name, cmap in _maps(C).items():
        want_hits, want_pc, want_pred = eval_ref.eval_hits(logits, target, (1, 5), cmap)
        hits, per, pred, _ = _run_hits(o, logits, target, (1, 5), cmap)
        assert hits.t.tolist() == want_hits.tolist(), name
        assert per.cpu().numpy().tolist() == want_pc.tolist(), name
        assert pred.t.tolist() == want_pred.tolist(), name
        if name == "all":
            assert want_hits.tolist() == [B, B]                                   # every class is the target's group
    # the identity map is vl_topk_hits
    th, _ = o.topk_hits(torch.from_numpy(logits).to(DEV), torch.from_numpy(target).to(DEV), (1, 5))
    assert th.tolist() == eval_ref.eval_hits(logits, target, (1, 5))[0].tolist()


def test_eval_hits_ties_nan_bad_targets_and_accumulation():
    o = ops()
    B, C = 67, 7
    rng = np.random.default_rng(3)
    logits = rng.integers(0, 3, (B, C)).astype(np.float32)                        # three levels: ties everywhere
    target = rng.integers(0, C, B)
    logits[4] = np.nan                                                            # nothing is greater than a NaN: rank 0
    logits[9, 2] = np.nan
    logits[11, :3] = np.nan
    bad = target.copy()
    bad[0], bad[1] = -1, C                                                        # misses, no per-class update
    fold = np.array([0, 5, 2, 5, 4, 5, 6], np.int32)                              # classes 1, 3, 5 are one group
    for cmap in (None, fold, np.arange(C, dtype=np.int32)):
        for tgt in (target, bad):
            want_hits, want_pc, want_pred = eval_ref.eval_hits(logits, tgt, (1, 3), cmap)
            hits, per, pred, (gl, tg, cm) = _run_hits(o, logits, tgt, (1, 3), cmap)
            assert hits.t.tolist() == want_hits.tolist() and per.cpu().numpy().tolist() == want_pc.tolist()
            assert pred.t.tolist() == want_pred.tolist()
            o.eval_hits(gl.t, tg, (1, 3), class_map=cm, hits=hits.t, per_class=per)          # the counters accumulate
            assert hits.t.tolist() == (2 * want_hits).tolist() and per.cpu().numpy().tolist() == (2 * want_pc).tolist()
            if cmap is None or cmap is not fold:
                th, _ = o.topk_hits(gl.t, tg, (1, 3))
                assert th.tolist() == want_hits.tolist()
    assert eval_ref.eval_hits(logits, bad, (1, 3))[1][0].sum() == B - 2


def test_eval_hits_is_cond_acc_by_its_own_route():
    """Distinct logits: the group-best rank counts what top-k -> map -> any-equal counts."""
    o = ops()
    rng = np.random.default_rng(5)
    B, C = 63, 40
    logits = np.stack([rng.permutation(C) for _ in range(B)]).astype(np.float32) * 0.37 - 3.0
    target = rng.integers(0, C, B)
    mapping, merge = [2, 7, 9, 31], 39
    cmap = np.arange(C, dtype=np.int32)
    cmap[mapping] = merge
    hits, _, _, _ = _run_hits(o, logits, target, (1, 5), cmap)
    assert hits.t.tolist() == eval_ref.cond_acc_hits(logits, target, mapping, merge, (1, 5))
    assert o.class_map_from_merge(C, mapping, merge, DEV).tolist() == cmap.tolist()


@pytest.mark.parametrize("C", (1, 7, 65))
@pytest.mark.parametrize("N", (1, 2, 255, 257, 1025, 4099))
def test_average_precision_equals_the_restatement(N, C):
    o = ops()
    scores, targets = eval_ref.gridded_columns(N, C, seed=100 * N + C)
    if N >= 255:
        scores[3, 0], scores[N - 2, C - 1], scores[7, C // 2] = np.inf, -np.inf, np.inf          # +-inf order as numbers
    want = eval_ref.average_precision(scores, targets)
    gs = Boxed((N, C), torch.float32, float("nan"), ld=C + 3, src=scores)
    gt = Boxed((N, C), torch.float32, float("nan"), ld=C + 1, src=targets)
    out = Boxed((C,), torch.float64, -7.0)
    o.average_precision(gs.t, gt.t, out=out.t)
    torch.cuda.synchronize()
    assert gs.intact() and gt.intact() and out.intact()
    got = out.t.cpu().numpy()
    err = np.abs(got - want).max()
    print(f"average_precision N={N} C={C}: max |err| = {err:.3e}")
    assert err <= 1e-12
    again = o.average_precision(gs.t, gt.t)
    assert torch.equal(again, out.t)                                              # a fixed summation order: the same bits
    if C >= 3:
        assert got[2] == 0.0                                                      # a class without positives


def test_map_on_device_equals_the_host_path():
    pytest.importorskip("sklearn.metrics")
    import warnings
    from open_clip.metrics import MAP
    N, C = 1025, 17
    scores, targets = eval_ref.gridded_columns(N, C, seed=9)
    results = []
    for on_device in (False, True):
        m = MAP()
        m.initialize(on_device=on_device) if on_device else m.initialize()
        for a in range(0, N, 300):
            m.compute(torch.arange(a, min(a + 300, N), device=DEV), torch.from_numpy(scores[a:a + 300]).to(DEV),
                      torch.from_numpy(targets[a:a + 300]).to(DEV))
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            results.append(m.merge_results())
    host, dev = results
    assert set(host) == set(dev) == {"map", "map_cnt", "predict_results"}
    assert dev["map_cnt"] == host["map_cnt"] == N and dev["predict_results"] == host["predict_results"] == {}
    print(f"map host {host['map']!r} device {dev['map']!r}")
    assert abs(float(host["map"]) - float(dev["map"])) <= 1e-12


@pytest.mark.parametrize("B,n_clip,D", ((1, 1, 32), (5, 3, 768), (9, 3, 70), (4, 2, 1)))
def test_clip_mean_normalize(B, n_clip, D):
    """fp32 against fp64.  The outputs are at most 1 in magnitude; the roundings: n_clip - 1 adds and a division per element,
    the squared norm through at most D / 64 + 6 additions per path (relative error below (D / 64 + 7) eps / 2 on the norm), a
    reciprocal and a product: below 16 eps = 1e-6 at D = 768."""
    o = ops()
    rng = np.random.default_rng(B * 100 + D)
    x = rng.standard_normal((B * n_clip, D)).astype(np.float32)
    gx = Boxed((B * n_clip, D), torch.float32, float("nan"), ld=D + 5, src=x)
    got = o.clip_mean_normalize(gx.t, n_clip).cpu().numpy()
    assert gx.intact() and got.shape == (B, D)
    err = np.abs(got - eval_ref.clip_mean_normalize(x, n_clip)).max()
    print(f"clip_mean_normalize B={B} n_clip={n_clip} D={D}: max |err| = {err:.3e}")
    assert err <= 1e-6
    if n_clip == 1:
        assert torch.equal(torch.from_numpy(got).to(DEV), o.l2_normalize(torch.from_numpy(x).to(DEV)))


def test_refusals():
    o = ops()
    logits = torch.zeros(4, 5, device=DEV)
    target = torch.zeros(4, dtype=torch.int64, device=DEV)
    with pytest.raises(ValueError):
        o.eval_hits(logits, target, (1, 5), class_map=torch.zeros(4, dtype=torch.int32, device=DEV))
    with pytest.raises(ValueError):
        o.eval_hits(logits, target, (0, 5))
    with pytest.raises(ValueError):
        o.average_precision(logits, torch.zeros(4, 6, device=DEV))
    with pytest.raises(ValueError):
        o.clip_mean_normalize(logits, 3)
