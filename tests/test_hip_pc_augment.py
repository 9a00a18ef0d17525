"""GPU: vl_pc_augment against tests/pc_augment_ref.py (the dropped set against the Philox restatement exactly, the values
against the reference's sequence in fp64 under that mask), its flags and refusals, and PCProcessorTrain."""
import numpy as np
import pytest
import torch

import pc_augment_ref as R
from test_pc_augment_host import COMPOSED_ATOL, REFUSALS, refuse
from test_pc_processor import _cloud

pytestmark = pytest.mark.gpu

NORM_ATOL = 2e-5 + COMPOSED_ATOL      # 2e-5: what tests/test_pc_processor.py gives the fp32 reductions of the normalisation
RATIOS = (0.0, 0.4, 0.875)
# N, G, C, B, index list
CASES = {
    "basic": (700, 128, 3, 3, "fps"),
    "partial-group": (1030, 1030, 6, 3, None),        # G % 4 != 0: the last Philox group is partial
    "single-point": (64, 1, 3, 3, "fps"),
    "full-lds": (9000, 8192, 3, 2, "fps"),            # the whole 96 KiB of gathered points
    "re-read": (9000, 8500, 3, 2, "subset"),          # beyond the LDS budget: the points are read again
}


def _scalars(b):
    g = np.random.default_rng(40 + b)
    return dict(scale=g.uniform(0.8, 1.25), shift=g.uniform(-0.1, 0.1, 3), angles=np.clip(0.06 * g.standard_normal(3), -0.18, 0.18),
                final=g.uniform(0, 2 * np.pi))


def _inputs(N, G, C, B, kind):
    """Clouds whose xyz lie in the unit ball (the 2e-6 of the composed form is derived for |p| <= 1), the index list on the
    host and on the GPU, and the selected points."""
    from vitlens_hip import ops
    pcs = np.stack([_cloud(N, C, 10 + b) for b in range(B)])
    pcs[:, :, :3] /= np.float32(1.001) * np.sqrt((pcs[:, :, :3].astype(np.float64) ** 2).sum(-1)).max().astype(np.float32)
    x = torch.from_numpy(pcs).cuda()
    if kind == "fps":
        start = torch.tensor([7, N - 1, N // 2][:B], dtype=torch.int64, device="cuda")
        idx, _ = ops.fps(x[:, :, :3].contiguous(), start, G, want_centers=False)
    elif kind == "subset":
        idx = torch.from_numpy(np.stack([np.random.default_rng(b).permutation(N)[:G] for b in range(B)])).cuda()
    else:
        idx = None
    host_idx = np.tile(np.arange(N), (B, 1)) if idx is None else idx.cpu().numpy()
    sel = np.stack([pcs[b][host_idx[b]] for b in range(B)])
    for b in range(B):
        assert len(np.unique(sel[b][:, :3], axis=0)) == G                  # pairwise distinct: a dropped row is recognisable
    return pcs, x, idx, sel


@pytest.mark.parametrize("name", list(CASES))
def test_mask_and_values(name):
    from vitlens_hip import ops
    N, G, C, B, kind = CASES[name]
    pcs, x, idx, sel = _inputs(N, G, C, B, kind)
    sc = [_scalars(b) for b in range(B)]
    seeds = [0x9E3779B97F4A7C15 * (b + 1) % 2 ** 64 for b in range(B)]
    for flags, atol in ((0, COMPOSED_ATOL), (R.NORMALIZE | (R.NORM_GUARD if G == 1 else 0), NORM_ATOL)):
        rows = [R.record(sc[b]["scale"], sc[b]["shift"], sc[b]["angles"], sc[b]["final"], "y", RATIOS[b], flags, seeds[b]) for b in range(B)]
        out = ops.pc_augment(x, idx, ops.pc_augment_params(rows, "cuda")).cpu().numpy()
        assert out.shape == (B, G, C) and out.dtype == np.float32
        for b in range(B):
            mask = R.drop_mask(seeds[b], G, RATIOS[b])
            # exactly the points of u_j <= ratio were dropped: a dropped row IS row 0 (which is point 0 either way)
            got = (out[b, :, :3] == out[b, 0, :3]).all(axis=1)
            want = mask.copy()
            want[0] = True
            assert np.array_equal(got, want), (name, b, int(got.sum()), int(want.sum()))
            if RATIOS[b] == 0.4 and G >= 128:
                assert 0.25 < mask.mean() < 0.55
            xyz = sel[b][:, :3]
            if flags & R.NORMALIZE:
                xyz = R.normalize_f64(xyz, bool(flags & R.NORM_GUARD))
            ref = R.sequential_f64(xyz, mask, sc[b]["scale"], sc[b]["shift"], sc[b]["angles"], sc[b]["final"], "y")
            err = np.abs(out[b, :, :3] - ref).max()
            print(f"{name} flags={flags} b={b} ratio={RATIOS[b]}: dropped {int(mask.sum())}/{G}, max |out - fp64| = {err:.3e} (limit {atol:.1e})")
            assert err <= atol, (name, flags, b, err)
            assert np.array_equal(out[b, :, 3:], sel[b][:, 3:])          # the feature channels, bit for bit
        if G == 1 and flags:
            for b in range(B):                                            # the guard on one point: xyz = 0, the output is t
                assert np.array_equal(out[b, 0, :3], np.array(rows[b][1], dtype=np.float32))


def test_guard_and_colour_fill():
    from vitlens_hip import ops
    pt = np.array([0.5, -1.25, 2.0, 0.1, 0.2, 0.3], dtype=np.float32)
    pcs = np.stack([np.tile(pt, (50, 1)), _cloud(50, 6, 3), _cloud(50, 6, 4)])
    s = _scalars(0)
    rec = lambda flags: R.record(s["scale"], s["shift"], s["angles"], s["final"], "z", 0.4, flags, 77)
    rows = [rec(R.NORMALIZE | R.NORM_GUARD), rec(R.NORMALIZE | R.NORM_GUARD | R.FEAT_FILL), rec(R.NORMALIZE | R.NORM_GUARD)]
    out = ops.pc_augment(torch.from_numpy(pcs).cuda(), None, ops.pc_augment_params(rows, "cuda"), feat_fill=0.4).cpu().numpy()
    t = np.array(rows[0][1], dtype=np.float32)
    assert np.array_equal(out[0, :, :3], np.tile(t, (50, 1)))                   # identical points: xyz exactly 0, then + t
    assert np.array_equal(out[0, :, 3:], pcs[0, :, 3:])
    assert np.array_equal(out[1, :, 3:], np.full((50, 3), np.float32(0.4)))     # exactly 0.4
    assert np.array_equal(out[2, :, 3:], pcs[2, :, 3:])                         # bit-identical otherwise
    mask = R.drop_mask(77, 50, 0.4)
    for b in (1, 2):
        ref = R.sequential_f64(R.normalize_f64(pcs[b, :, :3], True), mask, s["scale"], s["shift"], s["angles"], s["final"], "z")
        assert np.abs(out[b, :, :3] - ref).max() <= NORM_ATOL
    # ratio -1 drops nothing, ratio 1 drops everything
    rows = [R.record(1.0, np.zeros(3), np.zeros(3), 0.0, "y", r, 0, 5) for r in (-1.0, 1.0, 0.0)]
    out = ops.pc_augment(torch.from_numpy(pcs).cuda(), None, ops.pc_augment_params(rows, "cuda")).cpu().numpy()
    want = pcs[2].copy()
    want[R.drop_mask(5, 50, 0.0), :3] = want[0, :3]                             # (ratio 0 drops a point whose u is exactly 0)
    assert np.array_equal(out[2], want)                                         # identity record: the cloud itself
    assert np.array_equal(out[0], pcs[0])
    assert np.array_equal(out[1, :, :3], np.tile(pcs[1, 0, :3], (50, 1))) and np.array_equal(out[1, :, 3:], pcs[1, :, 3:])


def test_processor():
    from open_clip.modal_3d.processors.pc_processor import PCProcessorEval, PCProcessorTrain
    B, N, G = 3, 700, 128
    pcs = np.stack([_cloud(N, 3, 20 + b) for b in range(B)])
    start = np.array([7, N - 1, N // 2], dtype=np.int64)
    a = PCProcessorTrain(G, True, seed=7).process_batch(pcs, start=start)
    b = PCProcessorTrain(G, True, seed=7).process_batch(pcs, start=start)
    c = PCProcessorTrain(G, True, seed=8).process_batch(pcs, start=start)
    assert a.is_cuda and a.shape == (B, G, 3) and a.dtype == torch.float32
    assert torch.equal(a, b) and not torch.equal(a, c) and bool(torch.isfinite(a).all())
    # augment=False is sampling + pc_norm: what PCProcessorEval gives, within the margin of two fp32 reductions in different orders
    plain = PCProcessorTrain(G, True, augment=False).process_batch(pcs, start=start)
    assert (plain - PCProcessorEval(G, True).process_batch(pcs, start=start)).abs().max().item() <= 2e-5
    # replaying the records of a processor reproduces its batch
    p = PCProcessorTrain(G, True, seed=7)
    rows = [p.draw_params() for _ in range(B)]
    assert torch.equal(PCProcessorTrain(G, True, seed=99).process_batch(pcs, start=start, params=rows), a)
    # the single-cloud call of the reference
    np.random.seed(3)
    one = PCProcessorTrain(G, True, seed=7)(pcs[0])
    assert one.shape == (G, 3) and bool(torch.isfinite(one).all())
    np.random.seed(3)
    assert torch.equal(one, PCProcessorTrain(G, True, seed=7).process_batch(pcs[:1], start=[np.random.randint(0, N)])[0])


def test_processor_openshape_y_up_equals_the_restatement_on_the_swapped_cloud():
    from open_clip.modal_3d.processors.pc_processor import PCProcessorTrain
    B, N, G = 3, 400, 200
    pcs = np.stack([_cloud(N, 6, 30 + b) for b in range(B)])
    sub = np.stack([np.random.default_rng(b).permutation(N)[:G] for b in range(B)])
    out = PCProcessorTrain(G, False, flavour="openshape", seed=9, y_up=True, rgb_random_drop_prob=0.5).process_batch(pcs, subset=sub)
    out = out.cpu().numpy()
    rng = np.random.RandomState(9)
    filled = 0
    for b in range(B):
        ratio = float(np.float32(rng.random_sample() * 0.875))
        seed = int(rng.randint(0, 2 ** 32, dtype=np.uint64)) << 32 | int(rng.randint(0, 2 ** 32, dtype=np.uint64))
        scale, shift = rng.uniform(0.8, 1.25, 1)[0], rng.uniform(-0.1, 0.1, (1, 3))[0]
        angles, theta = np.clip(0.06 * rng.randn(3), -0.18, 0.18), rng.uniform(0, 2 * np.pi)
        fill = rng.rand() < 0.5
        sw = pcs[b][sub[b]].copy()
        sw[:, [1, 2]] = sw[:, [2, 1]]
        ref = R.sequential_f64(R.normalize_f64(sw[:, :3], True), R.drop_mask(seed, G, ratio), scale, shift, angles, theta, "z")
        assert np.abs(out[b, :, :3] - ref).max() <= NORM_ATOL
        assert np.array_equal(out[b, :, 3:], np.full((G, 3), np.float32(0.4)) if fill else sw[:, 3:])
        filled += fill
    assert 0 < filled < B                                                 # both branches of the colour drop were seen


@pytest.mark.parametrize("case,text", REFUSALS)
def test_refusals_launch_nothing(case, text):
    from vitlens_hip import _lib
    lib = _lib.load_library()
    pts = torch.zeros(2, 8, 3, device="cuda")
    idx = torch.zeros(2, 4, dtype=torch.int64, device="cuda")
    out = torch.full((2, 8, 3), 123.0, device="cuda")
    params = torch.zeros(2, 16, dtype=torch.int32, device="cuda")
    real = dict(pts=pts.data_ptr(), idx=idx.data_ptr(), out=out.data_ptr(), params=params.data_ptr())
    real.update(case)
    assert refuse(lib, real) != 0
    err = lib.vl_last_error().decode()
    assert text in err and "vl_pc_augment" in err
    torch.cuda.synchronize()
    assert bool((out == 123.0).all())


def test_wrapper_refusals():
    from vitlens_hip import ops
    pts = torch.zeros(2, 8, 3, device="cuda")
    ok = ops.pc_augment_params([R.record(1.0, np.zeros(3), np.zeros(3), 0.0, "y", 0.0, 0, 0)] * 2, "cuda")
    for bad_pts in (torch.zeros(2, 8, 2, device="cuda"), torch.zeros(2, 8, 9, device="cuda")):
        with pytest.raises(RuntimeError, match="vl_pc_augment: bad shape"):
            ops.pc_augment(bad_pts, None, ok)
    with pytest.raises(ValueError, match="params"):
        ops.pc_augment(pts, None, ok[:1])
    with pytest.raises(ValueError, match="idx"):
        ops.pc_augment(pts, torch.zeros(2, 4, dtype=torch.int32, device="cuda"), ok)
    with pytest.raises(ValueError, match="drop_ratio"):
        ops.pc_augment_params([R.record(1.0, np.zeros(3), np.zeros(3), 0.0, "y", 1.25, 0, 0)], "cuda")
