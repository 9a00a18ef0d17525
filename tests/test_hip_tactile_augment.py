"""GPU: vl_tactile_augment and Tactile_Processor_Train against the sequential restatement of the reference's pipeline
(tests/tactile_augment_ref.py), every pixel compared.

Cases: sources of 61 x 45, 37 x 53 and 9 x 200 with each of the six boxes of test_hip_rgbd_augment._boxes (the whole image, a
1 x 1 box, a 7 x W box, two corners, the interior) at S = 32 and S = 33, in batches of 5, 4, 6 and 3 cases of mixed sizes
(antialiased and plain batches alternate), and one case of 120 x 160 -> 224.

1. Unrotated values.  With angle 0 and no flips every pixel lies within 4 e32 of the restatement in float64, where e32 is the
   largest distance between the restatement in float32 and in float64 over the cases of one output size - computed here from
   the restatement, never from the kernel.  It is the bound of this same resampler in tests/test_hip_rgbd_augment.py (the
   kernel's tap sums are associated differently and its multiply-adds are fused, each of which moves a value by about what
   the float32 restatement itself loses).  Measured on an MI355X: e32 = 6.0e-7 at S = 32, 3.1e-5 at
   S = 33 (the 7 x 200 box without antialiasing) and 3.1e-5 at S = 224; the kernel's largest distance is the same figure at
   each size.
2. Rotation and flips, exact.  The two flips and the nearest rotation only move pixels, and the device's coordinate arithmetic
   is IEEE float32 with nothing contracted, so the output under (flip_h, flip_v, angle) must be torch.equal to the same
   sample's unrotated output R gathered through the float32 index map (tactile_augment_ref.index_map) and the flips, with
   float32((0 - mean[c]) / std[c]) where the map says fill.  All four flip combinations, every angle of the host test and 45,
   30 and 60 degrees (whose diagonal ties are no excuse on the device), every case at S = 32 and 33; three angles at S = 224."""
import numpy as np
import pytest
import torch

import tactile_augment_ref as T
from test_hip_rgbd_augment import _boxes

pytestmark = pytest.mark.gpu

SOURCES = ((61, 45), (37, 53), (9, 200))
MEAN, STD = T.CLIP_MEAN, T.CLIP_STD
ANGLES = (0.0, 90.0, 180.0, 270.0, 360.0, 0.001, 359.999, 17.0, 123.456, 200.25, 333.3, 45.0, 30.0, 60.0)
FLIPS = ((False, False), (True, False), (False, True), (True, True))
BATCHES = (5, 4, 6, 3)                                   # 18 cases: 3 sources x 6 boxes
BIG = dict(src=0, box=(10, 20, 90, 120))                 # of the 120 x 160 source, to S = 224
BIG_VARIANTS = ((True, False, 17.0), (False, True, 123.456), (True, True, 45.0))


def _cases():
    """case k: source k mod 3, box (k // 3) of its six"""
    return [dict(src=k % 3, box=_boxes(*SOURCES[k % 3])[k // 3]) for k in range(18)]


def _draw(case, flip_h=False, flip_v=False, angle=0.0):
    return dict(box=case["box"], flip_h=flip_h, flip_v=flip_v, angle=angle)


def _run(srcs, cases, draws, antialias, size):
    """one plan, two launches into poisoned outputs (bit-identical) -> out [n,3,S,S] on the host"""
    from vitlens_hip import preproc
    plan = preproc.plan_tactile_train([srcs[c["src"]] for c in cases], draws, size, MEAN, STD, antialias=antialias)
    got = []
    for _ in range(2):
        out = torch.full((len(draws), 3, size, size), float("nan"), device="cuda")
        assert plan.launch(out=out) is out
        got.append(out.cpu())
    assert torch.equal(got[0].view(torch.int32), got[1].view(torch.int32)) and bool(torch.isfinite(got[0]).all())
    return got[0]


@pytest.fixture(scope="module")
def sources():
    return [T.source(H, W, 10 + i) for i, (H, W) in enumerate(SOURCES)]


@pytest.fixture(scope="module")
def big_source():
    return T.source(120, 160, 20)


VARIANTS = [(fh, fv, a) for fh, fv in FLIPS for a in ANGLES]          # VARIANTS[0] is the unrotated, unflipped sample


@pytest.fixture(scope="module")
def runs(sources, big_source):
    """Every case under every variant through the kernel, once for all tests: per output size and batch ONE plan that holds
    the batch's cases under all 56 variants, variant-major, so that neighbours differ in size and in transform.
    -> rows of dict(case, aa, size, srcs, out={variant: [3,S,S]})"""
    cases, rows = _cases(), []
    for size in (32, 33):
        first = 0
        for b, count in enumerate(BATCHES):
            group, aa = cases[first:first + count], b % 2 == 0
            first += count
            out = _run(sources, group * len(VARIANTS), [_draw(c, *v) for v in VARIANTS for c in group], aa, size)
            for i, c in enumerate(group):
                rows.append(dict(case=c, aa=aa, size=size, srcs=sources, label=f"S = {size} case {first - count + i}",
                                 out={v: out[j * count + i] for j, v in enumerate(VARIANTS)}))
    variants = [(False, False, 0.0)] + list(BIG_VARIANTS)
    out = _run([big_source], [BIG] * len(variants), [_draw(BIG, *v) for v in variants], True, 224)
    rows.append(dict(case=BIG, aa=True, size=224, srcs=[big_source], label="S = 224", out=dict(zip(variants, out))))
    return rows


def test_case_set_covers_what_it_claims():
    cases = _cases()
    assert len(cases) == sum(BATCHES) and len({(c["src"], c["box"]) for c in cases}) == 18
    for i, (H, W) in enumerate(SOURCES):
        boxes = [c["box"] for c in cases if c["src"] == i]
        assert (0, 0, H, W) in boxes and any(b[2:] == (1, 1) for b in boxes) and any(b[2:] == (min(7, H), W) for b in boxes)
    # each source meets both resamplers, and no batch holds one size only
    first = 0
    seen = set()
    for b, count in enumerate(BATCHES):
        group = cases[first:first + count]
        first += count
        seen |= {(c["src"], b % 2) for c in group}
        assert len({c["src"] for c in group}) == 3
    assert seen == {(s, a) for s in range(3) for a in range(2)}
    assert VARIANTS[0] == (False, False, 0.0) and len(VARIANTS) == 56


@pytest.fixture(scope="module")
def restated(runs):
    """The unrotated, unflipped restatement of every row in float32 and float64 (r["ref32"], r["ref64"]) -> e32 per output
    size: the largest distance between the two over the rows of that size."""
    e32 = {}
    for r in runs:
        img = r["srcs"][r["case"]["src"]]
        r["ref32"], r["ref64"] = (T.apply(img, _draw(r["case"]), r["size"], MEAN, STD, r["aa"], dt) for dt in (torch.float32, torch.float64))
        e32[r["size"]] = max(e32.get(r["size"], 0.0), float((r["ref32"].double() - r["ref64"]).abs().max()))
    return e32


def test_unrotated_values_against_the_float64_restatement(runs, restated):
    for size in (32, 33, 224):
        worst = 0.0
        for r in (r for r in runs if r["size"] == size):
            got = r["out"][(False, False, 0.0)]
            assert got.shape == r["ref64"].shape
            err, own = float((got.double() - r["ref64"]).abs().max()), float((r["ref32"].double() - r["ref64"]).abs().max())
            print(f"{r['label']:>16} box {r['case']['box']} antialias {r['aa']}: kernel {err:.3e}, float32 restatement {own:.3e}")
            worst = max(worst, err)
        print(f"S = {size}: e32 {restated[size]:.3e}; kernel {worst:.3e}; bound 4 e32")
        assert restated[size] > 0
        assert worst <= 4 * restated[size], (size, worst, restated[size])


def _fill():
    return torch.from_numpy((np.float32(0.0) - np.array(MEAN, np.float32)) / np.array(STD, np.float32))


def _moved(R, flip_h, flip_v, angle):
    """the unrotated output R [3,S,S] under the flips and the rotation's float32 index map, fill where the map says so"""
    idx = torch.from_numpy(T.index_map(R.shape[-1], angle))
    want = T.gather(T.flips(R, flip_h, flip_v), idx)
    return torch.where((idx < 0)[None], _fill()[:, None, None].expand_as(want), want), idx


def test_rotation_and_flips_are_exact_permutations_of_the_unrotated_output(runs):
    checked = fills = 0
    for r in runs:
        R = r["out"][(False, False, 0.0)]
        for (fh, fv, angle), got in r["out"].items():
            want, idx = _moved(R, fh, fv, angle)
            assert torch.equal(got, want), (r["label"], fh, fv, angle, int((got != want).sum()))
            checked += 1
            fills += int((idx < 0).sum())
    assert checked == 2 * 18 * 56 + 4 and fills > 0
    # the maps are not trivial: a flip and a generic angle each change the image of a full-size box
    full = runs[0]["out"]
    assert not torch.equal(full[(True, False, 0.0)], full[(False, False, 0.0)])
    assert not torch.equal(full[(False, True, 0.0)], full[(False, False, 0.0)])
    assert not torch.equal(full[(False, False, 17.0)], full[(False, False, 0.0)])
    assert torch.equal(full[(False, False, 360.0)], full[(False, False, 0.0)])
    assert torch.equal(full[(True, True, 0.0)], full[(False, False, 180.0)])


def test_fill_pixels_are_exactly_the_normalised_zero(runs):
    val = _fill()
    for r in runs[:3] + runs[-1:]:
        for (fh, fv, angle), got in r["out"].items():
            if angle not in (45.0, 17.0, 123.456):
                continue
            fill = torch.from_numpy(T.index_map(r["size"], angle)) < 0
            assert 0.05 < float(fill.float().mean()) < 0.25                          # the four corners
            for c in range(3):
                assert torch.equal(got[c][fill], val[c].expand(int(fill.sum())))


def test_a_sample_does_not_depend_on_its_place_its_neighbours_or_a_second_launch(sources, runs):
    cases = _cases()
    by_case = {(r["size"], r["aa"], r["case"]["src"], r["case"]["box"]): r for r in runs}
    picks = [(cases[7], (True, False, 17.0)), (cases[0], (False, True, 45.0)), (cases[14], (True, True, 200.25)), (cases[7], (True, False, 17.0))]
    for aa in (True, False):
        out = _run(sources, [c for c, _ in picks], [_draw(c, *v) for c, v in picks], aa, 32)        # _run launches twice
        alone = _run(sources, [picks[0][0]], [_draw(picks[0][0], *picks[0][1])], aa, 32)
        assert torch.equal(out[0], out[3]) and torch.equal(out[0], alone[0])
        for k, (c, v) in enumerate(picks):
            r = by_case.get((32, aa, c["src"], c["box"]))
            if r is not None:                                                     # the case ran with this resampler in `runs`
                assert torch.equal(out[k], r["out"][v]), (aa, k)
    assert sum((32, aa, c["src"], c["box"]) in by_case for aa in (True, False) for c, _ in picks) >= 4


def test_one_pixel_and_seven_row_boxes(runs, restated):
    """The two smallest boxes under a flip and a generic angle, against the restatement of that same draw.  A 1 x 1 box has one
    tap of weight 1 on each axis, so every kept pixel is (byte / 255 - mean) / std with three float32 roundings: at most
    (2^-24 + 2^-24) / 0.26 + 2^-23 = 5.8e-7 from the exact value.  The 7 x W box (enlarged vertically, shrunk horizontally)
    is held to the 4 e32 of its output size, away from the rotation's ties (where torch's own float32 may pick the other
    neighbour; the exact test above covers those pixels)."""
    seen = set()
    for r in runs[:-1]:
        top, left, bh, bw = r["case"]["box"]
        img = r["srcs"][r["case"]["src"]]
        got = r["out"][(True, False, 17.0)]
        if (bh, bw) == (1, 1):
            kept = torch.from_numpy(T.index_map(r["size"], 17.0)) >= 0
            px = img[top, left].double() / 255
            want = (px - torch.tensor(MEAN, dtype=torch.float32).double()) / torch.tensor(STD, dtype=torch.float32).double()
            assert float((got.double() - want[:, None, None])[:, kept].abs().max()) < 5.8e-7
            seen.add("1 x 1")
        elif bh == min(7, img.shape[0]) and bw == img.shape[1]:
            ref64 = T.apply(img, _draw(r["case"], True, False, 17.0), r["size"], MEAN, STD, r["aa"], torch.float64)
            clear = ~torch.from_numpy(T.ambiguous(r["size"], 17.0))
            assert float((got.double() - ref64)[:, clear].abs().max()) <= 4 * restated[r["size"]]
            seen.add("7 x W")
    assert seen == {"1 x 1", "7 x W"}


def test_a_refused_call_leaves_the_output_untouched(sources):
    from vitlens_hip import ops, preproc
    case = _cases()[0]
    plan = preproc.plan_tactile_train([sources[0]], [_draw(case, True, True, 30.0)], 32, MEAN, STD)
    out = torch.full((1, 3, 32, 32), float("nan"), device="cuda")
    with pytest.raises(RuntimeError, match="vl_tactile_augment: bad shape"):
        ops.tactile_augment(plan.records, plan.tables, plan.tmp, 32, 0, MEAN, STD, out=out)
    with pytest.raises(RuntimeError, match="vl_tactile_augment: std must be non-zero"):
        ops.tactile_augment(plan.records, plan.tables, plan.tmp, 32, plan.max_nrows, MEAN, (1.0, 0.0, 1.0), out=out)
    with pytest.raises(RuntimeError, match="aligned"):
        ops.tactile_augment(plan.records, plan.tables, plan.tmp.view(-1)[2:], 32, plan.max_nrows, MEAN, STD, out=out)
    with pytest.raises(ValueError, match="out must be"):
        ops.tactile_augment(plan.records, plan.tables, plan.tmp, 32, plan.max_nrows, MEAN, STD, out=out[:, :, :16])
    with pytest.raises(ValueError, match="records must be"):
        ops.tactile_augment(plan.records[:, :23], plan.tables, plan.tmp, 32, plan.max_nrows, MEAN, STD, out=out)
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())
    plan.launch(out=out)
    assert bool(torch.isfinite(out).all())


# ------------------------------------------------------------------------------------------------ the processors
def test_batch_equals_single_calls_under_the_same_seed(sources, tmp_path):
    from PIL import Image
    from open_clip.modal_tactile.processors.tact_processor import Tactile_Processor_Train
    proc = Tactile_Processor_Train.from_config()
    assert (proc.size, proc.antialias, proc.degrees) == (224, True, (0.0, 360.0))
    proc.size = 32
    Image.fromarray(sources[0].numpy()).save(tmp_path / "a.png")
    images = [str(tmp_path / "a.png"), Image.fromarray(sources[1].numpy()), sources[2].numpy(), sources[1].cuda()]
    which = (0, 1, 2, 1)
    torch.manual_seed(11)
    out = proc.batch(images)
    assert out.shape == (4, 3, 32, 32) and out.is_cuda and out.dtype == torch.float32
    torch.manual_seed(11)
    draws = []
    for k in range(4):
        state = torch.get_rng_state()
        draws.append(proc.draw(*SOURCES[which[k]]))
        torch.set_rng_state(state)
        one = proc(images[k])
        assert one.shape == (3, 32, 32) and torch.equal(one, out[k]), k
    assert draws[2]["box"] == (0, 94, 9, 12)                                      # the central fallback
    for k, d in enumerate(draws):                                                 # and it is the drawn transform
        want = T.apply(sources[which[k]], d, 32, MEAN, STD, True, torch.float64)
        differ = (out[k].cpu().double() - want).abs().amax(0) > 1e-4
        # a drawn angle may put a coordinate on a tie, where torch's own float32 picks the other neighbour
        assert not bool((differ & ~torch.from_numpy(T.ambiguous(32, d["angle"]))).any()), k
    assert torch.equal(proc.batch(images, draws=draws), out)


def test_eval_processor_is_the_existing_one(sources):
    from open_clip.modal_tactile.processors.tact_processor import Tactile_Processor_Eval, TactileRGBProcessorEval
    img = T.source(70, 90, 30).numpy()
    a = Tactile_Processor_Eval.from_config()
    b = TactileRGBProcessorEval()
    a.resize = b.resize = 48
    a.size = b.size = 40
    got = a(img)
    assert got.shape == (3, 40, 40) and torch.equal(got, b(img))
    assert torch.equal(Tactile_Processor_Eval({}, MEAN, STD, None, size=40, resize=48)(img), got)
