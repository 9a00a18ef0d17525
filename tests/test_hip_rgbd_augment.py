"""GPU: vl_rgbd_augment and RGBD_Processor_Train against the sequential restatement of the reference's pipeline
(tests/rgbd_augment_ref.py) in float64, every pixel compared.

The cases are hand-written draws at S = 32 on sources of 61 x 45, 37 x 53 and 9 x 200, in batches of five of mixed sizes
(antialiased and plain batches alternate), one sample alone, and one case at S = 224 from 120 x 160.  Between them: all 24
orders of the jitter terms (contrast first and last among them), hue shifts of +-0.4, factors of 0.6 and 1.4, the full-image
box, boxes on every border, a 1 x 1 box and a 7 x W box (enlarged), a six-fold shrink (multi-tap antialiasing), flip on and
off, erase rectangles and none, disabled terms, depth values below DepthNorm's minimum and above its maximum.

Bound: e32 is the largest distance, over all these cases, between the restatement run in float32 and in float64 (RGB and depth
apart) - computed here from the restatement, never from the kernel.  The kernel may be 4 e32 from the float64 values: its tap
sums are associated differently, its multiply-adds are fused, and its grey mean is reduced in another order, each of which
moves a value by about what the float32 restatement itself loses.  e32 is taken per output size, which asks more than one
figure over all cases.  Measured on an MI355X: at S = 32 e32 = 3.1e-6 (RGB), 6.4e-6 (depth) and the kernel is
2.4e-6 and 6.4e-6 from float64; at S = 224 both are 5.8e-5 and 3.2e-4."""
import itertools

import numpy as np
import pytest
import torch

import rgbd_augment_ref as R

pytestmark = pytest.mark.gpu

S = 32
SOURCES = ((61, 45), (37, 53), (9, 200))
MEAN, STD = R.CLIP_MEAN + (0.0418,), R.CLIP_STD + (0.0295,)
ORDERS = list(itertools.permutations(range(4)))


def _boxes(H, W):
    return [(0, 0, H, W),                                   # the whole image
            (H // 2, W // 3, 1, 1),                         # one pixel
            (H - min(7, H), 0, min(7, H), W),               # 7 x W on the bottom, left and right borders
            (0, 0, H // 2, W // 2),                         # top-left corner
            (H - H // 2, W - W // 2, H // 2, W // 2),       # bottom-right corner
            (H // 4, W // 4, H // 2, W // 2)]               # interior


def _cases():
    """25 draws: case k has order k mod 24, source k mod 3, and walks through the boxes, factors, shifts and rectangles"""
    factors = ((0.6, 1.4, 1.25), (1.4, 0.6, 0.8), (0.9, 1.1, 0.6), (1.25, 0.75, 1.4))
    hues = (0.4, -0.4, 0.13, -0.02)
    erases = (None, (0, 0, 9, 13), (20, 25, 12, 7), None, (5, 6, 3, 20))      # top-left corner, bottom-right corner, interior
    out = []
    for k in range(25):
        H, W = SOURCES[k % 3]
        b, c, s = factors[k % 4]
        out.append({"src": k % 3, "box": _boxes(H, W)[(k // 3) % 6], "flip": bool((k // 2) & 1), "order": ORDERS[k % 24],
                    "brightness": b, "contrast": c, "saturation": s, "hue": hues[k % 4], "erase": erases[k % 5]})
    out[7].update(brightness=None, hue=None)                                   # two terms off
    out[13].update(brightness=None, contrast=None, saturation=None, hue=None)  # all terms off
    out[18].update(contrast=None)
    return out


@pytest.fixture(scope="module")
def sources():
    return [R.sample(H, W, 10 + i) for i, (H, W) in enumerate(SOURCES)]


def _run(sources, draws, antialias, size=S):
    """one plan, one launch -> (rgb [n,3,S,S], depth [n,1,S,S]) on the host, and the plan"""
    from vitlens_hip import preproc
    plan = preproc.plan_rgbd([sources[d["src"]][0] for d in draws], [sources[d["src"]][1] for d in draws], draws, size, MEAN, STD,
                             R.DEPTH_CLAMP, antialias=antialias)
    rgb, depth = plan.launch()
    return rgb.cpu(), depth.cpu(), plan


def _ref(sources, d, antialias, dtype, size=S):
    rgb, depth = sources[d["src"]]
    return R.apply(rgb, depth, d, size, MEAN, STD, antialias, dtype)


@pytest.fixture(scope="module")
def runs(sources):
    """Every case through the kernel (five batches of five, antialiased and plain alternating, then case 3 alone and the
    S = 224 case) and through the restatement in float32 and float64, once for all tests."""
    cases = _cases()
    big_src = R.sample(120, 160, 20)
    big = {"src": 0, "box": (10, 20, 90, 120), "flip": True, "order": (2, 1, 3, 0), "brightness": 1.3, "contrast": 0.7, "saturation": 1.4,
           "hue": -0.3, "erase": (100, 50, 60, 120)}
    rows = []
    for b in range(5):
        aa = b % 2 == 0
        draws = cases[5 * b:5 * b + 5]
        rgb, depth, _ = _run(sources, draws, aa)
        rows += [dict(d=d, aa=aa, size=S, srcs=sources, rgb=rgb[i], depth=depth[i], label=f"case {5 * b + i}") for i, d in enumerate(draws)]
    rgb, depth, _ = _run(sources, [cases[3]], True)
    rows.append(dict(d=cases[3], aa=True, size=S, srcs=sources, rgb=rgb[0], depth=depth[0], label="case 3 alone"))
    rgb, depth, _ = _run([big_src], [big], True, 224)
    rows.append(dict(d=big, aa=True, size=224, srcs=[big_src], rgb=rgb[0], depth=depth[0], label="S = 224"))
    for r in rows:
        r["ref32"] = _ref(r["srcs"], r["d"], r["aa"], torch.float32, r["size"])
        r["ref64"] = _ref(r["srcs"], r["d"], r["aa"], torch.float64, r["size"])
    return rows


def test_case_set_covers_what_it_claims():
    cases = _cases()
    assert {c["order"] for c in cases} == set(ORDERS)
    assert any(c["order"][0] == 1 for c in cases) and any(c["order"][3] == 1 for c in cases)
    assert {0.4, -0.4} <= {c["hue"] for c in cases}
    assert {0.6, 1.4} <= {c[k] for c in cases for k in ("brightness", "contrast", "saturation")}
    assert {True, False} == {c["flip"] for c in cases}
    shapes = {(c["src"], c["box"]) for c in cases}
    for i, (H, W) in enumerate(SOURCES):
        assert (i, (0, 0, H, W)) in shapes                                       # 9 x 200 whole: 200 -> 32, more than six-fold
    assert any(c["box"][2:] == (1, 1) for c in cases) and any(c["box"][2] == 7 and c["box"][3] == SOURCES[c["src"]][1] for c in cases)
    assert any(c["erase"] is None for c in cases) and any(c["erase"] == (0, 0, 9, 13) for c in cases)
    assert any(c["erase"] is not None and c["erase"][0] + c["erase"][2] == S and c["erase"][1] + c["erase"][3] == S for c in cases)
    # each feature above meets both resamplers: batches alternate, and 25 cases walk 3 sources x 6 boxes out of step with 5
    assert {(c["box"] == (0, 0) + SOURCES[c["src"]], (k // 5) % 2) for k, c in enumerate(cases)} >= {(True, 0), (True, 1)}


def test_values_against_the_float64_restatement(runs):
    # e32 is taken per output size, which asks more than one figure over all cases would: the weights of a tap at source
    # coordinate x carry float32's rounding of x, so the S = 224 case (coordinates up to 120) loses ten times what the
    # S = 32 cases lose, in the restatement and in the kernel alike
    for size in (S, 224):
        group = [r for r in runs if r["size"] == size]
        e32 = [max(float((r["ref32"][c].double() - r["ref64"][c]).abs().max()) for r in group) for c in (0, 1)]
        worst = [0.0, 0.0]
        for r in group:
            for c, got in ((0, r["rgb"]), (1, r["depth"])):
                assert got.shape == r["ref64"][c].shape and bool(torch.isfinite(got).all())
                err = float((got.double() - r["ref64"][c]).abs().max())
                worst[c] = max(worst[c], err)
                print(f"{r['label']:>13} {'rgb' if c == 0 else 'depth':>5}: kernel {err:.3e}, float32 restatement "
                      f"{float((r['ref32'][c].double() - r['ref64'][c]).abs().max()):.3e}")
        print(f"S = {size}: e32 rgb {e32[0]:.3e} depth {e32[1]:.3e}; kernel rgb {worst[0]:.3e} depth {worst[1]:.3e}; bound 4 e32")
        assert e32[0] > 0 and e32[1] > 0
        assert worst[0] <= 4 * e32[0] and worst[1] <= 4 * e32[1], (size, worst, e32)


def _erased_value():
    m, s = np.array(MEAN, dtype=np.float32), np.array(STD, dtype=np.float32)
    return (np.float32(0.0) - m) / s


def test_erased_pixels_are_exactly_the_rectangle(sources):
    base = dict(_cases()[4], erase=None)
    draws = [base, dict(base, erase=(0, 0, 9, 13)), dict(base, erase=(20, 25, 12, 7)), dict(base, erase=(31, 0, 1, 32)),
             dict(base, erase=(4, 4, 0, 5))]                                      # none, two corners, the last row, an empty one
    rgb, depth, _ = _run(sources, draws, True)
    full = torch.cat([rgb, depth], dim=1).numpy()
    val = _erased_value()
    for k, d in enumerate(draws[1:], start=1):
        i, j, h, w = d["erase"]
        inside = np.zeros((S, S), bool)
        inside[i:i + h, j:j + w] = True
        for c in range(4):
            assert np.array_equal(full[k, c][inside], np.full(int(inside.sum()), val[c], np.float32)), (d["erase"], c)
            assert np.array_equal(full[k, c][~inside], full[0, c][~inside]), (d["erase"], c)
    assert not np.any(full[0, 3] == val[3])                                       # depth is at least 0.01 / 75: never 0 unless erased


def test_depth_does_not_depend_on_the_jitter(sources):
    base = _cases()[5]
    other = dict(base, order=(3, 0, 2, 1), brightness=0.61, contrast=None, saturation=1.39, hue=0.33)
    rgb, depth, _ = _run(sources, [base, other], False)
    assert torch.equal(depth[0], depth[1]) and not torch.equal(rgb[0], rgb[1])


def test_a_sample_does_not_depend_on_its_place_its_neighbours_or_a_second_launch(sources, runs):
    cases = _cases()
    assert torch.equal(runs[3]["rgb"], runs[25]["rgb"]) and torch.equal(runs[3]["depth"], runs[25]["depth"])      # in a batch of five, alone
    rgb, depth, plan = _run(sources, [cases[12], cases[3], cases[20], cases[3]], True)
    for k in (1, 3):
        assert torch.equal(rgb[k], runs[3]["rgb"]) and torch.equal(depth[k], runs[3]["depth"])
    assert torch.equal(rgb[0], runs[12]["rgb"]) and torch.equal(rgb[2], runs[20]["rgb"])
    rgb2, depth2 = plan.launch()
    assert torch.equal(rgb2.cpu(), rgb) and torch.equal(depth2.cpu(), depth)


def test_disabled_terms_leave_the_resampled_image(sources):
    off = dict(_cases()[2], brightness=None, contrast=None, saturation=None, hue=None)
    draws = [off, dict(off, order=(3, 2, 1, 0)), dict(off, brightness=1.3), dict(off, hue=0.25)]
    rgb, depth, _ = _run(sources, draws, True)
    assert torch.equal(rgb[0], rgb[1])
    assert not torch.equal(rgb[0], rgb[2]) and not torch.equal(rgb[0], rgb[3])


# ------------------------------------------------------------------------------------------------ the processors
def test_process_batch_equals_single_calls_under_the_same_seed(sources, tmp_path):
    from PIL import Image
    from open_clip.modal_depth.processors.vt_processor import RGBD_Processor_Train
    proc = RGBD_Processor_Train.from_config({"img_mean": None})
    assert proc.mean[3] == 0.0418 and proc.std[3] == 0.0295
    proc = RGBD_Processor_Train.from_config()
    proc.size = S
    Image.fromarray(sources[0][0].numpy()).save(tmp_path / "a.png")
    torch.save(sources[0][1], tmp_path / "a.pt")
    images = [str(tmp_path / "a.png"), Image.fromarray(sources[1][0].numpy()), sources[2][0].numpy(), sources[1][0].cuda()]
    depths = [str(tmp_path / "a.pt"), sources[1][1][None], sources[2][1].numpy(), sources[1][1].cuda()]
    torch.manual_seed(11)
    rgb, depth = proc.process_batch(images, depths)
    assert rgb.shape == (4, 3, S, S) and depth.shape == (4, 1, S, S) and rgb.is_cuda and rgb.dtype == torch.float32
    torch.manual_seed(11)
    draws = []
    for k in range(4):
        state = torch.get_rng_state()
        draws.append(proc.draw(*SOURCES[(0, 1, 2, 1)[k]]))
        torch.set_rng_state(state)
        r1, d1 = proc(images[k], depths[k])
        assert r1.shape == (3, S, S) and d1.shape == (1, S, S)
        assert torch.equal(r1, rgb[k]) and torch.equal(d1, depth[k]), k
    for k, d in enumerate(draws):                                                 # and it is the drawn transform
        want = R.apply(*sources[(0, 1, 2, 1)[k]], d, S, MEAN, STD, True, torch.float64)
        assert float((rgb[k].cpu().double() - want[0]).abs().max()) < 1e-4 and float((depth[k].cpu().double() - want[1]).abs().max()) < 1e-4
    r2, d2 = proc.process_batch(images, depths, draws=draws)
    assert torch.equal(r2, rgb) and torch.equal(d2, depth)


def test_eval_processor_equals_the_float_resamplers(sources):
    from open_clip.modal_depth.processors.vt_processor import DepthProcessorEval, RGBD_Processor_Eval
    from vitlens_hip import preproc
    rgb, depth = R.sample(70, 90, 30)
    proc = RGBD_Processor_Eval.from_config()
    proc.size = 48
    img, dep = proc(rgb.numpy(), depth)
    assert img.shape == (3, 48, 48) and dep.shape == (1, 48, 48)
    assert torch.equal(img, preproc.float_image_to_tensor(rgb.cuda(), 48, 48, R.CLIP_MEAN, R.CLIP_STD, antialias=True))
    assert torch.equal(dep, DepthProcessorEval(size=48)(depth))
