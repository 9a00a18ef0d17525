"""GPU: the plain-image training transform (Image_Processor_Train, vl_image_augment; csrc/vl_image_augment.hip).

The 8-bit stages (crop-resize, flip, every RandAugment op) are compared byte for byte with the Pillow calls themselves where
Pillow imports, otherwise with tests/image_augment_ref.py, which tests/test_image_augment_host.py pins to Pillow.  The float
tail is compared with the float64 restatement on every pixel, bound 4 e32 per size, e32 = the distance of the float32
restatement from the float64 one (the rule of DESIGN 4.7).  Outputs start as NaN / 0xA5, every case runs twice and the two
runs must be bit-identical."""
import itertools

import numpy as np
import pytest
import torch

import image_augment_ref as A

pytestmark = pytest.mark.gpu

try:
    import PIL  # noqa: F401
    HAVE_PIL = True
except ImportError:
    HAVE_PIL = False

JITTER = dict(order=(2, 0, 3, 1), brightness=0.8, contrast=1.3, saturation=0.7, hue=-0.1)


def expected_u8(img, d, S, **kw):
    from vitlens_hip.preproc import pil_bilinear_tables
    return A.eight_bit(img, d, S, tables=None if HAVE_PIL else pil_bilinear_tables, **kw)


def run(images, draws, S, **kw):
    """-> (out f32 [n,3,S,S], u8 [n,S,S,3]) on the host; two launches into poisoned outputs, bit-identical"""
    from vitlens_hip import preproc
    plan = preproc.plan_image_train([torch.from_numpy(im) for im in images], draws, S, A.CLIP_MEAN, A.CLIP_STD, device="cuda", **kw)
    got = []
    for _ in range(2):
        out = torch.full((len(images), 3, S, S), float("nan"), device="cuda")
        u8 = torch.full((len(images), S, S, 3), 0xA5, device="cuda", dtype=torch.uint8)
        plan.launch(out=out, out_u8=u8)
        torch.cuda.synchronize()
        got.append((out.cpu(), u8.cpu().numpy()))
    assert torch.equal(got[0][0].view(torch.int32), got[1][0].view(torch.int32)) and np.array_equal(got[0][1], got[1][1])
    assert bool(torch.isfinite(got[0][0]).all())
    return got[0]


def check_bytes(images, draws, S, **kw):
    _, u8 = run(images, draws, S, **kw)
    bad = []
    for i, (im, d) in enumerate(zip(images, draws)):
        want = expected_u8(im, d, S, **kw)
        if not np.array_equal(u8[i], want):
            diff = u8[i].astype(int) - want
            bad.append((i, d["ops"], d["box"], d["flip"], int((diff != 0).sum()), int(np.abs(diff).max())))
    assert not bad, f"{len(bad)} of {len(draws)} samples differ from Pillow (sample, ops, box, flip, bytes, max): {bad[:8]}"


def single_op_draws(H, W):
    """14 ops x 2 signs x bins {0, 9, 30}: 84 samples, boxes and flips varied"""
    boxes = [(0, 0, H, W), (min(3, H - 1), min(4, W - 1), max(H - 8, 1), max(W - 9, 1)), (0, W // 2, H, W - W // 2), (H - 1, 0, 1, W)]
    draws = []
    for k, (op, negative, mag_bin) in enumerate(itertools.product(range(14), (False, True), (0, 9, 30))):
        draws.append(dict(JITTER, box=boxes[k % len(boxes)], flip=bool((k // 2) % 2), ops=[(op, negative, mag_bin)]))
    return draws


# ------------------------------------------------------------------------------------------------ 1. all ops in one launch
@pytest.mark.parametrize("S", [32, 33])
def test_every_op_sign_and_bin_in_one_launch_equals_pillow(S):
    img = A.source(45, 37, "random", seed=1)
    draws = single_op_draws(45, 37)
    assert len(draws) == 84
    check_bytes([img] * 84, draws, S)


@pytest.mark.parametrize("kw", [dict(shear_atan=True), dict(solarize_from=255.0)])
def test_version_dependent_points_equal_pillow(kw):
    img = A.source(45, 37, "random", seed=2)
    draws = [d for d in single_op_draws(45, 37) if d["ops"][0][0] in (1, 2, 11)]
    check_bytes([img] * len(draws), draws, 32, **kw)


# ------------------------------------------------------------------------------------------------ 2. degenerate and mixed
@pytest.mark.parametrize("kind,H,W", [("constant", 45, 37), ("binary", 45, 37), ("random", 1, 1)])
def test_degenerate_sources_equal_pillow(kind, H, W):
    img = A.source(H, W, kind, seed=3)
    draws = single_op_draws(H, W)
    check_bytes([img] * len(draws), draws, 32)


def test_every_pair_of_ops_in_one_launch_equals_pillow():
    img = A.source(45, 37, "random", seed=4)
    draws = [dict(JITTER, box=(2, 1, 40, 33), flip=bool(k % 2), ops=[(a, bool(k % 3 == 0), 9), (b, bool(k % 2), 9)])
             for k, (a, b) in enumerate(itertools.product(range(14), range(14)))]
    assert len(draws) == 196
    check_bytes([img] * 196, draws, 32)


def test_four_ops_and_none_equal_pillow():
    img = A.source(45, 37, "random", seed=5)
    draws = [dict(JITTER, box=(0, 0, 45, 37), flip=False, ops=[]),
             dict(JITTER, box=(1, 2, 40, 30), flip=True, ops=[(13, False, 9), (5, True, 30), (9, False, 30), (12, False, 0)]),
             dict(JITTER, box=(1, 2, 40, 30), flip=True, ops=[(1, True, 30), (8, True, 30), (11, False, 20), (4, False, 30)])]
    check_bytes([img] * 3, draws, 32)


def test_full_size_from_480_by_640_equals_pillow():
    img = A.source(480, 640, "random", seed=6)
    draws = [dict(JITTER, box=(10 + op, 20, 400, 500 + op), flip=bool(op % 2), ops=[(op, bool(op % 2), 9)]) for op in range(14)]
    check_bytes([img] * 14, draws, 224)


def test_crop_resize_entry_alone_equals_pillow():
    """vl_image_crop_resize_u8 into its own (poisoned) output: sources of two sizes, boxes on the borders, both flips"""
    from vitlens_hip import preproc
    images = [A.source(45, 37, "random", seed=14), A.source(61, 50, "random", seed=15)]
    boxes = [(0, 0, 45, 37), (3, 4, 30, 22), (44, 0, 1, 37), (0, 0, 61, 50), (10, 45, 51, 5), (7, 9, 33, 33)]
    draws = [dict(JITTER, box=box, flip=bool(k % 2), ops=[(13, False, 9)]) for k, box in enumerate(boxes)]   # the ops are not run
    srcs = [images[0]] * 3 + [images[1]] * 3
    plan = preproc.plan_image_train([torch.from_numpy(im) for im in srcs], draws, 33, A.CLIP_MEAN, A.CLIP_STD, device="cuda")
    from vitlens_hip import ops
    got = []
    for _ in range(2):
        u8 = torch.full((6, 33, 33, 3), 0xA5, device="cuda", dtype=torch.uint8)
        assert ops.image_crop_resize_u8(plan.records, plan.tables, plan.tmp, 33, plan.max_nrows, out_u8=u8) is u8
        got.append(u8.cpu().numpy())
    assert np.array_equal(got[0], got[1]) and np.array_equal(plan.crop_resize().cpu().numpy(), got[0])
    for i, (im, d) in enumerate(zip(srcs, draws)):
        assert np.array_equal(got[0][i], expected_u8(im, dict(d, ops=[]), 33)), (i, d["box"], d["flip"])


# ------------------------------------------------------------------------------------------------ 3. independence
def test_a_sample_does_not_depend_on_its_place_in_the_batch():
    a, b, c = A.source(45, 37, "random", seed=7), A.source(50, 61, "random", seed=8), A.source(33, 90, "binary", seed=9)
    d = dict(JITTER, box=(3, 4, 30, 22), flip=True, ops=[(13, False, 9), (5, True, 9)])
    others = [dict(JITTER, box=(0, 0, 33, 50), flip=False, ops=[(8, False, 30)], order=(0, 1, 2, 3)),
              dict(JITTER, box=(5, 5, 20, 20), flip=True, ops=[(2, True, 30), (12, False, 9)], contrast=None)]
    alone_f, alone_u8 = run([a], [d], 32)
    mid_f, mid_u8 = run([b, c, a, c, b], [others[0], others[1], d, others[0], others[1]], 32)
    last_f, last_u8 = run([c, a], [others[1], d], 32)
    for f, u8, k in ((mid_f, mid_u8, 2), (last_f, last_u8, 1)):
        assert np.array_equal(u8[k], alone_u8[0])
        assert torch.equal(f[k].view(torch.int32), alone_f[0].view(torch.int32))


# ------------------------------------------------------------------------------------------------ 4. the float tail
def tail_draws(H, W):
    draws = [dict(box=(0, 0, H, W), flip=False, ops=[], order=order, brightness=0.6 + 0.03 * k, contrast=1.4 - 0.03 * k,
                  saturation=0.65 + 0.03 * k, hue=-0.4 + 0.033 * k) for k, order in enumerate(itertools.permutations(range(4)))]
    for off in (("brightness",), ("contrast",), ("saturation",), ("hue",), ("brightness", "contrast", "saturation", "hue"),
                ("contrast", "hue")):
        draws.append(dict(draws[7], **{name: None for name in off}))
    return draws


def tail_errors(out, u8, draws):
    """-> (e32, err): the float32 restatement's and the kernel's largest distance from the float64 restatement"""
    e32 = err = 0.0
    for i, d in enumerate(draws):
        ref64 = A.float_tail(u8[i], d, dtype=torch.float64)
        e32 = max(e32, float((A.float_tail(u8[i], d, dtype=torch.float32).double() - ref64).abs().max()))
        err = max(err, float((out[i].double() - ref64).abs().max()))
    return e32, err


@pytest.mark.parametrize("S,H,W", [(32, 45, 37), (224, 480, 640)])
def test_float_tail_every_order_and_disabled_terms_vs_float64(S, H, W):
    """Bound 4 e32 per size.  Measured on an MI355X: S = 32: e32 2.36e-06, kernel 1.83e-06; S = 224: e32 1.87e-06, kernel 1.87e-06."""
    img = A.source(H, W, "random", seed=10)
    draws = tail_draws(H, W)
    assert len(draws) == 30 and len({d["order"] for d in draws}) == 24
    out, u8 = run([img] * len(draws), draws, S)
    for i, d in enumerate(draws[:3]):
        assert np.array_equal(u8[i], expected_u8(img, d, S))
    e32, err = tail_errors(out, u8, draws)
    bound = 4 * e32
    print(f"float tail S={S}: e32 {e32:.3e}, kernel vs float64 {err:.3e}, bound {bound:.3e}")
    assert e32 > 0 and err <= bound
    # the check sees one 8 x 8 block scaled by 1 + 3 bound
    spoiled = out.clone()
    block = spoiled[11, 1, :8, :8]
    assert float(block.abs().max()) > 1.0
    block *= 1 + 3 * bound
    assert tail_errors(spoiled, u8, draws)[1] > bound


# ------------------------------------------------------------------------------------------------ 5. the processor
def test_processor_batch_equals_single_calls_and_the_pillow_pipeline(tmp_path):
    from open_clip.modal_eeg.processors.eeg_processor import Image_Processor_Train as FromEEG
    from open_clip.modal_tactile.processors.tact_processor import Image_Processor_Train
    assert FromEEG is Image_Processor_Train
    p = Image_Processor_Train(size=32)
    images = [A.source(45, 37, "random", seed=11), A.source(61, 50, "random", seed=12), A.source(9, 200, "random", seed=13)]
    torch.manual_seed(21)
    batch, batch_u8 = p.batch(images, want_u8=True)
    assert tuple(batch.shape) == (3, 3, 32, 32) and batch.dtype == torch.float32 and batch.is_cuda
    torch.manual_seed(21)
    singles = [p(im, want_u8=True) for im in images]
    torch.manual_seed(21)
    draws = [p.draw(im.shape[0], im.shape[1]) for im in images]
    for i, (f, u8) in enumerate(singles):
        assert tuple(f.shape) == (3, 32, 32)
        assert torch.equal(f.view(torch.int32), batch[i].view(torch.int32)) and torch.equal(u8, batch_u8[i])
        assert np.array_equal(u8.cpu().numpy(), expected_u8(images[i], draws[i], 32))
    assert torch.equal(p.batch(images, draws=draws).view(torch.int32), batch.view(torch.int32))
    if HAVE_PIL:                                     # a path, a PIL image and an array are the same source
        from PIL import Image
        path = tmp_path / "a.png"
        Image.fromarray(images[0]).save(path)
        outs = []
        for src in (str(path), Image.fromarray(images[0]), images[0]):
            torch.manual_seed(5)
            outs.append(p(src))
        assert torch.equal(outs[0], outs[1]) and torch.equal(outs[1], outs[2]) and tuple(outs[0].shape) == (3, 32, 32)
