"""CPU: the plain-image training transform (Image_Processor_Train, vl_image_augment).  Pillow is the oracle.

1. The restatement of each of the 14 RandAugment ops (tests/image_augment_ref.py, what the kernels compute) against the Pillow
   call at byte equality: bins 0, 9, 30, both signs, both shear conventions, four sizes, three kinds of content.
2. `pil_bilinear_tables`, applied with the kernels' integer arithmetic, against img.crop(box).resize((S, S), BILINEAR).
3. The magnitude table against the reference's RandAugment3d._augmentation_space, recorded through golden_util.reference_run.
4. The processor's draws: order, ranges, reproducibility, num_ops = 0, the crop fallback.
5. The 368-byte record, the refusals of ops.image_augment_pack, and the C ABI: declaration = binding, version 610
   everywhere, the entries' refusals (which launch nothing, so they run here too)."""
import ctypes
import os
import re
import struct

import numpy as np
import pytest
import torch
from PIL import Image

import image_augment_ref as A
from golden_util import reference_run
from open_clip.modal_eeg.processors.eeg_processor import EEG_Processor, EEGProcessorEval, Image_Processor_Train

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ 1. each op against Pillow
@pytest.mark.parametrize("kind", ["random", "constant", "binary"])
@pytest.mark.parametrize("H,W", [(32, 32), (33, 33), (1, 1), (7, 45)])
def test_each_op_equals_the_pillow_call(H, W, kind):
    img = A.source(H, W, kind, seed=H + W)
    table = A.magnitude_table(31, W)
    n = 0
    for op in range(14):
        for mag_bin in (0, 9, 30):
            for negative in (False, True):
                for shear_atan in ((False, True) if op in (1, 2) else (False,)):
                    mag = A.op_magnitude(table, op, negative, mag_bin)
                    want, got = A.pillow_op(img, op, mag, shear_atan), A.apply_op(img, op, mag, shear_atan)
                    assert got.dtype == np.uint8 and np.array_equal(got, want), (A.OPS[op], mag_bin, negative, shear_atan)
                    n += 1
    assert n == 14 * 6 + 2 * 6


def test_the_identities_of_the_lut_and_contrast_ops_are_hit():
    const = A.source(32, 32, "constant")
    for h in A.histograms(const):
        assert np.count_nonzero(h) == 1                                         # hi <= lo; at most one occupied bin
        assert np.array_equal(A.autocontrast_lut(h), np.arange(256)) and np.array_equal(A.equalize_lut(h), np.arange(256))
    for op in (12, 13):
        assert np.array_equal(A.pillow_op(const, op, 0.0), const)
    # step == 0: fewer than 255 pixels beside the last occupied bin
    small = A.source(7, 30, "random", seed=3)
    h = A.histograms(small)[0]
    assert np.count_nonzero(h) > 1 and (int(h.sum()) - int(h[np.nonzero(h)[0][-1]])) // 255 == 0
    assert np.array_equal(A.equalize_lut(h), np.arange(256)) and np.array_equal(A.pillow_op(small, 13, 0.0), small)
    # step == 1 on 7 x 45 pixels: the running sum over step passes 255 and Pillow clips it
    h = A.histograms(A.source(7, 45, "random", seed=52))[0]
    assert (int(h.sum()) - int(h[np.nonzero(h)[0][-1]])) // 255 == 1
    # Contrast on a flat image: the degenerate image is the image's own L value
    flat = np.full((32, 32, 3), 77, np.uint8)
    assert A.contrast_mean(flat) == 77
    for f in (-0.9, 0.9):
        assert np.array_equal(A.pillow_op(flat, 8, f), flat) and np.array_equal(A.apply_op(flat, 8, f), flat)


def test_rotate_at_bin_0_is_pillows_copy_and_an_identity_slot():
    from vitlens_hip import ops, preproc
    assert A.rotate_matrix(0.0, 32, 32) is None and A.rotate_matrix(-0.0, 32, 32) is None and A.rotate_matrix(360.0, 32, 32) is None
    slot = np.zeros(1, ops.IMAGE_OP_DTYPE)[0]
    preproc.randaugment_slot(slot, 5, -0.0, 32)
    assert int(slot["code"]) == 0
    preproc.randaugment_slot(slot, 5, 9.0, 32)
    assert int(slot["code"]) == 5 and list(slot["m"]) == A.rotate_matrix(9.0, 32, 32)


def test_host_matrices_and_payloads_equal_the_restatement():
    from vitlens_hip import ops, preproc
    for S in (32, 33, 224):
        table = A.magnitude_table(31, S)
        for op in range(14):
            for mag_bin, negative, shear_atan in ((0, True, False), (9, False, True), (30, True, False), (30, False, True)):
                mag = A.op_magnitude(table, op, negative, mag_bin)
                slot = np.zeros(1, ops.IMAGE_OP_DTYPE)[0]
                preproc.randaugment_slot(slot, op, mag, S, shear_atan)
                if op in A.GEOMETRIC:
                    m = A.op_matrix(op, mag, (S, S), shear_atan)
                    assert (int(slot["code"]) == 0) if m is None else (list(slot["m"]) == m)
                elif op in A.ENHANCE:
                    assert float(slot["fpay"]) == float(np.float32(1.0 + mag))
                elif op == 10:
                    assert int(slot["ipay"]) == (~(2 ** (8 - int(mag)) - 1) & 0xFF)
                elif op == 11:
                    assert int(slot["ipay"]) == A.solarize_threshold(mag)


# ------------------------------------------------------------------------------------------------ 2. the bilinear tables
@pytest.mark.parametrize("H,W,S,box", [
    (45, 37, 32, (0, 0, 45, 37)), (45, 37, 33, (0, 0, 45, 37)), (480, 640, 224, (0, 0, 480, 640)), (480, 640, 224, (57, 101, 301, 400)),
    (1, 1, 32, (0, 0, 1, 1)), (200, 220, 32, (2, 3, 192, 192)), (45, 37, 32, (0, 0, 10, 37)), (45, 37, 33, (35, 0, 10, 37)),
    (45, 37, 32, (0, 0, 45, 5)), (45, 37, 33, (0, 32, 45, 5)), (45, 37, 32, (44, 36, 1, 1)), (45, 37, 32, (5, 3, 32, 32))])
def test_bilinear_tables_equal_pillow_crop_resize(H, W, S, box):
    from vitlens_hip.preproc import pil_bilinear_tables
    img = A.source(H, W, "random", seed=H * W + S)
    for in_size in (box[2], box[3]):
        b, kk, ks = pil_bilinear_tables(in_size, S)
        assert b.dtype == np.int32 and kk.dtype == np.int32 and b.shape == (S, 2) and kk.shape == (S, ks)
        assert np.all(b[:, 0] >= 0) and np.all(b[:, 1] >= 1) and np.all(b[:, 0] + b[:, 1] <= in_size) and np.all(b[:, 1] <= ks)
    assert np.array_equal(A.crop_resize(img, box, S, pil_bilinear_tables), A.pillow_crop_resize(img, box, S))


# ------------------------------------------------------------------------------------------------ 3. the magnitude table
# Run where the reference is importable; transforms_rgbd.py needs torchvision only for names (oracle/ref_loader.py's shells).
_REF = r'''
import importlib.util, json, os, sys
import torch
sys.path.insert(0, sys.argv[1])
import ref_loader
ref_loader.install_shells()
import torchvision.transforms as T
if not hasattr(T.functional, "InterpolationMode"):
    T.functional.InterpolationMode = T.InterpolationMode
d = os.path.join(ref_loader.REF_SRC, "open_clip", "modal_depth", "processors")
spec = importlib.util.spec_from_file_location("ref_transforms_rgbd", os.path.join(d, "transforms_rgbd.py"))
m = importlib.util.module_from_spec(spec); spec.loader.exec_module(m)
out = {}
for S in (224, 32, 33):
    space = m.RandAugment3d(num_ops=2, magnitude=9, interpolation=2)._augmentation_space(31, (S, S))
    out[str(S)] = [[name, [float(v) for v in mags.reshape(-1)], bool(signed)] for name, (mags, signed) in space.items()]
print("JSON" + json.dumps(out))
'''


def test_magnitude_table_equals_the_references():
    from vitlens_hip import ops, preproc
    ref = reference_run("test_image_augment_host.randaugment_space", _REF, [os.path.join(ROOT, "oracle")])
    for S in (224, 32, 33):
        rows = ref[str(S)]
        assert tuple(r[0] for r in rows) == ops.IMAGE_OPS == A.OPS
        assert tuple(r[2] for r in rows) == preproc.RANDAUGMENT_SIGNED == A.SIGNED
        table, restated = preproc.randaugment_magnitudes(31, S), A.magnitude_table(31, S)
        for code, (name, mags, _) in enumerate(rows):
            want = mags * 31 if len(mags) == 1 else mags                        # the ops without a magnitude hold one 0.0
            assert list(table[code]) == want == restated[name], (S, name)
    assert preproc.randaugment_magnitudes(31, 224, 255.0)[11][0] == 255.0 and preproc.randaugment_magnitudes(31, 224)[11][0] == 256.0


# ------------------------------------------------------------------------------------------------ 4. the draws
def test_draw_order_is_the_pipelines():
    p = Image_Processor_Train(device="cpu")
    signed_seen = set()
    for seed in range(40):
        torch.manual_seed(seed)
        got = p.draw(480, 640)
        tail = float(torch.rand(1))
        # by hand: box, flip, per op the index and the sign only for a signed op, permutation, three factors, the hue
        torch.manual_seed(seed)
        box = A.R.crop_box(480, 640)
        flip = bool(torch.rand(1) < 0.5)
        chosen = []
        for _ in range(2):
            op = int(torch.randint(14, (1,)))
            negative = bool(torch.randint(2, (1,))) if 1 <= op <= 9 else False
            chosen.append((op, negative, 9))
            signed_seen.add(1 <= op <= 9)
        order = tuple(torch.randperm(4).tolist())
        b, c, s = (float(torch.empty(1).uniform_(0.6, 1.4)) for _ in range(3))
        h = float(torch.empty(1).uniform_(-0.4, 0.4))
        assert got == dict(box=box, flip=flip, ops=chosen, order=order, brightness=b, contrast=c, saturation=s, hue=h)
        assert float(torch.rand(1)) == tail
        torch.manual_seed(seed)
        assert A.draw(480, 640) == got
    assert signed_seen == {True, False}


def test_draw_ranges_and_reproducibility():
    p = Image_Processor_Train(args={"num_ops": 3, "magnitude": 30}, device="cpu", size=32)
    torch.manual_seed(3)
    a = [p.draw(61, 45) for _ in range(400)]
    torch.manual_seed(3)
    b = [p.draw(61, 45) for _ in range(400)]
    torch.manual_seed(4)
    c = [p.draw(61, 45) for _ in range(400)]
    assert a == b and a != c
    for d in a:
        top, left, h, w = d["box"]
        assert 0 <= top and 1 <= h and top + h <= 61 and 0 <= left and 1 <= w and left + w <= 45
        assert sorted(d["order"]) == [0, 1, 2, 3] and len(d["ops"]) == 3
        assert all(0 <= op < 14 and mag_bin == 30 and (not negative or A.SIGNED[op]) for op, negative, mag_bin in d["ops"])
        assert all(0.6 <= d[k] <= 1.4 for k in ("brightness", "contrast", "saturation")) and -0.4 <= d["hue"] <= 0.4
    assert 0.4 < np.mean([d["flip"] for d in a]) < 0.6
    assert {op for d in a for op, _, _ in d["ops"]} == set(range(14)) and len({d["order"] for d in a}) == 24
    assert 0.4 < np.mean([neg for d in a for op, neg, _ in d["ops"] if A.SIGNED[op]]) < 0.6


def test_num_ops_0_draws_nothing_for_randaugment():
    p = Image_Processor_Train(update_conf={"num_ops": 0}, device="cpu")
    torch.manual_seed(9)
    got = p.draw(61, 45)
    torch.manual_seed(9)
    box = A.R.crop_box(61, 45)
    flip = bool(torch.rand(1) < 0.5)
    order = tuple(torch.randperm(4).tolist())
    assert got["ops"] == [] and (got["box"], got["flip"], got["order"]) == (box, flip, order)


def test_a_9_by_200_source_takes_the_crop_fallback():
    # area 1800 * 0.08 = 144 at least, over an aspect of at most 4/3: h^2 >= 108 > 81, so no attempt fits 9 rows
    p = Image_Processor_Train(device="cpu")
    for seed in range(10):
        torch.manual_seed(seed)
        assert p.draw(9, 200)["box"] == (0, 94, 9, 12)


def test_constructor_from_config_and_eeg_processor():
    p = Image_Processor_Train.from_config()
    assert (p.num_ops, p.magnitude, p.size) == (2, 9, 224) and p.mean == list(A.CLIP_MEAN) and p.std == list(A.CLIP_STD)
    assert p.shear_atan is False and p.solarize_from == 256.0
    cfg = {"params": {"num_ops": 1, "magnitude": 5}, "update_conf": {"magnitude": 7}, "img_mean": (0.5, 0.5, 0.5)}
    q = Image_Processor_Train.from_config(cfg)
    assert (q.num_ops, q.magnitude, q.mean) == (1, 7, [0.5, 0.5, 0.5]) and "update_conf" in cfg

    class Args:
        num_ops, magnitude = 4, 30
    assert (Image_Processor_Train(Args(), device="cpu").num_ops, Image_Processor_Train(Args(), device="cpu").magnitude) == (4, 30)
    assert repr(p).startswith("(DataAugmentationForRGBD,\ntransform = ") and "RandAugment(num_ops=2, magnitude=9" in repr(p)
    for bad in ({"num_ops": 5}, {"num_ops": -1}, {"magnitude": 31}):
        with pytest.raises(ValueError):
            Image_Processor_Train(update_conf=bad, device="cpu")
    eeg = torch.from_numpy(np.random.default_rng(0).standard_normal((8, 500)).astype(np.float32))
    assert torch.equal(EEG_Processor()(eeg), EEGProcessorEval()(eeg)) and tuple(EEG_Processor()(eeg).shape) == (8, 512)
    e = EEG_Processor.from_config({"params": {"time_low": 10, "time_high": 300, "data_len": 64}, "update_conf": {"data_len": 9}})
    assert (e.time_low, e.time_high, e.data_len) == (10, 300, 64)                # the reference reads args before the update
    assert torch.equal(e(eeg), EEGProcessorEval(10, 300, 64)(eeg))


# ------------------------------------------------------------------------------------------------ 5. the record and the ABI
FIELDS = {"src": 0, "stride": 8, "H": 12, "W": 16, "top": 20, "left": 24, "bh": 28, "bw": 32, "row0": 36, "nrows": 40, "hb": 44,
          "hk": 48, "hks": 52, "vb": 56, "vk": 60, "vks": 64, "flags": 68, "tmp": 72, "b": 80, "b1": 84, "c": 88, "c1": 92, "s": 96,
          "s1": 100, "hue": 104, "num_ops": 108, "ops": 112}
OP_FIELDS = {"code": 0, "ipay": 4, "fpay": 8, "pad": 12, "m": 16}


SIZES = (32, 384, 0x0102030405 + 20 * 32 * 3)                                # S, words of tables, bytes of intermediate: just enough


def _row():
    from vitlens_hip import ops, preproc
    rec = np.zeros(1, dtype=ops.IMAGE_AUGMENT_DTYPE)
    r = rec[0]
    r["src"], r["stride"], r["H"], r["W"] = 0x1122334455667788, 135, 61, 45
    r["row0"], r["nrows"], r["hks"], r["vks"], r["tmp"] = 1, 20, 3, 5, 0x0102030405
    r["hb"], r["hk"], r["vb"], r["vk"] = 0, 64, 160, 224                       # [32,2] + [32,3] + [32,2] + [32,5] words
    preproc.image_record_scalars(r, dict(box=(3, 4, 30, 22), flip=True, ops=[(7, True, 30), (10, False, 30), (5, False, 9), (11, False, 9)],
                                         order=(3, 1, 0, 2), brightness=0.7, contrast=None, saturation=1.3, hue=-0.25), 32)
    return rec


def test_record_layout():
    from vitlens_hip import ops
    dt, odt = ops.IMAGE_AUGMENT_DTYPE, ops.IMAGE_OP_DTYPE
    assert dt.itemsize == 368 and {n: dt.fields[n][1] for n in dt.names} == FIELDS
    assert odt.itemsize == 64 and {n: odt.fields[n][1] for n in odt.names} == OP_FIELDS
    words = ops.image_augment_pack(_row(), *SIZES)
    assert words.dtype == np.int32 and words.shape == (1, 92)
    raw = words.tobytes()
    assert struct.unpack_from("<Q", raw, 0) == (0x1122334455667788,)
    assert struct.unpack_from("<15i", raw, 8) == (135, 61, 45, 3, 4, 30, 22, 1, 20, 0, 64, 3, 160, 224, 5)
    assert struct.unpack_from("<q", raw, 72) == (0x0102030405,)
    # flags: flip 1 | brightness 2 | saturation 8 | hue 16; order hue, contrast, brightness, saturation
    assert struct.unpack_from("<i", raw, 68) == (1 | 2 | 8 | 16 | ((3 | 1 << 2 | 0 << 4 | 2 << 6) << 8),)
    f = struct.unpack_from("<7f", raw, 80)
    assert f == (float(np.float32(0.7)), float(np.float32(1.0 - 0.7)), 0.0, 0.0, float(np.float32(1.3)), float(np.float32(1.0 - 1.3)), -0.25)
    assert struct.unpack_from("<i", raw, 108) == (4,)
    m9 = A.magnitude_table(31, 32)
    assert struct.unpack_from("<iif", raw, 112) == (7, 0, float(np.float32(1.0 - m9["Color"][30])))
    assert struct.unpack_from("<ii", raw, 112 + 64) == (10, 0xF0)
    assert struct.unpack_from("<i", raw, 112 + 128) == (5,)
    assert list(struct.unpack_from("<6d", raw, 112 + 128 + 16)) == A.rotate_matrix(m9["Rotate"][9], 32, 32)
    assert struct.unpack_from("<ii", raw, 112 + 192) == (11, A.solarize_threshold(m9["Solarize"][9]))
    src = open(os.path.join(ROOT, "vit-lens_amd", "csrc", "vl_image_augment.hip")).read()
    assert "static_assert(sizeof(ImageOp) == 64 && sizeof(ImageAugRec) == 368" in src


def _set(rec, field, value):
    if isinstance(field, tuple):
        slot, name = field
        if name == "m":
            rec[0]["ops"][slot]["m"][2] = value
        else:
            rec[0]["ops"][slot][name] = value
    else:
        rec[0][field] = value


@pytest.mark.parametrize("field,value,text", [
    ("src", 0, "null source"), ("stride", 134, "stride"), ("top", 32, "inside the image"), ("bw", 42, "inside the image"),
    ("bh", 0, "inside the image"), ("nrows", 30, "inside the box"), ("hks", 0, "offset"), ("tmp", -1, "offset"),
    ("tmp", 0x0102030406, "offset"), ("hb", 321, "offset"), ("hk", 289, "offset"), ("vb", 1 << 30, "offset"), ("vk", 225, "offset"),
    ("vks", 6, "offset"),
    ("flags", 1 << 8, "order"), ("flags", (0xE4 << 8) | (1 << 16), "unknown flag"), ("flags", (0xE4 << 8) | 32, "unknown flag"),
    ("b", float("nan"), "not finite"), ("num_ops", 5, "num_ops"), ("num_ops", -1, "num_ops"), ((0, "code"), 14, "op code"),
    ((1, "code"), -1, "op code"), ((2, "m"), float("inf"), "matrix"), ((2, "m"), float("nan"), "matrix"),
    ((0, "fpay"), float("nan"), "factor"), ((1, "ipay"), 256, "Posterize"), ((3, "ipay"), 257, "Solarize")])
def test_pack_refuses_a_bad_record(field, value, text):
    from vitlens_hip import ops
    rec = _row()
    ops.image_augment_pack(rec, *SIZES)
    _set(rec, field, value)
    with pytest.raises(ValueError, match=text):
        ops.image_augment_pack(rec, *SIZES)


def test_pack_ignores_unused_slots_and_plan_refuses_a_bad_draw():
    from vitlens_hip import ops, preproc
    rec = _row()
    rec[0]["num_ops"] = 2
    rec[0]["ops"][3]["code"] = 99                                             # beyond num_ops: never read
    ops.image_augment_pack(rec, *SIZES)
    img = torch.from_numpy(A.source(45, 37))
    d = dict(box=(0, 0, 45, 37), flip=False, ops=[(3, False, 9)], order=(0, 1, 2, 3), brightness=1.0, contrast=1.0, saturation=1.0, hue=0.0)
    for bad, text in ((dict(box=(0, 0, 46, 37)), "not inside"), (dict(ops=[(14, False, 9)]), "out of range"), (dict(ops=[(3, False, 31)]), "out of range"),
                      (dict(ops=[(0, False, 0)] * 5), "at most 4"), (dict(order=(0, 1, 2, 2)), "permutation")):
        with pytest.raises(ValueError, match=text):
            preproc.plan_image_train([img], [dict(d, **bad)], 32, A.CLIP_MEAN, A.CLIP_STD, device="cpu")


def _header():
    src = open(os.path.join(ROOT, "include", "vitlens_hip.h")).read()
    return src, re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def test_entries_are_declared_exported_and_bound_under_610():
    from vitlens_hip import _lib
    raw, hdr = _header()
    P, I, Fl = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    ctype = {"int": I, "float": Fl, "hipStream_t": P}
    for name, sig in (("vl_image_crop_resize_u8", [P, I, I, I, P, P, P, P]), ("vl_image_augment", [P, I, I, I, I, P, P, P, P, P, P, P, P])):
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, hdr)
        assert m, name
        want = [P if "*" in prm else ctype[prm.replace("const ", "").split()[0]] for prm in (q.strip() for q in m.group(1).split(","))]
        assert _lib.SIGNATURES[name] == want == sig
        assert hasattr(ctypes.CDLL(_lib.lib_path()), name)
    version = int(re.search(r"#define\s+VL_ABI_VERSION\s+(\d+)", hdr).group(1))
    assert version == 610 == _lib.ABI_VERSION == int(_lib.load_library().vl_version())
    # the layout is spelled out next to the declarations, and the NOTE on the version covers the entries
    doc = raw[:raw.index("int vl_image_crop_resize_u8(")].rsplit("/*", 1)[1]
    for word in ("368-byte", "uint64 src", "int32 stride", "int32 top, left, bh, bw", "int32 hb, hk, hks", "int64 tmp", "int32 flags",
                 "float b, 1-b, c, 1-c, s, 1-s", "float hue", "int32 num_ops", "int32 code", "int32 ipay", "float fpay", "double m[6]",
                 "NOTE on the version", "610"):
        assert word in doc, word


REFUSALS = (
    (dict(n=0), "bad shape"), (dict(n=-3), "bad shape"), (dict(n=70000), "bad shape"), (dict(S=0), "bad shape"), (dict(S=4097), "bad shape"),
    (dict(max_nrows=0), "bad shape"), (dict(max_ops=5), "num_ops"), (dict(max_ops=-1), "num_ops"), (dict(records=None), "null operand"),
    (dict(tables=None), "null operand"), (dict(tmp=None), "null operand"), (dict(work=None), "null operand"), (dict(mean=None), "null operand"),
    (dict(std=None), "null operand"), (dict(out=None), "null operand"), (dict(records=0x1004), "aligned"), (dict(std=(1.0, 0.0, 1.0)), "non-zero"),
)


@pytest.mark.parametrize("case,text", REFUSALS)
def test_entry_refuses_without_launching(case, text):
    """One operand made bad; the device pointers are non-null and never dereferenced by a refusal."""
    from vitlens_hip import _lib
    lib = _lib.load_library()
    a = dict(records=0x1000, n=2, S=32, max_nrows=8, max_ops=2, tables=0x2000, tmp=0x3000, work=0x6000, mean=(0.5, 0.5, 0.5),
             std=(0.25, 0.25, 0.25), out=0x4000, out_u8=0x5000)
    a.update(case)
    fl = lambda v: None if v is None else (ctypes.c_float * 3)(*v)
    assert lib.vl_image_augment(a["records"], a["n"], a["S"], a["max_nrows"], a["max_ops"], a["tables"], a["tmp"], a["work"], fl(a["mean"]),
                                fl(a["std"]), a["out"], a["out_u8"], None) != 0
    assert text in lib.vl_last_error().decode() and "vl_image_augment" in lib.vl_last_error().decode()


@pytest.mark.parametrize("case,text", [(dict(n=0), "bad shape"), (dict(S=-1), "bad shape"), (dict(max_nrows=0), "bad shape"),
                                       (dict(records=None), "null operand"), (dict(tables=None), "null operand"), (dict(tmp=None), "null operand"),
                                       (dict(out_u8=None), "null operand"), (dict(records=0x1004), "aligned")])
def test_crop_resize_entry_refuses_without_launching(case, text):
    from vitlens_hip import _lib
    lib = _lib.load_library()
    a = dict(records=0x1000, n=2, S=32, max_nrows=8, tables=0x2000, tmp=0x3000, out_u8=0x5000)
    a.update(case)
    assert lib.vl_image_crop_resize_u8(a["records"], a["n"], a["S"], a["max_nrows"], a["tables"], a["tmp"], a["out_u8"], None) != 0
    assert text in lib.vl_last_error().decode() and "vl_image_crop_resize_u8" in lib.vl_last_error().decode()
