"""CPU: the tactile recipe's training transform (Tactile_Processor_Train, vl_tactile_augment).

1. The rotation: the float32 statement the kernel implements (tactile_augment_ref.index_map) against torchvision's tensor path
   restated with torch's own linspace, bmm and grid_sample (tv_rotate).  The two may differ only where the source coordinate
   lies within 2^-12 of a half-integer (`ambiguous`), and for the angles listed such pixels are at most 0.5 % of the image;
   45, 30 and 60 degrees are left out on purpose (their diagonal ties make 3-6 % of the pixels ambiguous at S = 32 / 33).
   Quarter turns equal torch.rot90 exactly.
2. The processor's draws: order, generator position, the crop fallback.
3. The 96-byte record and the checks of tactile_augment_pack.
4. The C ABI: declaration = binding, version 610 everywhere, the refusals (which launch nothing, so they run here too)."""
import ctypes
import os
import re
import struct

import numpy as np
import pytest
import torch

import tactile_augment_ref as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (32, 33, 224)
ANGLES = (0.0, 90.0, 180.0, 270.0, 360.0, 0.001, 359.999, 17.0, 123.456, 200.25, 333.3)


# ------------------------------------------------------------------------------------------------ 1. the rotation
@pytest.mark.parametrize("S", SIZES)
def test_index_map_equals_grid_sample_away_from_ties(S):
    for angle in ANGLES:
        mine, tv, amb = T.index_map(S, angle), T.tv_index(S, angle).numpy(), T.ambiguous(S, angle)
        differ = mine != tv
        print(f"S = {S} angle {angle}: {int(differ.sum())} pixels differ, {100.0 * amb.mean():.3f} % ambiguous, "
              f"{int((mine < 0).sum())} fill")
        assert amb.mean() <= 0.005, (S, angle, amb.mean())
        assert not np.any(differ & ~amb), (S, angle, np.argwhere(differ & ~amb)[:5])


@pytest.mark.parametrize("S", SIZES)
def test_whole_and_quarter_turns_are_exact_permutations(S):
    identity = np.arange(S * S, dtype=np.int64).reshape(S, S)
    for angle in (0.0, 360.0):
        assert np.array_equal(T.index_map(S, angle), identity)
    img = torch.from_numpy(identity)[None]
    for angle in (90.0, 180.0, 270.0):
        want = torch.rot90(img, int(angle // 90) % 4, (-2, -1))[0].numpy()
        assert np.array_equal(T.index_map(S, angle), want), angle
        assert np.array_equal(T.tv_index(S, angle).numpy(), want), angle


def test_tv_rotate_fills_and_gathers():
    img = torch.rand(3, 33, 33, generator=torch.Generator().manual_seed(0)) + 1.0     # no pixel is 0: a 0 is a fill
    out = T.tv_rotate(img, 30.0)
    idx = T.tv_index(33, 30.0)
    assert torch.equal(out, T.gather(img, idx)) and bool((idx < 0).any()) and torch.equal(out[0] == 0, idx < 0)
    assert int((idx < 0).sum()) > 0.1 * 33 * 33                                        # the four corners


def test_record_scalars_are_the_rescaled_theta():
    from vitlens_hip import ops, preproc
    for S in SIZES:
        for angle in ANGLES + (45.0,):
            rec = np.zeros(1, dtype=ops.TACTILE_AUGMENT_DTYPE)
            preproc.tactile_record_scalars(rec[0], dict(box=(0, 0, 1, 1), flip_h=False, flip_v=True, angle=angle), S)
            theta = torch.tensor(T.inverse_matrix(angle), dtype=torch.float32).reshape(1, 2, 3)
            want = (theta.transpose(1, 2) / torch.tensor([0.5 * S, 0.5 * S]))[0]      # [3, 2]: column 0 feeds x, column 1 y
            got = [float(rec[0][k]) for k in ("t00", "t01", "t10", "t11")]
            assert got == [float(want[0, 0]), float(want[1, 0]), float(want[0, 1]), float(want[1, 1])]
            assert float(want[2, 0]) == 0.0 and float(want[2, 1]) == 0.0
            assert int(rec[0]["flags"]) == 2


# ------------------------------------------------------------------------------------------------ 2. the draws
def _proc(**kw):
    from open_clip.modal_tactile.processors.tact_processor import Tactile_Processor_Train
    return Tactile_Processor_Train(device="cpu", **kw)


def test_draw_order_is_the_pipelines():
    p = _proc()
    for seed in range(10):
        torch.manual_seed(seed)
        got = [p.draw(480, 640), p.draw(37, 53)]
        tail = float(torch.rand(1))
        torch.manual_seed(seed)
        want = [T.draw(480, 640), T.draw(37, 53)]
        assert got == want and float(torch.rand(1)) == tail
        assert all(0.0 <= d["angle"] <= 360.0 for d in got)
        # by hand: box, horizontal flip, vertical flip, angle
        torch.manual_seed(seed)
        box = T.crop_box(480, 640)
        fh, fv = bool(torch.rand(1) < 0.5), bool(torch.rand(1) < 0.5)
        angle = float(torch.empty(1).uniform_(0.0, 360.0))
        assert got[0] == {"box": box, "flip_h": fh, "flip_v": fv, "angle": angle}


def test_a_9_by_200_source_takes_the_crop_fallback():
    # area 1800 * 0.08 = 144 at least, over an aspect of at most 4/3: h^2 >= 108 > 81, so no attempt fits 9 rows
    p = _proc()
    for seed in range(10):
        torch.manual_seed(seed)
        got = p.draw(9, 200)
        assert got["box"] == (0, 94, 9, 12)
        torch.manual_seed(seed)
        assert T.draw(9, 200) == got
        torch.manual_seed(seed)
        for _ in range(20):                          # ten failed attempts: twenty uniforms and no randint
            torch.empty(1).uniform_(0, 1)
        assert got["flip_h"] == bool(torch.rand(1) < 0.5)


def test_constructor_from_config_and_repr():
    from open_clip.modal_tactile.processors.tact_processor import (OPENAI_CLIP_MEAN, OPENAI_CLIP_STD, Tactile_Processor_Eval,
                                                                   Tactile_Processor_Train, TactileRGBProcessorEval)
    p = Tactile_Processor_Train.from_config()
    assert p.mean == list(OPENAI_CLIP_MEAN) and p.std == list(OPENAI_CLIP_STD) and p.size == 224 and p.antialias is True
    assert p.degrees == (0.0, 360.0)
    cfg = {"img_mean": (0.5, 0.5, 0.5), "update_conf": {"k": 1}}
    q = Tactile_Processor_Train.from_config(cfg)
    assert q.mean == [0.5, 0.5, 0.5] and q.conf == {"k": 1} and "update_conf" in cfg     # the caller's mapping is left alone
    text = repr(_proc(size=32))
    assert text.startswith("(DataAugmentationForRGBD,\ntransform = ") and "RandomVerticalFlip" in text and "RandomRotation" in text
    with pytest.raises(ValueError, match="degrees"):
        _proc(degrees=(10.0, 0.0))
    e = Tactile_Processor_Eval.from_config({"img_std": (0.25, 0.25, 0.25)})
    assert isinstance(e, TactileRGBProcessorEval) and e.std == (0.25, 0.25, 0.25) and (e.resize, e.size) == (256, 224)
    assert Tactile_Processor_Eval({}, None, None, {"k": 2}, device="cpu").conf == {"k": 2}


# ------------------------------------------------------------------------------------------------ 3. the record
FIELDS = {"src": 0, "stride": 8, "H": 12, "W": 16, "top": 20, "left": 24, "bh": 28, "bw": 32, "row0": 36, "nrows": 40, "hb": 44, "hw": 48,
          "hks": 52, "vb": 56, "vw": 60, "vks": 64, "flags": 68, "tmp": 72, "t00": 80, "t01": 84, "t10": 88, "t11": 92}
BUFFERS = (420, 1000)             # words of tables (bounds 2 * 32 and weights 32 * ks for each axis), float4 of intermediate


def _row():
    from vitlens_hip import ops, preproc
    rec = np.zeros(1, dtype=ops.TACTILE_AUGMENT_DTYPE)
    r = rec[0]
    r["src"], r["stride"], r["H"], r["W"] = 0x1122334455667788, 135, 61, 45
    r["row0"], r["nrows"], r["hb"], r["hw"], r["hks"], r["vb"], r["vw"], r["vks"], r["tmp"] = 1, 20, 0, 64, 3, 160, 224, 5, 100
    preproc.tactile_record_scalars(r, dict(box=(3, 4, 30, 22), flip_h=True, flip_v=True, angle=30.0), 32)
    return rec


def test_record_layout():
    from vitlens_hip import ops
    dt = ops.TACTILE_AUGMENT_DTYPE
    assert dt.itemsize == 96 and {n: dt.fields[n][1] for n in dt.names} == FIELDS
    rec = _row()
    rec[0]["tmp"] = 0x0102030405
    words = ops.tactile_augment_pack(rec, 32, BUFFERS[0], 0x0102030405 + 20 * 32)
    assert words.dtype == np.int32 and words.shape == (1, 24)
    raw = words.tobytes()
    assert struct.unpack_from("<Q", raw, 0) == (0x1122334455667788,)
    assert struct.unpack_from("<16i", raw, 8) == (135, 61, 45, 3, 4, 30, 22, 1, 20, 0, 64, 3, 160, 224, 5, 3)
    assert struct.unpack_from("<q", raw, 72) == (0x0102030405,)
    m = np.array(T.inverse_matrix(30.0)).astype(np.float32)
    assert struct.unpack_from("<4f", raw, 80) == tuple(float(v) for v in m[[0, 1, 3, 4]] / np.float32(16.0))
    src = open(os.path.join(ROOT, "vit-lens_amd", "csrc", "vl_tactile_augment.hip")).read()
    assert "static_assert(sizeof(TactileAugRec) == 96" in src
    # the header's word numbers are these offsets
    hdr = open(os.path.join(ROOT, "include", "vitlens_hip.h")).read()
    doc = hdr[:hdr.index("int vl_tactile_augment(")].rsplit("/*", 1)[1]
    for first, names in ((0, "uint64 src"), (2, "int32 stride"), (3, "int32 H, W"), (5, "int32 top, left, bh, bw"), (9, "int32 row0, nrows"),
                         (11, "int32 hb, hw, hks"), (14, "int32 vb, vw, vks"), (17, "int32 flags"), (18, "int64 tmp"),
                         (20, "float t00, t01, t10, t11")):
        line = next(ln for ln in doc.splitlines() if names in ln)
        assert int(re.search(r"words?\s+(\d+)", line).group(1)) == first, line
        assert FIELDS[names.split()[1].rstrip(",")] == 4 * first, names


@pytest.mark.parametrize("field,value,text", [
    ("src", 0, "null source"), ("stride", 134, "stride"), ("top", 32, "inside the image"), ("bw", 42, "inside the image"),
    ("bh", 0, "inside the image"), ("left", -1, "inside the image"), ("nrows", 30, "inside the box"), ("row0", -1, "inside the box"),
    ("hks", 0, "offset"), ("tmp", -1, "offset"), ("tmp", 361, "offset"), ("hb", 357, "offset"), ("hw", 325, "offset"),
    ("vb", 1 << 30, "offset"), ("vw", 261, "offset"), ("vks", 7, "offset"),
    ("flags", 4, "unknown flag"), ("flags", 1 << 16, "unknown flag"), ("flags", -1, "unknown flag"),
    ("t00", float("nan"), "not finite"), ("t01", float("inf"), "not finite"), ("t10", float("-inf"), "not finite"),
    ("t11", float("nan"), "not finite")])
def test_pack_refuses_a_bad_record(field, value, text):
    from vitlens_hip import ops
    rec = _row()
    ops.tactile_augment_pack(rec, 32, *BUFFERS)
    rec[0][field] = value
    with pytest.raises(ValueError, match=text):
        ops.tactile_augment_pack(rec, 32, *BUFFERS)


def test_pack_accepts_the_last_fitting_offsets_and_plan_refuses_a_bad_draw():
    from vitlens_hip import ops, preproc
    rec = _row()
    for field, value in (("tmp", 360), ("hb", 356), ("hw", 324), ("vw", 260), ("vks", 6)):
        r = rec.copy()
        r[0][field] = value
        ops.tactile_augment_pack(r, 32, *BUFFERS)
    img = T.source(45, 37, 0)
    d = dict(box=(0, 0, 45, 37), flip_h=False, flip_v=False, angle=10.0)
    for bad, text in ((dict(box=(0, 0, 46, 37)), "not inside"), (dict(box=(0, -1, 45, 37)), "not inside"), (dict(angle=float("nan")), "not finite")):
        with pytest.raises(ValueError, match=text):
            preproc.plan_tactile_train([img], [dict(d, **bad)], 32, T.CLIP_MEAN, T.CLIP_STD, device="cpu")
    with pytest.raises(ValueError, match="1 images, 2 draws"):
        preproc.plan_tactile_train([img], [d, d], 32, T.CLIP_MEAN, T.CLIP_STD, device="cpu")
    plan = preproc.plan_tactile_train([img, T.source(9, 200, 1)], [d, dict(d, box=(0, 94, 9, 12))], 32, T.CLIP_MEAN, T.CLIP_STD, device="cpu")
    assert plan.records.shape == (2, 24) and plan.tmp.shape[1] == 4 and plan.max_nrows == 45


# ------------------------------------------------------------------------------------------------ 4. the C ABI
def test_entry_is_declared_exported_and_bound_under_610():
    from vitlens_hip import _lib
    raw = open(os.path.join(ROOT, "include", "vitlens_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    P, I, Fl = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    m = re.search(r"\bint\s+vl_tactile_augment\s*\(([^)]*)\)\s*;", hdr)
    assert m
    ctype = {"int": I, "float": Fl, "hipStream_t": P}
    names = [q.strip().split()[-1].lstrip("*") for q in m.group(1).split(",")]
    assert names == ["records", "n", "S", "max_nrows", "tables", "tmp", "mean", "stdv", "out", "stream"]
    want = [P if "*" in prm else ctype[prm.replace("const ", "").split()[0]] for prm in (q.strip() for q in m.group(1).split(","))]
    assert _lib.SIGNATURES["vl_tactile_augment"] == want == [P, I, I, I, P, P, P, P, P, P]
    assert hasattr(ctypes.CDLL(_lib.lib_path()), "vl_tactile_augment")
    version = int(re.search(r"#define\s+VL_ABI_VERSION\s+(\d+)", hdr).group(1))
    assert version == 610 == _lib.ABI_VERSION == int(_lib.load_library().vl_version())
    doc = raw[:raw.index("int vl_tactile_augment(")].rsplit("/*", 1)[1]
    for word in ("96-byte", "bit 0 horizontal flip, bit 1 vertical flip", "NOTE on the version", "610", "No existing entry changes"):
        assert word in doc, word


REFUSALS = (
    (dict(n=0), "bad shape"), (dict(n=-3), "bad shape"), (dict(n=70000), "bad shape"), (dict(S=0), "bad shape"), (dict(S=-1), "bad shape"),
    (dict(S=4097), "bad shape"), (dict(max_nrows=0), "bad shape"), (dict(records=None), "null operand"), (dict(tables=None), "null operand"),
    (dict(tmp=None), "null operand"), (dict(mean=None), "null operand"), (dict(std=None), "null operand"), (dict(out=None), "null operand"),
    (dict(records=0x1004), "aligned"), (dict(tmp=0x3008), "aligned"), (dict(std=(1.0, 0.0, 1.0)), "non-zero"),
)


@pytest.mark.parametrize("case,text", REFUSALS)
def test_entry_refuses_without_launching(case, text):
    """One operand made bad; the device pointers are non-null and never dereferenced by a refusal."""
    from vitlens_hip import _lib
    lib = _lib.load_library()
    a = dict(records=0x1000, n=2, S=32, max_nrows=8, tables=0x2000, tmp=0x3000, mean=(0.5, 0.5, 0.5), std=(0.25, 0.25, 0.25), out=0x4000)
    a.update(case)
    fl = lambda v: None if v is None else (ctypes.c_float * 3)(*v)
    assert lib.vl_tactile_augment(a["records"], a["n"], a["S"], a["max_nrows"], a["tables"], a["tmp"], fl(a["mean"]), fl(a["std"]), a["out"],
                                  None) != 0
    assert text in lib.vl_last_error().decode() and "vl_tactile_augment" in lib.vl_last_error().decode()
