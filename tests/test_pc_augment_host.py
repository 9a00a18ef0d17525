"""CPU: the 3D training augmentation (PCProcessorTrain, vl_pc_augment).

1. tests/pc_augment_ref.py pinned to the reference's own functions through golden_util.reference_run: both pipelines, the guard
   of normalize_pc and random_rotate_z, at atol = 0, the draws re-derived from the same seeded legacy generator.
2. The composed fp32 form xyz . A + t against that sequential restatement.
3. The processor's draws: order, ranges, reproducibility, the identity record, bad arguments.
4. The 64-byte record.
5. The C ABI: declaration = binding, version 610 everywhere, the refusals (which launch nothing, so they run here too)."""
import ctypes
import os
import re

import numpy as np
import pytest

import pc_augment_ref as R
from golden_util import reference_run
from open_clip.modal_3d.processors.pc_processor import PCProcessorTrain, compose_affine
from test_pc_processor import _cloud

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEEDS = (3, 11)

# Run where the reference is importable.  modal_3d/datasets.py imports h5py, lmdb and torchvision at module level, so only
# the FunctionDef nodes that are needed are compiled out of its syntax tree, into a namespace that holds numpy.
_REF = r'''
import ast, importlib.util, json, os, sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[2])
import ref_loader
from test_pc_processor import _cloud
seeds = json.loads(sys.argv[3])
spec = importlib.util.spec_from_file_location("ref_openshape_data", os.path.join(ref_loader.REF_ROOT, "VitLens-OpenShape", "src", "utils", "data.py"))
osd = importlib.util.module_from_spec(spec); spec.loader.exec_module(osd)
path = os.path.join(ref_loader.REF_SRC, "open_clip", "modal_3d", "datasets.py")
want = ("rotate_point_cloud", "random_point_dropout", "random_scale_point_cloud", "shift_point_cloud",
        "rotate_perturbation_point_cloud", "pc_norm")
nodes, seen = [], set()
for n in ast.walk(ast.parse(open(path).read(), path)):
    if isinstance(n, ast.FunctionDef) and n.name in want and n.name not in seen:
        nodes.append(n); seen.add(n.name)
assert seen == set(want), seen
ns = {"np": np}
exec(compile(ast.Module(body=nodes, type_ignores=[]), path, "exec"), ns)
out = {"vitlens": [], "openshape": [], "rotate_z": []}
for s in seeds:
    pc = ns["pc_norm"](None, _cloud(700, 3, 1))
    np.random.seed(s)
    pc = ns["random_point_dropout"](pc[None, ...])
    pc = ns["random_scale_point_cloud"](pc)
    pc = ns["shift_point_cloud"](pc)
    pc = ns["rotate_perturbation_point_cloud"](pc)
    pc = ns["rotate_point_cloud"](pc)
    pc = pc.squeeze()
    out["vitlens"].append({"dtype": str(pc.dtype), "pc": pc.tolist()})
    xyz = osd.normalize_pc(_cloud(700, 3, 1))
    np.random.seed(s)
    xyz = osd.random_rotate_z(osd.augment_pc(xyz))
    out["openshape"].append({"dtype": str(xyz.dtype), "pc": xyz.tolist()})
    np.random.seed(s)
    z = osd.random_rotate_z(_cloud(40, 3, 2))
    out["rotate_z"].append({"dtype": str(z.dtype), "pc": z.tolist()})
g = osd.normalize_pc(np.tile(np.array([[0.5, -1.25, 2.0]], dtype=np.float32), (50, 1)))
out["guard"] = {"dtype": str(g.dtype), "pc": g.tolist()}
g = osd.normalize_pc(np.tile(_cloud(1, 3, 4), (50, 1)))
out["no_guard"] = {"dtype": str(g.dtype), "pc": g.tolist()}
n = osd.normalize_pc(_cloud(700, 3, 1))
out["normalize_pc"] = {"dtype": str(n.dtype), "pc": n.tolist()}
print("JSON" + json.dumps(out))
'''


@pytest.fixture(scope="module")
def ref():
    import json
    return reference_run("test_pc_augment_host.reference_augmentation", _REF,
                         [os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests"), json.dumps(list(SEEDS))])


def _same(got, rec):
    want = np.array(rec["pc"], dtype=rec["dtype"])
    assert str(got.dtype) == rec["dtype"] and got.shape == want.shape
    assert np.array_equal(got, want), np.abs(got - want).max()


@pytest.mark.parametrize("k", range(len(SEEDS)))
def test_vitlens_pipeline_equals_the_reference(ref, k):
    np.random.seed(SEEDS[k])
    d = R.draw_reference(700, "vitlens")
    _same(R.vitlens_pipeline(R.pc_norm(_cloud(700, 3, 1)), d), ref["vitlens"][k])


@pytest.mark.parametrize("k", range(len(SEEDS)))
def test_openshape_pipeline_equals_the_reference(ref, k):
    np.random.seed(SEEDS[k])
    d = R.draw_reference(700, "openshape")
    _same(R.openshape_pipeline(R.normalize_pc(_cloud(700, 3, 1)), d), ref["openshape"][k])


def test_normalize_pc_its_guard_and_rotate_z_equal_the_reference(ref):
    _same(R.normalize_pc(_cloud(700, 3, 1)), ref["normalize_pc"])
    g = R.normalize_pc(np.tile(np.array([[0.5, -1.25, 2.0]], dtype=np.float32), (50, 1)))     # the fp32 mean is exact
    _same(g, ref["guard"])
    assert not g.any()
    # fifty copies of a point whose fp32 mean is NOT exact: the residue is above 1e-6 and is blown up to the unit sphere
    g = R.normalize_pc(np.tile(_cloud(1, 3, 4), (50, 1)))
    _same(g, ref["no_guard"])
    assert g.any()
    for k, s in enumerate(SEEDS):
        np.random.seed(s)
        _same(R.random_rotate_z(_cloud(40, 3, 2), np.random.uniform(0, 2 * np.pi)), ref["rotate_z"][k])


# ------------------------------------------------------------------------------------------------ 2. the composed form
# Normalisation off: the input is the normalised cloud itself (|p| <= 1), so every intermediate coordinate is at most
# 1.25 + 0.1 sqrt(3) = 1.43 in magnitude, where an fp32 rounding is at most 2^-24 * 2 = 1.2e-7 (half an ulp in [1, 2)).
#   reference: four fp32 roundings (scale, shift, two rotations)                                   4 * 1.2e-7  = 4.8e-7
#   composed:  12 rounded coefficients - per output three of A (each off by at most 2^-24 * 1.25 = 7.5e-8, times
#              |x| + |y| + |z| <= sqrt(3): 1.3e-7) and one of t (|t| < 0.25: 7.5e-9) - and three FMAs (3 * 1.2e-7)
#                                                                                                   about 5.0e-7
# together about 1e-6; the tolerance is 2e-6, about twice that.
COMPOSED_ATOL = 2e-6


@pytest.mark.parametrize("flavour,axis", [("vitlens", "y"), ("openshape", "z")])
def test_composed_form_equals_the_sequential_restatement(flavour, axis):
    worst = 0.0
    for s in range(20):
        np.random.seed(100 + s)
        d = R.draw_reference(700, flavour)
        x = (R.pc_norm if flavour == "vitlens" else R.normalize_pc)(_cloud(700, 3, 1 + s))
        assert x.dtype == np.float32
        mask = d["field"] <= d["ratio"]
        dropped = x.copy()
        dropped[mask] = dropped[0]
        A, t = compose_affine(d["scale"][0], d["shift"][0], d["angles"], d["final"], axis)
        A2, t2 = R.compose(d["scale"][0], d["shift"][0], d["angles"], d["final"], axis)
        assert A.dtype == np.float32 and t.dtype == np.float32
        assert np.abs(A - A2).max() <= 1.2e-7 and np.abs(t - t2).max() <= 1.5e-8          # one ulp of a coefficient <= 1.25 / 0.18
        got = R.apply_composed_f32(dropped, A, t).astype(np.float64)
        seq32 = (R.vitlens_pipeline if flavour == "vitlens" else R.openshape_pipeline)(x.copy(), d).astype(np.float64)
        seq64 = R.sequential_f64(x, mask, d["scale"][0], d["shift"][0], d["angles"], d["final"], axis)
        e32, e64 = np.abs(got - seq32).max(), np.abs(got - seq64).max()
        worst = max(worst, e32, e64)
        assert e32 <= COMPOSED_ATOL and e64 <= COMPOSED_ATOL, (s, e32, e64)
    print(f"composed vs sequential ({flavour}): max |diff| = {worst:.3e}")


def test_y_up_swap_folds_into_the_matrix():
    x = _cloud(300, 3, 5)
    sw = x.copy()
    sw[:, [1, 2]] = sw[:, [2, 1]]
    A, t = compose_affine(1.1, [0.05, -0.02, 0.1], [0.03, -0.1, 0.18], 2.0, "z", y_up=True)
    B, u = compose_affine(1.1, [0.05, -0.02, 0.1], [0.03, -0.1, 0.18], 2.0, "z")
    assert np.array_equal(t, u)
    # the same three products per output, added in another order: a few roundings of values below 16 (ulp 2^-20)
    assert np.abs(R.apply_composed_f32(x, A, t) - R.apply_composed_f32(sw, B, u)).max() <= 3 * 2.0 ** -21
    assert np.array_equal(A, R.compose(1.1, [0.05, -0.02, 0.1], [0.03, -0.1, 0.18], 2.0, "z", y_up=True)[0])


# ------------------------------------------------------------------------------------------------ 3. the draws
def _unpack(rec):
    A, t, ratio, flags, seed = rec
    return np.array(A, dtype=np.float32).reshape(3, 3), np.array(t, dtype=np.float32), ratio, flags, seed


@pytest.mark.parametrize("flavour,axis", [("vitlens", "y"), ("openshape", "z")])
def test_draw_order_is_the_references(flavour, axis):
    proc = PCProcessorTrain(1024, True, flavour=flavour, seed=7, device="cpu", rgb_random_drop_prob=0.5 if flavour == "openshape" else 0.0)
    rng = np.random.RandomState(7)
    for _ in range(3):
        A, t, ratio, flags, seed = _unpack(proc.draw_params())
        want_ratio = rng.random_sample() * 0.875
        hi, lo = int(rng.randint(0, 2 ** 32, dtype=np.uint64)), int(rng.randint(0, 2 ** 32, dtype=np.uint64))     # in place of the N-field
        scale = rng.uniform(0.8, 1.25, 1)[0]
        shift = rng.uniform(-0.1, 0.1, (1, 3))[0]
        angles = np.clip(0.06 * rng.randn(3), -0.18, 0.18)
        final = rng.uniform() * 2 * np.pi if flavour == "vitlens" else rng.uniform(0, 2 * np.pi)
        want_flags = R.NORMALIZE
        if flavour == "openshape":
            want_flags |= R.NORM_GUARD | (R.FEAT_FILL if rng.rand() < 0.5 else 0)
        A2, t2 = R.compose(scale, shift, angles, final, axis)
        assert ratio == float(np.float32(want_ratio)) and seed == (hi << 32 | lo) and flags == want_flags
        assert np.abs(A - A2).max() <= 1.2e-7 and np.abs(t - t2).max() <= 1.5e-8


def test_draw_ranges_and_reproducibility():
    a, b, c = (PCProcessorTrain(1024, True, seed=s, device="cpu") for s in (5, 5, 6))
    ra, rb, rc = ([p.draw_params() for _ in range(300)] for p in (a, b, c))
    assert ra == rb and ra != rc
    fills = 0
    for rec in ra + [PCProcessorTrain(64, False, flavour="openshape", seed=1, device="cpu", rgb_random_drop_prob=1.0).draw_params()]:
        A, t, ratio, flags, seed = _unpack(rec)
        assert 0.0 <= ratio < 0.875 and 0 <= seed < 2 ** 64
        s = np.sqrt((A.astype(np.float64) ** 2).sum(axis=0))              # a scaled rotation: columns of length `scale`
        assert np.all(s > 0.8 - 1e-6) and np.all(s < 1.25 + 1e-6) and np.abs(s - s[0]).max() < 1e-6
        assert np.abs(A.astype(np.float64).T @ A.astype(np.float64) - s[0] ** 2 * np.eye(3)).max() < 1e-6
        assert np.linalg.norm(t) <= 0.1 * np.sqrt(3) + 1e-6
        fills += bool(flags & R.FEAT_FILL)
    assert fills == 1                                                   # only the probability-1 openshape record
    assert len({r[4] for r in ra}) == 300                               # the device seeds differ from sample to sample


def test_augment_off_is_the_identity_record_and_draws_nothing():
    p = PCProcessorTrain(1024, True, augment=False, seed=3, device="cpu")
    state = p.rng.get_state()[1].copy()
    A, t, ratio, flags, seed = _unpack(p.draw_params())
    assert np.array_equal(A, np.eye(3, dtype=np.float32)) and not t.any() and ratio == -1.0 and flags == R.NORMALIZE and seed == 0
    assert np.array_equal(p.rng.get_state()[1], state)
    A, t, ratio, flags, _ = _unpack(PCProcessorTrain(64, False, augment=False, flavour="openshape", y_up=True, device="cpu").draw_params())
    assert np.array_equal(A, np.array([[1, 0, 0], [0, 0, 1], [0, 1, 0]], dtype=np.float32)) and flags == R.NORMALIZE | R.NORM_GUARD
    assert not R.drop_mask(123, 4096, -1.0).any()                       # -1 drops nothing, whatever the field


def test_bad_arguments_are_refused():
    with pytest.raises(ValueError, match="flavour"):
        PCProcessorTrain(1024, True, flavour="pointnext")
    with pytest.raises(ValueError, match="openshape"):
        PCProcessorTrain(1024, True, y_up=True)
    with pytest.raises(ValueError, match="rgb_random_drop_prob"):
        PCProcessorTrain(1024, True, flavour="openshape", rgb_random_drop_prob=1.5)
    with pytest.raises(ValueError, match="npoint"):
        PCProcessorTrain(0, True)
    p = PCProcessorTrain(64, True, flavour="vitlens", seed=1, device="cpu")
    with pytest.raises(ValueError, match="C == 3"):
        p.process_batch(np.stack([_cloud(100, 6, 1)]))
    with pytest.raises(ValueError, match="records"):
        p.process_batch(np.stack([_cloud(100, 3, 1)]), params=[p.draw_params(), p.draw_params()])


# ------------------------------------------------------------------------------------------------ 4. the record
def test_record_layout():
    from vitlens_hip import ops
    dt = ops.PC_AUGMENT_DTYPE
    assert dt.itemsize == 64
    assert {n: dt.fields[n][1] for n in dt.names} == {"A": 0, "t": 36, "drop_ratio": 48, "flags": 52, "seed": 56}
    rows = [R.record(1.1, [0.05, -0.02, 0.1], [0.03, -0.1, 0.18], 2.0, "y", 0.4, 1, 0xFEDCBA9876543210),
            R.record(0.9, [0.0, 0.1, -0.1], [0.0, 0.0, 0.0], 0.5, "z", -1.0, 7, 1)]
    words = ops.pc_augment_pack(rows)
    assert words.dtype == np.int32 and words.shape == (2, 16)
    assert words.tobytes() == b"".join(R.pack_record(*r) for r in rows)
    assert (int(words[0, 14]) & 0xFFFFFFFF, int(words[0, 15]) & 0xFFFFFFFF) == (0x76543210, 0xFEDCBA98)        # little-endian halves
    assert np.array_equal(ops.pc_augment_pack(np.frombuffer(words.tobytes(), dtype=dt)), words)
    for bad in (1.5, -0.5, float("nan"), -1.0000001):
        with pytest.raises(ValueError, match="drop_ratio"):
            ops.pc_augment_pack([rows[0][:2] + (bad,) + rows[0][3:]])
    assert ops.pc_augment_params(rows, "cpu").dtype.is_floating_point is False


def test_dropout_field_is_the_philox_stream():
    from philox_ref import noise_field
    u = R.dropout_field(0x0123456789ABCDEF, 1030)
    assert u.dtype == np.float32 and u.shape == (1030,) and u.min() >= 0.0 and u.max() < 1.0
    assert np.array_equal(u, noise_field(0x0123456789ABCDEF, 1, 1030).reshape(-1))       # same key, counter and word convention
    assert 0.35 < R.drop_mask(5, 8192, 0.4).mean() < 0.45


# ------------------------------------------------------------------------------------------------ 5. the C ABI
def _header():
    src = open(os.path.join(ROOT, "include", "vitlens_hip.h")).read()
    return src, re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def test_entry_is_declared_exported_and_bound_under_610():
    from vitlens_hip import _lib
    raw, hdr = _header()
    P, I, F = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    m = re.search(r"\bint\s+vl_pc_augment\s*\(([^)]*)\)\s*;", hdr)
    assert m
    ctype = {"int": I, "float": F, "hipStream_t": P}
    want = [P if "*" in prm else ctype[prm.replace("const ", "").split()[0]] for prm in (q.strip() for q in m.group(1).split(","))]
    assert _lib.SIGNATURES["vl_pc_augment"] == want == [P, P, P, I, I, I, I, P, F, P]
    assert hasattr(ctypes.CDLL(_lib.lib_path()), "vl_pc_augment")
    version = int(re.search(r"#define\s+VL_ABI_VERSION\s+(\d+)", hdr).group(1))
    assert version == 610 == _lib.ABI_VERSION == int(_lib.load_library().vl_version())
    # the layout is spelled out next to the declaration, and the NOTE on the version covers the entry
    doc = raw[:raw.index("int vl_pc_augment(")].rsplit("/*", 1)[1]
    for word in ("float A[9]", "float t[3]", "drop_ratio", "int32 flags", "uint64 seed", "64-byte", "NOTE on the version", "610"):
        assert word in doc, word


REFUSALS = (
    (dict(B=0), "bad shape"), (dict(N=0), "bad shape"), (dict(G=0), "bad shape"), (dict(C=2), "bad shape"), (dict(C=9), "bad shape"),
    (dict(pts=None), "null operand"), (dict(out=None), "null operand"), (dict(params=None), "null operand"),
    (dict(idx=None, G=5), "G must equal N"), (dict(out="pts"), "out of place"),
)


def refuse(lib, case):
    """Call the entry with one operand made bad; the other pointers are non-null and never dereferenced by a refusal."""
    a = dict(pts=0x1000, idx=0x2000, out=0x3000, B=2, N=8, G=4, C=3, params=0x4000)
    a.update(case)
    if a["out"] == "pts":
        a["out"] = a["pts"]
    return lib.vl_pc_augment(a["pts"], a["idx"], a["out"], a["B"], a["N"], a["G"], a["C"], a["params"], 0.4, None)


@pytest.mark.parametrize("case,text", REFUSALS)
def test_entry_refuses_without_launching(case, text):
    from vitlens_hip import _lib
    lib = _lib.load_library()
    assert refuse(lib, case) != 0
    assert text in lib.vl_last_error().decode() and "vl_pc_augment" in lib.vl_last_error().decode()
