"""CPU: the oracle against the reference at FULL size (ViT-L/14 towers, the audio Lens with its 2 x (cross + 3 self)
Perceiver, the point-cloud Lens).  The 1.7 GB state_dict cannot be a fixture: when the reference's outputs are recorded, its
model is built with a fixed seed and then loaded with tests/golden_util.seeded_like weights of the same per-tensor mean and
spread; the test rebuilds those weights from the stored statistics, hands them to the oracle, and the features of both must
agree to fp32 round-off."""
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_SCRIPT = r'''
import json, sys, torch
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[2])
import ref_loader
oc = ref_loader.load()
from golden_util import seeded_like
stat = lambda sd: {k: [list(v.shape), float(v.double().mean()) if v.numel() else 0.0, float(v.double().std()) if v.numel() > 1 else 0.0,
                       str(v.dtype)] for k, v in sd.items()}
torch.manual_seed(3)
model = oc.tri_create_model("ViT-L-14", None, precision="fp32", device="cpu", output_dict=True, args=ref_loader.lens_args("audio")).eval()
stats = stat(model.state_dict())
model.load_state_dict(seeded_like(stats, 3))
g = torch.Generator().manual_seed(4)
image = torch.randn(2, 3, 224, 224, generator=g)
audio = torch.randn(2, 512, 128, generator=g) * 0.5
text = oc.tokenize(["a dog barking", "rain on a tin roof"])
with torch.no_grad():
    out = {"audio_stats": stats, "text": text.tolist(), "image": model.encode_image(image).tolist(),
           "text_features": model.encode_text(text).tolist(), "audio": model.encode_visual(audio).tolist()}
del model
# point-cloud Lens (PointBERT tokenizer: FPS 512 centres of 8192 points, kNN 32, mini-PointNet; Perceiver depth 4)
torch.manual_seed(5)
model = oc.tri_create_model("ViT-L-14", None, precision="fp32", device="cpu", output_dict=True, args=ref_loader.lens_args("pc")).eval()
stats = stat(model.state_dict())
model.load_state_dict(seeded_like(stats, 5))
pts = torch.rand(2, 8192, 3, generator=g) * 2 - 1
torch.manual_seed(11)                                                 # what misc.fps draws (misc.py:60)
with torch.no_grad():
    out["pc"] = model.encode_visual(pts).tolist()
out["pc_stats"] = stats
print("JSON" + json.dumps(out))
'''


def test_oracle_equals_reference_at_vitl_size():
    import torch
    import vitlens_oracle as O
    from golden_util import reference_run, seeded_like
    ref = reference_run("test_oracle_fullsize.test_oracle_equals_reference_at_vitl_size", _SCRIPT,
                        [os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")], timeout=1500)
    rel = lambda a, b: float((a - b).norm() / b.norm())
    sd = seeded_like(ref["audio_stats"], 3)
    assert sum(v.numel() for v in sd.values()) > 8e8
    g = torch.Generator().manual_seed(4)
    image = torch.randn(2, 3, 224, 224, generator=g)
    audio = torch.randn(2, 512, 128, generator=g) * 0.5
    res = {}
    with torch.no_grad():
        res["image"] = rel(O.encode_image(sd, image, O.TowerSpec()), torch.tensor(ref["image"]))
        res["text"] = rel(O.encode_text(sd, torch.tensor(ref["text"]), O.TextSpec()), torch.tensor(ref["text_features"]))
        lens = O.LensSpec(modality="audio", perceiver_identity=False, depth=2, self_per_cross=3)
        res["audio"] = rel(O.encode_visual(sd, audio, O.TowerSpec(), lens), torch.tensor(ref["audio"]))
    del sd
    sd = seeded_like(ref["pc_stats"], 5)
    pts = torch.rand(2, 8192, 3, generator=g) * 2 - 1
    torch.manual_seed(11); start = torch.randint(0, 8192, (2,), dtype=torch.long)
    with torch.no_grad():
        lens = O.LensSpec(modality="pc", perceiver_identity=False, depth=4, self_per_cross=1, input_chan=384)
        res["pc"] = rel(O.encode_visual(sd, pts, O.TowerSpec(), lens, fps_start=start), torch.tensor(ref["pc"]))
    for k in ("image", "text", "audio", "pc"):
        assert res[k] < 2e-5, res


_FLOOR = r'''
import json, sys, torch
sys.path.insert(0, sys.argv[1])
import ref_loader
oc = ref_loader.load()
import vitlens_oracle as O
spec = O.TextSpec()
g = torch.Generator().manual_seed(77)            # the weights / texts of tests/test_hip_towers.py::test_vitl_text_tower_vs_oracle
sd = O.init_text(spec, g)
text = O.synth_text(4, g)
torch.manual_seed(0)
model = oc.tri_create_model("ViT-L-14", None, precision="fp32", device="cpu", output_dict=True, args=ref_loader.lens_args("depth")).eval()
model.load_state_dict(sd, strict=False)
with torch.no_grad():
    f32 = model.encode_text(text)
    with torch.autocast("cpu", dtype=torch.bfloat16):
        fbf = model.encode_text(text)
print("JSON" + json.dumps({"f32": f32.tolist(), "bf16": fbf.float().tolist()}))
'''


def test_reference_amp_bf16_floor_of_the_text_tower():
    """north_star asks for cosine matrices within 1e-3 of the fp32 CPU path.  On the random-init ViT-L text tower (features
    with a mutual cosine of ~0.6) the REFERENCE ITSELF under its amp_bf16 autocast is 1.4e-3 away from its own fp32 path;
    the HIP path (bf16 operands, fp32 residual stream) is held to 2e-3 on the same case (tests/test_hip_towers.py) and to
    1e-3 on the per-feature cosine.  This test pins that floor so the relaxed bound is a measured property of bf16
    arithmetic on this input, not a loosened criterion."""
    import torch
    import vitlens_oracle as O
    from golden_util import reference_run
    ref = reference_run("test_oracle_fullsize.test_reference_amp_bf16_floor_of_the_text_tower", _FLOOR, [os.path.join(ROOT, "oracle")],
                        timeout=1500)
    f32, fbf = torch.tensor(ref["f32"]), torch.tensor(ref["bf16"])
    cosm = lambda a: (lambda n: n @ n.t())(torch.nn.functional.normalize(a.float(), dim=-1))
    res = {"cos_matrix": float((cosm(fbf) - cosm(f32)).abs().max()),
           "feature_cos": float(torch.nn.functional.cosine_similarity(fbf, f32, dim=-1).min()), "mutual": float(cosm(f32)[0, 1])}
    # the fp32 side is the oracle's on the same weights and texts: the floor is measured against the path the HIP tower is
    spec = O.TextSpec()
    g = torch.Generator().manual_seed(77)
    sd = O.init_text(spec, g)
    text = O.synth_text(4, g)
    with torch.no_grad():
        mine = O.encode_text(sd, text, spec)
    assert float((mine - f32).norm() / f32.norm()) < 2e-5
    assert 1.0e-3 < res["cos_matrix"] < 2.0e-3, res
    assert res["feature_cos"] > 0.9999 and 0.5 < res["mutual"] < 0.7, res
