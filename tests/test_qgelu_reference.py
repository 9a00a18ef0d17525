"""CPU: QuickGELU towers (the OpenAI-pretrained CLIP activation, x * sigmoid(1.702 x)).

1. Pinned to the imported reference: its TriCLIP built from a tiny config that carries `"quick_gelu": true`, loaded with seeded
   weights (tests/golden_util.seeded_like), gives the features stored under tests/golden/reference/; the oracle with its GELU
   swapped for QuickGELU (tests/qgelu_ref.quick_gelu_oracle) must reproduce them to fp32 round-off, and the unpatched oracle must
   not.  This is the test that says the QuickGELU of the GPU tests' oracle is the reference's.
2. The public interface: TriCLIP(quick_gelu=True), force_quick_gelu=True and the `-quickgelu` config reach the cfg of every
   tower's executor; the state_dict is the erf model's; pretrained="openai" still raises, and says what works."""
import os
import warnings
from types import SimpleNamespace

import pytest
import torch

import vitlens_oracle as O
from golden_util import reference_run, seeded_like
from qgelu_ref import qgelu, qgelu_grad, quick_gelu_f32, quick_gelu_oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

TINY = {"embed_dim": 32, "quick_gelu": True,
        "vision_cfg": {"image_size": 32, "layers": 2, "width": 64, "patch_size": 8, "head_width": 32},
        "text_cfg": {"context_length": 16, "vocab_size": 96, "width": 64, "heads": 2, "layers": 2}}

_REF = r'''
import json, os, sys, tempfile, torch
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[2])
import ref_loader
oc = ref_loader.load()
from golden_util import seeded_like
cfg = json.loads(sys.argv[3])
args = ref_loader.lens_args("depth", perceiver_num_latents=16, perceiver_latent_dim=64, perceiver_latent_heads=2,
                            perceiver_latent_dim_head=32, perceiver_cross_dim_head=64, perceiver_cross_heads=1)
with tempfile.TemporaryDirectory() as td:
    with open(os.path.join(td, "tiny-quickgelu.json"), "w") as f:
        json.dump(cfg, f)
    oc.add_model_config(td)
    torch.manual_seed(31)
    model = oc.tri_create_model("tiny-quickgelu", None, precision="fp32", device="cpu", output_dict=True, args=args).eval()
stat = lambda sd: {k: [list(v.shape), float(v.double().mean()) if v.numel() else 0.0, float(v.double().std()) if v.numel() > 1 else 0.0,
                       str(v.dtype)] for k, v in sd.items()}
stats = stat(model.state_dict())
model.load_state_dict(seeded_like(stats, 31))
g = torch.Generator().manual_seed(32)
image = torch.randn(3, 3, 32, 32, generator=g)
depth = torch.rand(3, 1, 32, 32, generator=g)
text = torch.randint(1, 95, (3, 16), generator=g)
text[:, -1] = 95                                                     # the EOT token: the largest id, at the end
acts = sorted({type(m).__name__ for n, m in model.named_modules() if n.endswith("mlp.gelu")})
with torch.no_grad():
    out = {"stats": stats, "acts": acts, "identity": bool(args.perceiver_as_identity), "text": text.tolist(),
           "image": model.encode_image(image).tolist(), "text_features": model.encode_text(text).tolist(),
           "visual": model.encode_visual(depth).tolist()}
print("JSON" + json.dumps(out))
'''


def _inputs():
    g = torch.Generator().manual_seed(32)
    image = torch.randn(3, 3, 32, 32, generator=g)
    depth = torch.rand(3, 1, 32, 32, generator=g)
    return image, depth


def test_patched_oracle_reproduces_the_reference_quickgelu_towers():
    import json
    ref = reference_run("test_qgelu_reference.test_patched_oracle_reproduces_the_reference_quickgelu_towers", _REF,
                        [os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests"), json.dumps(TINY)])
    assert ref["acts"] == ["QuickGELU"] and ref["identity"] is True      # every block MLP of all three towers; no Perceiver
    sd = seeded_like(ref["stats"], 31)
    image, depth = _inputs()
    text = torch.tensor(ref["text"])
    tower = O.TowerSpec(width=64, layers=2, heads=2, patch=8, image_size=32, embed_dim=32)
    tspec = O.TextSpec(context_length=16, vocab_size=96, width=64, heads=2, layers=2, embed_dim=32)
    lens = O.LensSpec(modality="depth", perceiver_identity=True)
    want = {k: torch.tensor(ref[k]) for k in ("image", "text_features", "visual")}

    def run():
        with torch.no_grad():
            return {"image": O.encode_image(sd, image, tower), "text_features": O.encode_text(sd, text, tspec),
                    "visual": O.encode_visual(sd, depth, tower, lens)}
    with quick_gelu_oracle():
        got = run()
    assert O.gelu_erf is not quick_gelu_f32                               # the swap ends with the block
    for k in want:                                                        # the bound of tests/test_oracle_golden.py's tiny cases
        print(k, "max abs err", float((got[k] - want[k]).abs().max()))
        torch.testing.assert_close(got[k], want[k], rtol=2e-5, atol=2e-6)
    erf = run()
    for k in want:                                                        # and the erf oracle is NOT that tower
        assert float((erf[k] - want[k]).abs().max()) > 1e-3, k


def test_reference_arithmetic_helpers():
    """A check of the TEST helpers (tests/qgelu_ref.py), not of the feature: the fp64 derivative the GPU tests compare against
    is the autograd derivative of the reference's expression, and both helpers are finite at the ends of fp32."""
    x = torch.linspace(-30, 30, 2001, dtype=torch.float64).requires_grad_(True)
    y = x * torch.sigmoid(1.702 * x)
    (dy,) = torch.autograd.grad(y.sum(), x)
    assert torch.equal(qgelu(x.detach()), y.detach())
    torch.testing.assert_close(qgelu_grad(x.detach()), dy, rtol=1e-13, atol=1e-15)
    big = torch.tensor([-3.0e38, -1e4, 1e4, 3.0e38], dtype=torch.float32)
    assert torch.isfinite(qgelu(big)).all() and torch.isfinite(qgelu_grad(big)).all()


# ---- the public interface ---------------------------------------------------------------------------------------------------
def _oc():
    import open_clip as oc
    return oc


def _tri(**kw):
    oc = _oc()
    return oc.TriCLIP(TINY["embed_dim"], dict(TINY["vision_cfg"]), dict(TINY["text_cfg"]), **kw)


def _flags(model):
    return (model.image._cfgs()[0].quick_gelu, model.visual._cfgs()[0].quick_gelu, model._text_cfg().quick_gelu)


def test_triclip_quick_gelu_constructs_and_reaches_every_tower_cfg():
    torch.manual_seed(0)
    q = _tri(quick_gelu=True)
    torch.manual_seed(0)
    e = _tri()
    assert _flags(q) == (True, True, True) and _flags(e) == (False, False, False)
    # the activation has no parameters: the same keys, shapes and (same seed) values as the erf model
    sq, se = q.state_dict(), e.state_dict()
    assert list(sq) == list(se)
    for k in sq:
        assert torch.equal(sq[k], se[k]), k


def test_factory_honours_force_quick_gelu_and_the_quickgelu_config():
    oc = _oc()
    assert "ViT-B-32-quickgelu" in oc.list_models()
    base, quick = oc.get_model_config("ViT-B-32"), oc.get_model_config("ViT-B-32-quickgelu")
    assert quick.pop("quick_gelu") is True and quick == base              # our own ViT-B-32 plus the key
    import tempfile
    import json
    with tempfile.TemporaryDirectory() as td:
        for name, cfg in (("zz-tiny-erf", {k: v for k, v in TINY.items() if k != "quick_gelu"}), ("zz-tiny-quickgelu", TINY)):
            with open(os.path.join(td, name + ".json"), "w") as f:
                json.dump(cfg, f)
        oc.add_model_config(td)
        try:
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                assert _flags(oc.tri_create_model("zz-tiny-erf", None, device="cpu")) == (False, False, False)
                assert _flags(oc.tri_create_model("zz-tiny-erf", None, device="cpu", force_quick_gelu=True)) == (True, True, True)
                assert _flags(oc.tri_create_model("zz-tiny-quickgelu", None, device="cpu")) == (True, True, True)
                m = oc.tri_create_model_and_transforms("zz-tiny-erf", None, device="cpu", force_quick_gelu=True)[0]
                assert _flags(m) == (True, True, True)
                # the refusals that stay
                for kw in (dict(jit=True), dict(force_custom_text=True), dict(pretrained_image=True)):
                    with pytest.raises(NotImplementedError):
                        oc.tri_create_model("zz-tiny-erf", None, device="cpu", force_quick_gelu=True, **kw)
        finally:
            from open_clip import factory
            factory._CONFIG_PATHS.pop()
            factory._rescan()


def test_pretrained_openai_still_raises_and_says_what_works():
    oc = _oc()
    with pytest.raises(NotImplementedError) as ei:
        oc.tri_create_model("ViT-B-32-quickgelu", "openai", device="cpu")
    msg = str(ei.value)
    assert "force_quick_gelu=True" in msg and "-quickgelu" in msg and "open_clip layout" in msg
    with pytest.raises(NotImplementedError):
        oc.tri_create_model_and_transforms("ViT-B-32", "openai", device="cpu", force_quick_gelu=True)


def test_wrappers_pass_the_flag_through():
    """mm_vit_lens (force_quick_gelu of the model cfg) and openshape.CLIPBindWrap hand the flag to tri_create_model."""
    import mm_vit_lens.vitlens as V
    from mm_vit_lens.model_cfg import fetch_model_cfg
    seen = {}

    def fake(name, pretrained=None, **kw):
        seen.update(kw)
        raise KeyboardInterrupt                                         # (do not build ViT-L-14 here)
    orig = V.tri_create_model
    V.tri_create_model = fake
    try:
        cfg = fetch_model_cfg(modality="image")
        cfg.force_quick_gelu = True
        with pytest.raises(KeyboardInterrupt):
            V._create(cfg.model, "cpu", cfg)
    finally:
        V.tri_create_model = orig
    assert seen["force_quick_gelu"] is True
    # openshape.CLIPBindWrap builds its TriCLIP through tri_create_model_and_transforms
    import open_clip
    import openshape
    seen.clear()

    def fake_tt(name, pretrained=None, **kw):
        seen.update(kw)
        raise KeyboardInterrupt
    orig = open_clip.tri_create_model_and_transforms
    open_clip.tri_create_model_and_transforms = fake_tt
    try:
        args = SimpleNamespace(clip_model="ViT-B-32", pretrained=None, precision="fp32", force_quick_gelu=True,
                               model=SimpleNamespace(out_channel=512))
        with pytest.raises(KeyboardInterrupt):
            openshape.CLIPBindWrap(args)
    finally:
        open_clip.tri_create_model_and_transforms = orig
    assert seen["force_quick_gelu"] is True
