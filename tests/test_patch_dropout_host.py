"""CPU: patch dropout (FLIP token masking; PatchDropout, open_clip/transformer.py:53-90).

1. Pinned to the imported reference: its TriCLIP built with force_patch_dropout=p from a tiny config, in train mode, gives the
   features, kept indices and gradients stored under tests/golden/reference/; tests/patchdrop_ref.py (the oracle with the kept
   rows gathered between the positional add and ln_pre) must reproduce them, and the un-dropped oracle must not.  This is the
   test that says the patch dropout of the GPU tests' oracle is the reference's.
2. The kept-token count is the reference's expression.
3. The C ABI: the three entries are declared, exported and bound with the header's parameter lists; version >= 609 everywhere.
4. The public interface: the flag reaches both ViT towers, None / False / 0.0 mean off, 1.0 raises, the wrappers pass their
   False through, the fused steps' constructors take patch_dropout / drop_seed, and the sample numbers never collide."""
import ctypes
import inspect
import json
import os
import re
import tempfile
import warnings
from types import SimpleNamespace

import pytest
import torch

import vitlens_oracle as O
import patchdrop_ref as PR
from golden_util import reference_run, seeded_like

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

TINY = {"embed_dim": 32,
        "vision_cfg": {"image_size": 32, "layers": 2, "width": 64, "patch_size": 8, "head_width": 32},
        "text_cfg": {"context_length": 16, "vocab_size": 96, "width": 64, "heads": 2, "layers": 2}}
PS = (0.5, 0.75)
SEED = 77                     # torch.manual_seed in front of every train-mode forward
REF_KEY = "test_patch_dropout_host.reference_patch_dropout"
GRADS = {"visual": ("visual.class_embedding", "visual.positional_embedding", "visual.visual_adapter.conv1.weight",
                    "visual.visual_adapter.pos_emb"),
         "image": ("image.class_embedding", "image.positional_embedding")}

_REF = r'''
import json, os, sys, tempfile, torch
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[2])
import ref_loader
oc = ref_loader.load()
from golden_util import seeded_like
cfg = json.loads(sys.argv[3]); seed = int(sys.argv[4]); grads = json.loads(sys.argv[5])
args = ref_loader.lens_args("depth", perceiver_num_latents=16, perceiver_latent_dim=64, perceiver_latent_heads=2,
                            perceiver_latent_dim_head=32, perceiver_cross_dim_head=64, perceiver_cross_heads=1)
g = torch.Generator().manual_seed(32)
image = torch.randn(3, 3, 32, 32, generator=g)
depth = torch.rand(3, 1, 32, 32, generator=g)
dfeat = torch.randn(3, 32, generator=g)
stat = lambda sd: {k: [list(v.shape), float(v.double().mean()) if v.numel() else 0.0, float(v.double().std()) if v.numel() > 1 else 0.0,
                       str(v.dtype)] for k, v in sd.items()}
out = {"identity": bool(args.perceiver_as_identity), "cases": {}}
with tempfile.TemporaryDirectory() as td:
    with open(os.path.join(td, "tiny-patchdrop.json"), "w") as f:
        json.dump(cfg, f)
    oc.add_model_config(td)
    for p in json.loads(sys.argv[6]):
        torch.manual_seed(31)
        model = oc.tri_create_model("tiny-patchdrop", None, precision="fp32", device="cpu", output_dict=True, args=args,
                                    force_patch_dropout=p)
        stats = stat(model.state_dict())
        model.load_state_dict(seeded_like(stats, 31))
        out["stats"] = stats
        params = dict(model.named_parameters())
        case = {"layers": sorted({type(m).__name__ for n, m in model.named_modules() if n.endswith("patch_dropout")})}
        model.train()
        for tower, x, enc in (("visual", depth, model.encode_visual), ("image", image, model.encode_image)):
            T = params[tower + ".positional_embedding"].shape[0] - 1
            torch.manual_seed(seed)
            feat = enc(x)
            gs = torch.autograd.grad((feat * dfeat).sum(), [params[k] for k in grads[tower]])
            torch.manual_seed(seed)                      # the layer's own draw, repeated: randn(batch, T) then topk
            keep = torch.randn(x.shape[0], T).topk(max(1, int(T * (1 - p))), dim=-1).indices
            case[tower] = {"features": feat.detach().tolist(), "keep": keep.tolist(),
                           "grads": {k: v.tolist() for k, v in zip(grads[tower], gs)}}
        model.eval()
        with torch.no_grad():
            case["eval"] = {"visual": model.encode_visual(depth).tolist(), "image": model.encode_image(image).tolist()}
        out["cases"][repr(p)] = case
print("JSON" + json.dumps(out))
'''


def reference():
    """The recorded reference run (shared with tests/test_hip_patch_dropout.py)."""
    return reference_run(REF_KEY, _REF, [os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests"), json.dumps(TINY), str(SEED),
                                         json.dumps(GRADS), json.dumps(PS)])


def inputs():
    g = torch.Generator().manual_seed(32)
    image = torch.randn(3, 3, 32, 32, generator=g)
    depth = torch.rand(3, 1, 32, 32, generator=g)
    dfeat = torch.randn(3, 32, generator=g)
    return image, depth, dfeat


TOWER = O.TowerSpec(width=64, layers=2, heads=2, patch=8, image_size=32, embed_dim=32)
LENS = O.LensSpec(modality="depth", perceiver_identity=True)


def oracle_features(sd, tower, x, keep=None):
    """The oracle's tower with (keep) or without patch dropout; differentiable."""
    if tower == "image":
        tok, pos2 = O.image_tokens(sd, "image.", x, TOWER), None
    else:
        tok, pos2 = O.depth_tokens(sd, "visual.", x, TOWER)
    if keep is None:
        return O.vit_trunk(sd, tower + ".", tok if pos2 is None else tok + pos2, TOWER)
    return PR.vit_trunk_keep(sd, tower + ".", tok, TOWER, keep, pos2=pos2)


@pytest.mark.parametrize("p", PS)
def test_oracle_with_kept_rows_reproduces_the_reference(p):
    ref = reference()
    assert ref["identity"] is True
    case = ref["cases"][repr(p)]
    assert case["layers"] == ["PatchDropout"]                               # on both towers (one vision cfg)
    sd0 = seeded_like(ref["stats"], 31)
    image, depth, dfeat = inputs()
    for tower, x in (("visual", depth), ("image", image)):
        rec = case[tower]
        T = sd0[tower + ".positional_embedding"].shape[0] - 1
        torch.manual_seed(SEED)
        keep = PR.keep_indices(torch.randn(x.shape[0], T), PR.keep_count(T, p))
        assert keep.tolist() == rec["keep"], tower                           # the same tokens, exactly
        sd = {k: v.clone().requires_grad_(k in GRADS[tower]) for k, v in sd0.items()}
        feat = oracle_features(sd, tower, x, keep)
        want = torch.tensor(rec["features"])
        print(tower, p, "features max abs err", float((feat.detach() - want).abs().max()))
        torch.testing.assert_close(feat.detach(), want, rtol=2e-5, atol=2e-6)          # test_oracle_golden.py's tiny cases
        (feat * dfeat).sum().backward()
        for k in GRADS[tower]:
            g = torch.tensor(rec["grads"][k])
            print(k, "grad max abs err", float((sd[k].grad - g).abs().max()))
            torch.testing.assert_close(sd[k].grad, g, rtol=2e-4, atol=2e-6)             # test_oracle_golden.py's tiny gradients
        with torch.no_grad():
            dense = oracle_features(sd0, tower, x)
        assert float((dense - want).abs().max()) > 1e-3, tower                            # dropping is not the identity
        torch.testing.assert_close(dense, torch.tensor(case["eval"][tower]), rtol=2e-5, atol=2e-6)     # eval mode is


def test_keep_count_is_the_reference_expression():
    table = {(256, .5): 128, (256, .75): 64, (256, .9): 25, (49, .75): 12, (10, .9): 1, (10, .7): 3, (16, .5): 8, (16, .75): 4,
             (1, .5): 1, (257, .5): 128, (4096, .75): 1024}
    from vitlens_hip import ops
    for (T, p), want in table.items():
        assert PR.keep_count(T, p) == want == max(1, int(T * (1 - p))) == ops.patch_keep_count(T, p), (T, p)
    for p in (1.0, 1.5, -0.1):
        with pytest.raises(ValueError):
            ops.patch_keep_count(16, p)


# ---- the C ABI --------------------------------------------------------------------------------------------------------------
NEW = ("vl_patch_keep", "vl_assemble_ln_pre_keep", "vl_scatter_rows_keep")


def _header():
    src = open(os.path.join(ROOT, "include", "vitlens_hip.h")).read()
    return re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def test_new_entries_are_declared_exported_and_bound():
    from vitlens_hip import _lib
    names = set(re.findall(r"\b(vl_[a-z0-9_]+)\s*\(", _header()))
    lib = ctypes.CDLL(_lib.lib_path())
    for n in NEW:
        assert n in names and n in _lib.SIGNATURES and hasattr(lib, n), n
    assert names - {"vl_last_error"} == set(_lib.SIGNATURES)
    want = int(re.search(r"#define\s+VL_ABI_VERSION\s+(\d+)", _header()).group(1))
    assert want >= 609                          # 609 added the three entries above
    assert _lib.ABI_VERSION == want == int(_lib.load_library().vl_version())


def test_bound_signatures_match_the_header():
    from vitlens_hip import _lib
    P, I, F = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    ctype = {"int": I, "float": F, "uint64_t": ctypes.c_uint64, "int64_t": ctypes.c_int64, "long": ctypes.c_long, "hipStream_t": P}
    hdr = _header()
    for n in NEW:
        m = re.search(r"\bint\s+" + n + r"\s*\(([^)]*)\)\s*;", hdr)
        assert m, n
        want = []
        for prm in m.group(1).split(","):
            prm = prm.strip()
            want.append(P if "*" in prm else ctype[prm.replace("const ", "").split()[0]])
        assert _lib.SIGNATURES[n] == want, (n, _lib.SIGNATURES[n], want)


# ---- the public interface ---------------------------------------------------------------------------------------------------
def _tri(**vision):
    import open_clip as oc
    return oc.TriCLIP(TINY["embed_dim"], dict(TINY["vision_cfg"], **vision), dict(TINY["text_cfg"]))


def test_triclip_puts_the_value_on_both_towers_and_leaves_the_state_dict():
    from open_clip.model import CLIPVisionCfg
    assert CLIPVisionCfg().patch_dropout == 0.0
    torch.manual_seed(0)
    d = _tri(patch_dropout=0.5)
    torch.manual_seed(0)
    e = _tri()
    assert (d.image.patch_dropout, d.visual.patch_dropout) == (0.5, 0.5)
    assert (e.image.patch_dropout, e.visual.patch_dropout) == (0.0, 0.0)
    sq, se = d.state_dict(), e.state_dict()
    assert list(sq) == list(se)
    for k in sq:
        assert torch.equal(sq[k], se[k]), k
    with pytest.raises(AssertionError):
        _tri(patch_dropout=1.0)
    # nothing is dropped (and no key is drawn) in eval mode or with the flag off; a tower asked to drop on the CPU says why not
    assert d.eval().visual._drop_tokens(3) == (None, None) and e.train().visual._drop_tokens(3) == (None, None)
    state = torch.get_rng_state()
    assert d.eval().image._drop_tokens(3) == (None, None) and torch.equal(torch.get_rng_state(), state)
    with pytest.raises(RuntimeError):
        d.train().visual._drop_tokens(3)


def test_factory_honours_force_patch_dropout():
    import open_clip as oc
    with tempfile.TemporaryDirectory() as td:
        with open(os.path.join(td, "zz-tiny-drop.json"), "w") as f:
            json.dump(TINY, f)
        oc.add_model_config(td)
        try:
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                both = lambda m: (m.image.patch_dropout, m.visual.patch_dropout)
                assert both(oc.tri_create_model("zz-tiny-drop", None, device="cpu", force_patch_dropout=0.5)) == (0.5, 0.5)
                for off in (None, False, 0.0):
                    assert both(oc.tri_create_model("zz-tiny-drop", None, device="cpu", force_patch_dropout=off)) == (0.0, 0.0)
                assert both(oc.tri_create_model("zz-tiny-drop", None, device="cpu")) == (0.0, 0.0)
                m = oc.tri_create_model_and_transforms("zz-tiny-drop", None, device="cpu", force_patch_dropout=0.75)[0]
                assert both(m) == (0.75, 0.75)
                with pytest.raises(AssertionError):
                    oc.tri_create_model("zz-tiny-drop", None, device="cpu", force_patch_dropout=1.0)
                assert oc.get_model_config("zz-tiny-drop")["vision_cfg"].get("patch_dropout", 0.0) == 0.0      # the registry is not edited
        finally:
            from open_clip import factory
            factory._CONFIG_PATHS.pop()
            factory._rescan()


def test_wrappers_pass_their_false_through():
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
        with pytest.raises(KeyboardInterrupt):
            V._create(cfg.model, "cpu", cfg)
    finally:
        V.tri_create_model = orig
    assert seen["force_patch_dropout"] is False
    import open_clip
    import openshape
    seen.clear()

    def fake_tt(name, pretrained=None, **kw):
        seen.update(kw)
        raise KeyboardInterrupt
    orig = open_clip.tri_create_model_and_transforms
    open_clip.tri_create_model_and_transforms = fake_tt
    try:
        args = SimpleNamespace(clip_model="ViT-B-32", pretrained=None, precision="fp32", model=SimpleNamespace(out_channel=512))
        with pytest.raises(KeyboardInterrupt):
            openshape.CLIPBindWrap(args)
    finally:
        open_clip.tri_create_model_and_transforms = orig
    assert seen["force_patch_dropout"] is False


def test_steps_take_patch_dropout_and_drop_seed():
    from vitlens_hip import step as S
    for cls in (S.TriModalDepthStep, S.DualAudioStep, S.TriModalPCStep):
        prm = inspect.signature(cls.__init__).parameters
        assert prm["patch_dropout"].default == 0.0 and prm["drop_seed"].default == 0, cls.__name__
    prm = inspect.signature(S._StepState._init_host).parameters
    assert prm["patch_dropout"].default == 0.0 and prm["drop_seed"].default == 0

    class Host(S._StepState):           # the host half of a step: no engine, no kernel
        def __init__(self, **kw):
            self._init_host({"logit_scale": torch.tensor(2.0)}, "cpu", 4, kw.pop("rank", 0), 1, **kw)
    h = Host()
    assert (h.patch_dropout, h.drop_seed) == (0.0, 0)
    h = Host(patch_dropout=0.5, drop_seed=9)
    assert (h.patch_dropout, h.drop_seed) == (0.5, 9)
    assert Host(patch_dropout=False).patch_dropout == 0.0 and Host(patch_dropout=None).patch_dropout == 0.0
    with pytest.raises(AssertionError):
        Host(patch_dropout=1.0)
    with pytest.raises(ValueError):
        Host(patch_dropout=0.5, rank=1 << 14)


def test_sample_numbers_never_collide():
    from vitlens_hip.step import DROP_TOWER_IMAGE, DROP_TOWER_VISUAL, drop_sample0
    assert (DROP_TOWER_VISUAL, DROP_TOWER_IMAGE) == (0, 1)
    seen = set()
    steps, ranks, towers, offs = (0, 1, 2, 1000, (1 << 27) - 1), (0, 1, 7, (1 << 14) - 1), (0, 1), (0, 1, 255, 1023, (1 << 20) - 1)
    for t in steps:
        for r in ranks:
            for w in towers:
                for o in offs:
                    v = drop_sample0(t, r, w, o)
                    assert v == PR.sample0(t, r, w, o) and 0 <= v < 1 << 63
                    seen.add(v)
    assert len(seen) == len(steps) * len(ranks) * len(towers) * len(offs)
    # a micro-batch at offset o with row b is the sample at offset o + b
    assert drop_sample0(5, 1, 0, 256) + 3 == drop_sample0(5, 1, 0, 259)
    for bad in ((0, -1, 0, 0), (0, 0, 4, 0), (0, 0, 0, 1 << 20)):
        with pytest.raises(ValueError):
            drop_sample0(*bad)
