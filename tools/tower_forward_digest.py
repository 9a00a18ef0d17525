"""usage: python tools/tower_forward_digest.py [TREE]     (TREE: a checkout of this repository with its library built; default: this one)
sha256 of the output bytes of the tower executors bench.py does not reach - VitEngineF32.encode (image stem, depth adapter stem),
TextEngineF32.encode_text, TextEngine.encode_text in bf16x2, bf16, f16 dense and f16 packed (device and host tokens), each with
erf-GELU and QuickGELU - on seeded random parameters and inputs.  Two trees that print the same lines compute the same bits: what
a refactor of the host-side forward must show (profiles/tower_forward_ab.log).  A few seconds.  Not imported by the product."""
import hashlib
import os
import sys

ROOT = sys.argv[1] if len(sys.argv) > 1 else os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT + "/vit-lens_amd", ROOT + "/oracle"]
import torch  # noqa: E402

import vitlens_oracle as O  # noqa: E402
from vitlens_hip import engine as E, f32 as F  # noqa: E402

print("# tree:", E.__file__)


def sha(t):
    torch.cuda.synchronize()
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


g = torch.Generator().manual_seed(1234)
dev = "cuda:0"
# VitEngineF32.encode: width 128, 2 layers, B = 2
spec = O.TowerSpec(width=128, layers=2, heads=4, patch=14, image_size=56, embed_dim=64)
cfg = E.TowerCfg(width=128, layers=2, heads=4, patch=14, image_size=56, embed_dim=64)
sd = O.init_tower(spec, g, "t.")
img = torch.randn(2, 3, 56, 56, generator=g)
print("VitEngineF32.encode", sha(F.VitEngineF32(sd, "t.", cfg, dev).encode(img.to(dev))))
sd.update(O.init_lens(spec, O.LensSpec(modality="depth", perceiver_identity=True), g, "t."))
dep = torch.randn(2, 1, 56, 56, generator=g)
print("VitEngineF32.encode depth", sha(F.VitEngineF32(sd, "t.", cfg, dev, depth=True).encode(dep.to(dev), normalize=True)))

# text: width 512, 8 heads, 2 layers, B = 4, captions of lengths 3, 20, 77 and 1
ts = O.TextSpec(width=512, heads=8, layers=2, embed_dim=512)
tsd = O.init_text(ts, g)
text = torch.zeros(4, 77, dtype=torch.long)
for b, n in enumerate((3, 20, 77, 1)):
    text[b, :n - 1] = torch.randint(1, 49406, (n - 1,), generator=g)
    text[b, n - 1] = 49407
assert (text.argmax(-1) + 1).tolist() == [3, 20, 77, 1]
for quick in (False, True):
    tc = E.TextCfg(width=512, heads=8, layers=2, embed_dim=512, quick_gelu=quick)
    print(f"TextEngineF32 quick_gelu={quick}", sha(F.TextEngineF32(tsd, tc, dev).encode_text(text.to(dev))))
    for arith in ("bf16x2", "bf16"):
        eng = E.TextEngine(tsd, tc, dev, arith=arith)
        assert eng.arith == arith
        print(f"TextEngine {arith} quick_gelu={quick}", sha(eng.encode_text(text.to(dev))))
    eng = E.TextEngine(tsd, tc, dev, arith="f16")
    assert eng.arith == "f16" and E.PACK_TEXT
    print(f"TextEngine f16 dense quick_gelu={quick}", sha(eng.encode_text(text.to(dev), plan=False)))
    plan = eng.plan_text(text.to(dev))
    assert plan is not None and plan.rows == 101
    print(f"TextEngine f16 packed quick_gelu={quick}", sha(eng.encode_text(text.to(dev), plan=plan)))
    print(f"TextEngine f16 packed (host tokens, normalized) quick_gelu={quick}", sha(eng.encode_text(text, normalize=True)))
    print(f"TextEngine f16 dense again quick_gelu={quick}", sha(eng.encode_text(text.to(dev), plan=False)))
