"""usage: python tools/lens_front_digest.py [TREE]     (TREE: a checkout of this repository with its library built; default: this one)
sha256 of the output bytes of the front of a Lens where bench.py does not reach it - PointTokenizerEngine / PointTokenizerEngineF32
.forward, LensEngine / LensEngineF32.encode for pc, audio, EEG and depth, LensEngine.encode with the pnsa tokenizer and for pc after
update_params with changed adapter parameters, and PointTokenizerTrainer / PNSATokenizerTrainer with train- and eval-mode BatchNorm
(tokens, every gradient, the running statistics after the step) - on seeded random parameters and inputs with fps_start given:
B = 2, N = 256, G = 16, M = 8 on a tower of width 128 with 2 layers.  Two trees that print the same lines compute the same bits:
what a refactor of the host-side forward must show (profiles/lens_front_ab.log).  A few seconds.  Not imported by the product."""
import hashlib
import os
import sys

ROOT = sys.argv[1] if len(sys.argv) > 1 else os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT + "/vit-lens_amd", ROOT + "/oracle"]
import torch  # noqa: E402

import vitlens_oracle as O  # noqa: E402
from vitlens_hip import engine as E, f32 as F, points as P  # noqa: E402

print("# tree:", E.__file__)
dev = "cuda:0"
B, N, G, M, ENC, TRANS = 2, 256, 16, 8, 64, 128
A = "t.visual_adapter."


def sha(t):
    torch.cuda.synchronize()
    return hashlib.sha256(t.detach().contiguous().view(torch.uint8).cpu().numpy().tobytes()).hexdigest()     # (bf16 too)


def pnsa_state(g, in_dim=3):
    sd, c = {}, 3 + in_dim
    rn = lambda *s, std=1.0: torch.randn(*s, generator=g) * std
    for i, o in enumerate((64, 128, ENC)):           # (channel counts in multiples of 64, as the released tokenizer's)
        sd[A + f"sa.mlp_convs.{i}.weight"] = rn(o, c, 1, 1, std=c ** -0.5); sd[A + f"sa.mlp_convs.{i}.bias"] = rn(o, std=0.1)
        sd[A + f"sa.mlp_bns.{i}.weight"] = 1.0 + rn(o, std=0.05); sd[A + f"sa.mlp_bns.{i}.bias"] = rn(o, std=0.05)
        sd[A + f"sa.mlp_bns.{i}.running_mean"] = rn(o, std=0.1); sd[A + f"sa.mlp_bns.{i}.running_var"] = 1.0 + 0.2 * torch.rand(o, generator=g)
        c = o
    sd[A + "lift.0.weight"] = rn(TRANS, ENC + 3, 1, std=(ENC + 3) ** -0.5); sd[A + "lift.0.bias"] = rn(TRANS, std=0.1)
    sd[A + "lift.2.weight"] = 1.0 + rn(TRANS, std=0.02); sd[A + "lift.2.bias"] = rn(TRANS, std=0.02)
    return sd


g = torch.Generator().manual_seed(4321)
spec = O.TowerSpec(width=128, layers=2, heads=4, patch=14, image_size=56, embed_dim=64)
tcfg = E.TowerCfg(width=128, layers=2, heads=4, patch=14, image_size=56, embed_dim=64)
tower = O.init_tower(spec, g, "t.", with_conv=False)
PERC = dict(perceiver_identity=False, depth=2, self_per_cross=1, num_latents=16, latent_dim=128, input_chan=128, cross_heads=1,
            cross_dim_head=32, latent_heads=4, latent_dim_head=32)
PC = dict(pc_num_group=G, pc_group_size=M, pc_encoder_dims=ENC, pc_trans_dim=TRANS)
pts = torch.randn(B, N, 3, generator=g).to(dev)
feats = torch.randn(B, N, 3, generator=g).to(dev)
start = torch.tensor([3, 200], device=dev)
cases = {"pc": (dict(modality="pc", **PC, **PERC), pts, dict(fps_start=start)),
         "audio": (dict(modality="audio", audio_mel_bins=34, audio_target_length=54, **PERC), torch.randn(B, 54, 34, generator=g).to(dev), {}),
         "eeg": (dict(modality="eeg", eeg_chans=8, eeg_time_len=32, eeg_window_size=2, eeg_stride=2, **PERC),
                 torch.randn(B, 8, 32, generator=g).to(dev), {}),
         "depth": (dict(modality="depth", **PERC), torch.randn(B, 1, 56, 56, generator=g).to(dev), {})}

# ---- engines
for name, (kw, x, ekw) in cases.items():
    lc = E.LensCfg(**kw)
    sd = {**tower, **O.init_lens(spec, O.LensSpec(**kw), g, "t.")}
    if name == "pc":
        pc_sd, pc_cfg = sd, lc
        print("PointTokenizerEngine.forward", sha(P.PointTokenizerEngine(sd, A, lc, dev).forward(pts, start)))
        print("PointTokenizerEngineF32.forward", sha(F.PointTokenizerEngineF32(sd, A, lc, dev).forward(pts, start)))
    le = E.LensEngine(sd, "t.", tcfg, lc, dev)
    print(f"LensEngine.encode {name}", sha(le.encode(x, **ekw)))
    print(f"LensEngine.encode {name} normalized, second call", sha(le.encode(x, normalize=True, **ekw)))
    print(f"LensEngineF32.encode {name}", sha(F.LensEngineF32(sd, "t.", tcfg, lc, dev).encode(x, **ekw)))
    # every adapter parameter (and the running statistics) changed: update_params, then the next encode
    sd2 = {k: (v * 1.25 + 0.01 if k.startswith(A) else v) for k, v in sd.items()}
    le.update_params(sd2, "t.", [k[2:] for k in sd if k.startswith(A)])
    print(f"LensEngine.encode {name} after update_params(adapter)", sha(le.encode(x, **ekw)))
    print(f"LensEngine.encode {name} of the changed parameters, built afresh", sha(E.LensEngine(sd2, "t.", tcfg, lc, dev).encode(x, **ekw)))

pn_cfg = E.LensCfg(modality="pc", pc_tokenizer="pnsa", pc_radius=0.6, pc_in_dim=3, **PC, **PERC)
pn_sd = {**tower, **{k: v for k, v in pc_sd.items() if k.startswith("t.perceiver.")}, **pnsa_state(g)}
print("LensEngine.encode pnsa", sha(E.LensEngine(pn_sd, "t.", tcfg, pn_cfg, dev).encode(feats, xyz=pts, fps_start=start)))

# ---- trainers: tokens, every gradient, the running statistics after the step
dctx = torch.randn(B * G, TRANS, generator=g).to(dev)
for bn_training in (True, False):
    for cls, sd, lc, fwd in ((P.PointTokenizerTrainer, pc_sd, pc_cfg, lambda t: t.forward(pts, start)),
                             (P.PNSATokenizerTrainer, pn_sd, pn_cfg, lambda t: t.forward(feats, xyz=pts, fps_start=start))):
        tr = cls(sd, A, lc, dev, bn_training=bn_training)
        tag = f"{cls.__name__} bn_training={bn_training}"
        print(tag, "tokens", sha(fwd(tr)))
        tr.backward(dctx)
        for k in sorted(tr.grads):
            print(tag, "grad", k, sha(tr.grads[k]))
        for k in sorted(tr.running):
            print(tag, "running", k, sha(tr.running[k][0]), sha(tr.running[k][1]))
