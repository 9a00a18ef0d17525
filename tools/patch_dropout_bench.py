#!/usr/bin/env python
"""The C3 training step (ViT-L/14 tri-modal depth recipe, per-GPU batch 1024 in micro-batches of 256, bench.py's synthetic
inputs and weights) on `TriModalDepthStep` at patch dropout p = 0, 0.5, 0.75, alternated in ONE process on one step object:
ms/step, triplets/s and the algorithmic GFLOP per triplet for each p, the ratio of each p to p = 0 from the same run and
the spread of the repeated p = 0 steps -> profiles/patch_dropout_c3.json.

Every timed step is one device-synchronised window.  Switching p frees the activation stores of the other sequence length
(four micro-batches of ViT-L activations at 257 rows are 142 GB: three lengths do not fit one card side by side), so each
visit of a p starts with warm-up steps that re-allocate and are not timed.  There is no fallback: without a GPU this fails.

usage: python tools/patch_dropout_bench.py [--rounds 2] [--steps 3] [--warmup 2] [--batch 1024] [--micro-batch 256] [--out PATH]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "vit-lens_amd"))

PS = (0.0, 0.5, 0.75)


def gflop_per_triplet(Lv, Li, unlocked=4):
    """Algorithmic GFLOP of one (image, text, depth) triplet of the C3 step with Lv / Li rows (class token + kept tokens) in
    the visual / image trunk, by SURVEY section 8 (d)'s counting: 2 FLOP per multiply-add, the GEMMs and the two attention
    products of every block, attention backward at twice its forward, dX through all 24 visual blocks, dW for the unlocked
    blocks and the adapter; the tokenizers and the text tower stay dense.  Lv = Li = 257 gives the 531.3 of BASELINE.md."""
    D, layers, T, E = 1024, 24, 256, 768
    fwd = lambda L, W: L * (24 * W * W + 4 * L * W)          # qkv, out, fc, proj + QK^T, PV
    dx = lambda L, W: L * (24 * W * W + 8 * L * W)
    dw = lambda L, W: L * 24 * W * W
    pe_img, pe_depth, proj = 2 * T * 3 * 14 * 14 * D, 2 * T * 14 * 14 * D, 2 * D * E
    image = layers * fwd(Li, D) + pe_img + proj
    text = 12 * fwd(77, 768) + 2 * 768 * E
    vis_f = layers * fwd(Lv, D) + pe_depth + proj
    vis_b = layers * dx(Lv, D) + unlocked * dw(Lv, D) + pe_depth + proj
    return (image + text + vis_f + vis_b) / 1e9


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=2, help="visits of each p, alternating")
    ap.add_argument("--steps", type=int, default=3, help="timed steps per visit (rounds * steps >= 5)")
    ap.add_argument("--warmup", type=int, default=2, help="untimed steps at the start of every visit")
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--micro-batch", type=int, default=256)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "patch_dropout_c3.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("patch_dropout_bench: no GPU (this measurement has no CPU form)")
    if a.rounds * a.steps < 5:
        sys.exit("patch_dropout_bench: at least 5 timed steps per p (rounds * steps)")
    import bench
    from vitlens_hip import engine, ops, step as vstep
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    g = torch.Generator().manual_seed(1234)
    images = torch.randn(a.batch, 3, 224, 224, generator=g).to(dev)
    sd = bench.seeded_tri_weights()
    depths = torch.randn(a.batch, 1, 224, 224, generator=g).to(dev)
    texts = bench.synth_text(a.batch, g).to(dev)
    st = vstep.TriModalDepthStep(sd, engine.TowerCfg(), engine.TextCfg(), dev, micro_batch=a.micro_batch, unlock_first_n=4,
                                 frozen_res_dtype=torch.bfloat16, train_res_dtype=torch.bfloat16, patch_dropout=0.0, drop_seed=1234)
    T = st.lens.vit.T
    times = {p: [] for p in PS}
    losses = {}
    for rnd in range(a.rounds):
        for p in PS:
            st.patch_dropout = p
            for t in st.trainers:                 # the other length's activations go; this visit's warm-up allocates its own
                t.tower._saved.clear()
            st.image._ws.clear()
            torch.cuda.empty_cache()
            for _ in range(a.warmup):
                st.step(images, texts, depths)
            torch.cuda.synchronize()
            for _ in range(a.steps):
                t0 = time.perf_counter()
                loss = st.step(images, texts, depths)
                torch.cuda.synchronize()
                times[p].append((time.perf_counter() - t0) * 1e3)
            losses[p] = float(loss)
            print(f"round {rnd} p {p:4.2f}: " + " ".join(f"{x:8.2f}" for x in times[p][-a.steps:]) + f" ms   loss {losses[p]:.4f}", flush=True)
    rec = {"workload": f"C3 step, ViT-L/14, per-GPU batch {a.batch}, micro-batch {a.micro_batch}, bf16 streams, synthetic inputs",
           "device": torch.cuda.get_device_name(dev), "rounds": a.rounds, "steps_per_visit": a.steps, "warmup_per_visit": a.warmup,
           "timing": "one device-synchronised window per step; medians over all timed steps of a p", "p": {}}
    med0 = statistics.median(times[0.0])
    for p in PS:
        K = T if p == 0.0 else ops.patch_keep_count(T, p)
        med = statistics.median(times[p])
        gf = gflop_per_triplet(K + 1, K + 1)
        rec["p"][str(p)] = {"tokens_per_sample": K + 1, "ms_per_step": round(med, 3), "ms_steps": [round(x, 3) for x in times[p]],
                            "triplets_per_s": round(a.batch / med * 1e3, 2), "gflop_per_triplet": round(gf, 2),
                            "achieved_tflops": round(gf * a.batch / med, 1), "time_ratio_to_p0": round(med / med0, 4),
                            "gflop_ratio_to_p0": round(gf / gflop_per_triplet(T + 1, T + 1), 4), "last_loss": losses[p]}
        print(f"p {p:4.2f}: {K + 1:3d} tokens  {med:8.2f} ms/step  {a.batch / med * 1e3:8.1f} triplets/s  {gf:6.1f} GFLOP/triplet  "
              f"time x{med / med0:.3f} of p = 0", flush=True)
    rec["p0_spread"] = {"min_ms": round(min(times[0.0]), 3), "max_ms": round(max(times[0.0]), 3),
                        "relative": round((max(times[0.0]) - min(times[0.0])) / med0, 4)}
    print(f"p = 0 spread over {len(times[0.0])} steps: {rec['p0_spread']['min_ms']} .. {rec['p0_spread']['max_ms']} ms "
          f"({100 * rec['p0_spread']['relative']:.2f} % of the median)")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
