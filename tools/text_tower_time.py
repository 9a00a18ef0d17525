#!/usr/bin/env python
"""ViT-L text tower forward for the three operand modes of TextEngine, at the text batches of the C3 / C4 / C5 steps
(1 024 / 256 / 128 captions of the benchmark's kind: 6 to 22 tokens).  The fp16 mode is timed twice: packed (only the rows
up to each caption's pooled position, engine.PACK_TEXT; the plan request and its host wait included) and dense."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "vit-lens_amd")); sys.path.insert(0, os.path.join(ROOT, "oracle"))
import torch
import vitlens_oracle as O
from vitlens_hip import engine as E

REPS = 10
g = torch.Generator().manual_seed(0)
sd = O.init_text(O.TextSpec(), g)


def timed(eng, text):
    for _ in range(2):
        eng.encode_text(text)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(REPS):
        eng.encode_text(text)
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / REPS


print(f"{'captions':>8s} {'arith':>7s} {'packed ms':>10s} {'dense ms':>10s}   rows packed / dense")
for n in (1024, 256, 128):
    text = O.synth_text(n, g).cuda()
    rows = int((text.argmax(-1) + 1).sum())
    for arith in ("f16", "bf16x2", "bf16"):
        eng = E.TextEngine(sd, E.TextCfg(), "cuda", res_dtype=torch.bfloat16, arith=arith)
        E.PACK_TEXT = True
        packed = timed(eng, text) if arith == "f16" else None          # (the other arithmetics always run dense)
        E.PACK_TEXT = False
        dense = timed(eng, text)
        E.PACK_TEXT = True
        print(f"{n:8d} {arith:>7s} {'-' if packed is None else format(packed, '10.3f'):>10s} {dense:10.3f}   {rows} / {n * 77}")
