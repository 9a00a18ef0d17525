#!/usr/bin/env python
"""What Perceiver dropout costs: the C4 training step (audio Lens <-> text, ViT-L/14, per-GPU batch 256, bench.py's synthetic
inputs and seeded weights) on two `DualAudioStep` objects in ONE process, perceiver_attn_dropout = perceiver_ff_dropout = P
against 0.0, alternated step by step, and the attention kernels of the Lens alone at the C4 shapes (cross attention: 1 head,
256 latents over 600 tokens; latent self-attention: 16 heads, 256 x 256; head dim 64) - the p = 0 entries against the dropout
entries, forward and backward.  Prints a log (profiles/perceiver_dropout_ab.log holds one).  No fallback: without a GPU this
fails.

usage: python tools/perceiver_dropout_probe.py [--p 0.1] [--steps 6] [--warmup 2] [--batch 256] [--reps 20] [--digest]"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "vit-lens_amd"))


def kernel_ms(fn, reps):
    import torch
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return statistics.median(ts)


class AttnProblem:
    """Seeded bf16 operands of one attention shape in the trainer's layout (q, dO token-major, k | v packed) and the buffers of
    its forward and backward."""

    def __init__(self, B, H, Lq, Lk, dh, seed=1):
        import torch
        from vitlens_hip import ops
        BF, dev, self.inner = torch.bfloat16, "cuda", H * dh
        g = torch.Generator().manual_seed(seed)
        q2 = torch.randn(B * Lq, self.inner, generator=g).to(BF).to(dev)
        kv2 = torch.randn(B * Lk, 2 * self.inner, generator=g).to(BF).to(dev)
        dO2 = torch.randn(B * Lq, self.inner, generator=g).to(BF).to(dev)
        hv = lambda t, L, *off: ops.heads_view(t, B, L, H, dh, *off)
        self.q, self.k, self.v, self.dO = hv(q2, Lq), hv(kv2, Lk), hv(kv2, Lk, self.inner), hv(dO2, Lq)
        self.out, self.lse = torch.empty(B * Lq, self.inner, device=dev, dtype=BF), torch.empty(B, H, Lq, device=dev)
        self.delta, self.dq, self.dkv = torch.empty(B, H, Lq, device=dev), torch.empty_like(q2), torch.empty_like(kv2)
        self.o, self.qs, self.ops = hv(self.out, Lq), dh ** -0.5 * ops.LOG2E, ops

    def fwd(self, p=0.0):
        if p:
            return self.ops.attn_fwd_drop(self.q, self.k, self.v, self.out, p, 1, 2, 3, lse=self.lse, qscale=self.qs)
        return self.ops.attn_fwd(self.q, self.k, self.v, self.out, lse=self.lse, qscale=self.qs)

    def bwd(self, p=0.0, **kw):
        i = self.inner
        args = (self.q, self.k, self.v, self.dO, self.o, self.lse, self.delta, self.dq, self.dkv, self.dkv[:, i:], i, 2 * i)
        return self.ops.attn_bwd_drop(*args, p, 1, 2, 3) if p else self.ops.attn_bwd(*args, **kw)


def attention_times(B, H, Lq, Lk, dh, p, reps):
    """(forward p = 0, forward dropout, backward p = 0 as the trainer runs it, backward two-kernel p = 0, backward dropout) in ms."""
    a = AttnProblem(B, H, Lq, Lk, dh)
    a.fwd()
    return (kernel_ms(a.fwd, reps), kernel_ms(lambda: a.fwd(p), reps), kernel_ms(a.bwd, reps),
            kernel_ms(lambda: a.bwd(fused=False), reps), kernel_ms(lambda: a.bwd(p), reps))


def digests(shapes):
    """sha256 of dq, dk, dv, delta of the two-kernel backward, under dropout and at p = 0, for every (name, B, H, Lq, Lk, dh, p):
    what two builds of the library must agree on bit for bit."""
    import hashlib
    import torch
    for name, B, H, Lq, Lk, dh, p in shapes:
        a = AttnProblem(B, H, Lq, Lk, dh)
        for pp, kw in ((p, {}), (0.0, dict(fused=False))):
            for t in (a.dq, a.dkv, a.delta):
                t.fill_(float("nan"))
            a.fwd(pp); a.bwd(pp, **kw)
            torch.cuda.synchronize()
            i = a.inner
            sha = lambda t: hashlib.sha256(t.contiguous().cpu().view(torch.uint8).numpy().tobytes()).hexdigest()[:16]
            print(f"digest {name} B{B} H{H} {Lq}x{Lk} dh{dh} p={pp:.2f}: dq {sha(a.dq)} dk {sha(a.dkv[:, :i])} dv {sha(a.dkv[:, i:])} "
                  f"delta {sha(a.delta)}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--p", type=float, default=0.1)
    ap.add_argument("--steps", type=int, default=6, help="timed steps of each setting, alternating")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--reps", type=int, default=20, help="timed launches per kernel")
    ap.add_argument("--digest", action="store_true", help="digests of the attention backward's results (the ATTN_CASES of "
                    "tests/perceiver_drop_ref.py and the two C4 shapes) and the kernel rows; no training step")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("perceiver_dropout_probe: no GPU (this measurement has no CPU form)")
    import bench
    import open_clip
    from mm_vit_lens.model_cfg import fetch_model_cfg
    from vitlens_hip import engine, step as vstep
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    print(f"device: {torch.cuda.get_device_name(dev)}; C4 step, per-GPU batch {a.batch} in one micro-batch, bf16 streams, p = {a.p}")
    c4 = (("cross attention, 1 head, 256 x 600", (1, 256, 600)), ("latent self-attention, 16 heads, 256 x 256", (16, 256, 256)))
    if a.digest:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        from perceiver_drop_ref import ATTN_CASES
        digests([(n, *c[:6]) for n, c in ATTN_CASES.items()] + [(f"C4 {n.split(',')[0]}", a.batch, H, Lq, Lk, 64, a.p) for n, (H, Lq, Lk) in c4])
    for name, (H, Lq, Lk) in c4:
        f0, fd, b0, b2, bd = attention_times(a.batch, H, Lq, Lk, 64, a.p, a.reps)
        print(f"{name}, B = {a.batch}, median of {a.reps} launches:")
        print(f"  forward   p = 0 {f0:8.3f} ms   dropout {fd:8.3f} ms   x{fd / f0:.2f}")
        print(f"  backward  p = 0 {b0:8.3f} ms (as the trainer runs it)   two-kernel p = 0 {b2:8.3f} ms   dropout {bd:8.3f} ms   "
              f"x{bd / b0:.2f} of the trainer's, x{bd / b2:.2f} of the two-kernel")
    if a.digest:
        return
    g = torch.Generator().manual_seed(1234)
    torch.manual_seed(1234)
    model = open_clip.tri_create_model("ViT-L-14", None, device="cpu", args=fetch_model_cfg(modality="audio"))
    sd = {k: v.detach() for k, v in model.state_dict().items()}
    tower_cfg, lens_cfg = model.visual._cfgs()
    del model
    texts = bench.synth_text(a.batch, g).to(dev)
    audio = (torch.randn(a.batch, 512, 128, generator=g) * 0.5).to(dev)
    mk = lambda p: vstep.DualAudioStep(sd, tower_cfg, engine.TextCfg(), lens_cfg, dev, micro_batch=a.batch,
                                       frozen_res_dtype=torch.bfloat16, train_res_dtype=torch.bfloat16, drop_seed=1234,
                                       perceiver_attn_dropout=p, perceiver_ff_dropout=p)
    steps = {0.0: mk(0.0), a.p: mk(a.p)}
    times = {p: [] for p in steps}
    for p, st in steps.items():
        for _ in range(a.warmup):
            st.step(audio, texts)
    torch.cuda.synchronize()
    for _ in range(a.steps):
        for p, st in steps.items():
            t0 = time.perf_counter()
            loss = st.step(audio, texts)
            torch.cuda.synchronize()
            times[p].append((time.perf_counter() - t0) * 1e3)
    for p in steps:
        print(f"step p = {p:4.2f}: " + " ".join(f"{x:8.2f}" for x in times[p]) + f" ms   median {statistics.median(times[p]):8.2f}")
    m0, mp = statistics.median(times[0.0]), statistics.median(times[a.p])
    print(f"per-step cost of pa = pf = {a.p}: {mp - m0:+.2f} ms on {m0:.2f} ms ({100 * (mp - m0) / m0:+.2f} %); "
          f"spread of the p = 0 steps {max(times[0.0]) - min(times[0.0]):.2f} ms")


if __name__ == "__main__":
    main()
