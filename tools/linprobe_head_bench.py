"""Time one step of the linear-probe head (forward + backward + LARS, from given features) on the HIP kernels against the same
step written with torch ops on the GPU:  python tools/linprobe_head_bench.py [--out FILE] [--iters N].

Device events around `iters` consecutive steps after a warm-up of every shape, the two versions alternated over `rounds`
rounds; per version the median round is reported with the spread.  The torch version reads its two norms on the device too
(torch.where, as the reference's LARS does), so neither side synchronises inside the timed window."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "vit-lens_amd"))


def torch_step(st, feat, target, lr, wd=1e-4, momentum=0.9, trust=1e-3, eps=1e-6, bn_momentum=0.1):
    B = feat.shape[0]
    mean = feat.mean(0)
    var = feat.var(0, unbiased=False)
    xhat = (feat - mean) * torch.rsqrt(var + eps)
    st["rm"].mul_(1 - bn_momentum).add_(mean, alpha=bn_momentum)
    st["rv"].mul_(1 - bn_momentum).add_(var, alpha=bn_momentum * B / (B - 1))
    logits = torch.addmm(st["b"], xhat, st["w"].t())
    lse = torch.logsumexp(logits, dim=1)
    loss = (lse - logits.gather(1, target[:, None])[:, 0]).mean()
    G = torch.exp(logits - lse[:, None])
    G[torch.arange(B, device=feat.device), target] -= 1.0
    G /= B
    dw, db = G.t() @ xhat, G.sum(0)
    dp = dw.add(st["w"], alpha=wd)
    pn, un = torch.norm(st["w"]), torch.norm(dp)
    one = torch.ones_like(pn)
    q = torch.where(pn > 0.0, torch.where(un > 0, trust * pn / un, one), one)
    st["mu_w"].mul_(momentum).add_(dp.mul(q))
    st["w"].add_(st["mu_w"], alpha=-lr)
    st["mu_b"].mul_(momentum).add_(db)
    st["b"].add_(st["mu_b"], alpha=-lr)
    return loss


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / iters          # microseconds per step


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("linprobe_head_bench needs a GPU")
    from vitlens_hip.linprobe import ProbeHead
    dev, lr = "cuda", 0.1
    out = {"device": torch.cuda.get_device_name(0), "iters": a.iters, "rounds": a.rounds, "unit": "microseconds per head step", "shapes": {}}
    for B, D, C in ((1024, 1024, 1000), (1024, 1024, 2)):
        g = torch.Generator().manual_seed(0)
        feat = (torch.randn(B, D, generator=g) + 0.5).to(dev)
        target = torch.randint(0, C, (B,), generator=g).to(dev)
        w0, b0 = torch.randn(C, D, generator=g) * 0.02, torch.zeros(C)
        head = ProbeHead(D, C, dev, weight=w0, bias=b0, weight_decay=1e-4)
        st = dict(w=w0.to(dev), b=b0.to(dev), mu_w=torch.zeros(C, D, device=dev), mu_b=torch.zeros(C, device=dev),
                  rm=torch.zeros(D, device=dev), rv=torch.ones(D, device=dev))

        def hip():
            head.backward(head.forward(feat, True), target)
            head.optimizer_step(lr)

        def tch():
            torch_step(st, feat, target, lr)
        for _ in range(20):
            hip(); tch()
        torch.cuda.synchronize()
        drift = float((head.weight - st["w"]).abs().max() / st["w"].abs().max())          # the two versions compute the same step
        t_hip, t_tch = [], []
        for _ in range(a.rounds):
            t_hip.append(timed(hip, a.iters)); t_tch.append(timed(tch, a.iters))
        med = lambda v: sorted(v)[len(v) // 2]
        out["shapes"][f"B{B}_D{D}_C{C}"] = {
            "hip_us": med(t_hip), "hip_min_max_us": [min(t_hip), max(t_hip)], "torch_us": med(t_tch),
            "torch_min_max_us": [min(t_tch), max(t_tch)], "torch_over_hip": med(t_tch) / med(t_hip),
            "weight_rel_diff_after_warmup": drift}
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
