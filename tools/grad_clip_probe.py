"""Timing of the gradient-clipping path.

  python tools/grad_clip_probe.py optimizer
      Optimizer phase alone, on tensor lists with the depth recipe's and the audio recipe's tensor count and element total
      (51 tensors / 50.8 M, 105 tensors / 127.6 M; fp32 masters, moments and one flat gradient buffer as in the fused steps):
      the per-tensor loop (vl_adamw_step x tensors) against vl_sumsq_f32 + ONE vl_adamw_multi_step, alternated, HIP events
      around each phase, plus the sum of squares alone and a device-to-device copy of the gradients for the read bandwidth.

  python tools/grad_clip_probe.py ab OTHER_TREE [--rounds R] [--steps K] [--warmup W]
      `bench.py --gpus 1` (C3, grad_clip_norm off) as child processes alternately from this tree and from a built checkout of
      another commit (the parent): ms per step of every run, so a difference can be read against the run-to-run spread.
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def depth_shapes():
    """TriModalDepthStep at ViT-L/14, 4 unlocked blocks: logit_scale, 4 x 12 block tensors, pos_emb, conv1 as a GEMM operand."""
    D, H = 1024, 4096
    blk = [(3 * D, D), (D, D), (H, D), (D, H), (D,), (D,), (D,), (D,), (3 * D,), (D,), (H,), (D,)]
    return [(1,)] + blk * 4 + [(257, D), (D, 256)]


def audio_like_shapes():
    """105 tensors, 127.6 M elements: the audio recipe's count and total (35 matrices, 70 vectors; not its exact shapes)."""
    small = [(1,)] + [(1024,)] * 69
    left = 127_600_000 - sum(s[0] for s in small)
    rows = left // 35 // 1024
    big = [(rows, 1024)] * 34
    big.append(((left - sum(r * c for r, c in big)) // 1024, 1024))
    return small[:1] + big + small[1:]


def optimizer_phase(reps):
    sys.path.insert(0, os.path.join(ROOT, "vit-lens_amd"))
    import torch
    from vitlens_hip import ops
    from vitlens_hip.train import AdamW
    out = {}
    for name, shapes in (("depth", depth_shapes()), ("audio", audio_like_shapes())):
        params = {f"t{i}.weight" if len(s) > 1 else f"t{i}.bias": torch.randn(*s, device="cuda") * 0.02 for i, s in enumerate(shapes)}
        al = lambda n: (n + 3) // 4 * 4
        flat = torch.zeros(sum(al(p.numel()) for p in params.values()), device="cuda")
        grads, off = {}, 0
        for k, p in params.items():
            grads[k] = flat[off:off + p.numel()].view(p.shape); grads[k].normal_(); off += al(p.numel())
        opt = AdamW(params)
        sumsq = torch.zeros(1, device="cuda")
        copy = torch.empty_like(flat)

        def loop():
            opt.step(grads, grad_scale=0.125)

        def clipped():
            ops.grad_sumsq(flat, out=sumsq)
            opt.step(grads, grad_scale=0.125, max_norm=10.0, sumsq=sumsq)

        phases = {"per_tensor_loop": loop, "sumsq_plus_multi": clipped, "sumsq_alone": lambda: ops.grad_sumsq(flat, out=sumsq),
                  "d2d_copy_of_gradients": lambda: copy.copy_(flat)}
        for f in phases.values():
            f(); f()
        torch.cuda.synchronize()
        times = {k: [] for k in phases}
        for _ in range(reps):                       # alternated: one of each per round
            for k, f in phases.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(); f(); b.record(); b.synchronize()
                times[k].append(a.elapsed_time(b))
        n = sum(p.numel() for p in params.values())
        res = {"tensors": len(params), "elements": n, "reps": reps}
        for k, v in times.items():
            v = sorted(v)
            res[k] = {"median_ms": round(v[len(v) // 2], 4), "min_ms": round(v[0], 4), "max_ms": round(v[-1], 4)}
        res["sumsq_read_GBps"] = round(4 * flat.numel() / res["sumsq_alone"]["median_ms"] / 1e6, 1)
        res["copy_GBps_read_plus_write"] = round(8 * flat.numel() / res["d2d_copy_of_gradients"]["median_ms"] / 1e6, 1)
        res["adamw_multi_GBps"] = round(28 * n / (res["sumsq_plus_multi"]["median_ms"] - res["sumsq_alone"]["median_ms"]) / 1e6, 1)
        res["per_tensor_loop_GBps"] = round(28 * n / res["per_tensor_loop"]["median_ms"] / 1e6, 1)
        out[name] = res
        print(json.dumps({name: res}), flush=True)
        del params, flat, grads, opt, copy
        torch.cuda.empty_cache()
    return out


def ab(other, rounds, steps, warmup):
    runs = {"this": [], "other": []}
    for r in range(rounds):
        for tag, tree in (("this", ROOT), ("other", os.path.abspath(other))):
            p = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup)], cwd=tree,
                               capture_output=True, text=True, timeout=600)
            if p.returncode != 0:
                print(p.stdout[-2000:], p.stderr[-2000:])
                raise SystemExit(f"bench.py failed in {tree} (exit {p.returncode}): stopping")
            line = [l for l in p.stdout.splitlines() if l.startswith("{")][-1]
            j = json.loads(line)
            runs[tag].append(j["ms_per_step"])
            print(json.dumps({"round": r, "tree": tag, "ms_per_step": j["ms_per_step"], "final_loss": j.get("final_loss")}), flush=True)
    print(json.dumps({"c3_ms_per_step": runs}), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    o = sub.add_parser("optimizer"); o.add_argument("--reps", type=int, default=20)
    b = sub.add_parser("ab"); b.add_argument("other")
    b.add_argument("--rounds", type=int, default=3); b.add_argument("--steps", type=int, default=5); b.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    if a.cmd == "optimizer":
        optimizer_phase(a.reps)
    else:
        ab(a.other, a.rounds, a.steps, a.warmup)
