#!/usr/bin/env python
"""Column-reduction A/B probe on the GPU box: ops.layernorm_bwd_params / ops.colsum (stage 1 + finalize, csrc/vl_colreduce.hip) on
the step-sized shapes its source comments name, one per vector form, and two shapes that take the one-column-per-thread form.
Interleaved rounds over the cases in ONE process, seeded random data, HIP-event timing of CR_CALLS back-to-back calls.  Compare
two builds by running this script once per library, alternating (profiles/colreduce_ab.log).  CR_CASES selects the cases whose
label contains it, CR_ROUNDS / CR_TAG set the rounds and a tag for the lines.  Prints one line per case:
median / min ms per call and the GB/s of the operands read."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "vit-lens_amd"))
import torch  # noqa: E402
from vitlens_hip import ops  # noqa: E402

BF, F32 = torch.bfloat16, torch.float32
# label -> (kind, rows, cols, dtype of dy / a, dtype of x, shifted one column off its alignment)
CASES = {
    "ln bf16/bf16 V8": ("ln", 65792, 1024, BF, BF, False),
    "sum bf16 V8": ("sum", 65792, 4096, BF, None, False),
    "sum f32 V4": ("sum", 65536, 1024, F32, None, False),
    "ln bf16/f32 V4": ("ln", 65536, 1024, BF, F32, False),
    "ln f32/f32 scalar": ("ln", 65792, 1024, F32, F32, False),       # ln_pre on an fp32 stream
    "sum bf16 shifted": ("sum", 65792, 1024, BF, None, True),
}


def build(kind, rows, cols, ta, tx, shifted):
    g = torch.Generator(device="cuda").manual_seed(rows + cols)
    c0 = 1 if shifted else 0
    a = torch.randn(rows, cols + 8 * c0, device="cuda", generator=g).to(ta)[:, c0:c0 + cols]
    nbytes = rows * cols * a.element_size()
    if kind == "sum":
        out = torch.zeros(cols, device="cuda")
        return (lambda: ops.colsum(a, out)), nbytes
    x = torch.randn(rows, cols, device="cuda", generator=g).to(tx)
    mean, rstd = torch.randn(rows, device="cuda", generator=g), torch.rand(rows, device="cuda", generator=g) + 0.5
    dw, db = torch.zeros(cols, device="cuda"), torch.zeros(cols, device="cuda")
    return (lambda: ops.layernorm_bwd_params(a, x, mean, rstd, dw, db, rows, cols, dy_row_stride=a.stride(0))), \
        nbytes + rows * cols * x.element_size()


def main():
    rounds, calls, tag = int(os.environ.get("CR_ROUNDS", "15")), int(os.environ.get("CR_CALLS", "4")), os.environ.get("CR_TAG", "")
    only = os.environ.get("CR_CASES", "")        # a substring of the labels to run, e.g. "ln bf16"
    fns = {label: build(*case) for label, case in CASES.items() if only in label}
    for f, _ in fns.values():
        f(); f()
    torch.cuda.synchronize()
    ts = {label: [] for label in fns}
    for _ in range(rounds):
        for label, (f, _) in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(calls):
                f()
            e1.record(); torch.cuda.synchronize()
            ts[label].append(e0.elapsed_time(e1) / calls)
    for label, (_, nbytes) in fns.items():
        v = sorted(ts[label]); med = v[len(v) // 2]
        print(f"{tag:10s} {label:18s} med {med:7.4f} ms  min {v[0]:7.4f}  {nbytes / med / 1e6:7.1f} GB/s", flush=True)


if __name__ == "__main__":
    main()
