#!/usr/bin/env python
"""sha256 of what the two-stage column reductions write, on seeded operands: `dw` / `db` of ops.layernorm_bwd_params and `out`
of ops.colsum, one line per case, every dispatch branch of csrc/vl_colreduce.hip (the vector form of each dtype pair, the
one-column-per-thread form by column count, by a base shifted one column off its alignment, and by an fp32 dy; strided operands)
at the shapes of the tests (slab and lane edges: 3, 257, 261, 263 rows), at [1 030, 768] and at one step-sized shape per branch.
Two builds of the library that print the same lines compute the same bits - what a refactor of the reduction must show
(profiles/colreduce_digest.txt).  A few seconds.  Not imported by the product."""
import hashlib
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "vit-lens_amd"))
import torch  # noqa: E402
from vitlens_hip import ops  # noqa: E402

BF, F32 = torch.bfloat16, torch.float32
SMALL = ((3, 64), (257, 64), (261, 64), (263, 72), (1030, 768))
# (dy dtype, x dtype) -> the step-sized shape of that pair (the C3 tower's / the C4 Perceiver's LayerNorms, ln_pre)
LN_STEP = {(BF, BF): (65792, 1024), (BF, F32): (65536, 1024), (F32, F32): (65792, 1024), (F32, BF): (65792, 1024)}
SUM_STEP = {BF: (65792, 4096), F32: (65536, 1024)}


def digest(*ts):
    m = hashlib.sha256()
    for t in ts:
        m.update(t.contiguous().cpu().view(torch.uint8).numpy().tobytes())
    return m.hexdigest()


def window(rows, cols, dtype, g, how, scale=1.0, shift=0.0):
    """A seeded [rows, cols] operand: dense, a 16-byte aligned column window of a wider tensor, or one shifted by ONE column."""
    pad, c0 = {"dense": (0, 0), "strided": (16, 8), "shifted": (8, 1)}[how]
    return (torch.randn(rows, cols + pad, generator=g) * scale + shift).to(dtype).cuda()[:, c0:c0 + cols]


def ln_case(rows, D, dy_dtype, x_dtype, g, how="dense"):
    dy = window(rows, D, dy_dtype, g, how)
    x = window(rows, D, x_dtype, g, how, 2.0, 0.5)
    xh = x.cpu().float()                            # (statistics on the host: no second GPU reduction in the digest)
    mean = xh.mean(1).cuda(); rstd = (xh.var(1, unbiased=False) + 1e-5).rsqrt().cuda()
    dw = torch.full((D,), 2.0, device="cuda"); db = torch.full((D,), -1.0, device="cuda")
    ops.layernorm_bwd_params(dy, x, mean, rstd, dw, db, rows, D, x_row_stride=x.stride(0), dy_row_stride=dy.stride(0))
    return digest(dw, db)


def sum_case(rows, C, dtype, g, how="dense"):
    a = window(rows, C, dtype, g, how)
    out = torch.full((C,), -1.0, device="cuda")
    ops.colsum(a, out, 0.5)
    return digest(out)


def name(dtype):
    return "bf16" if dtype == BF else "f32"


def main():
    g = torch.Generator().manual_seed(23)
    for pair, step in LN_STEP.items():
        for rows, D in SMALL + ((41, 102), step):      # D = 102: no vector form takes it
            print(f"ln  dy {name(pair[0]):4s} x {name(pair[1]):4s} {rows:6d} x {D:4d} dense   {ln_case(rows, D, *pair, g)}", flush=True)
        for how in ("strided", "shifted"):
            print(f"ln  dy {name(pair[0]):4s} x {name(pair[1]):4s} {263:6d} x {72:4d} {how:7s} {ln_case(263, 72, *pair, g, how)}", flush=True)
    for dtype, step in SUM_STEP.items():
        for rows, C in SMALL + ((300, 100), step):
            print(f"sum a  {name(dtype):4s}        {rows:6d} x {C:4d} dense   {sum_case(rows, C, dtype, g)}", flush=True)
        for how in ("strided", "shifted"):
            print(f"sum a  {name(dtype):4s}        {263:6d} x {72:4d} {how:7s} {sum_case(263, 72, dtype, g, how)}", flush=True)


if __name__ == "__main__":
    main()
