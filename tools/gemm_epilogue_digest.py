#!/usr/bin/env python
"""sha256 of what every epilogue of vl_gemm_bf16_ex writes, on seeded operands: one line per (shape, kernel configuration,
epilogue / act), the hash over `out` and, where the case has one, `out2`; `refused` where the library declines the
combination (a cfg whose kernel does not take the shape or the epilogue).  Two builds of the library that print the same
lines compute the same bits - what a refactor of the epilogue code must show (profiles/gemm_epilogue_digest.txt).
(512, 512, 512): whole 256x256 / 256x128 tiles, the 16-byte transposes; (300, 196, 128): partial row tile, partial column
block, N % 8 == 4 - the fp32-transpose fallback and the direct epilogues.  A few seconds.  Not imported by the product."""
import hashlib
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "vit-lens_amd"))
import torch  # noqa: E402
from vitlens_hip import ops  # noqa: E402

CFGS = (-1, 0, 1, 5, 8, 9, 10, 11)
SHAPES = ((512, 512, 512), (300, 196, 128))
# label -> (epi, act, bias, second operand, out2, res_div)
CASES = {
    "bf16": (ops.EPI_BF16, ops.ACT_NONE, True, None, False, 1),
    "bf16_nobias": (ops.EPI_BF16, ops.ACT_NONE, False, None, False, 1),
    "gelu": (ops.EPI_BF16, ops.ACT_GELU, True, None, False, 1),
    "relu": (ops.EPI_BF16, ops.ACT_RELU, True, None, False, 1),
    "gelu+pre": (ops.EPI_BF16, ops.ACT_GELU, True, None, True, 1),
    "gelu_dsave": (ops.EPI_BF16, ops.ACT_GELU_DSAVE, True, None, True, 1),
    "qgelu": (ops.EPI_BF16, ops.ACT_QGELU, True, None, False, 1),
    "qgelu_dsave": (ops.EPI_BF16, ops.ACT_QGELU_DSAVE, True, None, True, 1),
    "f32": (ops.EPI_F32, ops.ACT_NONE, True, None, False, 1),
    "res_f32": (ops.EPI_RES_F32, ops.ACT_NONE, True, "f32", False, 1),
    "res_bf16": (ops.EPI_RES_BF16, ops.ACT_NONE, True, "bf16", False, 1),
    "res_bf16_relu": (ops.EPI_RES_BF16, ops.ACT_RELU, True, "bf16", False, 1),
    "res_bf16_div2": (ops.EPI_RES_BF16, ops.ACT_NONE, True, "bf16", False, 2),
    "dgelu": (ops.EPI_DGELU, ops.ACT_NONE, False, "bf16", False, 1),
    "dgelu_saved": (ops.EPI_DGELU, ops.ACT_GELU_DSAVE, False, "bf16", False, 1),
    "dgelu_qsaved": (ops.EPI_DGELU, ops.ACT_QGELU_DSAVE, False, "bf16", False, 1),
    "geglu": (ops.EPI_GEGLU, ops.ACT_NONE, True, None, False, 1),
    "geglu+pre": (ops.EPI_GEGLU, ops.ACT_NONE, True, None, True, 1),
    "dgeglu": (ops.EPI_DGEGLU, ops.ACT_NONE, False, "h", False, 1),
}


def digest(*ts):
    m = hashlib.sha256()
    for t in ts:
        m.update(t.contiguous().cpu().view(torch.uint8).numpy().tobytes())
    return m.hexdigest()


def main():
    g = torch.Generator().manual_seed(11)
    for (M, N, K) in SHAPES:
        a = (torch.randn(M, K, generator=g) * 0.6).bfloat16().cuda()
        w = (torch.randn(N, K, generator=g) * (4.0 / K ** 0.5)).bfloat16().cuda()      # pre-activations of a few units: both GELU tails
        bias = torch.randn(N, generator=g).cuda()
        second = {"f32": torch.randn(M, N, generator=g).cuda(), "bf16": (torch.randn(M, N, generator=g) * 2.0).bfloat16().cuda(),
                  "h": (torch.randn(M, 2 * N, generator=g) * 2.0).bfloat16().cuda()}
        for cfg in CFGS:
            for label, (epi, act, has_bias, res, has_out2, res_div) in CASES.items():
                n_out = N // 2 if epi == ops.EPI_GEGLU else 2 * N if epi == ops.EPI_DGEGLU else N
                out = torch.zeros(M, n_out, device="cuda", dtype=torch.float32 if epi in (ops.EPI_F32, ops.EPI_RES_F32) else torch.bfloat16)
                out2 = torch.zeros(M, N, device="cuda", dtype=torch.bfloat16) if has_out2 else None
                r = second[res] if res else None
                if res_div > 1:
                    r = r[:(M + res_div - 1) // res_div]
                try:
                    ops.gemm(a, w, bias if has_bias else None, out=out, res=r, epi=epi, act=act, cfg=cfg, out2=out2, res_div=res_div)
                    torch.cuda.synchronize()
                    line = digest(out, out2) if has_out2 else digest(out)
                except RuntimeError:
                    line = "refused"
                print(f"{M}x{N}x{K} cfg {cfg:2d} {label:14s} {line}", flush=True)


if __name__ == "__main__":
    main()
