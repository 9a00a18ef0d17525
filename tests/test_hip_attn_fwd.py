"""Attention forward (vl_attn_fwd_bf16 / _f16 / _f32 through ops.attn_fwd / ops.attn_fwd_f32) against float64 on every dispatch
branch, block by block.

Every case embeds its operands in larger NaN-filled allocations (packed [tokens, 3*width], q + packed k|v, or contiguous
heads with NaN rows behind the Lk rows of every head), writes into NaN-filled out / lse with guard rows on both sides, and
asserts: owned elements finite, guards bit-unchanged, out within tolerance in every (b, h, 32-query tile) block (the rows beyond
whole tiles are a block of their own), lse row by row, a second launch bit-identical, and that the per-block check does fail on
the kernel's own output once its last row block is scaled by 1 + 3 tol.  The reference is tests/attn_ref.py's attn_fwd_ref
(float64 on the GPU); every tolerance is a stated multiple of attn_fwd_model's distance from it (pinned on the CPU by
test_attn_ref_host.py), never of what the kernels give.

Case -> template instantiation <DH, TAILQ, MULTI, F16, DMA> (the id of every case ends in it; expected_branch restates the
dispatch of vl_attn.hip and test_attn_ref_host.py checks that every instantiation is covered):

  bf16, dh 64, Lk <= 288, Lq % 32 != 1 or Lq > 257 or causal with Lk > Lq      64/tiles/dma    <64, 0, 0, 0, 1>
  bf16, dh 64, Lk <= 288, Lq = 33 .. 257 step 32 (not causal with Lk > Lq)     64/lone/dma     <64, 1, 0, 0, 1>
  bf16, dh 64, Lk > 288                                                        64/multi        <64, 0, 1, 0, 0>
  bf16, dh 32: the same three conditions                                       32/tiles, 32/lone, 32/multi      (no DMA)
  bf16, dh 72 .. 128 (zero-padded to 128)                                      128/tiles, 128/lone, 128/multi   (no DMA)
  fp16, dh 64, Lk <= 288 (257 queries: a ninth tile in a second workgroup)     64/f16          <64, 0, 0, 1, 0>
  f32 (attn_f32_kernel<32 / 64>, one thread per query)                         f32/32, f32/64
Large scores (ramp, descend, negative, sink_first, sink_last, straddle) run on every one of them (straddle not on every <128, *, *>:
dh 104 runs it on the lone-row one only).
"""
import math

import pytest
import torch

import attn_ref as A

pytestmark = pytest.mark.gpu

BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
DT_NAME = {BF16: "bf16", F16: "fp16", F32: "f32"}

# ---- tolerances: (model, from the CPU: test_attn_ref_host.py pins it) x (factor of the issue); measured on the MI355X beside ----
# out, per (b, h, 32-query tile) block: 2 x the model's worst block of the family.  The factor pays for what the model leaves
# out: fp32 MFMA accumulation, v_exp_f32, P rounded relative to the lazily kept m_run instead of the true maximum.
MODEL_BLK = {BF16: 2.82e-3,     # one query against 257 keys, normal
             F16: 3.41e-4}      # L = 257, dh 32, normal (the lone row)
TOL_OUT = {BF16: 2 * MODEL_BLK[BF16],       # 5.64e-3; measured 3.24e-3 (negative, L = 257 causal, the lone row)
           F16: 2 * MODEL_BLK[F16]}         # 6.82e-4; measured 3.91e-4 (text tower geometry, causal)
# f32: the model is float32 arithmetic throughout and its error depends on the size of the scores, hence per score kind: the
# model's worst block over the f32 cases below, on their own inputs.  (A first table from one seed per geometry put ramp at
# 7.5e-6; the model's worst block is a one-row block whose error varies 2x from seed to seed, and on the inputs of ramp
# L = 257 the model itself is off by 1.52e-5 - as is the kernel, to four digits.)  Measured on the MI355X: normal 6.8e-7,
# ramp 1.52e-5, negative 2.23e-5, sink_last 4.2e-7 - the kernel reproduces the float32 model.
MODEL_BLK_F32 = {"normal": 5.12e-7, "ramp": 1.52e-5, "negative": 2.23e-5, "sink_last": 2.72e-7}
TOL_OUT_F32 = {k: 2 * e for k, e in MODEL_BLK_F32.items()}
# lse, per row, absolute: 8 x the worst row of the model's lse (scores from a float32 matmul) for the score kind, and no less
# than 4 ulp of fp32 at the largest |lse| of the case (m_run accumulated over several shifts, __log2f).  The bf16 / fp16
# scores of negative, sink_* and straddle are exact in fp32, so there the ulp term rules.
MODEL_LSE = {(BF16, "normal"): 3.19e-7, (BF16, "ramp"): 1.16e-4, (BF16, "descend"): 1.13e-4, (BF16, "negative"): 4.53e-6,
             (BF16, "sink_first"): 2.84e-11, (BF16, "sink_last"): 2.40e-8, (BF16, "straddle"): 0.0,
             (F16, "normal"): 9.41e-7, (F16, "ramp"): 2.83e-4, (F16, "descend"): 2.30e-4, (F16, "negative"): 5.14e-6,
             (F16, "sink_first"): 7.09e-11, (F16, "sink_last"): 3.85e-8, (F16, "straddle"): 0.0,
             (F32, "normal"): 6.33e-7, (F32, "ramp"): 1.83e-4, (F32, "negative"): 6.21e-5, (F32, "sink_last"): 7.81e-7}
# measured on the MI355X, worst row as a fraction of its tolerance: bf16 normal 1.18e-6 (0.46, dh 104, 600 keys), sink_last
# 1.56e-6 (0.41, bench geometry), straddle 9.1e-6 (0.30, 600 keys), ramp 1.4e-4 (0.14); fp16 sink_last 1.44e-6 (0.38), normal
# 9.7e-7 (0.13); f32 normal 1.45e-6 (0.29), sink_last 1.35e-6 (0.23), ramp 1.8e-4 (0.06)
LSE_FACTOR = 8
LSE_ULPS = 4

KC, NWMAX = 288, 8          # keys per LDS chunk, query waves per workgroup (vl_attn.hip)
GUARD = 8                   # guard rows around out and around every token-major operand
PAD = 5                     # NaN rows behind the L rows of every head in the heads layout


def expected_branch(dtype, Lq, Lk, dh, causal):
    """The instantiation vl_attn_fwd_bf16 / _f16 / _f32 dispatches, restated from vl_attn.hip / vl_f32.hip."""
    if dtype == F32:
        return f"f32/{dh}"
    if dtype == F16:
        return "64/f16"
    DH = dh if dh in (32, 64) else 128
    lone = Lq % 32 == 1 and Lq > 32 and Lq - 1 <= NWMAX * 32 and Lk <= KC and (not causal or Lk <= Lq)
    if lone:
        return f"{DH}/lone" + ("/dma" if DH == 64 else "")
    if Lk > KC:
        return f"{DH}/multi"
    return f"{DH}/tiles" + ("/dma" if DH == 64 else "")


def _case(dtype, kind, Lq, Lk, dh=64, causal=False, layout=None, B=2, H=3):
    if layout is None:
        layout = "qkv" if Lq == Lk else ("kv" if (Lq + Lk) % 2 else "heads")
    name = f"{DT_NAME[dtype]}-{kind}-{Lq}x{Lk}-dh{dh}-{'causal' if causal else 'full'}-{layout}-B{B}H{H}"
    return pytest.param(dtype, kind, B, H, Lq, Lk, dh, causal, layout, id=f"{name}[{expected_branch(dtype, Lq, Lk, dh, causal)}]")


LARGE = ("ramp", "descend", "negative", "sink_first", "sink_last", "straddle")


def _cases():
    c = []
    n = lambda *a, **k: c.append(_case(BF16, "normal", *a, **k))
    # DMA, whole tiles
    for L in (1, 31, 32, 63, 64, 256, 288):
        n(L, L)
    for Lq, Lk in ((289, 64), (321, 100), (600, 100), (64, 257), (64, 1)):
        n(Lq, Lk)
    n(64, 257, layout="heads")
    # DMA + lone row
    for L in (33, 65, 97, 129, 161, 193, 225, 257):
        n(L, L)
    for Lq in (257, 33):
        for Lk in (1, 7, 32, 33, 129, 288):
            if Lq != Lk:
                n(Lq, Lk)
    n(257, 129, layout="kv")
    # several key chunks
    for Lk in (289, 576, 577, 600):
        for Lq in (64, 256, 257):
            n(Lq, Lk)
    n(600, 600)
    n(321, 321)
    # head dim 32 and the padded head dims
    for dh in (32, 72, 80, 104, 128):
        n(257, 257, dh)
        n(256, 256, dh)
        n(50, 50, dh)
        n(64, 600, dh)
    # causal
    for L in (1, 31, 32, 33, 63, 64, 65, 77, 129, 225, 256, 257, 288, 289, 321, 600):
        n(L, L, causal=True)
    n(257, 129, causal=True)        # lone row
    n(129, 257, causal=True)        # Lk > Lq: the lone row is refused
    n(64, 600, causal=True)
    n(600, 100, causal=True)
    for dh in (32, 104):
        n(257, 257, dh, causal=True)
        n(600, 600, dh, causal=True)
    # fp16
    for causal in (False, True):
        for L in (1, 20, 77, 256, 257, 288):
            c.append(_case(F16, "normal", L, L, causal=causal))
        c.append(_case(F16, "normal", 600, 100, causal=causal))
        c.append(_case(F16, "normal", 64, 257, causal=causal))
    # score kinds
    for kind in LARGE:
        c.append(_case(BF16, kind, 257, 257))
        c.append(_case(F16, kind, 257, 257))
        c.append(_case(BF16, kind, 257, 257, causal=True))
        c.append(_case(F16, kind, 77, 77, causal=True))
        c.append(_case(BF16, kind, 64, 600))
        c.append(_case(BF16, kind, 257, 600))
        c.append(_case(BF16, kind, 257, 257, 32))
        c.append(_case(BF16, kind, 257, 257, 104))
    for kind in ("ramp", "sink_last", "straddle"):          # the remaining instantiations under large scores
        c.append(_case(BF16, kind, 256, 256))
        c.append(_case(BF16, kind, 600, 600, causal=True))
        c.append(_case(BF16, kind, 256, 256, 32))
        c.append(_case(BF16, kind, 64, 600, 32))
        if kind != "straddle":
            c.append(_case(BF16, kind, 256, 256, 104))
            c.append(_case(BF16, kind, 64, 600, 104))
    # bench geometry (C3: ViT-L/14 image tower, micro-batch 256; the 65-sample remainder; the text tower)
    c.append(_case(BF16, "normal", 257, 257, B=256, H=16))
    c.append(_case(BF16, "sink_last", 257, 257, B=256, H=16))
    c.append(_case(BF16, "normal", 257, 257, B=65, H=16))
    c.append(_case(BF16, "normal", 257, 257, causal=True, B=65, H=16))
    c.append(_case(F16, "normal", 77, 77, causal=True, B=256, H=12))
    # true fp32
    for kind in ("normal", "ramp", "negative", "sink_last"):
        for L in (1, 50, 257, 300):
            for causal in (False, True):
                for dh in (32, 64):
                    c.append(_case(F32, kind, L, L, dh, causal=causal))
    return c


CASES = _cases()


def _token_major(t):
    B, H, L, dh = t.shape
    return t.permute(0, 2, 1, 3).reshape(B * L, H * dh)


def _embed(q, k, v, layout):
    """The three operands as strided [B, H, L, dh] views into NaN-filled device allocations (see the module docstring)."""
    from vitlens_hip import ops
    B, H, Lq, dh = q.shape
    Lk, D, dt = k.shape[2], H * dh, q.dtype
    nan = float("nan")
    if layout == "qkv":
        assert Lq == Lk
        buf = torch.full((B * Lq + 2 * GUARD, 3 * D), nan, dtype=dt, device="cuda")
        own = buf[GUARD:GUARD + B * Lq]
        for i, t in enumerate((q, k, v)):
            own[:, i * D:(i + 1) * D] = _token_major(t).cuda()
        return tuple(ops.heads_view(own, B, Lq, H, dh, i * D) for i in range(3))
    if layout == "kv":
        qb = torch.full((B * Lq + 2 * GUARD, D), nan, dtype=dt, device="cuda")
        kvb = torch.full((B * Lk + 2 * GUARD, 2 * D), nan, dtype=dt, device="cuda")
        qo, kvo = qb[GUARD:GUARD + B * Lq], kvb[GUARD:GUARD + B * Lk]
        qo.copy_(_token_major(q))
        kvo[:, :D] = _token_major(k).cuda()
        kvo[:, D:] = _token_major(v).cuda()
        return ops.heads_view(qo, B, Lq, H, dh), ops.heads_view(kvo, B, Lk, H, dh), ops.heads_view(kvo, B, Lk, H, dh, D)
    assert layout == "heads"
    views = []
    for t in (q, k, v):
        L = t.shape[2]
        buf = torch.full((B, H, L + PAD, dh), nan, dtype=dt, device="cuda")
        buf[:, :, :L] = t.cuda()
        views.append(buf[:, :, :L])
    return tuple(views)


def _guarded(rows, cols, dtype):
    buf = torch.full((rows + 2 * GUARD, cols), float("nan"), dtype=dtype, device="cuda")
    return buf, buf[GUARD:GUARD + rows]


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def _launch(dtype, q, k, v, out, lse, causal, qscale):
    from vitlens_hip import ops
    if dtype == F32:
        ops.attn_fwd_f32(q, k, v, out, lse=lse, causal=causal, scale=qscale)
    else:
        ops.attn_fwd(q, k, v, out, lse=lse, causal=causal, qscale=qscale)


def _nan_prefill(B, H, Lq):
    """Best effort: the same bf16 dh-64 kernel once on all-NaN K and V with 288 keys into a scratch output, so that the LDS rows
    the case proper does not fetch are likely to hold NaN patterns (K garbage must be masked, V garbage zeroed)."""
    from vitlens_hip import ops
    q = torch.zeros(B, H, Lq, 64, dtype=BF16, device="cuda")
    kv = torch.full((2, B, H, KC, 64), float("nan"), dtype=BF16, device="cuda")
    ops.attn_fwd(q, kv[0], kv[1], torch.empty(B * Lq, H * 64, dtype=BF16, device="cuda"), qscale=1.0)


def case_seed(Lq, Lk, dh):
    return 1000 * Lq + Lk + dh


def _ulps(x):
    return LSE_ULPS * 2.0 ** (math.floor(math.log2(max(x, 1e-30))) - 23)


def run_case(dtype, kind, B, H, Lq, Lk, dh, causal, layout):
    """Runs one case and asserts everything the module docstring lists.  Returns (worst block error, worst lse row error)."""
    from errloc import assert_attn_blocks, attn_block_relerr
    log2 = dtype != F32
    q, k, v, qscale = A.make_scores(kind, B, H, Lq, Lk, dh, seed=case_seed(Lq, Lk, dh), dtype=dtype)
    if not log2 and kind == "normal":
        qscale /= A.LOG2E                                    # vl_attn_fwd_f32 takes the natural-log softmax scale
    q, k, v = _embed(q, k, v, layout)
    D = H * dh
    out_buf, out = _guarded(B * Lq, D, dtype)
    lse_buf, lse2 = _guarded(B * H, Lq, F32)
    lse = lse2.view(B, H, Lq)
    guards = [(b, _bits(b[:GUARD]).clone(), _bits(b[-GUARD:]).clone()) for b in (out_buf, lse_buf)]
    if dtype == BF16 and dh == 64 and Lk <= KC and Lk % 32:
        _nan_prefill(B, H, Lq)
    _launch(dtype, q, k, v, out, lse, causal, qscale)
    torch.cuda.synchronize()
    out1, lse1 = out.clone(), lse.clone()
    assert bool(torch.isfinite(out1).all()), "out has non-finite elements"
    assert bool(torch.isfinite(lse1).all()), "lse has non-finite elements"
    out.fill_(float("nan")); lse.fill_(float("nan"))
    _launch(dtype, q, k, v, out, lse, causal, qscale)
    torch.cuda.synchronize()
    assert torch.equal(_bits(out), _bits(out1)) and torch.equal(_bits(lse), _bits(lse1)), "a second launch differs"
    for buf, lo, hi in guards:
        assert torch.equal(_bits(buf[:GUARD]), lo) and torch.equal(_bits(buf[-GUARD:]), hi), "guard rows were written"

    ref, ref_lse = A.attn_fwd_ref(q, k, v, qscale, causal, dtype, log2)
    tol = TOL_OUT_F32[kind] if dtype == F32 else TOL_OUT[dtype]
    what = f"out ({DT_NAME[dtype]}, {kind})"
    blk, (wb, wh, w0, w1) = attn_block_relerr(out1, ref, B, H, Lq)
    d = (lse1.double() - ref_lse).abs()
    i = int(d.argmax())
    lse_err, lse_max = float(d.reshape(-1)[i]), float(ref_lse.abs().max())
    lse_tol = max(LSE_FACTOR * MODEL_LSE[(dtype, kind)], _ulps(lse_max))
    print(f"ATTNFWD blk {blk:.3e} tol {tol:.2e} lse {lse_err:.3e} tol {lse_tol:.2e} |lse| {lse_max:.1f}")
    assert blk <= tol, f"{what}: b={wb} h={wh} queries {w0}:{w1} has relative error {blk:.3e} > {tol:.1e}"
    b, r = divmod(i, H * Lq)
    assert lse_err <= lse_tol, f"lse: b={b} h={r // Lq} query {r % Lq} is off by {lse_err:.3e} > {lse_tol:.2e} (|lse| up to {lse_max:.1f})"

    # the per-block check can fail on this very output: the last row block of the (b, h) where it carries the most
    r0 = 32 * ((Lq - 1) // 32)
    e = ref[:, :, r0:Lq].pow(2).sum((-1, -2))
    b, h = divmod(int(e.argmax()), H)
    m = out1.clone()
    m.view(B, Lq, H, dh)[b, r0:Lq, h] *= 1 + 3 * tol
    with pytest.raises(AssertionError, match=f"b={b} h={h} queries {r0}:{Lq} "):
        assert_attn_blocks(m, ref, tol, B, H, Lq, "queries", what=what)
    return blk, lse_err


@pytest.mark.parametrize("dtype,kind,B,H,Lq,Lk,dh,causal,layout", CASES)
def test_attn_fwd_blocks(dtype, kind, B, H, Lq, Lk, dh, causal, layout):
    run_case(dtype, kind, B, H, Lq, Lk, dh, causal, layout)


def _refused(call, out, exc=RuntimeError):
    with pytest.raises(exc):
        call()
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()), "a refused call wrote to out"


def test_attn_fwd_bf16_refusals_launch_nothing():
    """Head dim 48, a row stride that is not a multiple of 8 elements, a base that is not 16-byte aligned and an empty problem
    are errors, and out stays NaN."""
    from vitlens_hip import ops
    B, H, L = 2, 2, 40
    nan = float("nan")
    mk = lambda dh, extra=0: torch.randn(B, H, L, dh + extra, device="cuda").to(BF16)
    out = torch.full((B * L, H * 64), nan, dtype=BF16, device="cuda")
    t48 = mk(48)
    _refused(lambda: ops.attn_fwd(t48, t48, t48, out), out)
    odd = mk(64, 4)[..., :64]                                               # row stride 68
    good = mk(64)
    for trio in ((odd, good, good), (good, odd, good), (good, good, odd)):
        _refused(lambda: ops.attn_fwd(*trio, out), out)
    flat = torch.randn(B * H * L * 64 + 8, device="cuda").to(BF16)
    off = flat[4:4 + B * H * L * 64].view(B, H, L, 64)                      # base 8 bytes into a 16-byte unit
    for trio in ((off, good, good), (good, off, good), (good, good, off)):
        _refused(lambda: ops.attn_fwd(*trio, out), out)
    empty = good[:, :, :0]
    _refused(lambda: ops.attn_fwd(good, empty, empty, out), out)


def test_attn_fwd_f16_refusals_launch_nothing():
    """The half entry takes head dim 64 and at most 288 keys of one operand type; anything else is an error, out stays NaN."""
    from vitlens_hip import ops
    B, H, L = 2, 2, 40
    nan = float("nan")
    mk = lambda L, dh, dt=F16: torch.randn(B, H, L, dh, device="cuda").to(dt)
    out = torch.full((B * L, H * 64), nan, dtype=F16, device="cuda")
    q32 = mk(L, 32)
    _refused(lambda: ops.attn_fwd(q32, q32, q32, out), out)
    q, k289 = mk(L, 64), mk(289, 64)
    _refused(lambda: ops.attn_fwd(q, k289, k289, out), out)
    kb = mk(L, 64, BF16)
    _refused(lambda: ops.attn_fwd(q, kb, kb, out), out, (RuntimeError, ValueError, TypeError))
    _refused(lambda: ops.attn_fwd(q, q, kb, out), out, (RuntimeError, ValueError, TypeError))
    outb = torch.full((B * L, H * 64), nan, dtype=BF16, device="cuda")
    _refused(lambda: ops.attn_fwd(q, q, q, outb), outb, (RuntimeError, ValueError, TypeError))
