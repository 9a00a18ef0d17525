"""CPU: which kernels a tower enqueues in each of its four arithmetics - bf16 (LayerNorm passes, not folded), IEEE half, two-term
bf16 ("bf16x2") and fp32 - recorded instead of executed (launch_trace.py), through VitEngine.trunk, VitEngineF32.trunk / .encode,
TextEngine.encode_text (dense) and TextEngineF32.encode_text.  The plan of one block and of each head is written out below;
every executor's plan is stem + blocks x layers + head, the fp16 and fp32 plans are the bf16 plan kernel for kernel, and the
two-term plan writes every LayerNorm twice and runs every residual projection as two launches.  (The LayerNorm-folded and
pruned bf16 plans: test_block_plan_host.py.  The packed fp16 text path sizes its launches from the data and needs a GPU:
test_hip_text_pack.py.)"""
import pytest
import torch

import vitlens_oracle as O
from launch_trace import recording, symbols

LAYERS, B = 2, 2
TEXT_B, CTX, TEXT_D, TEXT_H, VOCAB = 4, 77, 512, 8, 1000
VIT_D, VIT_H, IMG, PATCH, EMBED = 128, 4, 56, 14, 64

LN, GEMM, ATTN = "vl_layernorm_fwd", "vl_gemm_bf16_ex", "vl_attn_fwd_bf16"
# one pre-LN block with the LayerNorm passes: ln_1, in-projection, attention, out-projection + residual, ln_2, c_fc + activation,
# c_proj + residual
BLOCK = [LN, GEMM, ATTN, GEMM, LN, GEMM, GEMM]
# two-term weights: ln_1 into both halves of [rows, 2D], in-projection on [N, 2K], attention, out-projection hi + bias + residual,
# out-projection lo + residual, ln_2 twice, c_fc on [N, 2K] + activation, c_proj hi + bias + residual, c_proj lo + residual
BLOCK_X2 = [LN, LN, GEMM, ATTN, GEMM, GEMM, LN, LN, GEMM, GEMM, GEMM]
HEAD = [LN, GEMM]                      # ln_post of the class rows / ln_final of the pooled rows, the projection
HEAD_X2 = [LN, LN, GEMM]               # ln_final into both halves of [B, 2D], the projection on [E, 2D]
TO_F16 = {GEMM: "vl_gemm_f16", ATTN: "vl_attn_fwd_f16"}
TO_F32 = {GEMM: "vl_gemm_f32", ATTN: "vl_attn_fwd_f32"}
# argument positions: (M, N, K), activation, residual of the three GEMM symbols; (B, H, Lq, Lk, dh), causal of an attention;
# x, x row stride, row_mul, out, out row stride, rows, D of a LayerNorm
MNK = {GEMM: slice(6, 9), "vl_gemm_f16": slice(5, 8), "vl_gemm_f32": slice(5, 8)}
ACT = {GEMM: 14, "vl_gemm_f16": 13, "vl_gemm_f32": 12}
BIAS, OUT, RES = 2, 3, 4
ATTN_SHAPE, ATTN_CAUSAL = slice(6, 11), 12
LN_X, LN_XS, LN_MUL, LN_OUT, LN_OS, LN_ROWS, LN_D = 0, 2, 4, 7, 9, 12, 13


def mapped(plan, table):
    return [table.get(s, s) for s in plan]


@pytest.fixture(scope="module")
def traces():
    from vitlens_hip import engine as E, f32 as F
    g = torch.Generator().manual_seed(0)
    out = {}

    def rec(name, fn):
        with recording() as t:
            fn()
        out[name] = t
    # text towers: width 512, 8 heads, context 77, B = 4
    sd = O.init_text(O.TextSpec(context_length=CTX, vocab_size=VOCAB, width=TEXT_D, heads=TEXT_H, layers=LAYERS, embed_dim=TEXT_D), g)
    text = torch.zeros(TEXT_B, CTX, dtype=torch.long)
    for b, eot in enumerate((2, 19, 76, 0)):
        text[b, eot] = VOCAB - 1
    for quick in (False, True):
        cfg = E.TextCfg(context_length=CTX, vocab_size=VOCAB, width=TEXT_D, heads=TEXT_H, layers=LAYERS, embed_dim=TEXT_D, quick_gelu=quick)
        for arith in ("bf16", "f16", "bf16x2"):
            eng = E.TextEngine(sd, cfg, "cpu", arith=arith)
            assert eng.arith == arith
            rec(("text", arith, quick), lambda: eng.encode_text(text))
        f32 = F.TextEngineF32(sd, cfg, "cpu")
        rec(("text", "f32", quick), lambda: f32.encode_text(text))
    # ViT towers: width 128, 4 heads, 16 patches, B = 2; the bf16 one on an fp32 stream (nothing folds, nothing is pruned)
    spec = O.TowerSpec(width=VIT_D, layers=LAYERS, heads=VIT_H, patch=PATCH, image_size=IMG, embed_dim=EMBED)
    cfg = E.TowerCfg(width=VIT_D, layers=LAYERS, heads=VIT_H, patch=PATCH, image_size=IMG, embed_dim=EMBED)
    sd = O.init_tower(spec, g, "t.")
    tok = torch.zeros(B * (IMG // PATCH) ** 2, VIT_D)
    vit, vit32 = E.VitEngine(sd, "t.", cfg, "cpu", res_dtype=torch.float32), F.VitEngineF32(sd, "t.", cfg, "cpu")
    rec(("vit", "bf16"), lambda: vit.trunk(tok.bfloat16(), B))
    rec(("vit", "f32"), lambda: vit32.trunk(tok, B))
    rec(("vit", "f32", "encode"), lambda: vit32.encode(torch.zeros(B, 3, IMG, IMG)))
    sd.update(O.init_lens(spec, O.LensSpec(modality="depth", perceiver_identity=True), g, "t."))
    depth = F.VitEngineF32(sd, "t.", cfg, "cpu", depth=True)
    rec(("vit", "f32", "depth"), lambda: depth.encode(torch.zeros(B, 1, IMG, IMG)))
    return out


def test_every_plan_is_stem_blocks_head(traces):
    for quick in (False, True):
        assert symbols(traces["text", "bf16", quick]) == ["vl_text_embed"] + BLOCK * LAYERS + HEAD
        assert symbols(traces["text", "f16", quick]) == ["vl_text_embed"] + mapped(BLOCK * LAYERS + HEAD, TO_F16)
        assert symbols(traces["text", "f32", quick]) == ["vl_text_embed"] + mapped(BLOCK * LAYERS + HEAD, TO_F32)
        assert symbols(traces["text", "bf16x2", quick]) == ["vl_text_embed"] + BLOCK_X2 * LAYERS + HEAD_X2
    assert symbols(traces["vit", "bf16"]) == ["vl_assemble_ln_pre"] + BLOCK * LAYERS + HEAD
    trunk32 = ["vl_assemble_ln_pre"] + mapped(BLOCK * LAYERS + HEAD, TO_F32)
    assert symbols(traces["vit", "f32"]) == trunk32
    for stem in ("encode", "depth"):           # the conv stem (of the tower, of the depth adapter) as im2col + GEMM
        assert symbols(traces["vit", "f32", stem]) == ["vl_im2col_f32", "vl_gemm_f32"] + trunk32


def _same_problem(bf16, other, table, row_tile):
    """`other` is `bf16` kernel for kernel under the symbol map: LayerNorms over the same rows, GEMMs with the same N, K,
    activation and residual (M: the same, or padded to whole row tiles of the fp16 workspace), attentions with the same shape,
    strides and causal flag."""
    assert len(bf16) == len(other)
    pad = lambda m: (m + row_tile - 1) // row_tile * row_tile
    for (name, a), (oname, o) in zip(bf16, other):
        assert oname == table.get(name, name)
        if name == LN:
            assert [a[i] for i in (LN_XS, LN_MUL, LN_ROWS, LN_D)] == [o[i] for i in (LN_XS, LN_MUL, LN_ROWS, LN_D)]
            assert (a[3] is None) == (o[3] is None)                              # the pooled rows' index
        elif name == GEMM:
            (m, n, k), (om, on, ok) = a[MNK[name]], o[MNK[oname]]
            assert (pad(m), n, k) == (om, on, ok)
            assert a[ACT[name]] == o[ACT[oname]]
            if o is not other[-1][1]:                                            # (the head's projection: see the caller)
                assert (a[RES] is None) == (o[RES] is None)
        elif name == ATTN:
            assert tuple(a[3]) == tuple(o[3]) and a[ATTN_SHAPE] == o[ATTN_SHAPE] and a[ATTN_CAUSAL] == o[ATTN_CAUSAL]


def test_fp16_and_fp32_plans_are_the_bf16_plan_kernel_for_kernel(traces):
    from vitlens_hip import ops
    for quick in (False, True):
        bf16 = traces["text", "bf16", quick]
        _same_problem(bf16, traces["text", "f16", quick], TO_F16, 256)
        _same_problem(bf16, traces["text", "f32", quick], TO_F32, 1)
        # the head's projection has an fp32 output and no residual - but vl_gemm_f16 has no such epilogue: the fp16 one
        # accumulates in place into a (zeroed) fp32 buffer through the residual epilogue
        f16_head = traces["text", "f16", quick][-1][1]
        assert bf16[-1][1][RES] is None and traces["text", "f32", quick][-1][1][RES] is None
        assert _same_buffer(f16_head[OUT], f16_head[RES]) and f16_head[12] == ops.EPI_RES_F32
        fc =[args[ACT[GEMM]] for name, args in bf16 if name == GEMM and args[ACT[GEMM]] != ops.ACT_NONE]
        assert fc == [ops.mlp_act(quick)] * LAYERS                               # c_fc alone carries the activation
        assert all(args[ATTN_CAUSAL] == 1 for name, args in bf16 if name == ATTN)
    _same_problem(traces["vit", "bf16"], traces["vit", "f32"], TO_F32, 1)
    assert all(args[ATTN_CAUSAL] == 0 for name, args in traces["vit", "bf16"] if name == ATTN)


def _same_buffer(p, q, offset=0):
    return p.base == q.base and q.offset - p.offset == offset


def test_two_term_plan_writes_layernorms_twice_and_residuals_in_two_launches(traces):
    D, rows = TEXT_D, TEXT_B * CTX
    for quick in (False, True):
        x2, bf16 = traces["text", "bf16x2", quick], traces["text", "bf16", quick]
        stream = x2[0][1][3]                                                     # what vl_text_embed wrote: the residual stream
        blocks = [x2[1 + i * len(BLOCK_X2):1 + (i + 1) * len(BLOCK_X2)] for i in range(LAYERS)]
        plain = [bf16[1 + i * len(BLOCK):1 + (i + 1) * len(BLOCK)] for i in range(LAYERS)]
        pairs = [(blk[0][1], blk[1][1], blk[2][1], rows) for blk in blocks] + [(blk[6][1], blk[7][1], blk[8][1], rows) for blk in blocks]
        pairs.append((x2[-3][1], x2[-2][1], x2[-1][1], TEXT_B))                  # the head: ln_final of the pooled rows
        for first, second, gemm, n in pairs:
            # both LayerNorm launches read the same rows of the stream and write the two halves of ONE [n, 2D] bf16 buffer ...
            assert _same_buffer(stream, first[LN_X]) and _same_buffer(first[LN_X], second[LN_X])
            assert [first[i] for i in (LN_XS, LN_MUL, LN_ROWS, LN_D)] == [second[i] for i in (LN_XS, LN_MUL, LN_ROWS, LN_D)]
            assert (first[3] is None and second[3] is None) if n == rows else _same_buffer(first[3], second[3])   # the pooled rows' index
            assert (first[LN_ROWS], first[LN_D], first[LN_OS], second[LN_OS]) == (n, D, 2 * D, 2 * D)
            assert _same_buffer(first[LN_OUT], second[LN_OUT], offset=2 * D)     # D bf16 elements further
            # ... which the GEMM behind them reads whole, against the K-concatenated [N, 2K] weight
            assert _same_buffer(first[LN_OUT], gemm[0]) and gemm[MNK[GEMM]][2] == 2 * D and gemm[RES] is None
        for blk, ref in zip(blocks, plain):
            for hi, lo, one in ((blk[4], blk[5], ref[3]), (blk[9], blk[10], ref[6])):
                # hi then lo: the bf16 plan's residual launch twice, both in place on the stream, the bias on the first only
                assert hi[1][MNK[GEMM]] == lo[1][MNK[GEMM]] == one[1][MNK[GEMM]]
                for args in (hi[1], lo[1]):
                    assert _same_buffer(stream, args[OUT]) and _same_buffer(stream, args[RES]) and args[ACT[GEMM]] == one[1][ACT[GEMM]]
                assert _same_buffer(hi[1][0], lo[1][0]) and hi[1][BIAS] is not None and lo[1][BIAS] is None
            # the projections that write an activation: the bf16 plan's M and N, twice its K
            for i, j in ((2, 1), (8, 5)):
                (m, n, k), (rm, rn, rk) = blk[i][1][MNK[GEMM]], ref[j][1][MNK[GEMM]]
                assert (m, n, k) == (rm, rn, 2 * rk) and blk[i][1][ACT[GEMM]] == ref[j][1][ACT[GEMM]]
            assert blk[3][1][ATTN_SHAPE] == ref[2][1][ATTN_SHAPE] and blk[3][1][ATTN_CAUSAL] == ref[2][1][ATTN_CAUSAL] == 1
