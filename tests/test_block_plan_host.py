"""CPU: which kernels one transformer block enqueues on a bf16 stream (engine.block_forward in engine.Bf16Arith, LayerNorm-folded
and pruned, through VitEngine.trunk and TowerTrainer.forward), recorded instead of executed (launch_trace.py; the block with its
LayerNorm passes in each of the four arithmetics: test_tower_plan_host.py).  The host-side branch selection of the LayerNorm folding depends on how many
rows the persistent GEMM takes of each problem (vl_gemm_main_rows), so the plan differs with the batch; the three plans of a
ViT-L-width tower at L = 257 are written out below.  No GPU test reaches the B = 50 one."""
import pytest
import torch

from launch_trace import recording, shape_of as _shape_of, symbols

D, H, L, LAYERS = 1024, 16, 257, 3

# one folded block in full; the in-projection and c_fc always leave leftover rows to a plain GEMM at these sizes
# B = 32 (8224 rows): the persistent kernel takes no rows of an N = 1024 problem - out_proj and c_proj are plain GEMMs
FULL_32 = ["vl_ln_row_stats", "vl_gemm_lnfold_bf16", "vl_gemm_bf16_ex",      # ln_1 statistics, in-projection (main, leftover)
           "vl_attn_fwd_bf16",
           "vl_gemm_bf16_ex",                                                # out_proj + residual
           "vl_ln_row_stats", "vl_gemm_lnfold_bf16", "vl_gemm_bf16_ex",      # ln_2 statistics, c_fc (main, leftover)
           "vl_gemm_bf16_ex"]                                                # c_proj + residual
# B = 64 (16448 rows): every GEMM takes 16384 main rows; the residual GEMMs leave their partial row sums
FULL_64 = ["vl_ln_row_stats", "vl_gemm_lnfold_bf16", "vl_gemm_bf16_ex",
           "vl_attn_fwd_bf16",
           "vl_gemm_res_rowstats_bf16", "vl_gemm_bf16_ex",                   # out_proj + residual (main, leftover)
           "vl_ln_row_stats", "vl_gemm_lnfold_bf16", "vl_gemm_bf16_ex",
           "vl_gemm_res_rowstats_bf16", "vl_gemm_bf16_ex"]                   # c_proj + residual (main, leftover)
# B = 50 (12850 rows): out_proj takes 12800 main rows, c_fc (N = 4096) only 12288 - the row-statistics launch cannot write
# the LayerNorm output of c_fc's leftover rows (some of their statistics come from the partial sums), a LayerNorm pass does
FULL_50 = FULL_64[:8] + ["vl_layernorm_fwd"] + FULL_64[8:]
# the last block of a class-token-pooled tower: dense up to the in-projection, then the class rows only
PRUNED = ["vl_ln_row_stats", "vl_gemm_lnfold_bf16", "vl_gemm_bf16_ex",
          "vl_attn_fwd_q1", "vl_gemm_bf16_ex", "vl_layernorm_fwd", "vl_gemm_bf16_ex", "vl_gemm_bf16_ex"]
HEAD = ["vl_layernorm_fwd", "vl_gemm_bf16_ex"]                               # ln_post of the class rows, the projection


@pytest.fixture(scope="module")
def tower_sd():
    sd = {"class_embedding": torch.zeros(D), "positional_embedding": torch.zeros(L, D), "proj": torch.zeros(D, 768)}
    for ln in ("ln_pre", "ln_post"):
        sd[ln + ".weight"], sd[ln + ".bias"] = torch.ones(D), torch.zeros(D)
    for l in range(LAYERS):
        p = f"transformer.resblocks.{l}."
        for ln in ("ln_1", "ln_2"):
            sd[p + ln + ".weight"], sd[p + ln + ".bias"] = torch.ones(D), torch.zeros(D)
        for name, (n, k) in (("attn.in_proj_", (3 * D, D)), ("attn.out_proj.", (D, D)), ("mlp.c_fc.", (4 * D, D)),
                             ("mlp.c_proj.", (D, 4 * D))):
            sd[p + name + "weight"], sd[p + name + "bias"] = torch.zeros(n, k), torch.zeros(n)
    return {"visual." + k: v for k, v in sd.items()}


@pytest.mark.parametrize("B,full", [(32, FULL_32), (50, FULL_50), (64, FULL_64)])
def test_block_plan_of_engine_and_trainer(B, full, tower_sd, monkeypatch):
    from vitlens_hip import engine as E, train as T
    monkeypatch.setattr(E, "LN_FOLD", True)
    monkeypatch.setattr(E, "PRUNE_LAST_BLOCK", True)
    cfg = E.TowerCfg(width=D, layers=LAYERS, heads=H, embed_dim=768)
    eng = E.VitEngine(tower_sd, "visual.", cfg, "cpu", res_dtype=torch.bfloat16)
    tok = torch.zeros(B * (L - 1), D, dtype=torch.bfloat16)
    with recording() as inference:
        eng.trunk(tok, B)
    assert symbols(inference) == ["vl_assemble_ln_pre"] + full + full + PRUNED + HEAD
    # a trainer whose first block is trainable: that block runs its LayerNorm passes and leaves the partial row sums for the
    # next one; the frozen blocks behind it are the engine's launches on other buffers
    trainer = T.TowerTrainer(eng, train_blocks=[0])
    with recording() as training:
        trainer.forward(tok, B)
    frozen = len(full) + len(PRUNED) + len(HEAD)
    trained = ["vl_layernorm_fwd", "vl_gemm_bf16_ex", "vl_attn_fwd_bf16", "vl_gemm_bf16_ex", "vl_layernorm_fwd", "vl_gemm_bf16_ex"]
    assert symbols(training) == ["vl_assemble_ln_pre"] + trained + full[-(1 if B == 32 else 2):] + full + PRUNED + HEAD
    assert [_shape_of(c) for c in training[-frozen:]] == [_shape_of(c) for c in inference[-frozen:]]
    # and the trainer does save what the engine does not, e.g. the attention's lse of the frozen block
    lse = lambda trace: next(args[5] for name, args in trace[-frozen:] if name == "vl_attn_fwd_bf16")
    assert lse(training) is not None and lse(inference) is None
