"""CPU: which kernels the Perceiver enqueues - PerceiverEngine.forward (bf16 operands), PerceiverEngineF32.forward and
PerceiverTrainer.forward / backward - recorded instead of executed (launch_trace.py), on a zero-filled state dict at depth 2
with 2 latent self-attention layers per cross attention.  The plans of one cross-attention, one FeedForward and one latent
self-attention sub-layer are written out below, forward and backward; every executor's plan is their concatenation, the
trainer's forward is the engine's plus the outputs it saves, the fp32 engine's is the bf16 engine's kernel for kernel."""
import pytest
import torch

from launch_trace import OPTIONAL_OUTPUTS, Ptr, recording, shape_of, symbols

DEPTH, SELFS, B, TC = 2, 2, 2, 16
N_LAT, D, C, HEADS, DH = 32, 128, 64, 2, 64

LN, GEMM, ATTN = "vl_layernorm_fwd", "vl_gemm_bf16_ex", "vl_attn_fwd_bf16"
# forward, bf16 operands
CROSS = [LN, LN, GEMM, GEMM, ATTN, GEMM]              # LN(x), LN_ctx(data), to_q, to_kv, attention, to_out + residual
FF = [LN, GEMM, GEMM]                                  # LN, GEGLU GEMM, down-projection + residual
SELF = [LN, GEMM, ATTN, GEMM]                          # LN, packed to_qkv, attention, to_out + residual
# forward, fp32
CROSS_F32 = [LN, LN, "vl_gemm_f32", "vl_gemm_f32", "vl_attn_fwd_f32", "vl_gemm_f32"]
FF_F32 = [LN, "vl_gemm_f32_ex", "vl_gemm_f32"]
SELF_F32 = [LN, "vl_gemm_f32", "vl_attn_fwd_f32", "vl_gemm_f32"]
# backward.  The weight gradients of 64 latent rows / 32 context rows take the transposing NT path (two transposed copies, one
# GEMM that accumulates); the latent self-attention (Lq = Lk) has the fused attention backward, the cross attention has not
DW = ["vl_transpose_to_bf16", "vl_transpose_to_bf16", GEMM]
LN_BWD = ["vl_layernorm_bwd_params", "vl_layernorm_bwd_g"]
FF_BWD = DW + ["vl_colsum", GEMM] + DW + ["vl_colsum", GEMM] + LN_BWD          # dW2, db2, dGEGLU GEMM; dW0, db0, dX GEMM; LN
SELF_BWD = DW + ["vl_colsum", GEMM, "vl_attn_bwd_fused_bf16"] + DW + [GEMM] + LN_BWD      # to_out; attention; to_qkv; LN
CROSS_BWD = DW + ["vl_colsum", GEMM, "vl_attn_bwd_bf16"] + DW + [GEMM] + LN_BWD + DW + [GEMM] + LN_BWD    # ...; to_q, LN; to_kv, LN_ctx


def plan(cross, ff, self_):
    return (cross + ff + (self_ + ff) * SELFS) * DEPTH


def lens_cfg(tied):
    from vitlens_hip.engine import LensCfg
    return LensCfg(modality="audio", perceiver_identity=False, depth=DEPTH, self_per_cross=SELFS, num_latents=N_LAT, latent_dim=D,
                   input_chan=C, cross_heads=1, cross_dim_head=DH, latent_heads=HEADS, latent_dim_head=DH, weight_tie_layers=tied)


def perceiver_sd(c, P="p."):
    """A zero-filled Perceiver state dict under the reference's parameter names (a tied one repeats layer 1's tensors)."""
    z = torch.zeros
    xi, si = c.cross_heads * c.cross_dim_head, c.latent_heads * c.latent_dim_head
    sd = {P + "latents": z(c.num_latents, c.latent_dim)}

    def attn(q, inner, ctx):
        sd[q + "norm.weight"], sd[q + "norm.bias"] = torch.ones(c.latent_dim), z(c.latent_dim)
        sd[q + "fn.to_q.weight"], sd[q + "fn.to_kv.weight"] = z(inner, c.latent_dim), z(2 * inner, ctx)
        sd[q + "fn.to_out.weight"], sd[q + "fn.to_out.bias"] = z(c.latent_dim, inner), z(c.latent_dim)

    def ff(q):
        sd[q + "norm.weight"], sd[q + "norm.bias"] = torch.ones(c.latent_dim), z(c.latent_dim)
        sd[q + "fn.net.0.weight"], sd[q + "fn.net.0.bias"] = z(8 * c.latent_dim, c.latent_dim), z(8 * c.latent_dim)
        sd[q + "fn.net.2.weight"], sd[q + "fn.net.2.bias"] = z(c.latent_dim, 4 * c.latent_dim), z(c.latent_dim)
    for i in range(c.depth):
        q = f"{P}layers.{i}."
        attn(q + "0.", xi, c.input_chan)
        sd[q + "0.norm_context.weight"], sd[q + "0.norm_context.bias"] = torch.ones(c.input_chan), z(c.input_chan)
        ff(q + "1.")
        for j in range(c.self_per_cross):
            attn(f"{q}2.{j}.0.", si, c.latent_dim)
            ff(f"{q}2.{j}.1.")
    return sd


@pytest.fixture(scope="module", params=[False, True], ids=["untied", "tied"])
def traces(request):
    """The three executors built from one state dict, and their recorded launches."""
    from vitlens_hip import engine as E, f32 as F, train as T
    c = lens_cfg(request.param)
    sd = perceiver_sd(c)
    pe, pf = E.PerceiverEngine(sd, "p.", c, "cpu"), F.PerceiverEngineF32(sd, "p.", c, "cpu")
    pt = T.PerceiverTrainer(pe, "p.")
    data = torch.zeros(B * TC, C, dtype=torch.bfloat16)
    with recording() as bf16:
        pe.forward(data, B)
    with recording() as f32:
        pf.forward(data.float(), B)
    with recording() as fwd:
        lat = pt.forward(data, B)
    with recording() as bwd:
        pt.backward(torch.zeros_like(lat))
    return {"bf16": bf16, "f32": f32, "fwd": fwd, "bwd": bwd, "trainer": pt}


def test_plans_are_the_written_out_units(traces):
    assert symbols(traces["bf16"]) == plan(CROSS, FF, SELF)
    assert symbols(traces["fwd"]) == plan(CROSS, FF, SELF)
    assert symbols(traces["f32"]) == plan(CROSS_F32, FF_F32, SELF_F32)
    # the backward: the residual gradient's bf16 copy, the layers in reverse (each: its self layers in reverse, FeedForward
    # before attention; then the cross attention's FeedForward, then the cross attention), the latents' gradient
    assert symbols(traces["bwd"]) == (["vl_cast_f32_bf16"] + ((FF_BWD + SELF_BWD) * SELFS + FF_BWD + CROSS_BWD) * DEPTH
                                      + ["vl_batch_rowsum"])


def test_trainer_forward_is_the_engine_forward_plus_saved_outputs(traces):
    """Same scalars, same pointer offsets; the trainer writes every optional output (mean / rstd of a LayerNorm, lse of an
    attention, out2 = the pre-activation of a GEGLU GEMM), the engine none."""
    from vitlens_hip import ops
    assert [shape_of(c) for c in traces["fwd"]] == [shape_of(c) for c in traces["bf16"]]
    for (name, targs), (_, eargs) in zip(traces["fwd"], traces["bf16"]):
        geglu = name == GEMM and targs[13] == ops.EPI_GEGLU
        for i in OPTIONAL_OUTPUTS[name]:
            assert eargs[i] is None
            assert isinstance(targs[i], Ptr) if (name != GEMM or geglu) else targs[i] is None


def test_fp32_plan_is_the_bf16_plan_kernel_for_kernel(traces):
    """Same length; at every position the fp32 kernel of the bf16 one with the same problem: rows / width of a LayerNorm,
    M / N / K / the three leading dimensions of a GEMM, B / H / Lq / Lk / dh and the element strides of an attention."""
    from vitlens_hip import ops
    assert len(traces["f32"]) == len(traces["bf16"])
    for (name, a), (fname, f) in zip(traces["bf16"], traces["f32"]):
        if name == LN:
            assert fname == LN and (a[2], a[12], a[13]) == (f[2], f[12], f[13])
        elif name == GEMM:
            assert fname == ("vl_gemm_f32_ex" if a[13] == ops.EPI_GEGLU else "vl_gemm_f32")
            assert a[6:12] == f[5:11]
            assert (a[4] is None) == (f[4] is None)                    # a residual on the same launches
        else:
            assert (name, fname) == (ATTN, "vl_attn_fwd_f32")
            assert tuple(a[3]) == tuple(f[3]) and a[6:11] == f[6:11]


def _numbered(layers):
    """Every GEMM weight of the operand table filled with arange (mod 113: exact in bf16) plus a number of its own."""
    k = 0
    for lay in layers:
        for d in [lay["x_attn"], lay["x_ff"]] + [sl[key] for sl in lay["selfs"] for key in ("attn", "ff")]:
            for key, w in d.items():
                if w.dim() == 2:
                    w.copy_((torch.arange(w.numel()) % 113 + 3 * k).reshape(w.shape))
                    k += 1
    assert 112 + 3 * k < 256


def test_refresh_derived_transposes_every_operand(traces):
    pt = traces["trainer"]
    layers = pt.pe.layers
    _numbered(layers)
    pt.refresh_derived()
    assert len(pt.wT) == len(layers) == DEPTH
    for d, lay in zip(pt.wT, layers):
        pairs = [(d["x"]["q"], lay["x_attn"]["q_w"]), (d["x"]["kv"], lay["x_attn"]["kv_w"]), (d["x"]["out"], lay["x_attn"]["to_out_w"]),
                 (d["xff"]["w0"], lay["x_ff"]["w0"]), (d["xff"]["w2"], lay["x_ff"]["w2"])]
        assert len(d["selfs"]) == len(lay["selfs"]) == SELFS
        for ds, sl in zip(d["selfs"], lay["selfs"]):
            pairs += [(ds["qkv"], sl["attn"]["qkv_w"]), (ds["out"], sl["attn"]["to_out_w"]), (ds["w0"], sl["ff"]["w0"]),
                      (ds["w2"], sl["ff"]["w2"])]
        for wt, w in pairs:
            assert wt.dtype == torch.bfloat16 and wt.is_contiguous() and torch.equal(wt, w.t())


def test_tied_layers_share_operands_and_transposes():
    """weight_tie_layers at depth 3: layers 1 and 2 are one set of operands and one set of transposes, in the engine of either
    arithmetic and in the trainer."""
    from dataclasses import replace
    from vitlens_hip import engine as E, f32 as F, train as T
    c = replace(lens_cfg(True), depth=3)
    sd = perceiver_sd(c)
    pe, pf = E.PerceiverEngine(sd, "p.", c, "cpu"), F.PerceiverEngineF32(sd, "p.", c, "cpu")
    pt = T.PerceiverTrainer(pe, "p.")
    for layers in (pe.layers, pf.layers, pt.wT):
        assert len(layers) == 3 and layers[2] is layers[1] and layers[1] is not layers[0]
    assert pf.layers[0]["x_attn"]["q_w"].dtype == torch.float32 and pe.layers[0]["x_attn"]["q_w"].dtype == torch.bfloat16
    pt.refresh_derived()
    assert pt.wT[2] is pt.wT[1]
