"""CPU: which kernels the front of a point-cloud Lens enqueues - recorded instead of executed (launch_trace.py), through the
public classes only: PointTokenizerEngine / PointTokenizerEngineF32.forward, PointTokenizerTrainer and PNSATokenizerTrainer forward +
backward (train-mode, eval-mode and SyncBatchNorm), LensEngine / LensEngineF32.encode and LensEngine.update_params.  The PointBERT
plan is written out below; the fp32 plan is the bf16 plan kernel for kernel, the trainer's forward is the engine's plan with the
BatchNorm launches inserted behind the first conv and behind the local half of second_conv.0, its backward is 45 launches made
of the per-layer pieces below.  G = 8, M = 4, B = 2, N = 32 (the transposing weight-gradient path).  The last test checks the folded
operand tables of the two engines against each other on random running statistics."""
import pytest
import torch

import vitlens_oracle as O
from launch_trace import Ptr, normalised, recording, shape_of, symbols

B, N, G, M, ENC, TRANS = 2, 32, 8, 4, 256, 384
A = "t.visual_adapter."
FPS, KNN, GEMM, GMAX, PAD3 = "vl_fps", "vl_knn_group", "vl_gemm_bf16_ex", "vl_group_max", "vl_pad3_bf16"
# FPS, kNN patches, conv 3->128 (+BN+ReLU), conv 128->256, group max, global half of second_conv.0 on the maxima, local half with
# the group's row added in front of the (BN+)ReLU, conv 512->enc, group max, reduce_dim, padded centres, centre MLP (GELU), second
# Linear of the centre MLP + tokens
ENGINE_PLAN = [FPS, KNN, GEMM, GEMM, GMAX, GEMM, GEMM, GEMM, GMAX, GEMM, PAD3, GEMM, GEMM]
BN_AFTER = (2, 6)                          # the plan's launches a BatchNorm follows in the trainer: first_conv.0, second_conv.0 (local)
TO_F32 = {KNN: "vl_knn_group_f32", GEMM: "vl_gemm_f32", GMAX: "vl_group_max_f32", PAD3: "vl_pad3_f32"}
BN = {"train": ["vl_bn_stats", "vl_bn_apply"], "eval": ["vl_bn_apply"],
      "sync": ["vl_bn_stats_local", "all_gather", "vl_bn_stats_merge", "vl_bn_apply"]}
BN_BWD = {"train": ["vl_bn_bwd"], "eval": ["vl_bn_bwd"], "sync": ["vl_bn_bwd_reduce", "all_reduce_sum", "vl_bn_bwd_apply"]}
# backward pieces: a weight gradient on the transposing path (dy^T, x^T, product), a bias gradient, a data gradient
DW, DB, DX = ["vl_transpose_to_bf16", "vl_transpose_to_bf16", GEMM], ["vl_colsum"], [GEMM]
DW3 = DW + ["vl_axpy_f32"]                 # a 3-channel input: the padded product, then its real columns accumulated


def backward_plan(mode):
    return (["vl_cast_f32_bf16"]
            + DW + DB + DX                 # pos_embed.2, and du through the GELU derivative
            + DW3 + DB                     # pos_embed.0
            + DW + DB + DX                 # reduce_dim
            + ["vl_group_max_bwd"]
            + DW + DB + DX                 # second_conv.3
            + BN_BWD[mode] + ["vl_group_sum"]
            + DW + DW + DB + DX + DX       # second_conv.0: local half, global half, bias; dg, dfl
            + ["vl_group_max_bwd"]
            + DW + DB + DX                 # first_conv.3
            + BN_BWD[mode]
            + DW3 + DB)                    # first_conv.0


class Comm:
    """A communicator that writes its calls into the trace."""

    def __init__(self):
        self.trace = None

    def all_gather(self, out, local):
        self.trace.append(("all_gather", ()))

    def all_reduce_sum(self, x):
        self.trace.append(("all_reduce_sum", ()))


PC = dict(pc_num_group=G, pc_group_size=M, pc_encoder_dims=ENC, pc_trans_dim=TRANS)
PERC = dict(perceiver_identity=False, depth=1, self_per_cross=1, num_latents=16, latent_dim=128, input_chan=TRANS, cross_heads=1,
            cross_dim_head=32, latent_heads=4, latent_dim_head=32)
SPEC = O.TowerSpec(width=128, layers=2, heads=4, patch=14, image_size=56, embed_dim=64)


def _state(seed=0):
    g = torch.Generator().manual_seed(seed)
    return {**O.init_tower(SPEC, g, "t.", with_conv=False),
            **O.init_lens(SPEC, O.LensSpec(modality="pc", **PC, **PERC), g, "t.")}


def _pnsa_state():
    sd, c = {}, 6
    for i, o in enumerate((64, 128, ENC)):
        sd[A + f"sa.mlp_convs.{i}.weight"], sd[A + f"sa.mlp_convs.{i}.bias"] = torch.zeros(o, c, 1, 1), torch.zeros(o)
        for n in ("weight", "bias", "running_mean", "running_var"):
            sd[A + f"sa.mlp_bns.{i}.{n}"] = torch.zeros(o)
        c = o
    sd.update({A + "lift.0.weight": torch.zeros(TRANS, ENC + 3, 1), A + "lift.0.bias": torch.zeros(TRANS),
               A + "lift.2.weight": torch.zeros(TRANS), A + "lift.2.bias": torch.zeros(TRANS)})
    return sd


@pytest.fixture(scope="module")
def traces():
    from vitlens_hip import engine as E, f32 as F, points as P
    sd = _state()
    lens = E.LensCfg(modality="pc", **PC, **PERC)
    pnsa = E.LensCfg(modality="pc", pc_tokenizer="pnsa", pc_in_dim=3, **PC, **PERC)
    tower = E.TowerCfg(width=128, layers=2, heads=4, patch=14, image_size=56, embed_dim=64)
    pts, start = torch.zeros(B, N, 3), torch.zeros(B, dtype=torch.long)
    out = {}

    def rec(name, fn):
        with recording() as t:
            out[name + " result"] = fn(t)
        out[name] = t
    rec("bf16", lambda t: P.PointTokenizerEngine(sd, A, lens, "cpu").forward(pts, start))
    rec("f32", lambda t: F.PointTokenizerEngineF32(sd, A, lens, "cpu").forward(pts, start))
    for mode, kw in (("train", dict(bn_training=True)), ("eval", dict(bn_training=False)),
                     ("sync", dict(bn_training=True, bn_sync=Comm(), world_size=2))):
        for cls, key, state, cfg, args in ((P.PointTokenizerTrainer, "trainer", sd, lens, dict()),
                                           (P.PNSATokenizerTrainer, "pnsa", _pnsa_state(), pnsa, dict(xyz=pts))):
            tr = cls(state, A, cfg, "cpu", **kw)

            def run(t, call, tr=tr):
                if tr.bn_sync is not None:
                    tr.bn_sync.trace = t
                return call()
            rec(f"{key} {mode} forward", lambda t, tr=tr, args=args: run(t, lambda: tr.forward(pts, fps_start=start, **args)))
            rec(f"{key} {mode} backward", lambda t, tr=tr: run(t, lambda: tr.backward(torch.zeros(B * G, TRANS))))
    # the Lens: tokenizer -> Perceiver -> trunk
    for cls, key in ((E.LensEngine, "lens bf16"), (F.LensEngineF32, "lens f32")):
        le = cls(sd, "t.", tower, lens, "cpu")
        rec(key, lambda t: le.encode(pts, fps_start=start))
        rec(key + " tokenizer", lambda t: le.points.forward(pts, start))
        rec(key + " perceiver", lambda t: le.perceiver.forward(out[key + " tokenizer result"], B))
        rec(key + " trunk", lambda t: le.vit.trunk(out[key + " perceiver result"], B))
    out["lens cfg"] = (sd, tower, lens, pts, start)
    return out


def test_engine_plan_and_fp32_plan_kernel_for_kernel(traces):
    from vitlens_hip import ops
    bf16, f32 = traces["bf16"], traces["f32"]
    assert symbols(bf16) == ENGINE_PLAN
    want = [TO_F32.get(s, s) for s in ENGINE_PLAN]
    want[6] = "vl_gemm_f32_ex"                                    # the projection with the group's row as a residual
    assert symbols(f32) == want
    acts, kpad = [], []
    for (name, a), (oname, o) in zip(bf16, f32):
        if name == GEMM:
            m, n, k = a[6:9]
            assert o[5:8] == (m, n, 4 if kpad_of(a) else k)
            assert a[14] == o[12]                                 # activation
            assert a[15] == (o[13] if oname == "vl_gemm_f32_ex" else 1)      # res_div
            if oname == "vl_gemm_f32_ex":
                assert a[15] == M and a[13] == ops.EPI_RES_BF16 and o[14] == 1 and o[15] == 0     # res_pre, not GEGLU
            assert [x is None for x in a[2:5]] == [x is None for x in o[2:5]]               # bias, out, residual
            acts.append(a[14]); kpad.append(kpad_of(a))
        elif name == KNN:
            assert a[4:8] == o[4:8] == (B, N, G, M) and (a[8], o[8]) == (64, 4)
        elif name == GMAX:
            assert a[5:8] == o[4:7]                               # groups, M, C
        elif name == PAD3:
            assert (a[2], o[2]) == (B * G, B * G) and (a[3], o[3]) == (64, 4)
        else:
            assert shape_of((name, a)) == shape_of((oname, o))
    assert acts == [ops.ACT_RELU, 0, 0, ops.ACT_RELU, 0, 0, ops.ACT_GELU, 0]
    assert kpad == [True, False, False, False, False, False, True, False]


def kpad_of(a):
    """Is this bf16 GEMM one on a 3-channel input zero-padded to K = 64 (patches, centres)?"""
    return a[8] == 64 and a[7] == 128 and a[6] in (B * G * M, B * G)


@pytest.mark.parametrize("mode", ["train", "eval", "sync"])
def test_trainer_forward_is_the_engine_plan_with_batchnorm_inserted(traces, mode):
    from vitlens_hip import ops
    eng, fwd = traces["bf16"], traces[f"trainer {mode} forward"]
    want = []
    for i, s in enumerate(ENGINE_PLAN):
        want += [s] + (BN[mode] if i in BN_AFTER else [])
    assert symbols(fwd) == want
    assert len(fwd) - (mode == "sync") * 2 == {"train": 17, "eval": 15, "sync": 19}[mode]
    rest = [c for c in fwd if c[0] not in sum(BN.values(), [])]
    for i, (e, t) in enumerate(zip(eng, rest)):
        if i in BN_AFTER:      # the ReLU moves from the GEMM's epilogue into the BatchNorm launch behind it
            assert e[1][14] == ops.ACT_RELU and t[1][14] == ops.ACT_NONE
            e = (e[0], e[1][:14] + (ops.ACT_NONE,) + e[1][15:])
        assert shape_of(e) == shape_of(t), i
    assert [c[1][7] for c in fwd if c[0] == "vl_bn_apply"] == [1, 1]         # relu
    assert rest[11][1][14] == ops.ACT_GELU_DSAVE and rest[11][1][5] is not None and eng[11][1][5] is None


@pytest.mark.parametrize("mode", ["train", "eval", "sync"])
def test_trainer_backward_is_45_launches_of_per_layer_pieces(traces, mode):
    bwd = traces[f"trainer {mode} backward"]
    assert symbols(bwd) == backward_plan(mode)
    assert len([c for c in bwd if c[1] != ()]) == 45 + (2 if mode == "sync" else 0)       # SyncBatchNorm: reduce + apply for bn_bwd


@pytest.mark.parametrize("mode", ["train", "eval", "sync"])
def test_pnsa_plan(traces, mode):
    """Three conv + BatchNorm rounds, the group maximum, lift (Conv1d as a GEMM) and LayerNorm; the backward in reverse."""
    fwd = [FPS, "vl_ball_group"] + ([GEMM] + BN[mode]) * 3 + [GMAX, GEMM, "vl_layernorm_fwd"]
    assert symbols(traces[f"pnsa {mode} forward"]) == fwd
    bwd = (["vl_layernorm_bwd_params", "vl_layernorm_bwd_g"] + DW3 + DB + DX + ["vl_group_max_bwd"]
           + (BN_BWD[mode] + DW + DB + DX) * 2 + BN_BWD[mode] + DW3 + DB)
    assert symbols(traces[f"pnsa {mode} backward"]) == bwd


@pytest.mark.parametrize("arith", ["bf16", "f32"])
def test_lens_encode_is_tokenizer_perceiver_trunk(traces, arith):
    key = f"lens {arith}"
    parts = symbols(traces[key + " tokenizer"]) + symbols(traces[key + " perceiver"]) + symbols(traces[key + " trunk"])
    assert symbols(traces[key]) == parts
    assert symbols(traces[key + " tokenizer"]) == symbols(traces[arith])
    assert [shape_of(c) for c in traces[key]] == [shape_of(c) for k in ("tokenizer", "perceiver", "trunk") for c in traces[f"{key} {k}"]]


def test_update_params_rebuilds_the_tokenizer_only_for_an_adapter_name(traces):
    from vitlens_hip import engine as E
    sd, tower, lens, pts, start = traces["lens cfg"]
    le = E.LensEngine(sd, "t.", tower, lens, "cpu")
    before = le.points
    le.update_params(sd, "t.", ["class_embedding", "perceiver.latents"])
    with recording() as t:
        le.encode(pts, fps_start=start)
    assert le.points is before and normalised(t) == normalised(traces["lens bf16"])
    sd2 = _state(seed=1)
    le.update_params(sd2, "t.", ["visual_adapter.reduce_dim.weight"])
    with recording() as t:
        le.encode(pts, fps_start=start)
    assert le.points is not before
    with recording() as fresh:
        E.LensEngine(sd2, "t.", tower, lens, "cpu").encode(pts, fps_start=start)
    assert normalised(t) == normalised(fresh)
    got = [c[1][1].t for c in t if c[0] == GEMM][:8]
    new = [c[1][1].t for c in fresh if c[0] == GEMM][:8]
    assert all(torch.equal(a, b) for a, b in zip(got, new)) and not torch.equal(got[5], [c[1][1].t for c in traces["lens bf16"] if c[0] == GEMM][5])


def test_bf16_operands_are_the_rounded_fp32_table():
    """Random running statistics: every weight the bf16 engine hands a GEMM is bit for bit the bf16 rounding of the fp32 table's
    (the 3-channel ones zero-padded to K = 64 instead of 4), every bias is the fp32 table's."""
    from vitlens_hip import engine as E, f32 as F, points as P
    sd = _state(seed=7)
    lens = E.LensCfg(modality="pc", **PC, **PERC)
    table = F.point_tokenizer_operands_f32(sd, A)
    with recording() as t:
        P.PointTokenizerEngine(sd, A, lens, "cpu").forward(torch.zeros(B, N, 3), torch.zeros(B, dtype=torch.long))
    gemms = [c[1] for c in t if c[0] == GEMM]
    names = [("w1", "b1"), ("w2", "b2"), ("w3g", "b3"), ("w3l", None), ("w4", "b4"), ("wr", "br"), ("wp0", "bp0"), ("wp2", "bp2")]
    assert len(gemms) == len(names)
    for a, (w, b) in zip(gemms, names):
        got, want = a[1].t, table[w]
        assert isinstance(a[1], Ptr) and got.dtype == torch.bfloat16
        if w in ("w1", "wp0"):
            assert got.shape[1] == 64 and want.shape[1] == 4 and float(got[:, 3:].abs().max()) == 0.0 and float(want[:, 3:].abs().max()) == 0.0
            got, want = got[:, :3], want[:, :3]
        assert torch.equal(got, want.bfloat16()), w
        if b is None:
            assert a[2] is None
        else:
            assert a[2].t.dtype == torch.float32 and torch.equal(a[2].t, table[b]), b
