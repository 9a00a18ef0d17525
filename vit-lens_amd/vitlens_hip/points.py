"""The point-cloud tokenizers of the 3D Lens on the HIP kernels.

PointBERT (PointTokenizer.forward, open_clip/modal_3d/models/pointbert/point_encoder.py:350-362): FPS -> kNN grouping ->
mini-PointNet (Encoder, dvae.py:179-212) -> reduce_dim, plus the centre MLP positional embedding; returns x + pos.  The dataflow
is written once, `pointbert_forward`, and run by three executors: PointTokenizerEngine (bf16 operands, the eval-mode BatchNorms
folded into the 1x1 convolutions at load time), f32.PointTokenizerEngineF32 (the same in fp32) and PointTokenizerTrainer (the
BatchNorm layers as launches of their own - batch statistics per rank or, with a communicator, SyncBatchNorm over the ranks, with
the running-statistics update; or the running statistics in eval mode - activations kept, and the backward pass).
`pnsa` (PointNSATokenizer, pointnet_util.py:345-368): PNSATokenizerTrainer, forward and backward, which also serves inference.
"""
import torch

from . import ops
from .engine import Bf16Arith, _dev

BF = torch.bfloat16


def fold_bn(w, b, gamma, beta, running_mean, running_var, eps=1e-5):
    """Eval-mode BatchNorm after a 1x1 conv, folded into it IN FP32: bn(x W^T + b) = x (s W)^T + (b - mean) s + beta with
    s = gamma / sqrt(var + eps) (dvae.py:183-194 in eval mode).  -> (W' [O, K], b' [O]) f32."""
    f = lambda t: t.detach().float()
    s = f(gamma) / torch.sqrt(f(running_var) + eps)
    return f(w) * s[:, None], (f(b) - f(running_mean)) * s + f(beta)


def point_tokenizer_operands(sd, a: str, dtype, Kp: int, eps: float = 1e-5):
    """The folded operand table of the PointBERT tokenizer from the reference's parameters (prefix `a` = "...visual_adapter."),
    computed in fp32 on the device the parameters live on: the two eval-mode BatchNorms folded into the convs before them, the
    3-channel inputs zero-padded to a multiple of `Kp` columns, second_conv.0 split into its global (first half of the input
    channels: the broadcast group maximum, dvae.py:207-209) and local halves.  Weights w* in `dtype`, biases b* f32."""
    f = lambda k: sd[a + k].detach().float()
    conv = lambda k: f(k + ".weight")[:, :, 0]
    bn = lambda k: [f(k + n) for n in (".weight", ".bias", ".running_mean", ".running_var")]

    def padk(w):
        out = torch.zeros(w.shape[0], (w.shape[1] + Kp - 1) // Kp * Kp, dtype=torch.float32, device=w.device)
        out[:, :w.shape[1]] = w
        return out
    w1, b1 = fold_bn(conv("encoder.first_conv.0"), f("encoder.first_conv.0.bias"), *bn("encoder.first_conv.1"), eps=eps)
    w3, b3 = fold_bn(conv("encoder.second_conv.0"), f("encoder.second_conv.0.bias"), *bn("encoder.second_conv.1"), eps=eps)
    half = w3.shape[1] // 2
    w = {"w1": padk(w1), "w2": conv("encoder.first_conv.3"), "w3g": w3[:, :half], "w3l": w3[:, half:], "w4": conv("encoder.second_conv.3"),
         "wr": f("reduce_dim.weight"), "wp0": padk(f("pos_embed.0.weight")), "wp2": f("pos_embed.2.weight")}
    b = {"b1": b1, "b2": f("encoder.first_conv.3.bias"), "b3": b3, "b4": f("encoder.second_conv.3.bias"), "br": f("reduce_dim.bias"),
         "bp0": f("pos_embed.0.bias"), "bp2": f("pos_embed.2.bias")}
    return {**{k: v.to(dtype) for k, v in w.items()}, **b}


def point_groups(lens, pts: torch.Tensor, fps_start, ar, Kp: int, device, want_idx=False):
    """FPS centres and their kNN patches: -> (centre indices, centres f32 [B,G,3], centred patches [B*G*M, Kp] in the
    arithmetic's dtype, neighbour indices or None)."""
    pts = pts.to(device).contiguous().float()
    if fps_start is None:   # misc.py:60 draws the first centre at random
        fps_start = torch.randint(0, pts.shape[1], (pts.shape[0],), device=device, dtype=torch.long)
    cidx, centers = ops.fps(pts, fps_start.to(device), lens.pc_num_group)
    patches, nidx = ar.knn_group(pts, cidx, lens.pc_group_size, Kp=Kp, want_idx=want_idx)
    return cidx, centers, patches, nidx


def pointbert_forward(op, lens, pts: torch.Tensor, fps_start, ar, device, train=None) -> torch.Tensor:
    """pts [B,N,3] -> tokens + pos [B*G, trans_dim] in the arithmetic `ar` (engine.Bf16Arith, f32.F32Arith) on the operand table
    `op` (w1 .. wp2, b1 .. bp2).
    train None: an engine - the table is point_tokenizer_operands' (BatchNorms folded), ReLU rides in the GEMM epilogues, nothing
    is kept.  train = a PointTokenizerTrainer: the convs run without activation and its `_bn` follows each, the centre MLP saves
    the GELU derivative, and the tensors the backward reads are left in `train.ctx`."""
    M = lens.pc_group_size
    relu = ops.ACT_RELU if train is None else ops.ACT_NONE
    bn = (lambda z, k: (z, None)) if train is None else train._bn

    def lin(x, w, b, act=ops.ACT_NONE, res=None, out2=None):
        out = torch.empty(x.shape[0], w.shape[0], device=x.device, dtype=ar.dtype)
        ar.linear(x, w, b, out, res=res, act=act, out2=out2)
        return out
    _, centers, patches, _ = point_groups(lens, pts, fps_start, ar, op["w1"].shape[1], device)
    z1 = lin(patches, op["w1"], op["b1"], relu)                           # conv 3->128 (+ folded BN + ReLU)
    h1, s1 = bn(z1, "encoder.first_conv.1")
    f = lin(h1, op["w2"], op["b2"])                                       # conv 128->256
    g = ar.group_max(f, M)
    t = lin(g, op["w3g"], op["b3"])                                       # global half of conv 512->512: one row per group
    z3 = torch.empty(f.shape[0], op["w3l"].shape[0], device=f.device, dtype=ar.dtype)
    ar.linear_rowres(f, op["w3l"], z3, t, M, relu)                        # + local half, the group's row added before the ReLU
    h2, s3 = bn(z3, "encoder.second_conv.1")
    f2 = lin(h2, op["w4"], op["b4"])
    g2 = ar.group_max(f2, M)
    tok = lin(g2, op["wr"], op["br"])                                     # [B*G, trans]
    c3 = ar.pad3(centers, op["wp0"].shape[1])
    if train is None:
        p1 = lin(c3, op["wp0"], op["bp0"], ops.ACT_GELU)
    else:
        u = torch.empty(c3.shape[0], op["wp0"].shape[0], device=c3.device, dtype=ar.dtype)
        p1 = lin(c3, op["wp0"], op["bp0"], ops.ACT_GELU_DSAVE, out2=u)
        train.ctx = (patches, z1, s1[0], s1[1], h1, f, g, z3, s3[0], s3[1], h2, f2, g2, c3, u, p1, s1[2], s3[2])
    return lin(p1, op["wp2"], op["bp2"], res=tok)                         # pos + tokens


class PointTokenizerEngine:
    """PointTokenizer.forward in eval mode on folded operands: bf16 by default (the fold runs on the host), in the arithmetic
    `arith` otherwise (f32.PointTokenizerEngineF32).  forward -> tokens + pos [B*G, trans_dim]."""
    fold_on_host = True

    def __init__(self, sd, a: str, lens, device, gemm_cfg=-1, bn_training=False, arith=None):
        if bn_training:
            raise NotImplementedError("the inference engine folds the running statistics; train-mode BatchNorm = PointTokenizerTrainer")
        self.lens, self.device = lens, torch.device(device)
        self.ar = Bf16Arith(gemm_cfg) if arith is None else arith
        if self.fold_on_host:
            sd = {k: v.detach().cpu() for k, v in sd.items() if k.startswith(a)}
        self.op = {k: _dev(v, device, v.dtype) for k, v in point_tokenizer_operands(sd, a, self.ar.dtype, self.ar.point_kp).items()}

    def group(self, pts: torch.Tensor, fps_start=None, want_idx=False):
        return point_groups(self.lens, pts, fps_start, self.ar, self.op["w1"].shape[1], self.device, want_idx)

    def forward(self, pts: torch.Tensor, fps_start=None) -> torch.Tensor:
        """pts [B,N,3] -> tokens + pos [B*G, trans_dim]."""
        return pointbert_forward(self.op, self.lens, pts, fps_start, self.ar, self.device)


class PointTokenizerTrainer:
    """Trainable PointTokenizer (point_encoder.py:325-362): same dataflow as PointTokenizerEngine but with the
    BatchNorm layers kept apart from the 1x1 convolutions (train-mode batch statistics + running-stat update, or
    eval-mode running statistics), activations kept for the backward pass, and all parameter gradients
    accumulated into `grads` under the reference's parameter names (conv weights as [out, in] matrices;
    the 3-channel inputs are zero-padded to 64 for the GEMM, gradients are cut back to 3 columns).

    FPS / kNN produce indices only (misc.fps, knn_point run under no_grad-equivalent integer ops), so the
    backward stops at the gathered, centre-subtracted patches."""

    BN_EPS, BN_MOMENTUM = 1e-5, 0.1           # nn.BatchNorm1d defaults (dvae.py:186,191)

    def __init__(self, sd, a: str, lens, device, grads=None, gemm_cfg=-1, bn_training=True, bn_sync=None, world_size=1):
        """bn_sync: a communicator (all_gather / all_reduce_sum, e.g. step.TorchComm) turns the two BatchNorm layers into
        SyncBatchNorm over `world_size` ranks (--use-bn-sync); None = per-rank statistics, the reference's default."""
        f32 = self._init_common(sd, a, lens, device, grads, gemm_cfg, bn_training, bn_sync, world_size)
        m = self.masters
        for k in ("encoder.first_conv.0", "encoder.first_conv.3", "encoder.second_conv.0", "encoder.second_conv.3"):
            m[a + k + ".weight"] = f32(k + ".weight")[:, :, 0].contiguous(); m[a + k + ".bias"] = f32(k + ".bias")
        for k in ("encoder.first_conv.1", "encoder.second_conv.1", "reduce_dim", "pos_embed.0", "pos_embed.2"):
            m[a + k + ".weight"] = f32(k + ".weight"); m[a + k + ".bias"] = f32(k + ".bias")
        self.running = {k: (f32(k + ".running_mean"), f32(k + ".running_var")) for k in ("encoder.first_conv.1", "encoder.second_conv.1")}
        self.refresh_operands()

    def _init_common(self, sd, a, lens, device, grads, gemm_cfg, bn_training, bn_sync, world_size):
        """The fields both tokenizer trainers have; -> the reader of an fp32 master (never an alias of the caller's tensor)."""
        self.a, self.lens, self.device, self.cfg, self.bn_training = a, lens, torch.device(device), gemm_cfg, bn_training
        self.bn_sync, self.world = bn_sync, world_size
        self.grads = {} if grads is None else grads
        self.ar = Bf16Arith(gemm_cfg)
        self.masters, self.op, self.ctx = {}, {}, None
        return lambda k: sd[a + k].detach().float().to(device).contiguous().clone()

    def load_params(self, sd):
        """Masters and running statistics re-read from `sd` (reference names and shapes), in place; operands re-derived."""
        for name, m in self.masters.items():
            m.copy_(sd[name].detach().reshape(m.shape))
        for k, (rm, rv) in self.running.items():
            rm.copy_(sd[self.a + k + ".running_mean"]); rv.copy_(sd[self.a + k + ".running_var"])
        self.refresh_operands()

    # bf16 GEMM operands (forward: W, backward: W^T) derived from the f32 masters, under pointbert_forward's names; the biases
    # are the masters themselves
    def refresh_operands(self):
        a, m, o = self.a, self.masters, self.op
        bf = lambda t: t.to(BF).contiguous()

        def padk(w):
            out = torch.zeros(w.shape[0], self.ar.point_kp, device=w.device, dtype=BF)
            out[:, :w.shape[1]] = w.to(BF)
            return out
        w3 = m[a + "encoder.second_conv.0.weight"]
        half = w3.shape[1] // 2
        o["w1"] = padk(m[a + "encoder.first_conv.0.weight"])
        o["w2"] = bf(m[a + "encoder.first_conv.3.weight"]); o["w2T"] = bf(m[a + "encoder.first_conv.3.weight"].t())
        o["w3g"], o["w3l"] = bf(w3[:, :half]), bf(w3[:, half:])
        o["w3gT"], o["w3lT"] = bf(w3[:, :half].t()), bf(w3[:, half:].t())
        o["w4"] = bf(m[a + "encoder.second_conv.3.weight"]); o["w4T"] = bf(m[a + "encoder.second_conv.3.weight"].t())
        o["wr"] = bf(m[a + "reduce_dim.weight"]); o["wrT"] = bf(m[a + "reduce_dim.weight"].t())
        o["wp0"] = padk(m[a + "pos_embed.0.weight"])
        o["wp2"] = bf(m[a + "pos_embed.2.weight"]); o["wp2T"] = bf(m[a + "pos_embed.2.weight"].t())
        for b, k in (("b1", "encoder.first_conv.0"), ("b2", "encoder.first_conv.3"), ("b3", "encoder.second_conv.0"),
                     ("b4", "encoder.second_conv.3"), ("br", "reduce_dim"), ("bp0", "pos_embed.0"), ("bp2", "pos_embed.2")):
            o[b] = m[a + k + ".bias"]

    def grad_buffer(self, name):
        g = self.grads.get(name)
        if g is None:
            g = torch.zeros_like(self.masters[name]); self.grads[name] = g
        return g

    def _bn(self, z, k):
        a, m = self.a, self.masters
        total = None
        if self.bn_training and self.bn_sync is not None:
            rm, rv = self.running[k]
            local = ops.bn_stats_local(z)
            gathered = torch.empty(self.world, local.numel(), device=self.device, dtype=torch.float32)
            self.bn_sync.all_gather(gathered.view(-1), local)
            mean, var, total = ops.bn_stats_merge(gathered, rm, rv, self.BN_MOMENTUM)
        elif self.bn_training:
            rm, rv = self.running[k]
            mean, var = ops.bn_stats(z, rm, rv, self.BN_MOMENTUM)
        else:
            mean, var = self.running[k]
        h = ops.bn_apply(z, mean, var, m[a + k + ".weight"], m[a + k + ".bias"], self.BN_EPS, relu=True)
        return h, (mean, var, total)

    def _bn_bwd(self, dh, z, stats, k):
        a, m = self.a, self.masters
        mean, var, total = stats
        args = (dh, z, mean, var, m[a + k + ".weight"], m[a + k + ".bias"])
        if total is None:
            return ops.bn_bwd(*args, self.grad_buffer(a + k + ".weight"), self.grad_buffer(a + k + ".bias"), self.BN_EPS, relu=True,
                              train=self.bn_training)
        sums = ops.bn_bwd_reduce(*args, self.grad_buffer(a + k + ".weight"), self.grad_buffer(a + k + ".bias"), self.BN_EPS, relu=True)
        self.bn_sync.all_reduce_sum(sums)
        return ops.bn_bwd_apply(*args, sums, total, self.BN_EPS, relu=True)

    def forward(self, pts: torch.Tensor, fps_start=None) -> torch.Tensor:
        """pts [B,N,3] -> tokens + pos, bf16 [B*G, trans_dim]; the activations the backward reads are kept in self.ctx."""
        return pointbert_forward(self.op, self.lens, pts, fps_start, self.ar, self.device, train=self)

    def _dw_into(self, dy, x, g):
        """g += dy^T x (bf16 [rows, *] operands): token-major operands for the dW kernel (narrow channel counts zero-padded to
        whole tiles, ops.gemm_dw_tn_any) - the rows are B * groups * points, two transposed copies of them per weight were
        3 % of the C5 step; the transposing NT path where the row count is not a multiple of 64."""
        ops.weight_grad(dy, x, g, cfg=self.cfg)

    def _dw(self, name, dy, x, cols=None):
        """grads[name] += dy^T x (both bf16 [rows, *])."""
        g = self.grad_buffer(name)
        if cols is None:
            self._dw_into(dy, x, g)
        else:       # zero-padded input channels: compute the padded product, accumulate the real columns
            full = torch.zeros(dy.shape[1], x.shape[1], device=self.device, dtype=torch.float32)
            self._dw_into(dy, x, full)
            ops.axpy(g, full[:, :cols].contiguous(), 1.0)

    def _db(self, name, dy):
        ops.colsum(dy, self.grad_buffer(name))

    def backward(self, dctx: torch.Tensor):
        """dctx f32|bf16 [B*G, trans_dim] = gradient w.r.t. the returned tokens+pos."""
        L, a, m, o, c = self.lens, self.a, self.masters, self.op, self.cfg
        M = L.pc_group_size
        patches, z1, m1, v1, h1, f, g, z3, m3, v3, h2, f2, g2, c3, u, p1, t1, t3 = self.ctx
        dout = dctx if dctx.dtype == BF else ops.cast_bf16(dctx.contiguous())
        # positional MLP: pos = W2 gelu(W0 c + b0) + b2
        self._dw(a + "pos_embed.2.weight", dout, p1); self._db(a + "pos_embed.2.bias", dout)
        du = torch.empty_like(u)
        ops.gemm(dout, o["wp2T"], None, out=du, res=u, epi=ops.EPI_DGELU, act=ops.ACT_GELU_DSAVE, cfg=c)
        self._dw(a + "pos_embed.0.weight", du, c3, cols=3); self._db(a + "pos_embed.0.bias", du)
        # token branch
        self._dw(a + "reduce_dim.weight", dout, g2); self._db(a + "reduce_dim.bias", dout)
        dg2 = ops.gemm(dout, o["wrT"], None, cfg=c)
        df2 = ops.group_max_bwd(f2, dg2, M)
        self._dw(a + "encoder.second_conv.3.weight", df2, h2); self._db(a + "encoder.second_conv.3.bias", df2)
        dh2 = ops.gemm(df2, o["w4T"], None, cfg=c)
        dz3 = self._bn_bwd(dh2, z3, (m3, v3, t3), "encoder.second_conv.1")
        dt = ops.group_sum(dz3, M)
        gw = self.grad_buffer(a + "encoder.second_conv.0.weight")
        half = gw.shape[1] // 2
        self._dw_into(dz3, f, gw[:, half:])
        self._dw_into(dt, g, gw[:, :half])
        self._db(a + "encoder.second_conv.0.bias", dt)
        dg = ops.gemm(dt, o["w3gT"], None, cfg=c)
        dfl = ops.gemm(dz3, o["w3lT"], None, cfg=c)
        df = ops.group_max_bwd(f, dg, M, base=dfl)
        self._dw(a + "encoder.first_conv.3.weight", df, h1); self._db(a + "encoder.first_conv.3.bias", df)
        dh1 = ops.gemm(df, o["w2T"], None, cfg=c)
        dz1 = self._bn_bwd(dh1, z1, (m1, v1, t1), "encoder.first_conv.1")
        self._dw(a + "encoder.first_conv.0.weight", dz1, patches, cols=3); self._db(a + "encoder.first_conv.0.bias", dz1)


class PNSATokenizerTrainer(PointTokenizerTrainer):
    """The `pnsa` point tokenizer (PointNSATokenizer, open_clip/modal_3d/models/pointnet/pointnet_util.py:345-368) on the
    HIP kernels, forward and backward: PointNetSetAbstraction (:184-227: FPS centres, ball query, centre-subtracted xyz ++
    point features, three 1x1 Conv2d + BatchNorm2d + ReLU, max over the group) then `lift` = Conv1d over
    [centre xyz ++ group feature] + LayerNorm.  forward(features [B,N,in_dim], xyz [B,N,3]) -> tokens bf16 [B*S, trans_dim]
    (no positional term: the Sample holds "x" only).

    One class serves inference and training: bn_training=False applies the running statistics and updates nothing.
    FPS / ball query produce indices only, so the backward stops at the gathered rows."""

    def __init__(self, sd, a: str, lens, device, grads=None, gemm_cfg=-1, bn_training=True, bn_sync=None, world_size=1):
        f32 = self._init_common(sd, a, lens, device, grads, gemm_cfg, bn_training, bn_sync, world_size)
        m = self.masters
        for i in range(3):
            w = f32(f"sa.mlp_convs.{i}.weight")
            m[a + f"sa.mlp_convs.{i}.weight"] = w.reshape(w.shape[0], -1).contiguous(); m[a + f"sa.mlp_convs.{i}.bias"] = f32(f"sa.mlp_convs.{i}.bias")
            m[a + f"sa.mlp_bns.{i}.weight"] = f32(f"sa.mlp_bns.{i}.weight"); m[a + f"sa.mlp_bns.{i}.bias"] = f32(f"sa.mlp_bns.{i}.bias")
        wl = f32("lift.0.weight")
        m[a + "lift.0.weight"] = wl.reshape(wl.shape[0], -1).contiguous(); m[a + "lift.0.bias"] = f32("lift.0.bias")
        m[a + "lift.2.weight"] = f32("lift.2.weight"); m[a + "lift.2.bias"] = f32("lift.2.bias")
        self.running = {f"sa.mlp_bns.{i}": (f32(f"sa.mlp_bns.{i}.running_mean"), f32(f"sa.mlp_bns.{i}.running_var")) for i in range(3)}
        self.in_ch = m[a + "sa.mlp_convs.0.weight"].shape[1]               # 3 + in_dim
        self.refresh_operands()

    @staticmethod
    def _pad64(n):
        return (n + 63) // 64 * 64

    def refresh_operands(self):
        a, m, o = self.a, self.masters, self.op

        def padk(w):
            out = torch.zeros(w.shape[0], self._pad64(w.shape[1]), device=w.device, dtype=BF)
            out[:, :w.shape[1]] = w.to(BF)
            return out
        for i in range(3):
            w = m[a + f"sa.mlp_convs.{i}.weight"]
            o[f"w{i}"] = padk(w)
            if i:
                o[f"w{i}T"] = w.t().to(BF).contiguous()
        wl = m[a + "lift.0.weight"]
        o["wl"] = padk(wl)
        o["wlT_feat"] = wl[:, 3:].t().to(BF).contiguous()                    # [C', trans]: dX of the group-feature columns only

    def forward(self, features: torch.Tensor, xyz: torch.Tensor = None, fps_start=None) -> torch.Tensor:
        if xyz is None:
            raise ValueError("the pnsa tokenizer needs the point coordinates: visual(features, xyz=xyz) (pointnet_util.py:362-363)")
        L, a, m, o, c = self.lens, self.a, self.masters, self.op, self.cfg
        S, ns = L.pc_num_group, L.pc_group_size
        xyz = xyz.to(self.device).contiguous().float()
        feats = features.to(self.device).contiguous().float()
        if fps_start is None:       # farthest_point_sample draws its first centre at random (pointnet_util.py:91)
            fps_start = torch.randint(0, xyz.shape[1], (xyz.shape[0],), device=self.device, dtype=torch.long)
        cidx, centers = ops.fps(xyz, fps_start.to(self.device), S)
        patches, bidx = ops.ball_group(xyz, feats, cidx, L.pc_radius, ns, Kp=o["w0"].shape[1], want_idx=True)
        x, zs, stats = patches, [], []
        for i in range(3):
            z = ops.gemm(x, o[f"w{i}"], m[a + f"sa.mlp_convs.{i}.bias"], cfg=c)
            h, st = self._bn(z, f"sa.mlp_bns.{i}")
            zs.append((x, z, h)); stats.append(st)
            x = h
        feat = ops.group_max(x, ns)                                           # [B*S, C']
        Kl = o["wl"].shape[1]
        lift_in = torch.zeros(feat.shape[0], Kl, device=self.device, dtype=BF)
        lift_in[:, :3] = centers.reshape(-1, 3)
        lift_in[:, 3:3 + feat.shape[1]] = feat
        y = ops.gemm(lift_in, o["wl"], m[a + "lift.0.bias"], cfg=c)           # Conv1d(C' + 3 -> trans)
        R, Tr = y.shape
        mean = torch.empty(R, device=self.device, dtype=torch.float32); rstd = torch.empty_like(mean)
        tok = torch.empty(R, Tr, device=self.device, dtype=BF)
        ops.layernorm(y, m[a + "lift.2.weight"], m[a + "lift.2.bias"], tok, R, Tr, mean=mean, rstd=rstd)
        self.ctx = (zs, stats, feat, lift_in, y, mean, rstd)
        self.last_idx = (cidx, bidx)
        return tok

    def backward(self, dctx: torch.Tensor):
        """dctx f32|bf16 [B*S, trans_dim] = gradient w.r.t. the returned tokens."""
        L, a, m, o, c = self.lens, self.a, self.masters, self.op, self.cfg
        ns = L.pc_group_size
        zs, stats, feat, lift_in, y, mean, rstd = self.ctx
        R, Tr = y.shape
        dtok = dctx.contiguous()
        ops.layernorm_bwd_params(dtok, y, mean, rstd, self.grad_buffer(a + "lift.2.weight"), self.grad_buffer(a + "lift.2.bias"), R, Tr)
        dy = torch.empty(R, Tr, device=self.device, dtype=BF)
        ops.layernorm_bwd(dtok, y, mean, rstd, m[a + "lift.2.weight"], R, Tr, dx=dy)
        self._dw(a + "lift.0.weight", dy, lift_in, cols=m[a + "lift.0.weight"].shape[1]); self._db(a + "lift.0.bias", dy)
        dfeat = ops.gemm(dy, o["wlT_feat"], None, cfg=c)                      # [B*S, C']
        dh = ops.group_max_bwd(zs[2][2], dfeat, ns)
        for i in (2, 1, 0):
            x, z, _ = zs[i]
            dz = self._bn_bwd(dh, z, stats[i], f"sa.mlp_bns.{i}")
            self._dw(a + f"sa.mlp_convs.{i}.weight", dz, x, cols=self.in_ch if i == 0 else None)
            self._db(a + f"sa.mlp_convs.{i}.bias", dz)
            if i:
                dh = ops.gemm(dz, o[f"w{i}T"], None, cfg=c)
