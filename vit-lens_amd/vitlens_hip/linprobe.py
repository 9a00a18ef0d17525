"""Linear probing on the HIP kernels (the reference's open_clip/linprobe_model.py ViTLensLP + training/optimizer.py LARS):
a frozen tower's pooled feature -> Dropout -> BatchNorm1d(affine=False, eps=1e-6) -> Linear, label cross-entropy, LARS.

    ProbeHead        the head alone, from given features: fp32 weight / bias, running statistics, LARS momenta, workspaces.
                     forward = vl_lp_bn_fwd + vl_gemm_f32; backward = vl_ce_label + vl_gemm_f32 (dW = GT xhatT^T);
                     optimizer_step = (vl_sumsq_f32 when clipping) + vl_lars_multi_step; hits = vl_topk_hits.
    LinearProbeStep  backbone forward (no graph) + the head's step, no host read anywhere: 8 launches behind the backbone.

The head runs in true fp32: it is about 2 B C D flops against a whole ViT forward, 16-bit operands would gain nothing."""
import torch

from . import ops

BN_EPS = 1e-6            # nn.BatchNorm1d(lp_input_dim, affine=False, eps=1e-6)
BN_MOMENTUM = 0.1        # nn.BatchNorm1d's default, which the reference leaves alone
STATE_KEYS = ("lp_head.1.running_mean", "lp_head.1.running_var", "lp_head.1.num_batches_tracked", "lp_head.2.weight",
              "lp_head.2.bias")


def _pad4(n):
    return (int(n) + 3) // 4 * 4


class ProbeHead:
    """Dropout(p) -> BatchNorm1d(D, affine=False, eps=1e-6) -> Linear(D, C) with its cross-entropy backward and LARS.
    weight / bias: the initial values (f32 [C, D] / [C]); None draws nn.Linear's default initialisation.  With `params`
    (weight, bias tensors on the device) the head works ON those tensors instead of on copies (the module path)."""

    def __init__(self, in_dim, num_classes, device, dropout=0.0, weight=None, bias=None, weight_decay=0.0, momentum=0.9,
                 trust_coefficient=1e-3, drop_seed=0, params=None):
        D, C = int(in_dim), int(num_classes)
        if D < 4 or D % 4:
            raise ValueError(f"ProbeHead: the feature width must be a multiple of 4, got {D}")
        if C < 1:
            raise ValueError("ProbeHead: at least one class")
        if not 0.0 <= float(dropout) < 1.0:
            raise ValueError(f"ProbeHead: dropout must be in [0, 1), got {dropout}")
        self.D, self.C, self.device = D, C, torch.device(device)
        self.dropout, self.drop_seed = float(dropout), int(drop_seed)
        self.weight_decay, self.momentum, self.trust_coefficient = float(weight_decay), float(momentum), float(trust_coefficient)
        f = dict(device=self.device, dtype=torch.float32)
        if params is not None:
            self.weight, self.bias = params
            if tuple(self.weight.shape) != (C, D) or tuple(self.bias.shape) != (C,):
                raise ValueError("ProbeHead: params must be (weight [C, D], bias [C])")
        else:
            if weight is None:
                lin = torch.nn.Linear(D, C)
                weight, bias = lin.weight.detach(), lin.bias.detach()
            self.weight = weight.detach().to(**f).contiguous().clone()
            self.bias = bias.detach().to(**f).contiguous().clone()
        self.running_mean, self.running_var = torch.zeros(D, **f), torch.ones(D, **f)
        self.num_batches_tracked = 0
        self.mu_w, self.mu_b = torch.zeros(C, D, **f), torch.zeros(C, **f)
        self.flat_grad = torch.zeros(C * D + C, **f)          # dW then db: one buffer, one squared norm
        self.dw, self.db = self.flat_grad[:C * D].view(C, D), self.flat_grad[C * D:]
        self.loss = torch.zeros(1, **f)
        self.hit_counts = torch.zeros(2, device=self.device, dtype=torch.int32)
        self.forwards = 0                                     # generation of xhat / xhatT (a backward belongs to one forward)
        self.samples_seen = 0                                 # Philox sample number of the next train-mode row
        self._sumsq = torch.zeros(1, **f)
        self._B = None
        self._slots = self._slot_key = None
        self._lars_ws = torch.empty(ops.lars_ws_floats(C * D + C, 2) // 2 + 1, device=self.device, dtype=torch.float64)

    def _buffers(self, B):
        if self._B != B:
            f = dict(device=self.device, dtype=torch.float32)
            self.xhat, self.xhatT = torch.empty(B, self.D, **f), torch.empty(self.D, _pad4(B), **f)
            self.logits, self.GT = torch.empty(B, self.C, **f), torch.empty(self.C, _pad4(B), **f)
            self._ce_ws = torch.empty(ops.ce_label_ws_floats(B, self.C), **f)
            self._B = B

    def forward(self, feat, train, keep=None, sample0=None):
        """feat f32 [B, D] on the device -> logits f32 [B, C] (the head's buffer: valid until the next forward).  train: batch
        statistics (and the running ones move), dropout with `keep` (u8 / bool [B, D]) or, without it, the kernel's own draw
        for the samples sample0 .. (default: the rows this head has seen in train mode so far)."""
        if feat.dim() != 2 or feat.shape[1] != self.D or feat.dtype != torch.float32:
            raise ValueError(f"ProbeHead.forward: features must be f32 [B, {self.D}], got {feat.dtype} {tuple(feat.shape)}")
        B = feat.shape[0]
        self._buffers(B)
        self.forwards += 1
        if train:
            s0 = self.samples_seen if sample0 is None else int(sample0)
            ops.lp_bn_fwd(feat, self.running_mean, self.running_var, True, p=self.dropout, keep=keep, seed=self.drop_seed,
                          sample0=s0, momentum=BN_MOMENTUM, eps=BN_EPS, xhat=self.xhat, xhatT=self.xhatT)
            self.num_batches_tracked += 1
            if sample0 is None:
                self.samples_seen += B
        else:
            ops.lp_bn_fwd(feat, self.running_mean, self.running_var, False, eps=BN_EPS, xhat=self.xhat)
        ops.gemm_f32(self.xhat, self.weight, bias=self.bias, out=self.logits)
        return self.logits

    def backward(self, logits, target, gscale=1.0):
        """nn.CrossEntropyLoss()(logits, target) -> self.loss, and its gradients -> self.dw, self.db (times gscale); the
        normalised features are those of the last train-mode forward."""
        ops.ce_label(logits, target, gscale=gscale, loss=self.loss, GT=self.GT, dbias=self.db, ws=self._ce_ws)
        self.weight_grad_from(self.GT)
        return self.loss

    def weight_grad_from(self, GT):
        """dW = dlogits^T xhat as ONE GEMM over the zero-padded transposes: GT [C, pad4(B)] against xhatT [D, pad4(B)]."""
        ops.gemm_f32(GT, self.xhatT, out=self.dw)

    def _slot_table(self, p_w, g_w, mu_w, p_b, g_b, mu_b):
        key = tuple(t.data_ptr() for t in (p_w, g_w, mu_w, p_b, g_b, mu_b)) + (self.weight_decay,)
        if key != self._slot_key:
            host = ops.pack_lars_slots([(p_w, g_w, mu_w, self.weight_decay, True), (p_b, g_b, mu_b, self.weight_decay, False)])
            self._slots, self._slot_key = host.to(self.device), key
        return self._slots

    def optimizer_step(self, lr, grad_scale=1.0, max_norm=None):
        """One LARS step on (weight, bias) with the gradients of the last backward; max_norm: clip_grad_norm_ first."""
        slots = self._slot_table(self.weight, self.dw, self.mu_w, self.bias, self.db, self.mu_b)
        clip = max_norm is not None and float(max_norm) > 0.0
        if clip:
            ops.grad_sumsq(self.flat_grad, out=self._sumsq)
        ops.lars_multi_step(slots, 2, lr, self.momentum, self.trust_coefficient, grad_scale, max_norm if clip else None,
                            self._sumsq if clip else None, ws=self._lars_ws)

    def hits(self, logits, target, ks=(1, 5)):
        """Adds the top-k hit counts of this batch into self.hit_counts (int32 [2] on the device) and returns it."""
        return ops.topk_hits(logits, target, ks, hits=self.hit_counts)[0]

    def state_dict(self):
        return {"lp_head.1.running_mean": self.running_mean.clone(), "lp_head.1.running_var": self.running_var.clone(),
                "lp_head.1.num_batches_tracked": torch.tensor(self.num_batches_tracked, dtype=torch.long),
                "lp_head.2.weight": self.weight.clone(), "lp_head.2.bias": self.bias.clone()}

    def load_state_dict(self, sd):
        missing = [k for k in STATE_KEYS if k not in sd]
        if missing:
            raise KeyError(f"ProbeHead.load_state_dict: missing {missing}")
        with torch.no_grad():
            self.running_mean.copy_(sd["lp_head.1.running_mean"]); self.running_var.copy_(sd["lp_head.1.running_var"])
            self.weight.copy_(sd["lp_head.2.weight"]); self.bias.copy_(sd["lp_head.2.bias"])
        self.num_batches_tracked = int(sd["lp_head.1.num_batches_tracked"])


class LinearProbeStep:
    """The reference's linear-probe recipe as one step object: `backbone` (an open_clip VisionTransformer on the GPU, frozen)
    in train mode without a graph, the head, nn.CrossEntropyLoss(), both gradients and LARS - nothing is read on the host.
    enable_vit_proj=False drops the tower's output projection (`backbone.proj = None`): the head sees ln_post(cls)."""

    def __init__(self, backbone, num_classes, lr, weight_decay=0.0, momentum=0.9, trust_coefficient=1e-3, dropout=0.0,
                 enable_vit_proj=False, grad_clip_norm=None, drop_seed=0, weight=None, bias=None):
        if any(p.requires_grad for p in backbone.parameters()):
            raise NotImplementedError("LinearProbeStep: the backbone is frozen in this recipe (a parameter requires grad); "
                                      "fine-tuning through the head is not built")
        if not enable_vit_proj:
            backbone.drop_output_projection()
        self.backbone, self.lr, self.grad_clip_norm = backbone, float(lr), grad_clip_norm
        dev = backbone.class_embedding.device
        self.head = ProbeHead(backbone.embed_dim, num_classes, dev, dropout=dropout, weight=weight, bias=bias,
                              weight_decay=weight_decay, momentum=momentum, trust_coefficient=trust_coefficient, drop_seed=drop_seed)

    def features(self, x, train):
        self.backbone.train(train)
        with torch.no_grad():
            return self.backbone(x).float().contiguous()

    def step(self, x, target, lr=None):
        """One training step on the batch -> the loss, a 1-element device tensor."""
        h = self.head
        self.feat = self.features(x, True)          # (kept for inspection until the next step)
        logits = h.forward(self.feat, True)
        h.backward(logits, target.to(h.device))
        h.optimizer_step(self.lr if lr is None else float(lr), max_norm=self.grad_clip_norm)
        return h.loss.clone()

    def evaluate(self, x, target, ks=(1, 5)):
        """Eval mode -> the top-k hit counts of this batch, int32 [2] on the device."""
        h = self.head
        logits = h.forward(self.features(x, False), False)
        return ops.topk_hits(logits, target.to(h.device), ks)[0]

    def state_dict(self):
        return self.head.state_dict()

    def load_state_dict(self, sd):
        self.head.load_state_dict(sd)
