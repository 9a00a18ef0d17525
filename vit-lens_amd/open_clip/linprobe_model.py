"""`ViTLensLP`, the linear-probe model of the reference (open_clip/linprobe_model.py): the `visual` tower of a TriCLIP as a
frozen backbone and `lp_head` = Dropout -> BatchNorm1d(affine=False, eps=1e-6) -> Linear on its pooled feature.  Same
constructor arguments, attribute names and state_dict keys, so probe checkpoints move both ways.

`lp_head` holds the parameters and the running statistics; the arithmetic is vitlens_hip.linprobe.ProbeHead working on those
very tensors.  forward is one autograd.Function that yields `.grad` for `lp_head.2.weight` and `lp_head.2.bias` only: the
backbone runs its no-grad forward (train mode included: the point tokenizer's BatchNorm then uses batch statistics, as the
reference's `model.train()` makes it), and there is no gradient into the features.

`LabelCrossEntropyLoss` is nn.CrossEntropyLoss() on vl_ce_label; handed the logits of a ViTLensLP it also leaves the
transposed gradient and the bias gradient for the head's backward, so that `loss.backward(); optimizer.step()` with
training.optimizer.LARS runs the launches of vitlens_hip.linprobe.LinearProbeStep and gives the same bits.  Any other loss works
too (the gradient of the logits is then transposed and column-summed behind it)."""
import logging

import torch
import torch.nn as nn

from .factory import tri_create_model_and_transforms


def pt_load(file_path, map_location=None):
    return torch.load(file_path, map_location=map_location)


class _Link:
    """What a LabelCrossEntropyLoss leaves for the head's backward: its gradient tensor, the padded transpose, the bias gradient."""
    grad = gt = dbias = None


class _HeadFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, module, feat, link, weight, bias):
        head = module._executor()
        train = module.lp_head.training
        bn = module.lp_head[1]
        logits = head.forward(feat, train)
        if train:
            bn.num_batches_tracked += 1
        ctx.head, ctx.link, ctx.gen = head, link, head.forwards
        return logits.clone()

    @staticmethod
    def backward(ctx, dlogits):
        from vitlens_hip import ops
        head, link = ctx.head, ctx.link
        if head.forwards != ctx.gen:
            raise RuntimeError("the probe head ran another forward before this backward: its normalised features "
                               "were overwritten.  Run backward after each forward.")
        B, C = dlogits.shape
        if link.grad is not None and link.grad.data_ptr() == dlogits.data_ptr():
            gt, db = link.gt, link.dbias                       # left by LabelCrossEntropyLoss: vl_ce_label's own outputs
        else:
            d = dlogits.contiguous().float()
            gt = torch.zeros(C, head.GT.shape[1], device=d.device, dtype=torch.float32)
            gt[:, :B] = d.t()
            db = torch.zeros(C, device=d.device, dtype=torch.float32)
            ops.colsum(d, db)
        head.weight_grad_from(gt)
        return None, None, None, head.dw.clone(), db.clone()


class _CEFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, target, link):
        from vitlens_hip import ops
        lg = logits.detach()
        if lg.dtype != torch.float32 or lg.stride(-1) != 1:
            lg = lg.float().contiguous()
        loss, G, GT, dbias = ops.ce_label(lg, target, need_g=True, need_gt=link is not None, need_dbias=link is not None)
        ctx.G, ctx.GT, ctx.dbias, ctx.link = G, GT, dbias, link
        return loss.reshape(())

    @staticmethod
    def backward(ctx, dloss):
        g = ctx.G.mul_(dloss)                                  # a device scalar (1, or a GradScaler's scale): no host read
        if ctx.link is not None:
            ctx.link.grad, ctx.link.gt, ctx.link.dbias = g, ctx.GT.mul_(dloss), ctx.dbias.mul_(dloss)
        return g, None, None


class LabelCrossEntropyLoss(nn.Module):
    """torch.nn.CrossEntropyLoss() (mean reduction, no weights, no smoothing) on the GPU kernel: logits [B, C], target int64 [B]."""

    def forward(self, logits, target):
        return _CEFn.apply(logits, target, getattr(logits, "_lp_link", None))


class ViTLensLP(nn.Module):
    def __init__(self, args):
        super().__init__()
        self.args = args
        model, _, _ = tri_create_model_and_transforms(
            args.model, args.pretrained, precision=args.precision, device="cpu", jit=False,
            force_quick_gelu=args.force_quick_gelu, force_custom_text=args.force_custom_text, force_patch_dropout=False,
            force_image_size=args.force_image_size, pretrained_image=args.pretrained_image, load_ckpt_strict=False,
            image_mean=None, image_std=None, aug_cfg=None, output_dict=True, cache_dir=args.cache_dir, args=args)
        self.backbone = model.visual          # (the text and image towers are not kept)
        if args.lp_enable_vit_proj:
            lp_input_dim = self.backbone.embed_dim
        else:
            self.backbone.drop_output_projection()      # `backbone.proj = None`: the tower returns ln_post(cls)
            lp_input_dim = self.backbone.cfg.width
        self.lp_head = nn.Sequential(nn.Dropout(args.lp_dropout_rate), nn.BatchNorm1d(lp_input_dim, affine=False, eps=1e-6),
                                     nn.Linear(lp_input_dim, args.lp_num_classes))
        self._head = self._head_key = None

    def _executor(self):
        """The ProbeHead working on lp_head's own tensors (rebuilt when they move: .to(device), load_state_dict keeps them)."""
        from vitlens_hip.linprobe import ProbeHead
        bn, lin = self.lp_head[1], self.lp_head[2]
        w, b = lin.weight.data, lin.bias.data
        if not w.is_cuda:
            raise RuntimeError("the ViT-Lens towers run on the MI355X kernels only: move the model to a GPU")
        key = (w.data_ptr(), b.data_ptr(), bn.running_mean.data_ptr(), bn.running_var.data_ptr())
        if self._head is None or key != self._head_key:
            head = ProbeHead(w.shape[1], w.shape[0], w.device, dropout=self.lp_head[0].p, params=(w, b),
                             drop_seed=int(getattr(self.args, "seed", 0) or 0))
            head.running_mean, head.running_var = bn.running_mean, bn.running_var
            self._head, self._head_key = head, key
        self._head.dropout = float(self.lp_head[0].p)
        return self._head

    def forward(self, x, **kwargs):
        if any(p.requires_grad for p in self.backbone.parameters()):
            raise NotImplementedError("ViTLensLP: a backbone parameter requires grad.  The linear probe trains lp_head only "
                                      "(call lp_lock_parameters()); fine-tuning through the head is not this recipe.")
        with torch.no_grad():
            feat = self.backbone(x, **kwargs).float().contiguous()
        lin = self.lp_head[2]
        link = _Link()
        logits = _HeadFn.apply(self, feat, link, lin.weight, lin.bias)
        logits._lp_link = link
        return logits

    def lp_lock_parameters(self):
        """Only lp_head trains: every other parameter is frozen."""
        head = {id(p) for p in self.lp_head.parameters()}
        for p in self.parameters():
            p.requires_grad = id(p) in head

    def load_vitlens_weights_from_ckpt(self, args):
        """The `visual.` entries of a ViT-Lens training checkpoint (args.lp_ckpt_path; with or without DistributedDataParallel's
        `module.` prefix) -> the backbone, non-strict."""
        sd = pt_load(args.lp_ckpt_path, map_location="cpu")["state_dict"]
        strip = len("module.") if next(iter(sd)).startswith("module.") else 0
        tower = {k[strip + len("visual."):]: v for k, v in sd.items() if k[strip:].startswith("visual.")}
        msg = self.backbone.load_state_dict(tower, strict=False)
        logging.info(f"[Linear Probe load ViT-Lens Pretrained ckpt] : {msg}.")
