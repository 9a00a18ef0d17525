"""One tri-modal contrastive training step (the reference's `tri_train_one_epoch` loop body,
training/train.py:115-249) for the depth recipe, entirely on the HIP kernels:

    image tower fwd (frozen) | text tower fwd (frozen) | Lens(depth)->ViT fwd (saved activations)
      -> [one packed RCCL all-gather of img|txt|vis embeddings when world_size > 1]
      -> TriClipLoss (logits GEMM + fused row/col CE) and its gradient w.r.t. the visual embeddings
      -> backward through the visual tower (dX all blocks, dW for the unlocked first n + adapter)
      -> [one flat RCCL all-reduce of the fp32 gradient buffer = DDP mean]
      -> AdamW on the fp32 masters, bf16 operand refresh, logit_scale.clamp_(0, ln 100)

Micro-batching follows the reference's feature-cache scheme (train.py:154-210): every micro-batch sees the
full batch of negatives; here the activations of all micro-batches stay resident in the 288 GB of HBM so
nothing is recomputed.
"""
import math
from typing import Dict, Optional

import torch

from . import ops
from .engine import LensCfg, LensEngine, TextCfg, TextEngine, TowerCfg, VitEngine
from .train import AdamW, DepthLensTrainer, at_path


class TorchComm:
    """The two collectives of a step on `torch.distributed` (backend "nccl" = RCCL over xGMI, one process per GPU).
    A step takes any object with these two methods (the tests drive two ranks on one GPU through an in-process one)."""

    def all_gather(self, out: torch.Tensor, inp: torch.Tensor):
        import torch.distributed as dist
        if inp.is_cuda:
            dist.all_gather_into_tensor(out, inp)
        else:          # gloo
            dist.all_gather(list(out.chunk(dist.get_world_size(), dim=0)), inp.contiguous())

    def all_reduce_sum(self, t: torch.Tensor):
        import torch.distributed as dist
        dist.all_reduce(t, op=dist.ReduceOp.SUM)

    def reduce_scatter_sum(self, out: torch.Tensor, inp: torch.Tensor):
        """out [b, E] = this rank's slice of the sum over ranks of inp [W*b, E] (backward of a gather WITH grad)."""
        import torch.distributed as dist
        if inp.is_cuda:
            dist.reduce_scatter_tensor(out, inp, op=dist.ReduceOp.SUM)
        else:          # gloo (CPU tests) has no reduce_scatter
            t = inp.clone()
            dist.all_reduce(t, op=dist.ReduceOp.SUM)
            r = dist.get_rank()
            out.copy_(t[r * out.shape[0]:(r + 1) * out.shape[0]])

    def all_reduce_sum_async(self, t: torch.Tensor):
        """Start an all-reduce and return a handle with .wait(): on RCCL the collective runs on the communicator's own
        stream behind the kernels already enqueued, so a gradient bucket is reduced under the rest of the backward."""
        import torch.distributed as dist
        return dist.all_reduce(t, op=dist.ReduceOp.SUM, async_op=True)


class AbiComm:
    """The same collectives through the library's OWN RCCL entry points (include/vitlens_hip.h: vl_comm_create,
    vl_allgather_embed, vl_reducescatter_grad, vl_allreduce_grad; csrc/vl_comm.cpp) instead of torch.distributed - the calls a
    non-Python host of the C ABI makes, driven from Python so that they are tested with the steps.  fp32 payloads (what the steps
    exchange).  The 128-byte unique id is made on rank 0 and shipped by the caller: `AbiComm.over_torch_distributed()` uses an
    initialised process group (any backend) for that one broadcast; a one-rank communicator needs no shipping."""

    def __init__(self, rank: int = 0, world: int = 1, unique_id: Optional[bytes] = None, device=None):
        import ctypes as C
        from ._lib import check, load_library
        self._lib, self._check, self._C = load_library(), check, C
        self.rank, self.world = rank, world
        if device is not None:
            torch.cuda.set_device(device)
        if unique_id is None:
            if world != 1:
                raise ValueError("AbiComm: ranks > 0 need the unique id rank 0 made (AbiComm.make_unique_id / over_torch_distributed)")
            unique_id = self.make_unique_id()
        if len(unique_id) != 128:
            raise ValueError("AbiComm: the unique id is 128 bytes")
        self._h = C.c_void_p()
        buf = C.create_string_buffer(bytes(unique_id), 128)
        check(self._lib.vl_comm_create(C.byref(self._h), buf, rank, world))
        self._stream = None          # the bucket all-reduces run on their own stream, beside the backward

    @staticmethod
    def make_unique_id() -> bytes:
        import ctypes as C
        from ._lib import check, load_library
        buf = C.create_string_buffer(128)
        check(load_library().vl_comm_unique_id(buf))
        return buf.raw

    @classmethod
    def over_torch_distributed(cls, device=None):
        import torch.distributed as dist
        rank, world = dist.get_rank(), dist.get_world_size()
        box = [cls.make_unique_id() if rank == 0 else None]
        dist.broadcast_object_list(box, src=0)
        return cls(rank, world, box[0], device)

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._lib.vl_comm_destroy(self._h)
            self._h = self._C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:          # interpreter shutdown: the library or ctypes may already be gone
            pass

    def _s(self):
        return self._C.c_void_p(torch.cuda.current_stream().cuda_stream)

    @staticmethod
    def _f32(t, name):
        if t.dtype != torch.float32 or not t.is_contiguous() or not t.is_cuda:
            raise ValueError(f"AbiComm.{name}: contiguous fp32 GPU tensors only")
        return t

    def all_gather(self, out: torch.Tensor, inp: torch.Tensor):
        self._f32(out, "all_gather"); inp = self._f32(inp.contiguous(), "all_gather")
        self._check(self._lib.vl_allgather_embed(self._h, inp.data_ptr(), out.data_ptr(), inp.numel(), self._s()))

    def all_reduce_sum(self, t: torch.Tensor):
        self._f32(t, "all_reduce_sum")
        self._check(self._lib.vl_allreduce_grad(self._h, t.data_ptr(), t.numel(), self._s()))

    def reduce_scatter_sum(self, out: torch.Tensor, inp: torch.Tensor):
        self._f32(out, "reduce_scatter_sum"); inp = self._f32(inp.contiguous(), "reduce_scatter_sum")
        self._check(self._lib.vl_reducescatter_grad(self._h, inp.data_ptr(), out.data_ptr(), out.numel(), self._s()))

    def all_reduce_sum_async(self, t: torch.Tensor):
        """The bucket's all-reduce on the communicator's own stream behind what the launch stream has enqueued so far;
        .wait() makes the launch stream wait for it."""
        self._f32(t, "all_reduce_sum_async")
        if self._stream is None:
            self._stream = torch.cuda.Stream()
        main = torch.cuda.current_stream()
        ready, done = torch.cuda.Event(), torch.cuda.Event()
        ready.record(main)
        self._stream.wait_event(ready)
        with torch.cuda.stream(self._stream):
            self.all_reduce_sum(t)
            done.record(self._stream)

        class _Handle:
            def wait(self_h):
                torch.cuda.current_stream().wait_event(done)
        return _Handle()


# ------------------------------------------------------------------------------------------------ checkpointing
def _master_from_sd(name: str, sd, like: torch.Tensor) -> torch.Tensor:
    """Value of master `name` (kernel layout) from a reference-layout state_dict."""
    from .engine import conv_weight_as_gemm, interleave_geglu
    dev = like.device
    f32 = lambda k: sd[k].detach().float().to(dev).clone()
    if name.endswith("conv1.weight_gemm"):                       # conv-as-GEMM, K zero-padded to 64
        return conv_weight_as_gemm(sd[name[:-5]], dev, torch.float32)
    if name.endswith("net.0.weight_il") or name.endswith("net.0.bias_il"):      # GEGLU rows interleaved (a_j, gate_j)
        base = name[:name.rindex("net.0.")] + "net.0."
        w, b = interleave_geglu(f32(base + "weight"), f32(base + "bias"))
        return (w if name.endswith("weight_il") else b).contiguous()
    if name.endswith("fn.to_qkv.weight"):                        # self-attention: [to_q ; to_kv]
        return torch.cat([f32(name.replace("to_qkv", "to_q")), f32(name.replace("to_qkv", "to_kv"))], 0).contiguous()
    return f32(name).reshape(like.shape).contiguous()


def _master_to_sd(name: str, m: torch.Tensor, base_sd, cfg) -> Dict[str, torch.Tensor]:
    """Reference-layout entries produced by master `name`."""
    from .train import deinterleave_geglu
    if name.endswith("conv1.weight_gemm"):
        ref = base_sd[name[:-5]]
        return {name[:-5]: m[:, :ref[0].numel()].reshape(ref.shape)}
    if name.endswith("_il"):
        return {name[:-3]: deinterleave_geglu(m)}
    if name.endswith("fn.to_qkv.weight"):
        inner = cfg.latent_heads * cfg.latent_dim_head
        return {name.replace("to_qkv", "to_q"): m[:inner], name.replace("to_qkv", "to_kv"): m[inner:]}
    return {name: m.reshape(base_sd[name].shape)}


# ------------------------------------------------------------------------------------------------ patch dropout
DROP_TOWER_VISUAL, DROP_TOWER_IMAGE = 0, 1      # tower ids of `drop_sample0`
DROP_TOWER_LENS = 2                             # the Perceiver's own attention / FeedForward dropout (csrc/vl_lens_drop.hip)
_DROP_OFFSET_BITS, _DROP_TOWER_BITS, _DROP_RANK_BITS, _DROP_STEP_BITS = 20, 2, 14, 27


def drop_sample0(step: int, rank: int, tower: int, offset: int) -> int:
    """The Philox sample number (vl_patch_keep's `sample0 + b`) of the sample at `offset` in the per-GPU batch, for tower
    `tower` of rank `rank` at optimizer step count `step` - a 63-bit field layout, so no two of them share keys:

        sample0 = (step mod 2^27) << 36  |  rank << 22  |  tower << 20  |  offset        rank < 2^14, tower < 4, offset < 2^20

    A micro-batch that starts at `offset` passes this as sample0 and the kernel adds the row index: the kept set of a sample
    depends on its place in the per-GPU batch, not on the micro-batch size."""
    if not (0 <= rank < 1 << _DROP_RANK_BITS and 0 <= tower < 1 << _DROP_TOWER_BITS and 0 <= offset < 1 << _DROP_OFFSET_BITS):
        raise ValueError(f"drop_sample0: rank {rank}, tower {tower} or sample offset {offset} outside the key layout "
                         f"(rank < 2^{_DROP_RANK_BITS}, tower < 2^{_DROP_TOWER_BITS}, offset < 2^{_DROP_OFFSET_BITS})")
    step = int(step) & ((1 << _DROP_STEP_BITS) - 1)
    o, t = _DROP_OFFSET_BITS, _DROP_OFFSET_BITS + _DROP_TOWER_BITS
    return (step << (t + _DROP_RANK_BITS)) | (rank << t) | (tower << o) | offset


class _StepState:
    """What the fused training steps have in common, one copy of each piece: the step (`_forward_backward`, `finish_reduce`,
    `optimizer_step`, `step`), the flat gradient buffers and their per-block buckets, the trainers of the micro-batches.  A
    step class supplies what differs: `_build` (engines, masters, the trainer factory `_mk`), `_refresh_operands`, and
    where needed `_share_operands`, `_bind_grads`, `_bucket_blocks`, `_loss`, `pack_text`.

    state_dict / load_state_dict of a step in the REFERENCE's names and layouts (a TriCLIP state_dict:
    trained tensors from the fp32 masters, everything else as it was given), plus the AdamW moments - so training can be
    checkpointed, resumed, and handed back to `TriCLIP.load_state_dict` (training/train.py checkpoints `model.state_dict()`
    and `optimizer.state_dict()`).

    patch_dropout / drop_seed (--force-patch-dropout; PatchDropout, open_clip/transformer.py:53-90): with patch_dropout > 0
    every ViT tower of the step - the trainable `visual` tower and, where there is one, the frozen `image` tower, which the
    reference's model.train() puts in train mode too - keeps the class token and K = max(1, int(T (1 - p))) of the T tokens
    in front of its trunk, per micro-batch.  The keys are drawn on the device (vl_patch_keep with keys = NULL: Philox4x32-10,
    no host round trip, no torch RNG): key words (lo32, hi32) of `drop_seed`, and for the sample at offset o of the per-GPU
    batch the sample number `drop_sample0(self.opt.t, rank, tower, o)`,

        ((opt.t mod 2^27) << 36) | (rank << 22) | (tower << 20) | o        tower: 0 = visual, 1 = image

    with opt.t the number of optimizer steps taken so far (checkpointed by `optimizer_state_dict`).  So two towers, ranks,
    steps or samples never share keys, a resumed run draws what the uninterrupted run would have drawn, and a sample's kept
    set does not depend on the micro-batch size.  (Two forward_backward calls without an optimizer step between them draw the
    same sets.)  The default 0.0 is the code path without the argument: no launch is added.

    perceiver_attn_dropout / perceiver_ff_dropout (--perceiver_attn_dropout, --perceiver_ff_dropout; perceiver.py:91-102, 105-154;
    the steps whose Lens has a Perceiver): nn.Dropout on the attention probabilities and behind every FeedForward of the Lens.
    The masks are never stored - forward and backward of a micro-batch, on whichever stream, redraw them from numbers
    (csrc/vl_lens_drop.hip): the same `drop_seed`, the sample number `drop_sample0(opt.t, rank, DROP_TOWER_LENS = 2, o)` and the
    sub-layer's position in the forward.  The properties above hold for them in the same way; 0.0 adds no launch."""

    def _init_host(self, sd, device, micro_batch, rank, world_size, comm=None, local_loss=False, gather_with_grad=False,
                   force_comm=False, overlap_frozen=False, overlap_backward=True, grad_clip_norm=None,
                   patch_dropout: float = 0.0, drop_seed: int = 0, perceiver_attn_dropout: float = 0.0,
                   perceiver_ff_dropout: float = 0.0):
        """Everything of a step that is HOST state - flags, the communicator, the (still empty apart from logit_scale) master
        table, the gradient-bucket bookkeeping - and nothing that touches an engine or a kernel.  Every step's `__init__`
        runs this first and then its `_build()` (engines, masters of the trainable set); tests/test_step_gloo.py drives the
        REAL `__init__` of the product classes on CPU + gloo with `_build` / `_trainer` / `_refresh_operands` overridden by
        linear stand-in towers, so a field added here can never be missing from the object under test."""
        self.dev, self.mb, self.rank, self.world = torch.device(device), micro_batch, rank, world_size
        # the multi-rank path (packed all-gather, bucketed async all-reduce, optional reduce-scatter) runs when there are
        # peers - or when asked for on ONE rank, so that the RCCL calls execute on a single GPU (tests, bench --force-dist)
        self._force_comm = bool(force_comm)
        self.comm = comm or TorchComm()
        self.local_loss, self.gather_with_grad = local_loss, gather_with_grad
        # the frozen towers' forwards on a second HIP stream beside the trainable tower's forward: a request;
        # `_overlap_active` says whether this device can honour it (a CPU device - the gloo tests - runs the serial order,
        # the same arithmetic)
        self.overlap_frozen = bool(overlap_frozen)
        # with it: the two halves of a step's micro-batches run their BACKWARD on the two streams too (_backward_all)
        self.overlap_backward = bool(overlap_backward)
        self._one_stream_backward = False      # a `_build` whose backward talks to the communicator (SyncBatchNorm) sets it
        self._side = None
        self._base_sd = {k: v.detach() for k, v in sd.items()}
        self.logit_scale = sd["logit_scale"].detach().float().reshape(1).to(device).clone()
        self.masters: Dict[str, torch.Tensor] = {"logit_scale": self.logit_scale}
        self.bf16_targets = {}   # depth step: master name -> (block, operand key)
        self.refresh = []        # Perceiver steps: (master name, forward bf16 tensor, key path of the transposed copy in trainer.perc.wT)
        self.trainers = []       # one activation store per micro-batch (created lazily)
        self.flat_grad, self.grads = None, {}
        self._pending, self._reduced_upto, self._reduce_done = [], None, False
        # --grad-clip-norm / training.grad_clip_norm: clip the global norm of the (mean) gradient before AdamW; None = off
        if grad_clip_norm is not None and not float(grad_clip_norm) > 0.0:
            raise ValueError(f"grad_clip_norm must be positive (or None), got {grad_clip_norm}")
        self.grad_clip_norm = None if grad_clip_norm is None else float(grad_clip_norm)
        self._sumsq = None
        # --force-patch-dropout: the fraction of tokens every ViT tower of the step drops (None / False: off, as in the factory)
        self.patch_dropout = float(patch_dropout or 0.0)
        if self.patch_dropout > 0.0:
            assert 0 <= self.patch_dropout < 1.0, f"patch_dropout must be in [0, 1), got {self.patch_dropout}"
            drop_sample0(0, rank, 0, 0)                # (a rank outside the key layout is refused here, not in the first step)
        self.drop_seed = int(drop_seed)
        # --perceiver_attn_dropout / --perceiver_ff_dropout: nn.Dropout inside the Lens's Perceiver (class docstring)
        self.perceiver_attn_dropout, self.perceiver_ff_dropout = float(perceiver_attn_dropout or 0.0), float(perceiver_ff_dropout or 0.0)
        self._lens_drop = False          # a `_build` with a Perceiver that drops sets it (_collect_perceiver)
        for name in ("perceiver_attn_dropout", "perceiver_ff_dropout"):
            if not 0.0 <= getattr(self, name) < 1.0:
                raise ValueError(f"{name} must be in [0, 1), got {getattr(self, name)}")
        if self.perceiver_attn_dropout > 0.0 or self.perceiver_ff_dropout > 0.0:
            drop_sample0(0, rank, DROP_TOWER_LENS, 0)

    def _lens_cfg(self, lens):
        """The step's LensCfg: the caller's, with the step's own Perceiver dropout arguments where they are given."""
        from dataclasses import replace
        pa, pf = self.perceiver_attn_dropout, self.perceiver_ff_dropout
        return replace(lens, attn_dropout=pa or lens.attn_dropout, ff_dropout=pf or lens.ff_dropout)

    def lens_draw(self, offset: int):
        """The Perceiver dropout draw (engine.LensDrop) of the micro-batch that starts at `offset` of the per-GPU batch at the
        current optimizer step count, or None when the Lens drops nothing."""
        return self.lens.perceiver.draw(self.drop_seed, drop_sample0(self.opt.t, self.rank, DROP_TOWER_LENS, offset))

    @property
    def last_grad_norm(self):
        """The unclipped global gradient norm of the last clipped optimizer step (of DDP's mean gradient), a 0-d tensor on the
        device; None before the first one or without `grad_clip_norm`."""
        return self.opt.last_grad_norm

    def _clipped_optimizer_step(self):
        """finish_reduce -> squared norm of the flat gradient buffer (its alignment padding is zero) -> every master in one
        launch with torch.nn.utils.clip_grad_norm_'s coefficient derived on the device: no host read of norm or coefficient."""
        self.finish_reduce()
        if self._sumsq is None:
            self._sumsq = torch.zeros(1, device=self.dev, dtype=torch.float32)
        ops.grad_sumsq(self._clipped_grads(), out=self._sumsq)
        self.opt.step(self.grads, grad_scale=1.0 / self.world, max_norm=self.grad_clip_norm, sumsq=self._sumsq)

    def _clipped_grads(self):
        """The contiguous range of the flat gradient buffer whose norm is clipped: all of it, unless a step class keeps
        tensors out of the clipped set (`_optimizer_groups`) - those lie outside the range it returns here."""
        return self.flat_grad

    def _optimizer_groups(self):
        """Keyword arguments of `AdamW` beyond (lr, betas, eps, weight_decay): per-tensor lr_scale / no_clip / decay of a step
        class whose recipe has parameter groups.  Called after `_build`, when the masters exist."""
        return {}

    def _clamp_logit_scale(self):
        """`logit_scale.clamp_(0, ln 100)` after the optimizer step (tri_train_one_epoch, training/train.py)."""
        ops.clamp_scalar(self.logit_scale, 0.0, math.log(100.0))

    @property
    def dist(self) -> bool:
        """The multi-rank code path is taken: there are peers, or `force_comm` asked for it on one rank."""
        return self.world > 1 or self._force_comm

    @property
    def _overlap_active(self) -> bool:
        return self.overlap_frozen and self.dev.type == "cuda"

    # Whether this step class runs its text tower packed (TextEngine.plan_text).  The plan request makes the host wait for the
    # device once per step, so the host no longer queues the front of a step while the previous one drains; a step class whose
    # front is bound by the host's launch rate turns it off (TriModalPCStep).
    pack_text = True

    def _text_plan(self, texts):
        """The text tower's packing plan (TextEngine.plan_text), or None: a step class with `pack_text` off, an engine without
        plan_text (a stand-in, a CPU device) or a batch that runs dense anyway.  Requested as the FIRST thing of a step, before
        anything of this step is queued: the host then waits for what the previous step left in the queue, and nothing of this
        one sits behind a blocked host."""
        plan_text = getattr(self.text, "plan_text", None)
        if plan_text is None or not self.pack_text:
            return None
        return plan_text(texts)

    def _encode_text(self, texts, plan):
        """The text features with the plan `_text_plan` gave.  No plan - whatever the reason - means dense: `plan=False` is the
        only way a step keeps the engine from making a plan of its own (and waiting for the device in the middle of the step);
        a direct `self.text.encode_text(texts)` packs whatever `pack_text` says."""
        if not hasattr(self.text, "plan_text"):
            return self.text.encode_text(texts)
        return self.text.encode_text(texts, plan=plan if plan is not None else False)      # (False: dense, no plan made there)

    def _side_by_side(self, beside, here):
        """Run two closures of independent work: `beside()` on the step's second HIP stream, `here()` on the launch stream,
        joined by events on both ends (one after the other on a CPU device or with `overlap_frozen` off).  Two callers: the
        forward (`beside` = the locked towers, forward only, results into buffers the caller allocated; `here` = the Lens
        tower with saved activations) and the backward (`_backward_all`: the two halves of the micro-batches, each into its
        own gradient buffer).  One closure's low-power phases (attention, LayerNorm, leftover rows) sit beside the other's
        GEMMs on a board that is power-limited in its GEMM phases (-1.35 % per C3 step for the forward, -3.2 % with the
        backward; bit-equal results: tests/test_hip_train.py)."""
        frozen, trainable = beside, here
        if not self._overlap_active:
            frozen(); trainable()
            return
        if self._side is None:
            self._side = torch.cuda.Stream(device=self.dev)
        main = torch.cuda.current_stream(self.dev)
        ready, done = torch.cuda.Event(), torch.cuda.Event()
        ready.record(main)
        self._side.wait_event(ready)                  # inputs and output buffers exist
        with torch.cuda.stream(self._side):
            frozen()
            done.record(self._side)
        trainable()
        main.wait_event(done)

    def drop_indices(self, tower: int, vit, offset: int, n: int):
        """(keep int32 [n,K], inv int32 [n,T]) of the n samples from `offset` of the per-GPU batch for ViT tower `vit` (tower id
        `tower`) at the current optimizer step count: what a forward of that micro-batch drops (class docstring)."""
        T = vit.T
        return ops.patch_keep(None, ops.patch_keep_count(T, self.patch_dropout), B=n, T=T, seed=self.drop_seed,
                              sample0=drop_sample0(self.opt.t, self.rank, tower, offset), device=self.dev)

    # ------------------------------------------------------------------------------------------- construction, trainers, buffers
    def _construct(self, host, adamw, *build, **build_kw):
        """The tail of every step's `__init__`: the host state, the engines and masters of the trainable set, AdamW on them."""
        self._init_host(*host)
        self._build(*build, **build_kw)
        self.opt = AdamW(self.masters, *adamw, **self._optimizer_groups())

    def _trainer(self, i):
        while len(self.trainers) <= i:
            t = self._mk()
            if self.trainers:                      # share what is derived from the weights across micro-batches
                self._share_operands(t, self.trainers[0])
            self.trainers.append(t)
        return self.trainers[i]

    def _share_operands(self, t, first):
        t.tower.wT, t.tower.proj = first.tower.wT, first.tower.proj

    def _bind_grads(self, t, grads=None):
        """Point every part of trainer `t` at one gradient dictionary (default: `self.grads`)."""
        t.tower.grads = self.grads if grads is None else grads

    def _alloc_flat_grads(self):
        """All gradient buffers are views into ONE flat fp32 tensor -> a single all-reduce per step.  Master order and the
        alignment of the views ARE the layout: the block buckets and the clipped AdamW's slot table rely on it."""
        al = lambda n: (n + 3) // 4 * 4                       # every view starts 16-byte aligned
        self.flat_grad = torch.zeros(sum(al(v.numel()) for v in self.masters.values()), device=self.dev, dtype=torch.float32)
        self.flat_grad_b = torch.zeros_like(self.flat_grad)  # the first half of a step's micro-batches accumulates here (_backward_all)
        self.grads_b, off = {}, 0
        for k, v in self.masters.items():
            self.grads[k] = self.flat_grad[off:off + v.numel()].view(v.shape)
            self.grads_b[k] = self.flat_grad_b[off:off + v.numel()].view(v.shape)
            off += al(v.numel())
        for t in self.trainers:
            self._bind_grads(t)

    # ---- gradient buckets: the masters of one block are contiguous in the flat buffer ----
    def _bucket_blocks(self):
        """The transformer blocks whose gradients are a bucket of their own (merged and all-reduced as soon as the backward
        has passed the block): the unlocked blocks of the depth step, none where every block is locked."""
        return ()

    def _block_range(self, l):
        p = f"visual.transformer.resblocks.{l}."
        names = [k for k in self.masters if k.startswith(p)]
        base = self.flat_grad.data_ptr()
        lo = min((self.grads[k].data_ptr() - base) // 4 for k in names)
        hi = max((self.grads[k].data_ptr() - base) // 4 + self.grads[k].numel() for k in names)
        return lo, min((hi + 3) // 4 * 4, self.flat_grad.numel())          # incl. the 16-byte alignment pad of the last view

    def _rest_ranges(self):
        """(lo, hi) of all buckets together: what lies outside it is merged / reduced at the end.  No buckets: everything."""
        rs = [self._block_range(l) for l in self._bucket_blocks()]
        return (min(r[0] for r in rs), max(r[1] for r in rs)) if rs else (0, 0)

    def _start_block_reduce(self, l):
        if self.dist and hasattr(self.comm, "all_reduce_sum_async"):
            lo, hi = self._block_range(l)
            self._pending.append(self.comm.all_reduce_sum_async(self.flat_grad[lo:hi]))
            self._reduced_upto = l

    # ------------------------------------------------------------------------------------------- the step
    def step(self, *a, **kw) -> torch.Tensor:
        loss = self.forward_backward(*a, **kw)
        self.optimizer_step()
        return loss

    def finish_reduce(self):
        """Bring `flat_grad` / `grads` to ONE state: the sum over ranks of every gradient, all collectives complete.

        Between `forward_backward()` and this call the buffer is MIXED: the unlocked blocks' buckets were all-reduced
        during the last micro-batch's backward (possibly still in flight on the collective's stream) while logit_scale
        and the adapter - produced last - are still rank-local (a step without buckets: all of it is rank-local, and one
        collective here sums it).  Anything that reads or rescales the gradients in between (clipping, norm logging, accumulation over several forward_backward calls) calls this first;
        `optimizer_step()` does.  Idempotent; a no-op on one rank.  The values are SUMS: the 1/world of DDP's mean is
        applied inside the optimizer step (`grad_scale`)."""
        if not self.dist or self._reduce_done:
            return
        for h in self._pending:
            h.wait()
        self._pending = []
        if self._reduced_upto is None:
            self.comm.all_reduce_sum(self.flat_grad)
        else:
            lo, hi = self._rest_ranges()
            for a, b in ((0, lo), (hi, self.flat_grad.numel())):
                if b > a:
                    self.comm.all_reduce_sum(self.flat_grad[a:b])
        self._reduced_upto = None
        self._reduce_done = True

    def reduced_grads(self):
        """The gradients by master name after `finish_reduce()` (sums over ranks)."""
        self.finish_reduce()
        return self.grads

    def optimizer_step(self):
        if self.grad_clip_norm is not None:
            self._clipped_optimizer_step()
        elif self.dist:
            # DDP semantics: mean of per-rank gradients.  Block buckets were started during the last micro-batch's backward
            # (reverse layer order); what is left - logit_scale and the adapter, produced last - goes in one more call.
            self.finish_reduce()
            self.opt.step(self.grads, grad_scale=1.0 / self.world)
        else:
            self.opt.step(self.grads)
        self._refresh_operands()
        self._clamp_logit_scale()

    def _prepare(self, B):
        """-> (micro-batch size, number of micro-batches); trainers and gradient buffers on the first call, `flat_grad` zero."""
        mb = min(self.mb, B)
        assert B % mb == 0, "per-GPU batch must be a multiple of the micro-batch"
        nmb = B // mb
        if self.flat_grad is None:
            for i in range(nmb):
                self._trainer(i)
            self._alloc_flat_grads()
        for h in self._pending:          # (a forward_backward without optimizer_step: finish what was started)
            h.wait()
        self._pending, self._reduced_upto, self._reduce_done = [], None, False
        self.flat_grad.zero_()
        return mb, nmb

    def _forward_backward(self, texts, images, *inputs) -> torch.Tensor:
        """One forward and backward over the per-GPU batch: the loss, and `flat_grad` = this rank's gradients (with the block
        buckets, if any, already summed over ranks or on their way: `finish_reduce`).  `images` None: a step without the image
        tower.  `inputs`: what the trainers' forward takes, each a per-sample tensor or None, cut into micro-batches here."""
        tplan = self._text_plan(texts)
        B = inputs[0].shape[0]
        mb, nmb = self._prepare(B)
        E = self.text.cfg.embed_dim
        fi = None if images is None else torch.empty(B, E, device=self.dev)
        ft = torch.empty(B, E, device=self.dev)
        fv = torch.empty(B, E, device=self.dev); vraw = torch.empty(B, E, device=self.dev)
        vnorm = torch.empty(B, device=self.dev)
        drop = self.patch_dropout > 0.0
        lens_drop = self._lens_drop
        # the frozen text tower sees the whole per-GPU batch in one pass: 77-token sequences give a micro-batch only 77 row
        # tiles (one uneven round of the persistent GEMM, 600-900 TF/s); four times the rows run whole rounds
        def frozen():
            ops.l2_normalize(self._encode_text(texts, tplan), out=ft)
            if images is None:
                return
            for i in range(nmb):
                s = slice(i * mb, (i + 1) * mb)
                kw = dict(keep=self.drop_indices(DROP_TOWER_IMAGE, self.image, i * mb, mb)[0]) if drop else {}
                ops.l2_normalize(self.image.encode_image(images[s], **kw), out=fi[s])

        def trainable():
            for i in range(nmb):
                s = slice(i * mb, (i + 1) * mb)
                kw = dict(zip(("keep", "inv"), self.drop_indices(DROP_TOWER_VISUAL, self.lens.vit, i * mb, mb))) if drop else {}
                if lens_drop:
                    kw["drop"] = self.lens_draw(i * mb)
                vraw[s] = self._trainer(i).forward(*(None if x is None else x[s] for x in inputs), **kw)
        self._side_by_side(frozen, trainable)
        ops.l2_normalize(vraw, out=fv, norms=vnorm)
        loss, dv, ds = self._loss(fi, ft, fv)
        dvraw = ops.l2_normalize_bwd(fv, dv, vnorm)
        self._backward_all(dvraw, nmb, mb)
        # logit_scale is exp()'d in forward (model.py:619); with the device-side scale pair_backward returns d/d(log-scale).
        # The pairs' parts are added here, after the backward has been enqueued
        self.grads["logit_scale"] += sum(ds[1:], ds[0])
        return loss

    def _gather(self, *feats):
        """The rank-major gathers [W*b, E] of the local features in ONE exchange: [b, k*E] per rank over xGMI (k*768 floats
        a row).  The features themselves on one rank."""
        if not self.dist:
            return feats
        E = feats[0].shape[1]
        packed = torch.cat(feats, dim=1)
        allp = torch.empty(self.world * packed.shape[0], len(feats) * E, device=self.dev)
        self.comm.all_gather(allp, packed)
        return [t.contiguous() for t in allp.split(E, dim=1)]

    def _loss(self, fi, ft, fv):
        """TriClipLoss, image and text towers frozen: (loss, d loss / d fv, the parts of d loss / d logit_scale).  The scale is
        the log-temperature, on the device: exp() is applied inside the loss section."""
        ai, at, av = self._gather(fi, ft, fv)
        kw = dict(local_loss=self.local_loss, gather_with_grad=self.gather_with_grad, need_x=False, dist=self.dist)
        l1, _, dv1, ds1 = pair_loss_and_grads(self.comm, self.rank, self.world, fi, fv, ai, av, self.logit_scale, **kw)
        l2, _, dv2, ds2 = pair_loss_and_grads(self.comm, self.rank, self.world, ft, fv, at, av, self.logit_scale, **kw)
        return l1 + l2, dv1 + dv2, (ds1, ds2)

    def _backward_all(self, dvraw, nmb, mb):
        """Backward of every micro-batch; parameter gradients accumulate over them.

        With two or more micro-batches the FIRST half accumulates into a second gradient buffer (`flat_grad_b`) and the second
        half into `flat_grad`; a block's bucket is merged (and, across ranks, its all-reduce started) when the LAST micro-batch
        of the second half has passed the block, the rest (adapter, position table; in a step without buckets: everything) at
        the end.  That makes the two halves independent streams of work: with `overlap_frozen` on a GPU the first half runs on the second HIP stream beside the
        second half - the backward is a chain of chip-filling GEMMs with latency-bound kernels between them (fused attention
        backward, LayerNorm backward, leftover rows, the drain of every persistent launch), exactly what the forward's two
        towers fill for each other.  The arithmetic - which products are added in which order - is the same on one stream
        and on two: results are bit-identical (tests/test_hip_train.py).  Not on two streams with SyncBatchNorm (its backward
        exchanges data on the communicator from inside the micro-batch: `_one_stream_backward`).  Reference: loss.backward()
        over the micro-batches of the accumulation loop, training/train.py:154-210 (gradients of all summed into .grad)."""
        blocks = self._bucket_blocks()
        dist_cb = self.dist and len(blocks) > 0
        dv = lambda i: dvraw[i * mb:(i + 1) * mb].contiguous()

        def backward(i, on_block_done=None):
            # (the trainers of a step without buckets take no callback, and none is passed to them)
            self._trainer(i).backward(dv(i), *((on_block_done,) if blocks else ()))
        half = nmb // 2
        for i in range(nmb):
            self._bind_grads(self._trainer(i), self.grads_b if i < half else self.grads)
        if half == 0:
            backward(0, self._start_block_reduce if dist_cb else None)
            return
        self.flat_grad_b.zero_()
        two_streams = self._overlap_active and self.overlap_backward and not self._one_stream_backward
        passed = {}          # block -> event on the first half's stream: its last micro-batch has passed the block

        def first_done(l):
            if two_streams:
                passed[l] = torch.cuda.Event()
                passed[l].record()

        def second_done(l):
            if two_streams:
                torch.cuda.current_stream(self.dev).wait_event(passed[l])
            lo, hi = self._block_range(l)
            ops.axpy(self.flat_grad[lo:hi], self.flat_grad_b[lo:hi])
            if dist_cb:
                self._start_block_reduce(l)

        def first_half():
            for i in range(half):
                backward(i, first_done if i == half - 1 else None)

        def second_half():
            for i in range(half, nmb):
                backward(i, second_done if i == nmb - 1 else None)
        if two_streams:
            self._side_by_side(first_half, second_half)      # (first closure on the second stream, joined at the end)
        else:
            first_half(); second_half()
        lo, hi = self._rest_ranges()
        for a, b in ((0, lo), (hi, self.flat_grad.numel())):
            if b > a:
                ops.axpy(self.flat_grad[a:b], self.flat_grad_b[a:b])

    # ------------------------------------------------------------------------------------------- checkpointing
    def state_dict(self) -> Dict[str, torch.Tensor]:
        out = {k: v.detach().clone() for k, v in self._base_sd.items()}
        cfg = getattr(self.lens, "lens", None)
        for name, m in self.masters.items():
            for k, v in _master_to_sd(name, m.detach(), self._base_sd, cfg).items():
                out[k] = v.to(device=self._base_sd[k].device, dtype=self._base_sd[k].dtype).clone()
        if cfg is not None and getattr(cfg, "weight_tie_layers", False):
            # the reference's state_dict repeats the shared modules under every tied layer index (perceiver.py:249-254)
            P1 = "visual.perceiver.layers.1."
            for k in [k for k in out if k.startswith(P1)]:
                for li in range(2, cfg.depth):
                    out[f"visual.perceiver.layers.{li}." + k[len(P1):]] = out[k].clone()
        tok = getattr(self, "tok", None)
        if tok is not None:                                      # BatchNorm running statistics of the PointTokenizer
            for k, (rm, rv) in tok.running.items():
                out["visual.visual_adapter." + k + ".running_mean"] = rm.detach().cpu().clone()
                out["visual.visual_adapter." + k + ".running_var"] = rv.detach().cpu().clone()
        return out

    def optimizer_state_dict(self):
        return {"step": self.opt.t, "exp_avg": {k: v.detach().clone() for k, v in self.opt.m.items()},
                "exp_avg_sq": {k: v.detach().clone() for k, v in self.opt.v.items()}}

    def load_state_dict(self, sd):
        """Re-read every TRAINABLE tensor from a reference-layout state_dict into the masters (in place: the kernels keep
        reading the same buffers) and refresh the bf16 operands.  Frozen towers are fixed at construction."""
        for name, m in self.masters.items():
            m.copy_(_master_from_sd(name, sd, m))
        tok = getattr(self, "tok", None)
        if tok is not None:
            for k, (rm, rv) in tok.running.items():
                rm.copy_(sd["visual.visual_adapter." + k + ".running_mean"].float()); rv.copy_(sd["visual.visual_adapter." + k + ".running_var"].float())
        if not self.trainers:
            self._trainer(0)
        self._refresh_operands()
        self._base_sd = {k: v.detach() for k, v in sd.items()}

    def load_optimizer_state_dict(self, st):
        self.opt.t = int(st["step"])
        for k in self.opt.m:
            self.opt.m[k].copy_(st["exp_avg"][k]); self.opt.v[k].copy_(st["exp_avg_sq"][k])


# ------------------------------------------------------------------------------------------------ loss core
# logits of this many elements or more are never materialised whole: the pair loss runs in row blocks (268 MB of f32)
LOGITS_CHUNK_ELEMS = 1 << 26
LOGITS_CHUNK_ROWS = 2048


def _chunk_rows(R: int, Cn: int, chunk_rows: Optional[int]) -> int:
    """Rows per block of the pair loss: 0 = whole matrix at once."""
    if chunk_rows is None:
        chunk_rows = LOGITS_CHUNK_ROWS if R * Cn >= LOGITS_CHUNK_ELEMS else 0
    return 0 if chunk_rows <= 0 or chunk_rows >= R else int(chunk_rows)


def _is_dev_scale(scale) -> bool:
    return torch.is_tensor(scale)


def _mask_operands(mask, R: int, Cn: int):
    """mask = (teacher features of the rows [R, D], teacher features of the columns [C, D], thres) -> the two bf16x3
    operands of the similarity GEMM and the threshold.  Always the UN-SCALED features: the similarity that is compared with
    `thres` is a cosine, whatever the temperature does to the logits' row operand."""
    trow, tcol, thres = mask
    if trow.shape[0] != R or tcol.shape[0] != Cn or trow.shape[1] != tcol.shape[1]:
        raise ValueError(f"pair loss mask: teacher features {tuple(trow.shape)} x {tuple(tcol.shape)} do not describe the "
                         f"{R} x {Cn} logits")
    return (ops.split_bf16x3(trow.detach().float().contiguous(), 0), ops.split_bf16x3(tcol.detach().float().contiguous(), 1),
            float(thres))


def _label_columns_only(col_lse, label_off: int, R: int):
    """The column loss is a mean over the R label columns [label_off, label_off + R).  A column outside them (R x C logits
    with C > R and w_col != 0) is in no term of it: its log-sum-exp becomes +inf, so that vl_ce_grad's column term
    exp(l - lse) - 0 is exactly 0 there (vl_ce_loss_accum reads label columns only).  Square logits: nothing to do."""
    if col_lse is not None and (label_off > 0 or label_off + R < col_lse.shape[0]):
        col_lse[:max(label_off, 0)] = float("inf")
        col_lse[label_off + R:] = float("inf")
    return col_lse


def pair_forward(x, y, scale, label_off: int = 0, w_row: float = 0.5, w_col: float = 0.5,
                 chunk_rows: Optional[int] = None, mask=None, loss_acc=None):
    """loss contribution w_row*CE(scale*x y^T) + w_col*CE(columns); returns (loss[1] tensor, ctx).

    scale: a Python float (the temperature itself), or - round 4 - the LEARNABLE LOG-temperature as a 1-element f32 tensor
    on the device (`logit_scale` as the model holds it, model.py:619): x is multiplied by exp(logit_scale) on the device
    (vl_scale_exp_f32) and the logits GEMM runs with alpha = 1, so the step never reads the scalar on the host and the loss
    section is capturable in a hipGraph.  In that mode pair_backward's third result is d/d(logit_scale) (the log-domain
    parameter) directly: sum(G * logits) - no division by the scale and re-multiplication.

    Row-blocked mode (chunk_rows, or automatically for B_glob^2 above LOGITS_CHUNK_ELEMS): the B_glob x B_glob logits
    are never held whole.  Forward = per block of rows: logits GEMM, exact row log-sum-exp, the block's column
    log-sum-exp; the column statistics of the blocks are merged by one logsumexp over [blocks, C].  Backward
    recomputes each block's logits (training/train.py:154-210 reaches batch 2048 by re-running the towers per
    accumulation step; here only one thin GEMM is re-run).

    mask (ClipLossSimMask, loss.py:522-598; None = the plain loss, untouched): (teacher features of the rows, teacher
    features of the columns, thres).  sim = rows @ columns^T comes from the same bf16x3 GEMM as the logits (alpha = 1, on
    the un-scaled teacher features, ~2^-17 relative), and an element off the label diagonal with sim >= thres enters both
    softmaxes as logit 0.0 - the reference multiplies the logits by the mask - and carries no gradient.  Row-blocked mode
    never holds sim whole either: each row block's sim block is computed next to its logits block, and recomputed next to
    the recomputed logits in the backward.

    loss_acc: a 1-element f32 device tensor the loss is ADDED to and that is returned (the caller zeroed it, `ops.fill`), instead
    of a new zeroed tensor - a step that keeps its accumulators runs the loss section without a framework fill."""
    R, Cn = x.shape[0], y.shape[0]
    rb = _chunk_rows(R, Cn, chunk_rows)
    dev_scale = _is_dev_scale(scale)
    alpha = 1.0 if dev_scale else scale
    xb = ops.split_bf16x3(ops.scale_exp(x.contiguous(), scale) if dev_scale else x, 0)
    yb = ops.split_bf16x3(y, 1)
    tr = tc = thres = None
    if mask is not None:
        tr, tc, thres = _mask_operands(mask, R, Cn)
    if rb == 0:
        logits = ops.logits_gemm(xb, yb, alpha)
        if mask is None:
            sim = None
            row_lse, col_lse, diag = ops.ce_stats(logits, label_off, want_cols=(w_col != 0.0))
        else:
            sim = ops.logits_gemm(tr, tc, 1.0)
            row_lse, col_lse, diag = ops.ce_stats(logits, label_off, want_cols=(w_col != 0.0), sim=sim, thres=thres)
        col_lse = _label_columns_only(col_lse, label_off, R)
        loss = torch.zeros(1, device=x.device, dtype=torch.float32) if loss_acc is None else loss_acc
        ops.ce_loss_accum(loss, row_lse if w_row != 0.0 else None, col_lse, diag, R, Cn, label_off, w_row, w_col)
        return loss, (x, y, logits, row_lse, col_lse, label_off, w_row, w_col, scale, 0, None, None, sim, None, thres)
    row_lse = torch.empty(R, device=x.device); diag = torch.empty(R, device=x.device)
    col_parts = []
    for r0 in range(0, R, rb):
        r1 = min(R, r0 + rb)
        lg = ops.logits_gemm(xb[r0:r1], yb, alpha)
        if mask is None:
            rl, cl, dg = ops.ce_stats(lg, label_off + r0, want_cols=(w_col != 0.0))
        else:
            sm = ops.logits_gemm(tr[r0:r1], tc, 1.0)
            rl, cl, dg = ops.ce_stats(lg, label_off + r0, want_cols=(w_col != 0.0), sim=sm, thres=thres)
            del sm
        row_lse[r0:r1] = rl; diag[r0:r1] = dg
        if cl is not None:
            col_parts.append(cl)
        del lg
    col_lse = _label_columns_only(torch.logsumexp(torch.stack(col_parts), dim=0), label_off, R) if col_parts else None
    loss = torch.zeros(1, device=x.device, dtype=torch.float32) if loss_acc is None else loss_acc
    ops.ce_loss_accum(loss, row_lse if w_row != 0.0 else None, col_lse, diag, R, Cn, label_off, w_row, w_col)
    return loss, (x, y, None, row_lse, col_lse, label_off, w_row, w_col, scale, rb, xb, yb, tr, tc, thres)


def pair_backward(ctx, g: float = 1.0, need_dx=True, need_dy=True, dscale_acc=None):
    """-> (dx, dy, dscale).  dscale = dL/d(scale) for a float scale, dL/d(logit_scale) (log domain) for a device scale.
    With a mask (pair_forward) the masked elements of dL/dlogits are zero, so they reach neither dx, dy nor dscale; the
    teacher features inside the mask receive nothing (the reference's mask is a comparison: no gradient).
    dscale_acc: as `pair_forward`'s loss_acc, for dscale."""
    x, y, logits, row_lse, col_lse, label_off, w_row, w_col, scale, rb, xb, yb, sim, tc, thres = ctx
    mk = (lambda sm: {}) if thres is None else (lambda sm: dict(sim=sm, thres=thres))
    dscale = torch.zeros(1, device=x.device, dtype=torch.float32) if dscale_acc is None else dscale_acc
    dev_scale = _is_dev_scale(scale)
    # vl_ce_grad accumulates sum(G * logits) / logit_scale: with 1.0 that IS d/d(log-scale)
    alpha, cscale = (1.0, 1.0) if dev_scale else (scale, scale)
    fin = (lambda t: ops.scale_exp(t, scale, out=t)) if dev_scale else (lambda t: t)
    if rb == 0:
        G, GT = ops.ce_grad(logits, row_lse if w_row != 0.0 else None, col_lse, label_off, w_row * g, w_col * g, cscale,
                            dscale, need_g=need_dx, need_gt=need_dy, **mk(sim))
        dx = dy = None
        if need_dx:
            dx = fin(ops.gemm(G, ops.transpose_to_bf16(y, ldo=G.shape[1]), None, epi=ops.EPI_F32, alpha=alpha))
        if need_dy:
            dy = fin(ops.gemm(GT, ops.transpose_to_bf16(x, ldo=GT.shape[1]), None, epi=ops.EPI_F32, alpha=alpha))
        return dx, dy, dscale
    R, Cn = x.shape[0], y.shape[0]
    dx = torch.empty(R, x.shape[1], device=x.device) if need_dx else None
    dy = torch.zeros(Cn, y.shape[1], device=x.device) if need_dy else None
    yt = None
    tr = sim                                   # row-blocked: the slot holds the teacher ROW operand, not a sim matrix
    for r0 in range(0, R, rb):
        r1 = min(R, r0 + rb)
        f = (r1 - r0) / R                      # the kernels average over the rows they are given: re-weight to the global mean
        lg = ops.logits_gemm(xb[r0:r1], yb, alpha)
        sm = None if thres is None else ops.logits_gemm(tr[r0:r1], tc, 1.0)
        G, GT = ops.ce_grad(lg, row_lse[r0:r1] if w_row != 0.0 else None, col_lse, label_off + r0, w_row * g * f, w_col * g * f,
                            cscale, dscale, need_g=need_dx, need_gt=need_dy, **mk(sm))
        if need_dx:
            if yt is None:
                yt = ops.transpose_to_bf16(y, ldo=G.shape[1])
            ops.gemm(G, yt, None, out=dx[r0:r1], epi=ops.EPI_F32, alpha=alpha)
        if need_dy:
            xt = ops.transpose_to_bf16(x[r0:r1].contiguous(), ldo=GT.shape[1])
            ops.gemm(GT, xt, None, out=dy, res=dy, epi=ops.EPI_RES_F32, alpha=alpha)       # dy += scale * G_b^T x_b
        del lg, G, GT, sm
    return (fin(dx) if need_dx else None), (fin(dy) if need_dy else None), dscale


def pair_loss_and_grads(comm, rank: int, world: int, xl, yl, ax, ay, scale, local_loss: bool = False,
                        gather_with_grad: bool = False, need_x: bool = True, need_y: bool = True, dist: Optional[bool] = None,
                        sim_teacher: Optional[str] = None, sim_thres: Optional[float] = None):
    """One (x, y) pair of ClipLossGeneral / TriClipLoss over the global batch (loss.py:116-138, 293-308) as rank `rank`
    computes it, and the gradients that arrive at THIS rank's features.

    xl, yl: local unit features [b, E]; ax, ay: their rank-major gathers [W*b, E] (= xl, yl at world 1).
      local_loss=False: full B_glob x B_glob logits on every rank (rows and columns CE).
      local_loss=True : b x B_glob logits for the rank's own rows of both directions, labels offset by rank*b.
      gather_with_grad=False: peers are constants; the own slot of the gather is differentiable unless local_loss
                              (gather_features re-inserts the local tensor only then, loss.py:71-74).
      gather_with_grad=True : the gather is differentiable everywhere -> backward = reduce-scatter (sum over ranks).
    dist: run the multi-rank code path (default: world > 1).  True at world 1 = every collective of the path executes on a
    one-rank communicator (`force_comm` of the steps: the RCCL calls, their streams and their buffer contracts are exercised
    on one GPU; the values are those of the single-rank path).
    sim_teacher ("x" | "y" | None) with sim_thres: ClipLossSimMask (loss.py:522-598) with the named side as the TEACHER, whose
      similarities teacher @ teacher^T >= sim_thres mask the off-diagonal logits (to logit 0.0, `pair_forward`).  The caller
      names the side because the argument order here is the caller's: the reference module has x = teacher, `DualAudioStep`
      calls with x = visual (student), y = text (teacher).  The full matrix is masked by the symmetric all_t @ all_t^T in
      either orientation; under local_loss BOTH directions use the one block sim[rank*b + i, j] = t_local @ all_t^T (the
      reference slices mask and mask^T, which are the same predicate because sim is symmetric): one sim block per rank.
    Returns (loss[1], dxl | None, dyl | None, dscale[1])."""
    b = xl.shape[0]
    dist = world > 1 if dist is None else dist
    if sim_teacher not in (None, "x", "y"):
        raise ValueError(f"pair_loss_and_grads: sim_teacher is 'x', 'y' or None, got {sim_teacher!r}")
    if sim_teacher is not None and sim_thres is None:
        raise ValueError("pair_loss_and_grads: sim_teacher needs sim_thres")
    tl, ta = (None, None) if sim_teacher is None else ((xl, ax) if sim_teacher == "x" else (yl, ay))
    if dist and local_loss:
        mk = {} if tl is None else dict(mask=(tl, ta, sim_thres))
        l1, c1 = pair_forward(xl, ay, scale, label_off=rank * b, w_row=0.5, w_col=0.0, **mk)
        l2, c2 = pair_forward(yl, ax, scale, label_off=rank * b, w_row=0.5, w_col=0.0, **mk)
        dxl, d_ay, ds1 = pair_backward(c1, need_dx=need_x, need_dy=need_y and gather_with_grad)
        dyl, d_ax, ds2 = pair_backward(c2, need_dx=need_y, need_dy=need_x and gather_with_grad)
        loss, ds = l1 + l2, ds1 + ds2
    else:
        loss, c = pair_forward(ax, ay, scale, **({} if ta is None else dict(mask=(ta, ta, sim_thres))))
        d_ax, d_ay, ds = pair_backward(c, need_dx=need_x, need_dy=need_y)
        dxl = dyl = None

    def fold(dl, d_all):
        if d_all is None:
            return dl
        if not dist:
            g = d_all
        elif gather_with_grad:
            g = torch.empty(b, d_all.shape[1], device=d_all.device, dtype=d_all.dtype)
            comm.reduce_scatter_sum(g, d_all.contiguous())
        else:
            g = d_all[rank * b:(rank + 1) * b].contiguous()
        return g if dl is None else dl + g
    return loss, (fold(dxl, d_ax) if need_x else None), (fold(dyl, d_ay) if need_y else None), ds


class TriModalDepthStep(_StepState):
    def __init__(self, sd: Dict[str, torch.Tensor], tower: TowerCfg, text: TextCfg, device, micro_batch: int = 256,
                 unlock_first_n: int = 4, lr: float = 5e-4, betas=(0.9, 0.98), eps: float = 1e-6, weight_decay: float = 0.2,
                 rank: int = 0, world_size: int = 1, gemm_cfg: int = -1, comm=None, frozen_res_dtype=torch.float32,
                 local_loss: bool = False, gather_with_grad: bool = False, train_res_dtype=torch.float32,
                 grad_checkpointing: bool = False, force_comm: bool = False, text_wsplit: Optional[bool] = None, text_arith: str = "f16",
                 overlap_frozen: bool = True, overlap_backward: bool = True,
                 grad_clip_norm: Optional[float] = None, patch_dropout: float = 0.0, drop_seed: int = 0):
        """overlap_frozen (default ON since round 6): the image / text towers' forwards run on a second HIP stream beside
        the trainable tower's forward (`_side_by_side`); results are bit-identical to the serial order."""
        self.grad_checkpointing = bool(grad_checkpointing)      # block recompute in the trainable tower (transformer.py:366-368)
        self.unlock_first_n = unlock_first_n
        self._construct((sd, device, micro_batch, rank, world_size, comm, local_loss, gather_with_grad, force_comm, overlap_frozen,
                         overlap_backward, grad_clip_norm, patch_dropout, drop_seed), (lr, betas, eps, weight_decay),
                        sd, tower, text, gemm_cfg=gemm_cfg, frozen_res_dtype=frozen_res_dtype, train_res_dtype=train_res_dtype,
                        text_wsplit=text_wsplit, text_arith=text_arith)

    def _build(self, sd, tower, text, gemm_cfg=-1, frozen_res_dtype=torch.float32, train_res_dtype=torch.float32,
               text_wsplit=None, text_arith="f16"):
        """Engines and the fp32 masters of the trainable set (reference lock recipe: adapter + first n blocks + logit_scale)."""
        device, unlock_first_n = self.dev, self.unlock_first_n
        # frozen towers: forward only; their residual stream may be kept in bf16 (= the reference's autocast)
        self.image = VitEngine(sd, "image.", tower, device, gemm_cfg=gemm_cfg, res_dtype=frozen_res_dtype)
        self.text = TextEngine(sd, text, device, gemm_cfg=gemm_cfg, res_dtype=frozen_res_dtype, wsplit=text_wsplit, arith=text_arith)
        # trainable tower: residual stream AND residual-gradient stream in `train_res_dtype` (bf16 = the reference's amp_bf16)
        self.lens = LensEngine(sd, "visual.", tower, LensCfg(modality="depth", perceiver_identity=True), device, gemm_cfg=gemm_cfg,
                               res_dtype=train_res_dtype)
        eng = self.lens.vit
        for l in range(unlock_first_n):
            p = f"visual.transformer.resblocks.{l}."
            w = eng.blocks[l]
            # a block whose LayerNorm parameters and weights move every step carries no LayerNorm-folded operands: they would
            # go stale at the first AdamW step, and `run_blocks` / the trainers decide the folding per block by their presence
            w.pop("in_f", None); w.pop("fc_f", None)
            for nm, key in (("attn.in_proj_weight", "in_w"), ("attn.out_proj.weight", "out_w"), ("mlp.c_fc.weight", "fc_w"),
                            ("mlp.c_proj.weight", "proj_w")):
                self.masters[p + nm] = sd[p + nm].detach().float().to(device).contiguous().clone()      # never an alias of the caller's tensor
                self.bf16_targets[p + nm] = (l, key)
            for nm, key in (("ln_1.weight", "ln1_w"), ("ln_1.bias", "ln1_b"), ("ln_2.weight", "ln2_w"), ("ln_2.bias", "ln2_b"),
                            ("attn.in_proj_bias", "in_b"), ("attn.out_proj.bias", "out_b"), ("mlp.c_fc.bias", "fc_b"),
                            ("mlp.c_proj.bias", "proj_b")):
                self.masters[p + nm] = w[key]                   # f32 tensors the kernels read directly
        self.masters["visual.visual_adapter.pos_emb"] = self.lens.adapter_pos
        from .engine import conv_weight_as_gemm
        self.masters["visual.visual_adapter.conv1.weight_gemm"] = conv_weight_as_gemm(       # from the fp32 weight, not the bf16 operand
            sd["visual.visual_adapter.conv1.weight"], device, torch.float32)

    def _mk(self):
        # (a method, not a closure kept on the instance: a step that holds itself in a reference cycle keeps its activations -
        # 142 GB at the C3 shape - until the cycle collector runs, not until the last reference goes)
        return DepthLensTrainer(self.lens, tower_kw=dict(train_blocks=range(self.unlock_first_n), checkpoint=self.grad_checkpointing))

    def _share_operands(self, t, first):      # weight transposes + gradient buffers
        t.tower.wT, t.tower.proj, t.tower.grads = first.tower.wT, first.tower.proj, first.tower.grads

    def _bucket_blocks(self):
        return range(self.unlock_first_n)

    def _refresh_operands(self):
        eng = self.lens.vit
        if not self.trainers:
            self._trainer(0)
        for name, (l, key) in self.bf16_targets.items():
            m = self.masters[name]
            ops.cast_bf16(m, out=eng.blocks[l][key])
            ops.transpose_to_bf16(m, ldo=m.shape[0], out=self.trainers[0].tower.wT[l][key])
        ops.cast_bf16(self.masters["visual.visual_adapter.conv1.weight_gemm"], out=self.lens.conv_w)

    def forward_backward(self, images: torch.Tensor, texts: torch.Tensor, depths: torch.Tensor) -> torch.Tensor:
        return self._forward_backward(texts, images, depths)


class _PerceiverLensStep(_StepState):
    """What the steps whose trainable part is a Lens (tokenizer + Perceiver) in front of a locked ViT add to the step:
    fp32 masters of the Perceiver under the reference's parameter names and their bf16 operand refresh.  No block is
    unlocked, so the flat gradient buffer has no buckets: a single all-reduce per step = DDP's mean of per-rank gradients."""

    def _collect_perceiver(self, sd):
        pe, P = self.lens.perceiver, "visual.perceiver."
        self._lens_drop = pe.draw(0, 0) is not None
        f32 = lambda k: sd[k].detach().float().to(self.dev).contiguous().clone()
        self.masters[P + "latents"] = pe.latents
        for li, lay in enumerate(pe.layers):
            if li >= 2 and lay is pe.layers[1]:
                continue      # tied to layer 1 (perceiver_weight_tie_layers): same tensors, same masters, summed gradients
            q = f"{P}layers.{li}."
            self._attn(q + "0.", lay["x_attn"], lay["x_norm"], (li, "x"), sd, f32, ctx_norm=lay["x_norm_ctx"])
            self._ff(q + "1.", lay["x_ff"], lay["x_ff_norm"], (li, "xff"), sd, f32)
            for sj, sl in enumerate(lay["selfs"]):
                r = f"{q}2.{sj}."
                self._attn(r + "0.", sl["attn"], sl["norm"], (li, "selfs", sj), sd, f32)
                self._ff(r + "1.", sl["ff"], sl["ff_norm"], (li, "selfs", sj), sd, f32)

    def _attn(self, p, a, norm, path, sd, f32, ctx_norm=None):
        self.masters[p + "norm.weight"], self.masters[p + "norm.bias"] = norm
        if ctx_norm is not None:
            self.masters[p + "norm_context.weight"], self.masters[p + "norm_context.bias"] = ctx_norm
            self.masters[p + "fn.to_q.weight"] = f32(p + "fn.to_q.weight"); self.refresh.append((p + "fn.to_q.weight", a["q_w"], path + ("q",)))
            self.masters[p + "fn.to_kv.weight"] = f32(p + "fn.to_kv.weight"); self.refresh.append((p + "fn.to_kv.weight", a["kv_w"], path + ("kv",)))
        else:
            self.masters[p + "fn.to_qkv.weight"] = torch.cat([f32(p + "fn.to_q.weight"), f32(p + "fn.to_kv.weight")], 0)
            self.refresh.append((p + "fn.to_qkv.weight", a["qkv_w"], path + ("qkv",)))
        self.masters[p + "fn.to_out.weight"] = f32(p + "fn.to_out.weight"); self.refresh.append((p + "fn.to_out.weight", a["to_out_w"], path + ("out",)))
        self.masters[p + "fn.to_out.bias"] = a["to_out_b"]

    def _ff(self, p, ff, norm, path, sd, f32):
        from .engine import interleave_geglu
        self.masters[p + "norm.weight"], self.masters[p + "norm.bias"] = norm
        w0, _ = interleave_geglu(f32(p + "fn.net.0.weight"), f32(p + "fn.net.0.bias"))
        self.masters[p + "fn.net.0.weight_il"] = w0.contiguous(); self.refresh.append((p + "fn.net.0.weight_il", ff["w0"], path + ("w0",)))
        self.masters[p + "fn.net.0.bias_il"] = ff["b0"]
        self.masters[p + "fn.net.2.weight"] = f32(p + "fn.net.2.weight"); self.refresh.append((p + "fn.net.2.weight", ff["w2"], path + ("w2",)))
        self.masters[p + "fn.net.2.bias"] = ff["b2"]

    def _share_operands(self, t, first):
        super()._share_operands(t, first)
        t.perc.wT = first.perc.wT

    def _bind_grads(self, t, grads=None):
        super()._bind_grads(t, grads)
        t.perc.grads = t.tower.grads

    def reference_named_grads(self):
        """The step's gradients (all micro-batches, after `forward_backward`) under the reference's parameter names / layouts."""
        return self.trainers[0].perc.reference_named_grads(self.grads)

    def _refresh_perceiver(self):
        wT = self.trainers[0].perc.wT
        for name, fwd, path in self.refresh:
            m = self.masters[name]
            ops.cast_bf16(m, out=fwd)
            ops.transpose_to_bf16(m, ldo=m.shape[0], out=at_path(wT, path))

    def _refresh_operands(self):
        self._refresh_perceiver()


class DualAudioStep(_PerceiverLensStep):
    """Audio <-> text dual-tower step (reference `train_dual_one_epoch` + ClipLossGeneral, training/train.py:315-470,
    recipe TRAIN_INFERENCE.md:283-299 with --use_dual_loss --align_to text): text tower frozen, visual tower =
    AST tokenizer + Perceiver (trainable) -> locked ViT with unlocked class_embedding.  Multi-GPU semantics are the
    tri-modal step's (packed all-gather, flat gradient all-reduce = mean of per-rank gradients of the global loss).

    contra_loss_type "general" (default) | "sim_mask" with sim_thres (--contra_loss_type / --sim_thres, params.py:43-54):
    "sim_mask" is ClipLossSimMask (loss.py:485-598) with the frozen TEXT tower as the teacher - audio clips whose captions
    are (nearly) the same text, text similarity >= sim_thres, are not each other's negatives; they enter the softmax as
    logit 0.0, as in the reference (`pair_forward`)."""

    def __init__(self, sd, tower: TowerCfg, text: TextCfg, lens: LensCfg, device, micro_batch: int = 256, lr: float = 2e-4,
                 betas=(0.9, 0.98), eps: float = 1e-6, weight_decay: float = 0.2, rank: int = 0, world_size: int = 1,
                 gemm_cfg: int = -1, comm=None, frozen_res_dtype=torch.float32, local_loss: bool = False,
                 gather_with_grad: bool = False, train_res_dtype=torch.float32, force_comm: bool = False, text_wsplit: Optional[bool] = None, text_arith: str = "f16",
                 overlap_frozen: bool = True, overlap_backward: bool = True,
                 grad_clip_norm: Optional[float] = None, contra_loss_type: str = "general", sim_thres: float = 0.8,
                 patch_dropout: float = 0.0, drop_seed: int = 0, perceiver_attn_dropout: float = 0.0,
                 perceiver_ff_dropout: float = 0.0):
        if contra_loss_type not in ("general", "sim_mask"):
            raise NotImplementedError(f"DualAudioStep: contra_loss_type is 'general' or 'sim_mask', got {contra_loss_type!r} "
                                      "(label_mask cannot run in the reference's drivers either)")
        self.contra_loss_type, self.sim_thres = contra_loss_type, float(sim_thres)
        self._construct((sd, device, micro_batch, rank, world_size, comm, local_loss, gather_with_grad, force_comm, overlap_frozen,
                         overlap_backward, grad_clip_norm, patch_dropout, drop_seed, perceiver_attn_dropout, perceiver_ff_dropout),
                        (lr, betas, eps, weight_decay),
                        sd, tower, text, lens, gemm_cfg=gemm_cfg, frozen_res_dtype=frozen_res_dtype, train_res_dtype=train_res_dtype,
                        text_wsplit=text_wsplit, text_arith=text_arith)

    def _build(self, sd, tower, text, lens, gemm_cfg=-1, frozen_res_dtype=torch.float32, train_res_dtype=torch.float32,
               text_wsplit=None, text_arith="f16"):
        from .train import AudioLensTrainer
        device = self.dev
        self.text = TextEngine(sd, text, device, gemm_cfg=gemm_cfg, res_dtype=frozen_res_dtype, wsplit=text_wsplit, arith=text_arith)
        self.lens = LensEngine(sd, "visual.", tower, self._lens_cfg(lens), device, gemm_cfg=gemm_cfg, res_dtype=train_res_dtype)
        self._mk = lambda: AudioLensTrainer(self.lens)
        self.masters["visual.class_embedding"] = self.lens.vit.cls
        self.masters["visual.visual_adapter.pos_emb"] = self.lens.adapter_pos
        from .engine import conv_weight_as_gemm
        self.masters["visual.visual_adapter.conv1.weight_gemm"] = conv_weight_as_gemm(
            sd["visual.visual_adapter.conv1.weight"], device, torch.float32)
        self._collect_perceiver(sd)

    def _refresh_operands(self):
        self._refresh_perceiver()
        ops.cast_bf16(self.masters["visual.visual_adapter.conv1.weight_gemm"], out=self.lens.conv_w)

    def forward_backward(self, audio: torch.Tensor, texts: torch.Tensor) -> torch.Tensor:
        return self._forward_backward(texts, None, audio)

    def _loss(self, fi, ft, fv):
        """ClipLossGeneral(x=visual, y=text), text tower frozen (the base's `_loss` with one pair and no image side)."""
        av, at = self._gather(fv, ft)
        # sim_mask: the TEACHER is the text side, which sits in the y position of this call
        mk = dict(sim_teacher="y", sim_thres=self.sim_thres) if self.contra_loss_type == "sim_mask" else {}
        loss, dv, _, ds = pair_loss_and_grads(self.comm, self.rank, self.world, fv, ft, av, at, self.logit_scale,
                                              local_loss=self.local_loss, gather_with_grad=self.gather_with_grad, need_y=False,
                                              dist=self.dist, **mk)
        return loss, dv, (ds,)


class TriModalAudioStep(DualAudioStep):
    """Audio tri-modal step (reference `tri_train_one_epoch` + TriClipLoss; the published AudioSet recipe,
    TRAIN_INFERENCE.md:283-299: --n_tower 3 --audio_load_vision --lock-visual --unlock-cls): image and text towers frozen,
    visual tower = `DualAudioStep`'s - AST tokenizer + Perceiver + class token trainable in front of the locked ViT.  The
    loss is the base class's (image <-> audio and text <-> audio).  `images`: the video frame that goes with each clip, after
    `AudioASTProcessorTrain.mix_frames` where mix-up is on."""

    def __init__(self, sd, tower: TowerCfg, text: TextCfg, lens: LensCfg, device, micro_batch: int = 256, lr: float = 2e-4,
                 betas=(0.9, 0.98), eps: float = 1e-6, weight_decay: float = 0.2, rank: int = 0, world_size: int = 1,
                 gemm_cfg: int = -1, comm=None, frozen_res_dtype=torch.float32, local_loss: bool = False,
                 gather_with_grad: bool = False, train_res_dtype=torch.float32, force_comm: bool = False, text_wsplit: Optional[bool] = None, text_arith: str = "f16",
                 overlap_frozen: bool = True, overlap_backward: bool = True,
                 grad_clip_norm: Optional[float] = None, patch_dropout: float = 0.0, drop_seed: int = 0,
                 perceiver_attn_dropout: float = 0.0, perceiver_ff_dropout: float = 0.0):
        self._construct((sd, device, micro_batch, rank, world_size, comm, local_loss, gather_with_grad, force_comm, overlap_frozen,
                         overlap_backward, grad_clip_norm, patch_dropout, drop_seed, perceiver_attn_dropout, perceiver_ff_dropout),
                        (lr, betas, eps, weight_decay),
                        sd, tower, text, lens, gemm_cfg=gemm_cfg, frozen_res_dtype=frozen_res_dtype, train_res_dtype=train_res_dtype,
                        text_wsplit=text_wsplit, text_arith=text_arith)

    def _build(self, sd, tower, text, lens, gemm_cfg=-1, frozen_res_dtype=torch.float32, train_res_dtype=torch.float32,
               text_wsplit=None, text_arith="f16"):
        self.image = VitEngine(sd, "image.", tower, self.dev, gemm_cfg=gemm_cfg, res_dtype=frozen_res_dtype)
        super()._build(sd, tower, text, lens, gemm_cfg=gemm_cfg, frozen_res_dtype=frozen_res_dtype, train_res_dtype=train_res_dtype,
                       text_wsplit=text_wsplit, text_arith=text_arith)

    def forward_backward(self, images: torch.Tensor, texts: torch.Tensor, audio: torch.Tensor) -> torch.Tensor:
        return self._forward_backward(texts, images, audio)

    _loss = _StepState._loss


class TriModalPCStep(_PerceiverLensStep):
    """Point-cloud tri-modal step (reference pc_tri_main.py -> `tri_train_one_epoch` + TriClipLoss; model
    mm_vit_lens/model_cfg.py:85-110): image and text towers frozen, visual tower = PointBERT tokenizer (FPS -> kNN ->
    mini-PointNet with BatchNorm) + Perceiver, both trainable, in front of the locked ViT.  BatchNorm uses the batch
    statistics of each forward call (per micro-batch, per rank - SyncBN off, as the reference's default) and updates the
    running statistics; `bn_training=False` freezes it at the running statistics (--lock-visual-freeze-bn-stats);
    `bn_sync=True` (--use-bn-sync, pc_tri_main.py:372-373) makes the statistics and the backward sums global over the
    ranks: one all-gather of [2C+1] floats per BatchNorm forward, one all-reduce of [2C] per backward."""

    def __init__(self, sd, tower: TowerCfg, text: TextCfg, lens: LensCfg, device, micro_batch: int = 32, lr: float = 2e-4,
                 betas=(0.9, 0.98), eps: float = 1e-6, weight_decay: float = 0.2, rank: int = 0, world_size: int = 1,
                 gemm_cfg: int = -1, bn_training: bool = True, unlock_cls: bool = False, comm=None,
                 frozen_res_dtype=torch.float32, local_loss: bool = False, gather_with_grad: bool = False,
                 train_res_dtype=torch.float32, bn_sync: bool = False, force_comm: bool = False, text_wsplit: Optional[bool] = None, text_arith: str = "f16",
                 overlap_frozen: bool = True, overlap_backward: bool = True,
                 grad_clip_norm: Optional[float] = None, patch_dropout: float = 0.0, drop_seed: int = 0,
                 perceiver_attn_dropout: float = 0.0, perceiver_ff_dropout: float = 0.0):
        self._construct((sd, device, micro_batch, rank, world_size, comm, local_loss, gather_with_grad, force_comm, overlap_frozen,
                         overlap_backward, grad_clip_norm, patch_dropout, drop_seed, perceiver_attn_dropout, perceiver_ff_dropout),
                        (lr, betas, eps, weight_decay),
                        sd, tower, text, lens, gemm_cfg=gemm_cfg, frozen_res_dtype=frozen_res_dtype, train_res_dtype=train_res_dtype,
                        text_wsplit=text_wsplit, text_arith=text_arith, bn_training=bn_training, bn_sync=bn_sync, unlock_cls=unlock_cls)

    def _build(self, sd, tower, text, lens, gemm_cfg=-1, frozen_res_dtype=torch.float32, train_res_dtype=torch.float32,
               text_wsplit=None, text_arith="f16", bn_training=True, bn_sync=False, unlock_cls=False):
        from .points import PointTokenizerTrainer
        from .train import PCLensTrainer
        device = self.dev
        self.image = VitEngine(sd, "image.", tower, device, gemm_cfg=gemm_cfg, res_dtype=frozen_res_dtype)
        self.text = TextEngine(sd, text, device, gemm_cfg=gemm_cfg, res_dtype=frozen_res_dtype, wsplit=text_wsplit, arith=text_arith)
        lens = self._lens_cfg(lens)
        self.lens = LensEngine(sd, "visual.", tower, lens, device, gemm_cfg=gemm_cfg, res_dtype=train_res_dtype)
        self.tok = PointTokenizerTrainer(sd, "visual.visual_adapter.", lens, device, gemm_cfg=gemm_cfg, bn_training=bn_training,
                                         bn_sync=self.comm if bn_sync and self.dist else None, world_size=self.world)
        self._one_stream_backward = bool(bn_sync and self.dist)       # SyncBatchNorm's backward talks to the communicator
        self._mk = lambda: PCLensTrainer(self.lens, self.tok, train_cls=unlock_cls)
        if unlock_cls:
            self.masters["visual.class_embedding"] = self.lens.vit.cls
        self.masters.update(self.tok.masters)
        self._collect_perceiver(sd)

    def _bind_grads(self, t, grads=None):
        super()._bind_grads(t, grads)
        t.tok.grads = t.tower.grads
        self.tok.grads = self.grads

    def _refresh_operands(self):
        self._refresh_perceiver()
        self.tok.refresh_operands()
        for t in self.trainers:
            t.tok.op = self.tok.op

    # The point-cloud step's front (FPS, kNN grouping, the mini-PointNet with BatchNorm: hundreds of small launches) is bound
    # by the host's launch rate and is queued while the previous step drains.  The plan's host wait exposes it: at the
    # benchmark's shape the step came out 0.33 % SLOWER with the packed text tower than without (disjoint ranges,
    # profiles/packed_text_ab.log), for a tower that saves 1.2 ms.  The text tower of this step class runs dense.
    pack_text = False

    def forward_backward(self, images, texts, points, fps_start=None) -> torch.Tensor:
        return self._forward_backward(texts, images, points, fps_start)


# ------------------------------------------------------------------------------------------------ OpenShape
def openshape_param_group(name: str, ndim: int, weight_decay: float = 0.2, trans_lr_scale: float = 0.1):
    """The OpenShape optimizer's group of parameter `name` (a name of `CLIPBindWrap.named_parameters()` or of the
    `LogitScaleNetwork`) with `ndim` dimensions -> (lr_scale, weight_decay), restated from the behaviour of
    VitLens-OpenShape/src/main.py:197-258: a name that contains "backbone.transformer" steps at 0.1 x lr, everything else at lr;
    within either, a parameter with fewer than two dimensions or with "bn", "ln", "bias" or "logit_scale" in its name does
    not decay."""
    no_decay = ndim < 2 or any(w in name for w in ("bn", "ln", "bias", "logit_scale"))
    return (float(trans_lr_scale) if "backbone.transformer" in name else 1.0), (0.0 if no_decay else float(weight_decay))


def _openshape_reference_key(master: str) -> str:
    """The state_dict key (`visual.` names) of the reference parameter a master holds: the interleaved GEGLU masters and the
    stacked self-attention projection are other layouts of `net.0.weight` / `net.0.bias` and of `to_q` + `to_kv`."""
    if master.endswith("_il"):
        master = master[:-3]
    return master.replace("fn.to_qkv.weight", "fn.to_q.weight")


class OpenShapeStep(_PerceiverLensStep):
    """The OpenShape recipe (VitLens-OpenShape/src/main.py + train.py `train_one_epoch_openclip` with
    training.use_openclip_loss / use_openclip_optimizer_scheduler; TRAIN_INFERENCE.md:108-133) as a fused step: the point-cloud
    tower of `CLIPBindWrap` - pnsa tokenizer with its three BatchNorms, Perceiver, class token and the first
    `unlock_trans_first_n_layers` blocks of the KEPT trunk trainable, the rest of the trunk and the tower's `proj` frozen -
    against PRECOMPUTED image and text features, which take the places of the frozen towers' outputs in the tri-modal loss.

    sd: the tower under `visual.` names as `CLIPBindWrap.backbone.state_dict()` holds it (the skipped blocks already gone, the
    kept ones numbered from 0: `tower.layers` is the kept count) and `logit_scale`, the `LogitScaleNetwork` parameter.

    Optimizer (main.py:197-258, train.py:970-975): `openshape_param_group` per tensor - the trunk at 0.1 x lr, the no-decay
    rule on the reference's names - in ONE launch (vl_adamw_multi_step_groups).  `grad_clip_norm` clips the tower's
    parameters only: the logit scale is in the optimizer (no decay, full lr) but outside the clipped norm, and it is not
    clamped after the step - this loop has no clamp.  Its master lies LAST in the flat gradient buffer, so the clipped set is
    one contiguous range in front of it and the unlocked blocks' buckets lie at the start; what is left - Lens, class token,
    logit scale - is one all-reduce.

    Micro-batches are the base class's feature-cache scheme, which is the accumulation of train.py:848-942: every micro-batch
    sees the whole batch of negatives.  The tower's gradient is that loop's sum over j; the logit scale's is the gradient of
    the loss, once (the reference's loop adds it accum_freq times: INTEGRATION.md).  BatchNorm in train mode uses the
    statistics of each micro-batch and updates the running statistics once per micro-batch.

    `last_metrics`: the loss terms and the four retrieval accuracies of openshape.TriClipLoss as device tensors, counted by
    vl_eval_hits on the step's similarity matrices; nothing is read on the host."""

    pack_text = False

    def __init__(self, sd, tower: TowerCfg, lens: LensCfg, device, micro_batch: int = 16, unlock_trans_first_n_layers: int = 2,
                 lr: float = 5e-4, betas=(0.9, 0.98), eps: float = 1e-8, weight_decay: float = 0.2, trans_lr_scale: float = 0.1,
                 rank: int = 0, world_size: int = 1, gemm_cfg: int = -1, bn_training: bool = True, bn_sync: bool = False, comm=None,
                 local_loss: bool = False, gather_with_grad: bool = False, train_res_dtype=torch.float32,
                 force_comm: bool = False, overlap_backward: bool = True, grad_clip_norm: Optional[float] = None,
                 patch_dropout: float = 0.0, drop_seed: int = 0, perceiver_attn_dropout: float = 0.0,
                 perceiver_ff_dropout: float = 0.0, out_channel: Optional[int] = None, use_text_proj: bool = False,
                 use_image_proj: bool = False, use_mask: bool = False):
        if out_channel is not None and tower is not None and int(out_channel) != tower.embed_dim:
            raise NotImplementedError(f"OpenShapeStep: out_channel {out_channel} != the tower's embed_dim {tower.embed_dim} makes "
                                      "CLIPBindWrap drop the tower's projection for a TRAINABLE proj_layer, which this step does not "
                                      "train (the module path, openshape.openclip_step, does)")
        if use_text_proj or use_image_proj:
            raise NotImplementedError("OpenShapeStep: training.use_text_proj / use_image_proj put trainable projections on the "
                                      "precomputed features; this step takes them as they are (the module path trains them)")
        if use_mask:
            raise NotImplementedError("OpenShapeStep: use_mask belongs to the reference's original OpenShape loop, not to the "
                                      "open_clip loss this step computes")
        self.unlock_n, self.trans_lr_scale = int(unlock_trans_first_n_layers or 0), float(trans_lr_scale)
        self._target_cache, self._last = {}, None
        # no frozen tower runs in this step: there is nothing for `overlap_frozen` to overlap
        self._construct((sd, device, micro_batch, rank, world_size, comm, local_loss, gather_with_grad, force_comm, False,
                         overlap_backward, grad_clip_norm, patch_dropout, drop_seed, perceiver_attn_dropout, perceiver_ff_dropout),
                        (lr, betas, eps, weight_decay),
                        sd, tower, lens, gemm_cfg=gemm_cfg, train_res_dtype=train_res_dtype, bn_training=bn_training, bn_sync=bn_sync)

    def _build(self, sd, tower, lens, gemm_cfg=-1, train_res_dtype=torch.float32, bn_training=True, bn_sync=False):
        from .points import PNSATokenizerTrainer
        device, n = self.dev, self.unlock_n
        if lens.pc_tokenizer != "pnsa":
            raise NotImplementedError(f"OpenShapeStep: the recipe's tokenizer is pnsa, got {lens.pc_tokenizer!r} (TriModalPCStep runs PointBERT)")
        if not 0 <= n <= tower.layers:
            raise ValueError(f"OpenShapeStep: cannot unlock {n} of the {tower.layers} kept blocks")
        lens = self._lens_cfg(lens)
        self.embed_dim = tower.embed_dim
        self.lens = LensEngine(sd, "visual.", tower, lens, device, gemm_cfg=gemm_cfg, res_dtype=train_res_dtype)
        eng = self.lens.vit
        for l in range(n):                                      # (as TriModalDepthStep: a trained block carries no LayerNorm-folded operands)
            p = f"visual.transformer.resblocks.{l}."
            w = eng.blocks[l]
            w.pop("in_f", None); w.pop("fc_f", None)
            for nm, key in (("attn.in_proj_weight", "in_w"), ("attn.out_proj.weight", "out_w"), ("mlp.c_fc.weight", "fc_w"),
                            ("mlp.c_proj.weight", "proj_w")):
                self.masters[p + nm] = sd[p + nm].detach().float().to(device).contiguous().clone()
                self.bf16_targets[p + nm] = (l, key)
            for nm, key in (("ln_1.weight", "ln1_w"), ("ln_1.bias", "ln1_b"), ("ln_2.weight", "ln2_w"), ("ln_2.bias", "ln2_b"),
                            ("attn.in_proj_bias", "in_b"), ("attn.out_proj.bias", "out_b"), ("mlp.c_fc.bias", "fc_b"),
                            ("mlp.c_proj.bias", "proj_b")):
                self.masters[p + nm] = w[key]
        self.tok = PNSATokenizerTrainer(sd, "visual.visual_adapter.", lens, device, gemm_cfg=gemm_cfg, bn_training=bn_training,
                                        bn_sync=self.comm if bn_sync and self.dist else None, world_size=self.world)
        self._one_stream_backward = bool(bn_sync and self.dist)
        # CLIPBindWrap.lock unlocks the class token whenever layers are skipped (clip_bind.py:69-80): it is always trained here
        self.masters["visual.class_embedding"] = eng.cls
        self.masters.update(self.tok.masters)
        self._collect_perceiver(sd)

    def _mk(self):
        from .train import PCLensTrainer
        return PCLensTrainer(self.lens, self.tok, tower_kw=dict(train_blocks=range(self.unlock_n), train_cls=True))

    def _bucket_blocks(self):
        return range(self.unlock_n)

    def _bind_grads(self, t, grads=None):
        super()._bind_grads(t, grads)
        t.tok.grads = t.tower.grads
        self.tok.grads = self.grads

    def _refresh_operands(self):
        if not self.trainers:
            self._trainer(0)
        eng = self.lens.vit
        for name, (l, key) in self.bf16_targets.items():
            m = self.masters[name]
            ops.cast_bf16(m, out=eng.blocks[l][key])
            ops.transpose_to_bf16(m, ldo=m.shape[0], out=self.trainers[0].tower.wT[l][key])
        self._refresh_perceiver()
        self.tok.refresh_operands()
        for t in self.trainers:
            t.tok.op = self.tok.op

    # ---- the optimizer's groups ----
    def param_groups(self) -> Dict[str, tuple]:
        """master name -> (lr_scale, weight_decay): `openshape_param_group` of the reference parameter the master holds, under
        the name `CLIPBindWrap` gives it (`visual.` -> `backbone.`) and with the dimensions it has there."""
        wd = self._adamw_wd
        out = {}
        for k, m in self.masters.items():
            key = _openshape_reference_key(k)
            ref = self._base_sd.get(key)
            name = key if key == "logit_scale" else "backbone." + key[len("visual."):]
            out[k] = openshape_param_group(name, m.ndim if ref is None else ref.ndim, wd, self.trans_lr_scale)
        return out

    def _optimizer_groups(self):
        groups = self.param_groups()
        return dict(lr_scale={k: g[0] for k, g in groups.items() if g[0] != 1.0}, no_clip=("logit_scale",),
                    decay={k: g[1] != 0.0 for k, g in groups.items()})

    def _construct(self, host, adamw, *build, **build_kw):
        self._adamw_wd = float(adamw[3])
        self._init_host(*host)
        ls = self.masters.pop("logit_scale")                    # re-inserted LAST: behind the clipped range of the flat buffer
        self._build(*build, **build_kw)
        self.masters["logit_scale"] = ls
        self.opt = AdamW(self.masters, *adamw, **self._optimizer_groups())

    def _alloc_flat_grads(self):
        super()._alloc_flat_grads()
        # the layout the optimizer relies on: the logit scale behind everything that is clipped
        last = self.grads["logit_scale"]
        self._clip_end = (last.data_ptr() - self.flat_grad.data_ptr()) // 4
        assert self._clip_end + 4 >= self.flat_grad.numel() and list(self.masters)[-1] == "logit_scale", "logit_scale must lie last"

    def _clipped_grads(self):
        return self.flat_grad[:self._clip_end]

    def _clamp_logit_scale(self):
        pass                                                    # (train.py:944-1000: the OpenShape loop does not clamp)

    def set_lr(self, lr: float):
        """The base learning rate (what `training.scheduler.cosine_lr(step.opt, ...)` assigns too); the trunk's group follows at
        `trans_lr_scale` x lr inside the kernel."""
        self.opt.lr = lr

    # ---- the step ----
    def forward_backward(self, features: torch.Tensor, xyz: torch.Tensor, img_feat: torch.Tensor, text_feat: torch.Tensor,
                         fps_start=None) -> torch.Tensor:
        """features [B,N,in_dim], xyz [B,N,3] (`CLIPBindWrap.forward(features, xyz=xyz)`); img_feat / text_feat: the precomputed
        [B,E] features, normalised here.  Returns the loss; `last_metrics` has its parts."""
        B, E, dev = features.shape[0], self.embed_dim, self.dev
        mb, nmb = self._prepare(B)
        f32 = lambda t: t.to(device=dev, dtype=torch.float32).contiguous()
        fi, ft = ops.l2_normalize(f32(img_feat)), ops.l2_normalize(f32(text_feat))
        if tuple(fi.shape) != (B, E) or tuple(ft.shape) != (B, E):
            raise ValueError(f"OpenShapeStep: img_feat / text_feat must be [{B}, {E}], got {tuple(fi.shape)} / {tuple(ft.shape)}")
        vraw, fv, vnorm = torch.empty(B, E, device=dev), torch.empty(B, E, device=dev), torch.empty(B, device=dev)
        drop = self.patch_dropout > 0.0
        for i in range(nmb):
            s = slice(i * mb, (i + 1) * mb)
            kw = dict(zip(("keep", "inv"), self.drop_indices(DROP_TOWER_VISUAL, self.lens.vit, i * mb, mb))) if drop else {}
            if self._lens_drop:
                kw["drop"] = self.lens_draw(i * mb)
            vraw[s] = self._trainer(i).forward(features[s], None if fps_start is None else fps_start[s], xyz=xyz[s], **kw)
        ops.l2_normalize(vraw, out=fv, norms=vnorm)
        loss, dv, ds = self._loss(fi, ft, fv)
        self._backward_all(ops.l2_normalize_bwd(fv, dv, vnorm), nmb, mb)
        ops.axpy(self.grads["logit_scale"], ds)
        return loss

    def _targets(self, n: int, off: int):
        key = (n, off)
        if key not in self._target_cache:
            self._target_cache[key] = torch.arange(off, off + n, device=self.dev, dtype=torch.int64)
        return self._target_cache[key]

    def _count_hits(self, hits, x, y_all, off: int, logits=None):
        """hits[0] += the rows of x whose best column of x @ y_all^T is their own (column row + off): vl_eval_hits with
        k0 = k1 = 1.  `logits`: the similarity matrix where the loss has it already (any positive scale)."""
        R = x.shape[0]
        if logits is not None:
            ops.eval_hits(logits, self._targets(R, off), ks=(1, 1), hits=hits)
            return
        xb, yb = ops.split_bf16x3(x, 0), ops.split_bf16x3(y_all, 1)
        rb = _chunk_rows(R, y_all.shape[0], None) or R
        for r0 in range(0, R, rb):
            r1 = min(R, r0 + rb)
            ops.eval_hits(ops.logits_gemm(xb[r0:r1], yb, 1.0), self._targets(r1 - r0, off + r0), ks=(1, 1), hits=hits)

    def _loss(self, fi, ft, fv):
        """The base class's tri-modal loss on the given image / text features, its two terms kept apart, and the retrieval hits
        of openshape.TriClipLoss (loss.py:80-185).  The accumulators are zeroed and added to by library launches: on one rank
        the section holds no framework kernel."""
        acc = ops.fill(torch.empty(4, device=self.dev, dtype=torch.float32))
        hits = ops.fill(torch.empty(3, 2, device=self.dev, dtype=torch.int32))
        li, lt, ds, total = acc[0:1], acc[1:2], acc[2:3], acc[3:4]
        b = fv.shape[0]
        if self.dist:
            ai, at, av = self._gather(fi, ft, fv)
            kw = dict(local_loss=self.local_loss, gather_with_grad=self.gather_with_grad, need_x=False, dist=True)
            l1, _, dv, ds1 = pair_loss_and_grads(self.comm, self.rank, self.world, fi, fv, ai, av, self.logit_scale, **kw)
            l2, _, dv2, ds2 = pair_loss_and_grads(self.comm, self.rank, self.world, ft, fv, at, av, self.logit_scale, **kw)
            for dst, src in ((li, l1), (lt, l2), (ds, ds1), (ds, ds2)):
                ops.axpy(dst, src)
            lg_i = lg_t = None
            off = self.rank * b if self.local_loss else 0
            qi, qt, qv = (fi, ft, fv) if self.local_loss else (ai, at, av)
        else:
            _, c1 = pair_forward(fi, fv, self.logit_scale, loss_acc=li)
            _, c2 = pair_forward(ft, fv, self.logit_scale, loss_acc=lt)
            _, dv, _ = pair_backward(c1, need_dx=False, dscale_acc=ds)
            _, dv2, _ = pair_backward(c2, need_dx=False, dscale_acc=ds)
            lg_i, lg_t = c1[2], c2[2]                           # (None where the pair loss ran row-blocked)
            ai, av, off = fi, fv, 0
            qi, qt, qv = fi, ft, fv
        ops.axpy(dv, dv2)
        ops.axpy(total, li); ops.axpy(total, lt)
        self._count_hits(hits[0], qi, av, off, lg_i)            # i2v
        self._count_hits(hits[1], qv, ai, off)                  # v2i
        self._count_hits(hits[2], qt, av, off, lg_t)            # t2v (= v2t: loss.py:161 counts the text rows for both)
        self._last = (acc, hits, qi.shape[0])
        return total, dv, ds

    @property
    def last_metrics(self) -> Dict[str, torch.Tensor]:
        """The loss dictionary of openshape.TriClipLoss for the last forward_backward, device tensors (built when asked for)."""
        acc, hits, n = self._last
        a = hits[:, 0].float() / n
        return {"contrastive_loss": acc[3], "i_contra_loss": acc[0], "t_contra_loss": acc[1], "i2v_acc": a[0], "v2i_acc": a[1],
                "t2v_acc": a[2], "v2t_acc": a[2]}
