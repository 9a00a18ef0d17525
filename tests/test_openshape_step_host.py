"""CPU: the host side of the OpenShape fused step (`vitlens_hip.step.OpenShapeStep`) and of `openshape.calculate_metrics`.

  * `openshape_param_group` - the recipe's optimizer groups (VitLens-OpenShape/src/main.py:197-258) - on the parameter names of
    a tiny `CLIPBindWrap` over the `tiny_pnsa` configuration with a 4-block tower, skip 1, unlock 2, against the four name
    lists written out below;
  * `OpenShapeStep`'s real `__init__` on a CPU device with `_build` replaced by linear stand-ins, in the manner of
    tests/test_step_gloo.py (its torch stand-in for `ops` and its towers): world 1 and gloo world 2 - the bucket layout, every
    gradient element reduced exactly once, the numbers against autograd of the global loss, identical replicas after two
    steps, the logit scale's slot behind the clipped range;
  * the counting of `calculate_metrics` against a plain-torch restatement on random logits with ties and an empty class, the
    kernel call stubbed by the restated counts of tests/eval_ref.py."""
import json
import os
import sys
import tempfile
import warnings
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import eval_ref
from golden_util import GOLDEN, load_npz, split

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

BASE_NO_DECAY = [
    'backbone.class_embedding', 'backbone.visual_adapter.sa.mlp_convs.0.bias',
    'backbone.visual_adapter.sa.mlp_convs.1.bias', 'backbone.visual_adapter.sa.mlp_convs.2.bias',
    'backbone.visual_adapter.sa.mlp_bns.0.weight', 'backbone.visual_adapter.sa.mlp_bns.0.bias',
    'backbone.visual_adapter.sa.mlp_bns.1.weight', 'backbone.visual_adapter.sa.mlp_bns.1.bias',
    'backbone.visual_adapter.sa.mlp_bns.2.weight', 'backbone.visual_adapter.sa.mlp_bns.2.bias',
    'backbone.visual_adapter.lift.0.bias', 'backbone.visual_adapter.lift.2.weight', 'backbone.visual_adapter.lift.2.bias',
    'backbone.perceiver.layers.0.0.norm.weight', 'backbone.perceiver.layers.0.0.norm.bias',
    'backbone.perceiver.layers.0.0.norm_context.weight', 'backbone.perceiver.layers.0.0.norm_context.bias',
    'backbone.perceiver.layers.0.0.fn.to_out.bias', 'backbone.perceiver.layers.0.1.norm.weight',
    'backbone.perceiver.layers.0.1.norm.bias', 'backbone.perceiver.layers.0.1.fn.net.0.bias',
    'backbone.perceiver.layers.0.1.fn.net.2.bias', 'backbone.perceiver.layers.0.2.0.0.norm.weight',
    'backbone.perceiver.layers.0.2.0.0.norm.bias', 'backbone.perceiver.layers.0.2.0.0.fn.to_out.bias',
    'backbone.perceiver.layers.0.2.0.1.norm.weight', 'backbone.perceiver.layers.0.2.0.1.norm.bias',
    'backbone.perceiver.layers.0.2.0.1.fn.net.0.bias', 'backbone.perceiver.layers.0.2.0.1.fn.net.2.bias',
    'backbone.perceiver.layers.1.0.norm.weight', 'backbone.perceiver.layers.1.0.norm.bias',
    'backbone.perceiver.layers.1.0.norm_context.weight', 'backbone.perceiver.layers.1.0.norm_context.bias',
    'backbone.perceiver.layers.1.0.fn.to_out.bias', 'backbone.perceiver.layers.1.1.norm.weight',
    'backbone.perceiver.layers.1.1.norm.bias', 'backbone.perceiver.layers.1.1.fn.net.0.bias',
    'backbone.perceiver.layers.1.1.fn.net.2.bias', 'backbone.perceiver.layers.1.2.0.0.norm.weight',
    'backbone.perceiver.layers.1.2.0.0.norm.bias', 'backbone.perceiver.layers.1.2.0.0.fn.to_out.bias',
    'backbone.perceiver.layers.1.2.0.1.norm.weight', 'backbone.perceiver.layers.1.2.0.1.norm.bias',
    'backbone.perceiver.layers.1.2.0.1.fn.net.0.bias', 'backbone.perceiver.layers.1.2.0.1.fn.net.2.bias', 'logit_scale',
]
TRANS_NO_DECAY = [
    'backbone.transformer.resblocks.0.ln_1.weight', 'backbone.transformer.resblocks.0.ln_1.bias',
    'backbone.transformer.resblocks.0.ln_2.weight', 'backbone.transformer.resblocks.0.ln_2.bias',
    'backbone.transformer.resblocks.0.attn.in_proj_bias', 'backbone.transformer.resblocks.0.attn.out_proj.bias',
    'backbone.transformer.resblocks.0.mlp.c_fc.bias', 'backbone.transformer.resblocks.0.mlp.c_proj.bias',
    'backbone.transformer.resblocks.1.ln_1.weight', 'backbone.transformer.resblocks.1.ln_1.bias',
    'backbone.transformer.resblocks.1.ln_2.weight', 'backbone.transformer.resblocks.1.ln_2.bias',
    'backbone.transformer.resblocks.1.attn.in_proj_bias', 'backbone.transformer.resblocks.1.attn.out_proj.bias',
    'backbone.transformer.resblocks.1.mlp.c_fc.bias', 'backbone.transformer.resblocks.1.mlp.c_proj.bias',
]
TRANS_DECAY = [
    'backbone.transformer.resblocks.0.attn.in_proj_weight', 'backbone.transformer.resblocks.0.attn.out_proj.weight',
    'backbone.transformer.resblocks.0.mlp.c_fc.weight', 'backbone.transformer.resblocks.0.mlp.c_proj.weight',
    'backbone.transformer.resblocks.1.attn.in_proj_weight', 'backbone.transformer.resblocks.1.attn.out_proj.weight',
    'backbone.transformer.resblocks.1.mlp.c_fc.weight', 'backbone.transformer.resblocks.1.mlp.c_proj.weight',
]
BASE_DECAY = [
    'backbone.visual_adapter.sa.mlp_convs.0.weight', 'backbone.visual_adapter.sa.mlp_convs.1.weight',
    'backbone.visual_adapter.sa.mlp_convs.2.weight', 'backbone.visual_adapter.lift.0.weight', 'backbone.perceiver.latents',
    'backbone.perceiver.layers.0.0.fn.to_q.weight', 'backbone.perceiver.layers.0.0.fn.to_kv.weight',
    'backbone.perceiver.layers.0.0.fn.to_out.weight', 'backbone.perceiver.layers.0.1.fn.net.0.weight',
    'backbone.perceiver.layers.0.1.fn.net.2.weight', 'backbone.perceiver.layers.0.2.0.0.fn.to_q.weight',
    'backbone.perceiver.layers.0.2.0.0.fn.to_kv.weight', 'backbone.perceiver.layers.0.2.0.0.fn.to_out.weight',
    'backbone.perceiver.layers.0.2.0.1.fn.net.0.weight', 'backbone.perceiver.layers.0.2.0.1.fn.net.2.weight',
    'backbone.perceiver.layers.1.0.fn.to_q.weight', 'backbone.perceiver.layers.1.0.fn.to_kv.weight',
    'backbone.perceiver.layers.1.0.fn.to_out.weight', 'backbone.perceiver.layers.1.1.fn.net.0.weight',
    'backbone.perceiver.layers.1.1.fn.net.2.weight', 'backbone.perceiver.layers.1.2.0.0.fn.to_q.weight',
    'backbone.perceiver.layers.1.2.0.0.fn.to_kv.weight', 'backbone.perceiver.layers.1.2.0.0.fn.to_out.weight',
    'backbone.perceiver.layers.1.2.0.1.fn.net.0.weight', 'backbone.perceiver.layers.1.2.0.1.fn.net.2.weight',
]


def _tiny_wrap():
    import open_clip as oc
    import openshape
    z = np.load(os.path.join(GOLDEN, "tiny_pnsa.npz"))
    cfg = json.loads(str(z["meta"]))["cfg"]
    _, _, _, _, meta = split(load_npz("tiny_pc.npz"))
    a = dict(meta["args"])
    a.update(pc_tokenizer="pnsa", pc_in_channel=cfg["in_dim"], pc_num_group=cfg["num_group"], pc_group_size=cfg["group_size"],
             pc_radius=cfg["radius"], pc_encoder_dims=cfg["encoder_dims"], pc_trans_dim=cfg["trans_dim"],
             perceiver_input_chan=cfg["trans_dim"], skip_trans_first_n_layers=1, unlock_cls=False)
    a.pop("model", None)
    mc = json.loads(json.dumps(meta["model_cfg"]))
    mc["vision_cfg"]["layers"] = 4
    args = SimpleNamespace(**a, model=SimpleNamespace(out_channel=mc["embed_dim"]))
    with tempfile.TemporaryDirectory() as td:
        with open(os.path.join(td, "tiny-lens4-host.json"), "w") as f:
            json.dump(mc, f)
        oc.add_model_config(td)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")          # (precision="fp32" describes what training does with it)
            tri = oc.tri_create_model("tiny-lens4-host", None, precision="fp32", device="cpu", output_dict=True, args=args)
    w = openshape.CLIPBindWrap(args, model=tri)
    w.lock(unlocked_groups=0, freeze_bn_stats=False, unlock_cls=False, unlock_trans_first_n_layers=2)
    return w, openshape.LogitScaleNetwork()


def test_param_groups_of_a_tiny_clip_bind_wrap():
    from vitlens_hip.step import openshape_param_group
    wrap, scale = _tiny_wrap()
    named = [(n, p) for n, p in list(wrap.named_parameters()) + list(scale.named_parameters()) if p.requires_grad]
    assert len(wrap.backbone.transformer.resblocks._modules) == 3
    got = {}
    for n, p in named:
        got.setdefault(openshape_param_group(n, p.ndim, weight_decay=0.2), []).append(n)
    assert set(got) == {(1.0, 0.0), (0.1, 0.0), (0.1, 0.2), (1.0, 0.2)}
    assert got[(1.0, 0.0)] == BASE_NO_DECAY
    assert got[(0.1, 0.0)] == TRANS_NO_DECAY
    assert got[(0.1, 0.2)] == TRANS_DECAY
    assert got[(1.0, 0.2)] == BASE_DECAY
    shape = dict((n, tuple(p.shape)) for n, p in named)
    A = "backbone.visual_adapter."
    # which clause of the rule decides each of these
    assert A + "sa.mlp_bns.0.weight" in BASE_NO_DECAY and "bn" in A + "sa.mlp_bns.0.weight"
    assert A + "lift.2.weight" in BASE_NO_DECAY and len(shape[A + "lift.2.weight"]) < 2 and not any(w in A + "lift.2.weight" for w in ("bn", "ln", "bias"))
    assert "backbone.class_embedding" in BASE_NO_DECAY and len(shape["backbone.class_embedding"]) < 2
    assert "backbone.perceiver.latents" in BASE_DECAY and len(shape["backbone.perceiver.latents"]) == 2
    assert A + "sa.mlp_convs.0.weight" in BASE_DECAY and len(shape[A + "sa.mlp_convs.0.weight"]) == 4
    assert "backbone.transformer.resblocks.0.ln_1.weight" in TRANS_NO_DECAY
    assert "logit_scale" in BASE_NO_DECAY and not any(n.startswith("backbone.transformer.resblocks.2.") for n, _ in named)
    # a frozen name is grouped by the same rule (the helper does not look at requires_grad)
    assert openshape_param_group("backbone.transformer.resblocks.2.mlp.c_fc.weight", 2, 0.05) == (0.1, 0.05)
    assert openshape_param_group("backbone.proj", 2, 0.05, trans_lr_scale=0.5) == (1.0, 0.05)


def test_masters_take_the_group_of_the_reference_parameter_they_hold():
    from vitlens_hip import step as ST
    assert ST._openshape_reference_key("visual.perceiver.layers.0.1.fn.net.0.weight_il") == "visual.perceiver.layers.0.1.fn.net.0.weight"
    assert ST._openshape_reference_key("visual.perceiver.layers.0.1.fn.net.0.bias_il") == "visual.perceiver.layers.0.1.fn.net.0.bias"
    assert ST._openshape_reference_key("visual.perceiver.layers.0.2.0.0.fn.to_qkv.weight") == "visual.perceiver.layers.0.2.0.0.fn.to_q.weight"
    st = ST.OpenShapeStep.__new__(ST.OpenShapeStep)
    st._adamw_wd, st.trans_lr_scale = 0.2, 0.1
    st._base_sd = {"visual.visual_adapter.sa.mlp_convs.0.weight": torch.zeros(8, 6, 1, 1), "visual.class_embedding": torch.zeros(4),
                   "visual.perceiver.layers.0.1.fn.net.0.weight": torch.zeros(8, 4), "visual.perceiver.layers.0.1.fn.net.0.bias": torch.zeros(8),
                   "visual.perceiver.layers.0.2.0.0.fn.to_q.weight": torch.zeros(4, 4),
                   "visual.transformer.resblocks.0.mlp.c_fc.weight": torch.zeros(16, 4), "visual.transformer.resblocks.0.ln_1.weight": torch.zeros(4)}
    st.masters = {"visual.transformer.resblocks.0.mlp.c_fc.weight": torch.zeros(16, 4), "visual.transformer.resblocks.0.ln_1.weight": torch.zeros(4),
                  "visual.class_embedding": torch.zeros(4), "visual.visual_adapter.sa.mlp_convs.0.weight": torch.zeros(8, 6),
                  "visual.perceiver.layers.0.1.fn.net.0.weight_il": torch.zeros(8, 4), "visual.perceiver.layers.0.1.fn.net.0.bias_il": torch.zeros(8),
                  "visual.perceiver.layers.0.2.0.0.fn.to_qkv.weight": torch.zeros(12, 4), "logit_scale": torch.zeros(1)}
    assert list(st.param_groups().values()) == [(0.1, 0.2), (0.1, 0.0), (1.0, 0.0), (1.0, 0.2), (1.0, 0.2), (1.0, 0.0), (1.0, 0.2), (1.0, 0.0)]
    kw = st._optimizer_groups()
    assert kw["no_clip"] == ("logit_scale",) and set(kw["lr_scale"]) == {k for k in st.masters if "transformer" in k}
    assert [k for k, d in kw["decay"].items() if d] == [k for k, g in st.param_groups().items() if g[1] > 0]


def test_refusals_name_their_reason():
    from vitlens_hip.step import OpenShapeStep
    tower = SimpleNamespace(embed_dim=32, layers=3)
    for kw, word in ((dict(out_channel=48), "proj_layer"), (dict(use_text_proj=True), "use_text_proj"),
                     (dict(use_image_proj=True), "use_image_proj"), (dict(use_mask=True), "use_mask")):
        with pytest.raises(NotImplementedError, match=word):
            OpenShapeStep({"logit_scale": torch.tensor(0.0)}, tower, None, "cpu", **kw)


# ------------------------------------------------------------------------------------------------ the step's host logic
E_DIM, D_IN, NBLK = 16, 24, 2


def _ops():
    from test_step_gloo import _fake_ops
    o = _fake_ops()
    o.fill = lambda p, value=0.0: p.fill_(value)

    def eval_hits(logits, target, ks=(1, 5), class_map=None, hits=None, per_class=None, pred=None, need_pred=False):
        h, _, _ = eval_ref.eval_hits(logits.detach().numpy(), target.numpy(), ks)
        hits += torch.tensor(h, dtype=hits.dtype)
        return hits, None
    o.eval_hits = eval_hits
    return o


def _worker(rank, world, port, nmb, ret):
    sys.path.insert(0, os.path.join(ROOT, "vit-lens_amd")); sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch.distributed as dist
    from test_step_gloo import _LinearTower, _Rec
    os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from vitlens_hip import step as ST, train as TR
    ST.ops = _ops(); TR.ops = ST.ops
    g = torch.Generator().manual_seed(0)
    Wv = torch.randn(D_IN, E_DIM, generator=g) * 0.3
    b = 2 * nmb
    gd = torch.Generator().manual_seed(100)
    X = {k: torch.randn(world * b, n, generator=gd) for k, n in (("img", E_DIM), ("txt", E_DIM), ("vis", D_IN + 3))}
    mine = {k: v[rank * b:(rank + 1) * b] for k, v in X.items()}
    comm = _Rec(ST.TorchComm())
    errs = []

    class Tower(_LinearTower):
        def forward(self, x, fps_start=None, xyz=None):
            self.xyz = xyz
            return super().forward(x, fps_start)

    class Host(ST.OpenShapeStep):
        def _build(self, sd, tower, lens, **kw):
            self.embed_dim = E_DIM
            for l in range(self.unlock_n):
                self.masters[f"visual.transformer.resblocks.{l}.mlp.c_fc.weight"] = torch.zeros(3, 5)
            self.masters["visual.W"] = Wv.clone()

        def _mk(self):
            return Tower(self.masters["visual.W"], self.grads, "visual.W", self.unlock_n)

        def _trainer(self, i):
            while len(self.trainers) <= i:
                self.trainers.append(self._mk())
            return self.trainers[i]

        def _bind_grads(self, t, grads=None):
            t.grads = self.grads if grads is None else grads

        def _refresh_operands(self):
            pass

    st = Host({"logit_scale": torch.tensor(2.0).log()}, None, None, "cpu", micro_batch=2, unlock_trans_first_n_layers=NBLK, lr=1e-2,
              rank=rank, world_size=world, comm=comm)
    # ---- layout: blocks first (their buckets), the rest, the logit scale last and outside the clipped range ----
    if list(st.masters) != [f"visual.transformer.resblocks.{l}.mlp.c_fc.weight" for l in range(NBLK)] + ["visual.W", "logit_scale"]:
        errs.append(f"master order {list(st.masters)}")
    if st.opt.no_clip != frozenset({"logit_scale"}) or st.overlap_frozen:
        errs.append("logit_scale is clipped, or overlap_frozen is on")
    fps = torch.arange(rank * b, (rank + 1) * b)
    fb = lambda: st.forward_backward(mine["vis"], mine["vis"][:, :3], mine["img"], mine["txt"], fps_start=fps)
    loss = fb()
    al = lambda n: (n + 3) // 4 * 4
    want_ranges = [(l * al(15), (l + 1) * al(15)) for l in range(NBLK)]
    if [st._block_range(l) for l in range(NBLK)] != want_ranges or st._rest_ranges() != (0, NBLK * al(15)):
        errs.append(f"bucket layout {[st._block_range(l) for l in range(NBLK)]} rest {st._rest_ranges()}")
    clipped = st._clipped_grads()
    gl = st.grads["logit_scale"]
    if clipped.data_ptr() != st.flat_grad.data_ptr() or clipped.numel() != st.flat_grad.numel() - 4 \
            or gl.data_ptr() != st.flat_grad.data_ptr() + 4 * clipped.numel():
        errs.append("the clipped range does not end where the logit scale's slot begins")
    if st.opt.group_rows(st.grads)[-1] != (1.0, True) or any(r[1] for r in st.opt.group_rows(st.grads)[:-1]):
        errs.append(f"group rows {st.opt.group_rows(st.grads)}")
    if st.opt.group_rows(st.grads)[:NBLK] != [(0.1, False)] * NBLK:
        errs.append("the trunk's masters do not step at a tenth")
    if [len(t.xyz) for t in st.trainers] != [2] * nmb or not torch.equal(torch.cat([t.fps_start for t in st.trainers]), fps):
        errs.append("micro-batch slices of xyz / fps_start")
    st.finish_reduce()
    summed = {n: v.clone() for n, v in st.reduced_grads().items()}
    metrics = {k: float(v) for k, v in st.last_metrics.items()}
    st.optimizer_step()
    # ---- every element reduced exactly once: NBLK async buckets + ONE call for the Lens and the logit scale ----
    if world > 1:
        red = [e for e in comm.log if e[0].startswith("all_reduce")]
        if sum(e[1] for e in red) != st.flat_grad.numel() or [e[0] for e in red].count("all_reduce_async") != NBLK \
                or [e[0] for e in red].count("all_reduce") != 1:
            errs.append(f"gradient all-reduces {red} over {st.flat_grad.numel()} elements")
        if [e[0] for e in comm.log].count("all_gather") != 1:
            errs.append(f"all_gather: {comm.log}")
    elif comm.log:
        errs.append(f"collectives on one rank: {comm.log}")
    # ---- numbers: autograd of the global loss ----
    Wr = Wv.clone().requires_grad_(True); ls = torch.tensor(2.0, requires_grad=True)
    nrm = lambda t: t / t.norm(dim=-1, keepdim=True)
    fv, ft, fi = nrm(X["vis"][:, :D_IN] @ Wr), nrm(X["txt"]), nrm(X["img"])
    lab = torch.arange(world * b)
    ce = torch.nn.functional.cross_entropy
    pair = lambda x, y: (ce(ls * x @ y.t(), lab) + ce((ls * x @ y.t()).t(), lab)) / 2
    li, lt = pair(fi, fv), pair(ft, fv)
    (li + lt).backward()
    for name, got, want in (("loss", float(loss), float(li + lt)), ("i", metrics["i_contra_loss"], float(li)),
                            ("t", metrics["t_contra_loss"], float(lt)), ("total", metrics["contrastive_loss"], float(li + lt))):
        if abs(got - want) > 1e-4:
            errs.append(f"{name}: {got} vs {want}")
    acc = lambda s: float((s.argmax(1) == lab).float().mean())
    sim_i, sim_t = (fi @ fv.t()).detach(), (ft @ fv.t()).detach()
    for k, want in (("i2v_acc", acc(sim_i)), ("v2i_acc", acc(sim_i.t())), ("t2v_acc", acc(sim_t)), ("v2t_acc", acc(sim_t))):
        if abs(metrics[k] - want) > 1e-6:
            errs.append(f"{k}: {metrics[k]} vs {want}")
    got = summed["visual.W"] / world
    if not torch.allclose(got, Wr.grad / world, rtol=2e-4, atol=1e-6):
        errs.append(f"grad mismatch {float((got - Wr.grad / world).abs().max()):.3e}")
    if not torch.allclose(summed["logit_scale"] / world, (ls.grad * 2.0).reshape(1), rtol=1e-3, atol=1e-5):
        errs.append(f"logit_scale grad {float(summed['logit_scale'] / world)} vs {float(ls.grad * 2.0)}")
    # ---- the groups are felt by the optimizer: the trunk moved a tenth as far; the logit scale is not clamped ----
    if float((st.masters["visual.W"] - Wv).abs().max()) == 0.0:
        errs.append("optimizer step did not move the master")
    blk = st.masters["visual.transformer.resblocks.1.mlp.c_fc.weight"]
    if not torch.allclose(blk.abs(), torch.full_like(blk, 1e-3), rtol=1e-3):          # first Adam step: lr * lr_scale
        errs.append(f"trunk step {float(blk.abs().max())} is not 0.1 x lr")
    st.logit_scale.fill_(7.0)
    fb(); st.optimizer_step()
    if float(st.logit_scale) < 6.9:
        errs.append("the logit scale was clamped")
    # ---- replicas identical after two steps ----
    cs = torch.tensor([float(sum(m.double().sum() for m in st.masters.values()))])
    lst = [torch.zeros(1) for _ in range(world)]
    dist.all_gather(lst, cs)
    if any(abs(float(x) - float(lst[0])) > 1e-9 for x in lst):
        errs.append(f"replicas diverged: {lst}")
    ret[rank] = errs
    dist.destroy_process_group()


@pytest.mark.parametrize("world,nmb", [(1, 1), (1, 2), (2, 1), (2, 3)])
def test_openshape_step_host_logic(world, nmb):
    port = 29960 + 4 * world + nmb
    mgr = mp.Manager()
    ret = mgr.dict()
    mp.spawn(_worker, args=(world, port, nmb, ret), nprocs=world, join=True)
    for r in range(world):
        assert ret[r] == [], (r, ret[r])


# ------------------------------------------------------------------------------------------------ calculate_metrics
def test_calculate_metrics_counting_against_plain_torch(monkeypatch):
    import openshape
    from openshape import eval as EV
    from vitlens_hip import ops
    C, B = 6, 16
    g = torch.Generator().manual_seed(3)
    logits = [(torch.randint(0, 4, (B, C), generator=g) / 4.0) for _ in range(3)]          # few distinct values: ties in every row
    labels = [torch.randint(0, C - 1, (B,), generator=g) for _ in range(3)]                  # class 5 has no sample
    labels[1][labels[1] == 2] = 0
    calls = []

    def fake_hits(lg, target, ks=(1, 5), class_map=None, hits=None, per_class=None, pred=None, need_pred=False):
        h, pc, _ = eval_ref.eval_hits(lg.numpy(), target.numpy(), ks)
        hits += torch.tensor(h, dtype=hits.dtype)
        if per_class is not None:
            per_class += torch.tensor(pc, dtype=per_class.dtype)
        calls.append((tuple(ks), per_class is not None))
        return hits, None
    monkeypatch.setattr(ops, "eval_hits", fake_hits)
    monkeypatch.setattr(EV, "_classifier", lambda feat, device: feat)
    it = iter(logits)
    monkeypatch.setattr(EV, "_logits", lambda pred, cls: next(it))
    seen = []

    def model(features, xyz=None):
        seen.append((features.shape, xyz.shape))
        return features
    batches = [{"features_dense": torch.zeros(B, 4, 3), "xyz_dense": torch.zeros(B, 4, 3), "category": lab} for lab in labels]
    m = openshape.calculate_metrics(model, batches, torch.zeros(C, 8), C, device="cpu")
    assert calls == [((1, 3), True), ((1, 5), False)] * 3 and len(seen) == 3
    # plain torch: rank of the label among the row's logits, the lower index first among equals
    lg, lab = torch.cat(logits), torch.cat(labels)
    own = lg[torch.arange(len(lab)), lab]
    ahead = (lg > own[:, None]).sum(1) + ((lg == own[:, None]) & (torch.arange(C)[None, :] < lab[:, None])).sum(1)
    n = len(lab)
    assert m.samples == n
    assert m.topk_acc == [100.0 * int((ahead < k).sum()) / n for k in (1, 3, 5)]
    assert m.topk_acc[0] < m.topk_acc[1] < m.topk_acc[2] < 100.0
    count = torch.bincount(lab, minlength=C)
    correct = torch.bincount(lab[ahead < 1], minlength=C)
    assert torch.equal(m.per_cat_count, count) and torch.equal(m.per_cat_correct, correct)
    assert int(count[5]) == 0 and torch.isnan(m.per_cat_acc[5]) and not torch.isnan(m.per_cat_acc[:5]).any()
    assert torch.equal(m.per_cat_acc[:5], correct[:5].double() / count[:5].double())
    assert m.overall_acc == float(correct.sum()) / n


def test_the_three_wrappers_supply_their_class_counts(monkeypatch):
    import openshape
    from openshape import eval as EV
    got = []
    monkeypatch.setattr(EV, "calculate_metrics", lambda model, loader, feat, num_class, device: got.append((num_class, feat)) or num_class)
    loader = SimpleNamespace(dataset=SimpleNamespace(clip_cat_feat="from the dataset"))
    model = torch.nn.Linear(2, 2).train()
    assert openshape.test_modelnet40(model, loader) == 40 and model.training
    assert openshape.test_objaverse_lvis(model, loader, clip_text_feat="given") == 1156
    assert openshape.test_scanobjectnn(model, loader) == 15
    assert got == [(40, "from the dataset"), (1156, "given"), (15, "from the dataset")]
