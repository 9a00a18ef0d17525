"""GPU: TriModalAudioStep - the audio Lens (AST tokenizer + Perceiver + class token) trained against the frozen image AND text
towers - on the tiny golden model (tests/golden/tiny_audio.npz): the reference's tri-modal `step_loss` and every
`grad/visual.*` of the trainable set."""
import pytest
import torch

from golden_util import load_npz, split, specs_from_meta

pytestmark = pytest.mark.gpu


def relerr(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


@pytest.fixture(scope="module")
def tiny():
    from vitlens_hip import engine as E
    sd, ins, outs, grads, meta = split(load_npz("tiny_audio.npz"))
    tower, text, lens = specs_from_meta(meta)
    tc = E.TowerCfg(width=tower.width, layers=tower.layers, heads=tower.heads, patch=tower.patch,
                    image_size=tower.image_size, embed_dim=tower.embed_dim)
    xc = E.TextCfg(context_length=text.context_length, vocab_size=text.vocab_size, width=text.width, heads=text.heads,
                   layers=text.layers, embed_dim=text.embed_dim)
    lc = E.LensCfg(**{k: getattr(lens, k) for k in E.LensCfg.__dataclass_fields__ if hasattr(lens, k)})
    args = (ins["image"].cuda(), ins["text"].cuda(), ins["visual_x"].cuda())
    return sd, args, outs, grads, (tc, xc, lc)


def _step(tiny, **kw):
    from vitlens_hip import step as ST
    sd, _, _, _, cfgs = tiny
    return ST.TriModalAudioStep(sd, *cfgs, "cuda", **{"micro_batch": 4, "lr": 1e-3, **kw})


def test_interface(tiny):
    import inspect
    from vitlens_hip import step as ST
    dual = set(inspect.signature(ST.DualAudioStep.__init__).parameters)
    tri = set(inspect.signature(ST.TriModalAudioStep.__init__).parameters)
    assert tri == dual - {"contra_loss_type", "sim_thres"}
    assert list(inspect.signature(ST.TriModalAudioStep.forward_backward).parameters) == ["self", "images", "texts", "audio"]
    st = _step(tiny)
    assert "visual.class_embedding" in st.masters and not any(k.startswith(("image.", "transformer.")) for k in st.masters)


def test_loss_and_gradients_vs_the_reference(tiny):
    sd, args, outs, grads, _ = tiny
    st = _step(tiny)
    loss = st.forward_backward(*args)
    print(f"loss {float(loss):.5f}, reference {float(outs['step_loss']):.5f}")
    assert abs(float(loss) - float(outs["step_loss"])) < 3e-2, (float(loss), float(outs["step_loss"]))
    got = dict(st.grads)
    got.update(st.reference_named_grads())
    perceiver = [k for k in grads if k.startswith("visual.perceiver.")]
    errs = {}
    for name in perceiver + ["visual.visual_adapter.conv1.weight", "visual.visual_adapter.pos_emb", "visual.class_embedding", "logit_scale"]:
        ref = grads[name]
        if name.endswith("conv1.weight"):                 # the step keeps the convolution as a (column-padded) GEMM operand
            g = got[name + "_gemm"]
            ref = ref.reshape(g.shape[0], -1)
            assert g.shape[1] == ref.shape[1] or float(g[:, ref.shape[1]:].abs().max()) == 0.0
            g = g[:, :ref.shape[1]]
        else:
            g = got[name]
            ref = ref.reshape(g.shape)
        errs[name] = relerr(g, ref)
    worst = max(errs, key=errs.get)
    print(f"{len(errs)} gradients compared, worst {worst}: {errs[worst]:.4f}")
    assert len(errs) >= len(perceiver) + 3 and len(perceiver) >= 40
    bad = {k: round(v, 4) for k, v in errs.items() if not v < 8e-2}
    assert not bad, bad
    # frozen towers have no gradient buffers
    assert not any(k.startswith(("image.", "transformer.", "visual.transformer.")) for k in st.grads)


def test_micro_batches_overlap_and_descent(tiny):
    _, args, _, _, _ = tiny
    l4 = float(_step(tiny).forward_backward(*args))
    l2 = float(_step(tiny, micro_batch=2).forward_backward(*args))
    assert abs(l4 - l2) < 1e-3, (l4, l2)
    runs = {}
    for overlap in (True, False):
        st = _step(tiny, micro_batch=2, overlap_frozen=overlap)
        losses = [st.step(*args) for _ in range(3)]
        torch.cuda.synchronize()
        runs[overlap] = (torch.stack(losses).cpu(), {k: v.clone().cpu() for k, v in st.masters.items()})
    assert torch.equal(runs[True][0], runs[False][0]), (runs[True][0], runs[False][0])
    for k, v in runs[True][1].items():
        assert torch.equal(v, runs[False][1][k]), k
    losses = runs[True][0].tolist()
    print("losses over 3 steps:", losses)
    assert all(torch.isfinite(runs[True][0])) and losses[2] < losses[0], losses
