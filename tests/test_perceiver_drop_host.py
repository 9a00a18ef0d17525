"""CPU: Perceiver dropout (--perceiver_attn_dropout / --perceiver_ff_dropout) without a GPU - the mask rule restated in numpy
(tests/perceiver_drop_ref.py) and its properties, the fp64 restatement of the arithmetic against the reference's own Perceiver
under supplied masks, the launch plans with and without a draw (launch_trace.py), and the plumbing from the model arguments
down to LensCfg and the fused steps' host state."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import perceiver_drop_ref as R
from launch_trace import recording, symbols
from philox_ref import philox4x32_10
from test_perceiver_plan_host import (B, CROSS, CROSS_BWD, DEPTH, FF, FF_BWD, SELF, SELF_BWD, SELFS, TC, C, D, N_LAT, lens_cfg,
                                      perceiver_sd, plan)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vit-lens_amd", "csrc")


# ------------------------------------------------------------------------------------------------ 1. the mask
def _word(seed, sample, sub, group, word):
    w = philox4x32_10(np.array([group]), np.array([sample & 0xFFFFFFFF]), np.array([sample >> 32]), np.array([sub]),
                      seed & 0xFFFFFFFF, seed >> 32)
    return int(w[word][0])


def test_masks_follow_the_documented_counter_layout():
    seed, s0, sub, p = (7 << 32) | 11, R.sample0(5, 3, 9), 4, 0.3
    Bn, H, Lq, Lk = 2, 3, 5, 10                        # ceil(10 / 4) = 3 groups per (head, query), the last one ragged
    m = R.attn_keep(seed, s0, sub, p, Bn, H, Lq, Lk)
    thr = R.threshold(p)
    assert thr == round(0.3 * 2 ** 32)
    for b, h, i, j in [(0, 0, 0, 0), (1, 2, 4, 9), (0, 1, 3, 6), (1, 0, 2, 3)]:
        assert m[b, h, i, j] == (_word(seed, s0 + b, sub, (h * Lq + i) * 3 + j // 4, j % 4) >= thr)
    n, Dd = 6, 12
    f = R.ff_keep(seed, s0, sub, p, Bn, n, Dd)
    for b, i, c in [(0, 0, 0), (1, 5, 11), (0, 3, 6)]:
        assert f[b * n + i, c] == (_word(seed, s0 + b, sub, i * (Dd // 4) + c // 4, c % 4) >= thr)
    # the per-sample number: step.drop_sample0 with the Lens's tower id, which patch dropout's two towers do not use
    from vitlens_hip import step as ST
    assert ST.DROP_TOWER_LENS == R.DROP_TOWER_LENS == 2 and ST.DROP_TOWER_LENS not in (ST.DROP_TOWER_VISUAL, ST.DROP_TOWER_IMAGE)
    assert ST.drop_sample0(5, 3, ST.DROP_TOWER_LENS, 9) == s0
    # the scale is an fp32 quotient
    assert R.scale32(0.1) == np.float32(1.0) / np.float32(0.9) and R.scale32(0.1).dtype == np.float32
    # the sub-layer id is the position in the forward: attention and FeedForward alternate, nothing repeats
    from vitlens_hip import engine as E
    c = lens_cfg(True)
    ids = []
    for li in range(c.depth):
        ids += [E.lens_sublayer(c, li), E.lens_sublayer(c, li, ff=True)]
        for sj in range(c.self_per_cross):
            ids += [E.lens_sublayer(c, li, sj), E.lens_sublayer(c, li, sj, ff=True)]
    assert ids == list(range(E.perceiver_residuals(c) - 1))
    assert [R.sublayer(c.self_per_cross, 1, 0, True), R.sublayer(c.self_per_cross, 1)] == [E.lens_sublayer(c, 1, 0, True), E.lens_sublayer(c, 1)]


def test_distinct_numbers_give_distinct_masks_and_equal_numbers_equal_masks():
    seed, p, shape = 99, 0.5, (1, 2, 16, 24)
    base = dict(step=4, rank=1, offset=0, sub=2)

    def mask(seed=seed, **kw):
        a = dict(base, **kw)
        return R.attn_keep(seed, R.sample0(a["step"], a["rank"], a["offset"]), a["sub"], p, *shape)
    m0 = mask()
    assert np.array_equal(m0, mask())
    for other in (mask(step=5), mask(rank=2), mask(offset=1), mask(sub=3), mask(seed=seed + 1), mask(seed=seed + (1 << 32))):
        assert not np.array_equal(m0, other)
    assert not np.array_equal(m0[0, 0], m0[0, 1])                       # heads
    # samples: row 1 of a batch that starts at offset 0 IS row 0 of a batch that starts at offset 1 (micro-batch independence)
    two = R.attn_keep(seed, R.sample0(4, 1, 0), 2, p, 2, *shape[1:])
    assert not np.array_equal(two[0], two[1]) and np.array_equal(two[1], mask(offset=1)[0])
    # an attention and a FeedForward never share a draw even at equal group numbers: the sub-layer word differs
    f0 = R.ff_keep(seed, R.sample0(4, 1, 0), 2, p, 1, 16, 24)
    f1 = R.ff_keep(seed, R.sample0(4, 1, 0), 3, p, 1, 16, 24)
    assert not np.array_equal(f0, f1)


@pytest.mark.parametrize("name", list(R.ATTN_CASES) + list(R.FF_CASES) + ["tiny"])
def test_kept_fraction_of_every_gpu_shape_is_within_4_sigma(name):
    if name in R.ATTN_CASES:
        Bn, H, Lq, Lk, _, p, seed = R.ATTN_CASES[name]
        m = R.attn_keep(seed, R.ATTN_SAMPLE0, R.ATTN_SUB, p, Bn, H, Lq, Lk)
    elif name in R.FF_CASES:
        Bn, n, Dd, p, seed = R.FF_CASES[name]
        m = R.ff_keep(seed, R.ATTN_SAMPLE0, R.ATTN_SUB + 1, p, Bn, n, Dd)
    else:                                                   # every mask of the tiny Perceiver's forward, together
        from types import SimpleNamespace
        p = 0.1
        lens = SimpleNamespace(depth=2, self_per_cross=2, num_latents=16, latent_dim=64, cross_heads=1, latent_heads=2)
        m = np.concatenate([k.reshape(-1) for k in R.perceiver_masks(R.TINY_SEED, R.sample0(0, 0, 0), p, p, 4, 40, lens)])
    sigma = np.sqrt(p * (1 - p) / m.size)
    z = (m.mean() - (1 - p)) / sigma
    print(f"{name}: kept {m.mean():.5f} of {m.size}, {z:+.2f} sigma")
    assert abs(z) < 4.0


# ------------------------------------------------------------------------------------------------ 2. against the reference
def _reference_perceiver_module():
    import ref_loader
    if not ref_loader.available():
        pytest.skip("reference tree not present")
    ref_loader.load()
    import importlib
    return importlib.import_module("open_clip.perceiver")


class _SuppliedMasks:
    """torch.nn.functional.dropout for the test: applies the supplied masks in call order, M * x / (1 - p) with the fp32 scale."""

    def __init__(self, masks):
        self.masks, self.calls = list(masks), 0

    def __call__(self, x, p=0.5, training=True, inplace=False):
        assert training
        m = self.masks[self.calls]
        self.calls += 1
        return x * torch.as_tensor(np.asarray(m).reshape(x.shape), dtype=x.dtype) * float(R.scale32(p))


def test_restatement_equals_the_reference_perceiver_under_supplied_masks(monkeypatch):
    P = _reference_perceiver_module()
    assert not P.USE_XOPS, "the einsum branch is the one with an nn.Dropout on the probabilities"
    from types import SimpleNamespace
    torch.manual_seed(0)
    pa, pf, Bn, Tc = 0.25, 0.4, 2, 10
    lens = SimpleNamespace(depth=2, self_per_cross=2, num_latents=6, latent_dim=16, input_chan=12, cross_heads=1,
                           cross_dim_head=8, latent_heads=2, latent_dim_head=8)
    mod = P.Perceiver(num_freq_bands=2, depth=lens.depth, max_freq=10.0, input_channels=lens.input_chan, input_axis=1,
                      num_latents=lens.num_latents, latent_dim=lens.latent_dim, cross_heads=1, latent_heads=2, cross_dim_head=8,
                      latent_dim_head=8, attn_dropout=pa, ff_dropout=pf, fourier_encode_data=False,
                      self_per_cross_attn=lens.self_per_cross, final_classifier_head=False).double().train()
    data = torch.randn(Bn, Tc, lens.input_chan, dtype=torch.float64)
    masks = R.perceiver_masks(17, R.sample0(2, 0, 4), pa, pf, Bn, Tc, lens)
    # the reference flattens (b h) for its attention and keeps [b, n, d] for its FeedForward: same elements, reshaped
    supplied = _SuppliedMasks(masks)
    monkeypatch.setattr(torch.nn.functional, "dropout", supplied)
    want = mod(data, return_embeddings=True)
    assert supplied.calls == len(masks) == lens.depth * (2 + 2 * lens.self_per_cross)
    sd = {k: v.detach() for k, v in mod.state_dict().items()}
    got = R.perceiver(sd, "", data, lens, masks, pa, pf)
    assert float((got - want).detach().abs().max()) < 1e-12 * float(want.detach().abs().max())
    # ... and it is the masks that were compared: without them the result differs, eval mode never drops
    assert float((R.perceiver(sd, "", data, lens) - want).detach().abs().max()) > 1e-3
    monkeypatch.undo()
    assert float((R.perceiver(sd, "", data, lens) - mod.eval()(data, return_embeddings=True)).abs().max()) < 1e-12


def test_one_attention_and_one_feed_forward_equal_the_reference_modules(monkeypatch):
    P = _reference_perceiver_module()
    torch.manual_seed(1)
    p, Bn, H, n, m, dh, Dq = 0.3, 2, 2, 5, 7, 4, 12
    att = P.Attention(Dq, Dq, heads=H, dim_head=dh, dropout=p).double().train()
    x, ctx = torch.randn(Bn, n, Dq, dtype=torch.float64), torch.randn(Bn, m, Dq, dtype=torch.float64)
    keep = R.attn_keep(3, R.sample0(0, 0, 0), 0, p, Bn, H, n, m)
    monkeypatch.setattr(torch.nn.functional, "dropout", _SuppliedMasks([keep]))
    want = att(x, context=ctx)
    hf = lambda t, L: t.reshape(Bn, L, H, dh).permute(0, 2, 1, 3)
    kk, vv = att.to_kv(ctx).chunk(2, dim=-1)
    o, lse = R.attention(hf(att.to_q(x), n), hf(kk, m), hf(vv, m), dh ** -0.5, keep, p)
    got = att.to_out(o.permute(0, 2, 1, 3).reshape(Bn, n, H * dh))
    assert float((got - want).abs().max()) < 1e-12
    assert torch.equal(lse, R.attention(hf(att.to_q(x), n), hf(kk, m), hf(vv, m), dh ** -0.5)[1])       # lse ignores the mask
    ffm = P.FeedForward(Dq, dropout=p).double().train()
    fk = R.ff_keep(3, R.sample0(0, 0, 0), 1, p, Bn, n, Dq)
    monkeypatch.setattr(torch.nn.functional, "dropout", _SuppliedMasks([fk]))
    want = ffm(x) + x                                                   # (the residual is added outside, undropped)
    y = ffm.net[2](ffm.net[1](ffm.net[0](x)))                           # second Linear's output, bias included
    got = R.feed_forward(x, y, fk.reshape(Bn, n, Dq), p)
    assert float((got - want).abs().max()) < 1e-12


# ------------------------------------------------------------------------------------------------ 3. launch plans
ATTN_DROP, ATTN_BWD_DROP, FF_DROP, FF_DROP_BWD = "vl_attn_fwd_drop_bf16", "vl_attn_bwd_drop_bf16", "vl_ff_drop_fwd", "vl_ff_drop_bwd"


def _sub(unit, old, new):
    assert unit.count(old) == 1
    return [new if s == old else s for s in unit]


# the p = 0 units of test_perceiver_plan_host.py with exactly these substitutions and additions
CROSS_D = _sub(CROSS, "vl_attn_fwd_bf16", ATTN_DROP)
SELF_D = _sub(SELF, "vl_attn_fwd_bf16", ATTN_DROP)
FF_D = FF + [FF_DROP]                                                      # the down-projection without residual, then the row kernel
CROSS_BWD_D = _sub(CROSS_BWD, "vl_attn_bwd_bf16", ATTN_BWD_DROP)
SELF_BWD_D = _sub(SELF_BWD, "vl_attn_bwd_fused_bf16", ATTN_BWD_DROP)       # the two-kernel backward also for Lq = Lk
FF_BWD_D = [FF_DROP_BWD] + FF_BWD                                          # the masked bf16 copy first


def _bwd_plan(ff, self_, cross):
    return ["vl_cast_f32_bf16"] + ((ff + self_) * SELFS + ff + cross) * DEPTH + ["vl_batch_rowsum"]


def _executors(tied, pa, pf):
    from dataclasses import replace
    from vitlens_hip import engine as E, train as T
    c = replace(lens_cfg(tied), attn_dropout=pa, ff_dropout=pf)
    pe = E.PerceiverEngine(perceiver_sd(c), "p.", c, "cpu")
    return c, pe, T.PerceiverTrainer(pe, "p.")


def _record(pe, pt, drop):
    data = torch.zeros(B * TC, C, dtype=torch.bfloat16)
    with recording() as eng:
        pe.forward(data, B, drop)
    with recording() as fwd:
        lat = pt.forward(data, B, drop)
    with recording() as bwd:
        pt.backward(torch.zeros_like(lat))
    return eng, fwd, bwd


@pytest.mark.parametrize("tied", [False, True], ids=["untied", "tied"])
def test_plans_with_dropout_are_the_p0_plans_with_the_written_substitutions(tied):
    from vitlens_hip import engine as E, ops
    c, pe, pt = _executors(tied, 0.1, 0.2)
    drop = pe.draw(seed=(5 << 32) | 9, sample0=R.sample0(3, 1, 8))
    assert drop == E.LensDrop((5 << 32) | 9, R.sample0(3, 1, 8), 0.1, 0.2)
    eng, fwd, bwd = _record(pe, pt, drop)
    assert symbols(eng) == symbols(fwd) == plan(CROSS_D, FF_D, SELF_D)
    assert symbols(bwd) == _bwd_plan(FF_BWD_D, SELF_BWD_D, CROSS_BWD_D)
    nsub = DEPTH * (2 + 2 * SELFS)
    # the draw's numbers reach every launch; the sub-layer ids are the positions in the forward, and the backward redraws
    # every sub-layer with the id the forward used
    fa = [a for n, a in fwd if n == ATTN_DROP]
    ff = [a for n, a in fwd if n == FF_DROP]
    assert [a[-2] for a in fa] == list(range(0, nsub, 2)) and [a[-2] for a in ff] == list(range(1, nsub, 2))
    assert all(a[-5:-2] == (0.1, drop.seed, drop.sample0) for a in fa) and all(a[-5:-2] == (0.2, drop.seed, drop.sample0) for a in ff)
    assert all(a[3:6] == (B, N_LAT, D) for a in ff)
    ba = [a for n, a in bwd if n == ATTN_BWD_DROP]
    bf = [a for n, a in bwd if n == FF_DROP_BWD]
    assert [a[-2] for a in ba] == list(range(0, nsub, 2))[::-1] and [a[-2] for a in bf] == list(range(1, nsub, 2))[::-1]
    assert all(a[-5:-2] == (0.1, drop.seed, drop.sample0) for a in ba) and all(a[-5:-2] == (0.2, drop.seed, drop.sample0) for a in bf)
    # the down-projection in front of the row kernel: fp32 output, no residual operand
    for i, (n, a) in enumerate(fwd):
        if n == FF_DROP:
            g = fwd[i - 1][1]
            assert fwd[i - 1][0] == "vl_gemm_bf16_ex" and g[13] == ops.EPI_F32 and g[4] is None
            assert g[3].base == a[0].base                      # its output is the row kernel's y


@pytest.mark.parametrize("pa,pf", [(0.1, 0.0), (0.0, 0.2)])
def test_each_probability_switches_only_its_own_kernels(pa, pf):
    c, pe, pt = _executors(False, pa, pf)
    eng, fwd, bwd = _record(pe, pt, pe.draw(1, 2))
    assert symbols(eng) == symbols(fwd) == plan(CROSS_D if pa else CROSS, FF_D if pf else FF, SELF_D if pa else SELF)
    assert symbols(bwd) == _bwd_plan(FF_BWD_D if pf else FF_BWD, SELF_BWD_D if pa else SELF_BWD, CROSS_BWD_D if pa else CROSS_BWD)


@pytest.mark.parametrize("pa,pf", [(0.0, 0.0), (0.1, 0.2)])
def test_without_a_draw_the_trace_is_todays_plan(pa, pf):
    """No draw - eval mode, or a configuration that drops nothing, whose `draw` is None - is today's plan symbol for symbol."""
    c, pe, pt = _executors(False, pa, pf)
    if pa == 0.0:
        assert pe.draw(1, 2) is None
    eng, fwd, bwd = _record(pe, pt, None)
    assert symbols(eng) == symbols(fwd) == plan(CROSS, FF, SELF)
    assert symbols(bwd) == _bwd_plan(FF_BWD, SELF_BWD, CROSS_BWD)


def test_fp32_engine_never_drops():
    from dataclasses import replace
    from vitlens_hip import engine as E, f32 as F
    c = replace(lens_cfg(False), attn_dropout=0.1, ff_dropout=0.1)
    pf = F.PerceiverEngineF32(perceiver_sd(c), "p.", c, "cpu")
    data = torch.zeros(B * TC, C)
    with recording() as tr:
        pf.forward(data, B)
    assert not [s for s in symbols(tr) if "drop" in s]
    X, slots = E.perceiver_slots(c, B, TC, "cpu", torch.float32)
    with pytest.raises(ValueError), recording():
        E.perceiver_forward(pf.layers, slots, data, B, c, pf.arith, E.LensDrop(1, 2, 0.1, 0.1))


# ------------------------------------------------------------------------------------------------ 4. plumbing
def _product_packages():
    """The reference's packages of the same names (loaded by the tests above, or by another test file) out of the way."""
    import sys
    import ref_loader
    while ref_loader.REF_SRC in sys.path:
        sys.path.remove(ref_loader.REF_SRC)
    for k in [k for k in sys.modules if k.split(".")[0] in ("open_clip", "training", "mm_vit_lens")]:
        if "vit-lens_amd" not in (getattr(sys.modules[k], "__file__", "") or ""):
            del sys.modules[k]


def _tiny_model(**over):
    import importlib
    import json
    import tempfile
    from types import SimpleNamespace
    from golden_util import load_npz, split
    _product_packages()
    oc = importlib.import_module("open_clip")
    meta = split(load_npz("tiny_audio.npz"))[4]
    args = dict(meta["args"])
    for k, v in over.items():
        if v is None:
            args.pop(k, None)
        else:
            args[k] = v
    with tempfile.TemporaryDirectory() as td:
        json.dump(meta["model_cfg"], open(os.path.join(td, "tiny-lens.json"), "w"))
        oc.add_model_config(td)
        return oc.tri_create_model("tiny-lens", None, device="cpu", args=SimpleNamespace(**args))


def test_model_arguments_reach_lens_cfg():
    m = _tiny_model(perceiver_attn_dropout=0.1, perceiver_ff_dropout=0.25)
    lens = m.visual._cfgs()[1]
    assert (lens.attn_dropout, lens.ff_dropout) == (0.1, 0.25)
    assert (m.visual.drop_seed, m.visual._drop_forwards) == (0, 0)
    # train / eval switch it; every train-mode forward draws anew; re-seeding and resetting the count repeats the sequence
    m.eval()
    assert m.visual._lens_draw() is None
    m.train()
    a, b = m.visual._lens_draw(), m.visual._lens_draw()
    assert (a.pa, a.pf, a.seed) == (0.1, 0.25, 0) and a.sample0 == R.sample0(0, 0, 0) and b.sample0 == R.sample0(1, 0, 0)
    m.visual.set_drop_seed(77)
    assert m.visual._lens_draw() == type(a)(77, R.sample0(0, 0, 0), 0.1, 0.25)
    # defaults, also for arguments that do not carry the keys at all
    for mm in (_tiny_model(), _tiny_model(perceiver_attn_dropout=None, perceiver_ff_dropout=None)):
        lens = mm.visual._cfgs()[1]
        assert (lens.attn_dropout, lens.ff_dropout) == (0.0, 0.0) and mm.train().visual._lens_draw() is None
    # the drivers' way in: from their args, after construction
    from training.train import _lens_dropout_from_args
    from types import SimpleNamespace
    mm = _tiny_model()
    _lens_dropout_from_args(mm.visual, SimpleNamespace(perceiver_attn_dropout=0.2, perceiver_ff_dropout=0.0))
    assert mm.visual._cfgs()[1].attn_dropout == 0.2 and mm.visual._cfgs()[1].ff_dropout == 0.0
    _lens_dropout_from_args(mm.visual, SimpleNamespace())
    assert mm.visual._cfgs()[1].attn_dropout == 0.2


def test_drivers_never_change_what_the_model_was_built_with():
    """training.train._lens_dropout_from_args: the model's own values win; a missing key, None or a parser's 0.0 switches nothing
    off and rebuilds nothing; a positive value fills in a probability the model has at 0.0; two positive values that differ are
    refused."""
    from types import SimpleNamespace
    m = _tiny_model(perceiver_attn_dropout=0.1, perceiver_ff_dropout=0.25)
    _product_packages()
    from training.train import _lens_dropout_from_args
    v = m.visual
    v._engine = marker = object()
    for args in (SimpleNamespace(), SimpleNamespace(perceiver_attn_dropout=0.0, perceiver_ff_dropout=0.0),
                 SimpleNamespace(perceiver_attn_dropout=None, perceiver_ff_dropout=None),
                 SimpleNamespace(perceiver_attn_dropout=0.1, perceiver_ff_dropout=0.25)):
        _lens_dropout_from_args(v, args)
        assert (v.perceiver_attn_dropout, v.perceiver_ff_dropout) == (0.1, 0.25) and v._engine is marker
    with pytest.raises(ValueError, match="perceiver_attn_dropout"):
        _lens_dropout_from_args(v, SimpleNamespace(perceiver_attn_dropout=0.3))
    assert v.perceiver_attn_dropout == 0.1 and v._engine is marker
    v._engine = None
    m0 = _tiny_model()
    m0.visual._engine = marker
    _lens_dropout_from_args(m0.visual, SimpleNamespace(perceiver_ff_dropout=0.2))
    assert (m0.visual.perceiver_attn_dropout, m0.visual.perceiver_ff_dropout) == (0.0, 0.2) and m0.visual._engine is None


@pytest.mark.parametrize("modality", ["image", "tactile"])
def test_a_tower_whose_executors_run_no_lens_refuses_the_dropout(modality):
    """An image / tactile tower with a (non-identity) Perceiver runs VitEngine / ImageTowerTrainer, which have no Lens: a positive
    probability is refused where the tower is built or set, never run without dropout."""
    m = _tiny_model(visual_modality_type=modality)
    assert m.visual.use_perceiver and not m.visual.perceiver_identity and m.train().visual._lens_draw() is None
    for key in ("perceiver_attn_dropout", "perceiver_ff_dropout"):
        with pytest.raises(NotImplementedError, match="run no Lens"):
            _tiny_model(visual_modality_type=modality, **{key: 0.1})
    with pytest.raises(NotImplementedError, match="run no Lens"):
        m.visual.set_perceiver_dropout(0.1, None)


def test_a_library_without_a_bound_symbol_is_named_as_stale(monkeypatch):
    """Entries can be added under one VL_ABI_VERSION: a library built before them reports the binding's number and lacks them.
    load_library says so and says what to do, instead of a bare AttributeError."""
    from vitlens_hip import _lib
    if not os.path.exists(_lib.lib_path()):
        import __graft_entry__ as g
        g.build()
    monkeypatch.setattr(_lib, "_LIB", None)
    monkeypatch.setitem(_lib.SIGNATURES, "vl_entry_of_a_newer_binding", [])
    with pytest.raises(RuntimeError, match=r"does not export vl_entry_of_a_newer_binding.*older sources.*rebuild the library"):
        _lib.load_library()
    monkeypatch.undo()
    assert _lib.load_library() is not None


@pytest.mark.parametrize("bad", [1.0, -0.1])
def test_values_outside_0_1_are_refused(bad):
    from dataclasses import replace
    from vitlens_hip import engine as E, step as ST
    for key in ("perceiver_attn_dropout", "perceiver_ff_dropout"):
        with pytest.raises(ValueError, match=key):
            _tiny_model(**{key: bad})
        with pytest.raises(ValueError, match=key):
            ST._StepState()._init_host({"logit_scale": torch.zeros(())}, "cpu", 2, 0, 1, **{key: bad})
    for field in ("attn_dropout", "ff_dropout"):
        c = replace(lens_cfg(False), **{field: bad})
        with pytest.raises(ValueError, match="perceiver_" + field):
            E.PerceiverEngine(perceiver_sd(c), "p.", c, "cpu")


def test_step_host_state_and_defaults():
    from vitlens_hip import step as ST
    st = ST._StepState()
    st._init_host({"logit_scale": torch.zeros(())}, "cpu", 2, 0, 1)
    assert (st.perceiver_attn_dropout, st.perceiver_ff_dropout, st._lens_drop) == (0.0, 0.0, False)
    st._init_host({"logit_scale": torch.zeros(())}, "cpu", 2, 3, 4, drop_seed=9, perceiver_attn_dropout=0.1)
    assert (st.perceiver_attn_dropout, st.perceiver_ff_dropout, st.drop_seed) == (0.1, 0.0, 9)
    c = st._lens_cfg(lens_cfg(False))
    assert (c.attn_dropout, c.ff_dropout) == (0.1, 0.0)
    import inspect
    for cls in (ST.DualAudioStep, ST.TriModalPCStep):
        sig = inspect.signature(cls.__init__).parameters
        assert sig["perceiver_attn_dropout"].default == 0.0 and sig["perceiver_ff_dropout"].default == 0.0


def test_vl_lens_drop_kernels_no_scratch_no_spills(tmp_path):
    """The recipe of test_f32_wide_heads_host.py on csrc/vl_lens_drop.hip (forward, FeedForward rows) and on the dropout
    instantiations of csrc/vl_attn_bwd.hip's two kernels (template arguments ..., TAIL = false, DROP = true), with the flags
    csrc/Makefile gives both files."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    bad, vgprs = [], {}
    for src in ("vl_lens_drop.hip", "vl_attn_bwd.hip"):
        r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fno-honor-nans", "-I" + CSRC,
                            "-I" + os.path.join(ROOT, "include"), "-x", "hip", "-c", os.path.join(CSRC, src), "-o",
                            str(tmp_path / "o.o"), "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True,
                           timeout=900)
        assert r.returncode == 0, r.stderr[-3000:]
        name = None
        for line in r.stderr.splitlines():
            m = re.search(r"Function Name: (\S+)", line)
            if m:
                name = m.group(1)
            if name and src == "vl_attn_bwd.hip" and not re.search(r"_kernelILi\d+ELi\d+ELb0ELb1E", name):
                continue                                     # a p = 0 instantiation: tests/test_kernel_resources.py
            m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
            if m and int(m.group(1)) > 0:
                bad.append((name, "scratch", int(m.group(1))))
            m = re.search(r"([SV]GPRs) Spill: (\d+)", line)
            if m and int(m.group(2)) > 0:
                bad.append((name, m.group(1) + " spill", int(m.group(2))))
            m = re.search(r" VGPRs: (\d+)", line)
            if m and name:
                vgprs[name] = int(m.group(1))
    for n, v in sorted(vgprs.items()):
        print(f"{n}: {v} VGPRs")
    # head dims 32 / 64 / padded 128 of the forward and of both backward kernels, and the two row kernels
    assert len([n for n in vgprs if "attn_fwd_drop_kernel" in n]) == 3
    for kern, inst in (("attn_bwd_dq_kernel", [(32, 160), (64, 160), (128, 160)]), ("attn_bwd_dkv_kernel", [(32, 288), (64, 288), (128, 96)])):
        got = [re.search(kern + r"ILi(\d+)ELi(\d+)ELb0ELb1E", n).groups() for n in vgprs if kern in n]
        assert sorted((int(dh), int(nc)) for dh, nc in got) == sorted(inst), sorted(vgprs)
    assert len([n for n in vgprs if "ff_drop_kernel" in n]) == 2
    assert len(vgprs) == 11
    assert not bad, bad
