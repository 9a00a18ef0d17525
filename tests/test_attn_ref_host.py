"""The attention forward's float64 reference, rounding model and score generators (tests/attn_ref.py) on the CPU: the reference
against torch's own attention, the model's distance from the reference pinned (it is the yardstick of every tolerance in
test_hip_attn_fwd.py), localized mutations that today's whole-tensor bound passes and the per-block check names, the straddle
generator's exact steps, and the coverage of the kernel's instantiations by the GPU cases."""
import math

import pytest
import torch
import torch.nn.functional as F

import attn_ref as A
import errloc
import test_hip_attn_fwd as G

BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32

# (name, Lq, Lk, dh, causal) with B = 2, H = 3: the geometries the GPU cases run every score kind on, one query against 257
# keys and the text tower's causal 77
GRID = (("L257", 257, 257, 64, False), ("L257c", 257, 257, 64, True), ("64x600", 64, 600, 64, False),
        ("257x600", 257, 600, 64, False), ("dh32", 257, 257, 32, False), ("dh104", 257, 257, 104, False),
        ("1x257", 1, 257, 64, False), ("L77c", 77, 77, 64, True))
# worst (b, h, 32-query tile) block of attn_fwd_model against attn_fwd_ref, per GRID entry, measured here with
# errloc.attn_block_relerr; asserted within [0.5, 1.25] x.  (One query of ramp / descend is one-hot: no rounding at all.)
ONE_HOT = 1e-6
PIN_BLK = {
    BF16: {"normal": (2.30e-03, 2.31e-03, 2.32e-03, 2.52e-03, 2.73e-03, 2.28e-03, 2.81e-03, 2.17e-03),
           "ramp": (1.92e-03, 1.92e-03, 1.14e-03, 1.91e-03, 1.73e-03, 1.92e-03, 0.0, 1.45e-03),
           "descend": (1.87e-03, 1.87e-03, 1.20e-03, 1.95e-03, 1.66e-03, 2.24e-03, 0.0, 1.21e-03),
           "negative": (1.80e-03, 1.99e-03, 2.18e-03, 1.92e-03, 2.13e-03, 2.13e-03, 2.09e-03, 2.10e-03),
           "sink_first": (1.99e-03, 2.10e-03, 1.91e-03, 1.66e-03, 2.02e-03, 1.83e-03, 1.88e-03, 1.91e-03),
           "sink_last": (1.99e-03, 1.99e-03, 1.91e-03, 1.66e-03, 2.02e-03, 1.83e-03, 1.88e-03, 5.08e-04),
           "straddle": (1.89e-03, 2.15e-03, 2.21e-03, 2.63e-03, 1.91e-03, 1.84e-03, 1.77e-03, 2.11e-03)},
    F16: {"normal": (2.87e-04, 2.87e-04, 2.90e-04, 3.15e-04, 3.40e-04, 3.06e-04, 3.36e-04, 2.81e-04),
          "ramp": (2.26e-04, 2.26e-04, 1.55e-04, 2.51e-04, 2.18e-04, 2.33e-04, 0.0, 1.91e-04),
          "descend": (2.36e-04, 2.36e-04, 1.66e-04, 2.09e-04, 2.28e-04, 2.85e-04, 0.0, 1.57e-04),
          "negative": (2.76e-04, 2.96e-04, 2.82e-04, 2.51e-04, 2.39e-04, 2.69e-04, 2.83e-04, 2.53e-04),
          "sink_first": (2.29e-04, 2.34e-04, 2.28e-04, 2.28e-04, 2.83e-04, 2.15e-04, 2.39e-04, 2.21e-04),
          "sink_last": (2.29e-04, 2.24e-04, 2.28e-04, 2.28e-04, 2.84e-04, 2.13e-04, 2.39e-04, 6.22e-05),
          "straddle": (2.34e-04, 2.71e-04, 2.82e-04, 3.02e-04, 2.29e-04, 2.26e-04, 2.28e-04, 2.53e-04)},
}
EXACT_LSE = 1e-7          # model lse below this: the 16-bit products are exact in float32 (only the ulp floor applies on the GPU)


def _within(got, pinned):
    return 0.5 * pinned <= got <= 1.25 * pinned


def _model_vs_ref(kind, dtype, Lq, Lk, dh, causal, B=2, H=3, seed=5):
    q, k, v, qs = A.make_scores(kind, B, H, Lq, Lk, dh, seed=seed, dtype=dtype)
    log2 = dtype != F32
    if not log2 and kind == "normal":
        qs /= A.LOG2E
    ro, rl = A.attn_fwd_ref(q, k, v, qs, causal, dtype, log2)
    mo, ml = A.attn_fwd_model(q, k, v, qs, causal, dtype, log2)
    blk, where = errloc.attn_block_relerr(mo, ro, B, H, Lq)
    return blk, float((ml - rl).abs().max()), ro


def _min_block_share(ref):
    """Smallest (block energy) / (the block's fair share of the tensor's energy) over the (b, h, 32-row tile) blocks."""
    B, H, L, dh = ref.shape
    edges = list(range(0, L, 32)) + [L]
    r2 = torch.stack([ref[:, :, a:b].pow(2).sum((-1, -2)) / (b - a) for a, b in zip(edges[:-1], edges[1:])], -1)
    return float(r2.min() / (ref.pow(2).sum() / (B * H * L)))


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("B,H,Lq,Lk,dh", [(2, 3, 5, 5, 8), (1, 2, 40, 40, 16), (2, 2, 33, 70, 8), (2, 1, 70, 33, 16),
                                          (1, 2, 9, 1, 8), (3, 2, 1, 1, 8)])
def test_reference_is_torch_attention_in_float64(B, H, Lq, Lk, dh, causal):
    g = torch.Generator().manual_seed(Lq * 100 + Lk)
    q, k, v = (torch.randn(B, H, L, dh, generator=g).bfloat16() for L in (Lq, Lk, Lk))
    qscale = dh ** -0.5 * A.LOG2E
    out, lse = A.attn_fwd_ref(q, k, v, qscale, causal, BF16)
    qe = A.q_rounded(q, qscale, BF16).double() / A.LOG2E
    mask = torch.ones(Lq, Lk, dtype=torch.bool).tril() if causal else None         # top-left aligned: key <= query
    want = F.scaled_dot_product_attention(qe, k.double(), v.double(), attn_mask=mask, scale=1.0)
    s = qe @ k.double().transpose(-1, -2)
    if causal:
        s = s.masked_fill(~mask, float("-inf"))
    assert float((out - want).abs().max()) < 1e-12
    assert float((lse - torch.logsumexp(s, -1)).abs().max()) < 1e-12
    # natural-log scores (the f32 entry) and the batch chunking
    out_n, lse_n = A.attn_fwd_ref(q.float(), k.float(), v.float(), dh ** -0.5, causal, F32, log2=False)
    s = _scores64(q, k, dh ** -0.5, causal)
    assert float((out_n - torch.softmax(s, -1) @ v.double()).abs().max()) < 1e-12
    assert float((lse_n - torch.logsumexp(s, -1)).abs().max()) < 1e-12
    assert A._batch_chunk(256, 16, 257, 257) * 16 * 257 * 257 * 8 <= 1 << 28 and A._batch_chunk(2, 1, 1 << 20, 1 << 20) == 1


def _scores64(q, k, scale, causal):
    s = (q.float() * scale).double() @ k.double().transpose(-1, -2)
    return A._mask(s, causal)


@pytest.mark.parametrize("dtype", [BF16, F16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("kind", A.KINDS)
def test_model_block_error_is_what_the_gpu_tolerances_assume(kind, dtype):
    worst_lse = 0.0
    for (name, Lq, Lk, dh, causal), pinned in zip(GRID, PIN_BLK[dtype][kind]):
        blk, lse, ref = _model_vs_ref(kind, dtype, Lq, Lk, dh, causal)
        if pinned == 0.0:
            assert blk <= ONE_HOT, (name, blk)
        else:
            assert _within(blk, pinned), f"{kind} {name}: model block error {blk:.3e}, pinned {pinned:.2e}"
        assert blk <= 1.25 * G.MODEL_BLK[dtype], (name, blk)
        # errloc's floor is the GPU test's only leniency: no block of these references sits below it
        assert _min_block_share(ref) > errloc.FLOOR ** 2, (name, _min_block_share(ref))
        worst_lse = max(worst_lse, lse)
    pinned = G.MODEL_LSE[(dtype, kind)]
    if pinned < EXACT_LSE:
        assert worst_lse < EXACT_LSE, worst_lse
    else:
        assert _within(worst_lse, pinned), f"{kind}: float32-score lse error {worst_lse:.3e}, pinned {pinned:.2e}"


def test_the_family_tolerances_are_twice_the_models_worst_block():
    for dt in (BF16, F16):
        worst = max(max(row) for row in PIN_BLK[dt].values())
        assert _within(worst, G.MODEL_BLK[dt]) and G.MODEL_BLK[dt] >= worst
        assert G.TOL_OUT[dt] == 2 * G.MODEL_BLK[dt]
    assert G.TOL_OUT_F32 == {k: 2 * e for k, e in G.MODEL_BLK_F32.items()}
    assert G.LSE_FACTOR == 8 and G.LSE_ULPS == 4


@pytest.mark.parametrize("kind", sorted(G.MODEL_BLK_F32))
def test_float32_model_error(kind):
    """The f32 entry's yardstick: float32 arithmetic throughout (natural-log scores); worst block and worst lse row over the
    GPU module's own f32 cases of the kind, on their own inputs."""
    worst_blk = worst_lse = 0.0
    cases = [p.values for p in G.CASES if p.values[0] == F32 and p.values[1] == kind]
    assert len(cases) == 16
    for dtype, _, B, H, Lq, Lk, dh, causal, layout in cases:
        blk, lse, ref = _model_vs_ref(kind, F32, Lq, Lk, dh, causal, B, H, seed=G.case_seed(Lq, Lk, dh))
        worst_blk, worst_lse = max(worst_blk, blk), max(worst_lse, lse)
        assert _min_block_share(ref) > errloc.FLOOR ** 2, (Lq, dh, causal)
    assert _within(worst_blk, G.MODEL_BLK_F32[kind]), f"{kind}: float32 model block error {worst_blk:.3e}"
    assert _within(worst_lse, G.MODEL_LSE[(F32, kind)]), f"{kind}: float32 model lse error {worst_lse:.3e}"


def _whole(a, b):
    return float((a.double() - b).norm() / b.norm())


def _old_check_passes(out, ref, v):
    """Today's forward tests: relerr < 1e-2 and max error < 2e-2 max|v|, both over the whole tensor."""
    return _whole(out, ref) < 1e-2 and float((out.double() - ref).abs().max()) < 2e-2 * float(v.float().abs().max())


def _per_block_names(out, ref, tol, where):
    B, H, L, _ = ref.shape
    with pytest.raises(AssertionError, match=where):
        errloc.assert_attn_blocks(out, ref, tol, B, H, L, "queries")


def test_localized_mutations_pass_the_whole_tensor_bound_and_fail_per_block():
    B, H, L, dh = 16, 16, 257, 64
    q, k, v, qs = A.make_scores("normal", B, H, L, L, dh, seed=3)
    ref, _ = A.attn_fwd_ref(q, k, v, qs, False, BF16)
    model, _ = A.attn_fwd_model(q, k, v, qs, False, BF16)
    tol = G.TOL_OUT[BF16]
    assert _old_check_passes(model, ref, v)
    errloc.assert_attn_blocks(model, ref, tol, B, H, L, "queries")
    # the lone row of one head, scaled by 1.05
    m = model.clone()
    m[5, 7, 256:] = (m[5, 7, 256:].float() * 1.05).bfloat16()
    assert _old_check_passes(m, ref, v)
    _per_block_names(m, ref, tol, "b=5 h=7 queries 256:257 ")
    # every lone row, scaled by 1.05
    m = model.clone()
    m[:, :, 256:] = (m[:, :, 256:].float() * 1.05).bfloat16()
    assert _old_check_passes(m, ref, v)
    _per_block_names(m, ref, tol, r"queries 256:257 ")
    # one 32-row tile of one head, scaled by 1.05
    m = model.clone()
    m[9, 2, 96:128] = (m[9, 2, 96:128].float() * 1.05).bfloat16()
    assert _old_check_passes(m, ref, v)
    _per_block_names(m, ref, tol, "b=9 h=2 queries 96:128 ")
    # one key tile's contribution dropped for one query tile (from the product and from the row sum)
    s = A.ref_scores(q[3:4, 11:12], k[3:4, 11:12], qs, False, BF16)
    s[..., 160:192, 64:96] = float("-inf")
    p = torch.exp2(s - s.amax(-1, keepdim=True))
    m = model.clone()
    m[3, 11, 160:192] = ((p @ v[3:4, 11:12].double()) / p.sum(-1, keepdim=True))[0, 0, 160:192].bfloat16()
    # (a whole tile of normal scores moves single elements by more than test_inproj_and_attention's 2e-2 max|v|; the average
    #  that every forward test relies on, and the cross-attention test relies on alone, does not see it)
    assert _whole(m, ref) < 1e-2 and not _old_check_passes(m, ref, v)
    _per_block_names(m, ref, tol, "b=3 h=11 queries 160:192 ")


@pytest.mark.parametrize("dtype", [BF16, F16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("kind", ["sink_first", "sink_last"])
def test_dropped_floor_mass_is_caught_per_block(kind, dtype):
    """A kernel that flushed the floor's probabilities (2^-15: half subnormals) would return the sink's value row alone."""
    B, H, L, dh = 8, 8, 257, 64
    q, k, v, qs = A.make_scores(kind, B, H, L, L, dh, seed=4, dtype=dtype)
    ref, _ = A.attn_fwd_ref(q, k, v, qs, False, dtype)
    model, _ = A.attn_fwd_model(q, k, v, qs, False, dtype)
    tol = G.TOL_OUT[dtype]
    errloc.assert_attn_blocks(model, ref, tol, B, H, L, "queries")
    sink = 0 if kind == "sink_first" else L - 1
    mass = (L - 1) * 2.0 ** -15
    assert 0.007 < mass < 0.009
    m = model.clone()
    m[2, 5] = v[2, 5, sink]
    assert _old_check_passes(m, ref, v)
    _per_block_names(m, ref, tol, "b=2 h=5 queries ")
    blk, _ = errloc.attn_block_relerr(m, ref, B, H, L)
    assert blk > 5e-3, blk                      # (|v_floor - v_sink| / |v_sink| x mass: about 8e-3 or more)


@pytest.mark.parametrize("Lq,Lk,dh", [(257, 257, 64), (64, 600, 32), (257, 600, 104)])
@pytest.mark.parametrize("dtype", [BF16, F16], ids=["bf16", "fp16"])
def test_straddle_really_straddles(Lq, Lk, dh, dtype):
    """From the reference's scores: over the whole key tiles the tile maximum of even query rows rises by exactly 7.5, 8.5, 7.5,
    ..., that of rows 4i + 1 by +0.25 and of rows 4i + 3 by -0.25 per tile - so, whenever an even row crosses the kernel's 2^8
    threshold, its wave (32 consecutive queries) also holds lanes at 0 < mx <= 8 and lanes at mx < 0."""
    q, k, v, qs = A.make_scores("straddle", 2, 3, Lq, Lk, dh, seed=8, dtype=dtype)
    s = A.ref_scores(q, k, qs, False, dtype)
    nt = Lk // 32
    tmax = s[..., :nt * 32].reshape(2, 3, Lq, nt, 32).amax(-1)
    step = tmax.diff(dim=-1)
    want_even = torch.tensor([A.STRADDLE_STEPS[t % 2] for t in range(nt - 1)], dtype=torch.float64)
    assert torch.equal(step[:, :, 0::2], want_even.expand_as(step[:, :, 0::2]))
    assert torch.equal(step[:, :, 1::4], torch.full_like(step[:, :, 1::4], 0.25))
    if Lq > 3:
        assert torch.equal(step[:, :, 3::4], torch.full_like(step[:, :, 3::4], -0.25))
    assert max(A.STRADDLE_STEPS) > 8 > min(A.STRADDLE_STEPS) and sum(A.STRADDLE_STEPS) == 16


def test_every_instantiation_the_dispatch_can_reach_has_a_normal_and_a_large_score_case():
    seen = {}
    for p in G.CASES:
        dtype, kind, B, H, Lq, Lk, dh, causal, layout = p.values
        br = G.expected_branch(dtype, Lq, Lk, dh, causal)
        assert p.id.endswith(f"[{br}]")
        seen.setdefault(br, set()).add(kind)
    want = {f"{d}/{w}" for d in (32, 128) for w in ("tiles", "lone", "multi")} | {"64/tiles/dma", "64/lone/dma", "64/multi", "64/f16",
                                                                                  "f32/32", "f32/64"}
    assert set(seen) == want
    for br, kinds in seen.items():
        assert "normal" in kinds, br
        assert kinds & set(G.LARGE), br
        if not br.startswith(("128/", "f32/")):
            assert {"ramp", "sink_last", "straddle"} <= kinds, (br, kinds)
    ids = [p.id for p in G.CASES]
    assert len(ids) == len(set(ids))


def test_expected_branch_restates_the_dispatch():
    eb = G.expected_branch
    assert eb(BF16, 257, 257, 64, False) == "64/lone/dma" and eb(BF16, 257, 257, 64, True) == "64/lone/dma"
    assert eb(BF16, 257, 289, 64, False) == "64/multi" and eb(BF16, 289, 289, 64, False) == "64/multi"
    assert eb(BF16, 289, 64, 64, False) == "64/tiles/dma" and eb(BF16, 321, 100, 64, False) == "64/tiles/dma"
    assert eb(BF16, 129, 257, 64, True) == "64/tiles/dma" and eb(BF16, 257, 129, 64, True) == "64/lone/dma"
    assert eb(BF16, 33, 1, 80, False) == "128/lone" and eb(BF16, 1, 1, 32, False) == "32/tiles"
    assert eb(F16, 257, 257, 64, False) == "64/f16" and eb(F32, 50, 50, 32, True) == "f32/32"
    assert math.isclose(A.LOG2E, math.log2(math.e)) and math.isclose(A.LN2, math.log(2))
