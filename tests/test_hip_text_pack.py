"""GPU: the packed text tower - the plan kernel, the packed embedding, the variable-length causal attention and the engine.

The feature of a caption is ln_final(x[b, argmax(text[b])]) @ text_projection of a CAUSAL tower, so only the rows up to the
argmax position are needed.  What is checked:
  * plan and packed embedding against the torch restatement of tests/test_text_pack_host.py, bit-exact;
  * the attention against tests/attn_ref.py's float64 reference caption by caption, with the fp16 bound of
    tests/test_hip_attn_fwd.py (restated below with its source, not derived from this kernel);
  * the engine against the oracle with the project's bounds for the fp16 text tower (tests/test_hip_towers.py), and the
    bit-level properties that make packing safe: ids behind the EOT do not matter, batch composition does not matter, stale
    or NaN workspaces do not matter, a CPU and a GPU token tensor agree, and PACK_TEXT = False still gives the dense bits.
"""
import math

import pytest
import torch

import attn_ref as A
import vitlens_oracle as O
from test_text_pack_host import plan_ref

pytestmark = pytest.mark.gpu

F16, F32 = torch.float16, torch.float32
NAN = float("nan")
GUARD = 8
# tests/test_hip_attn_fwd.py: TOL_OUT[F16] = 2 x MODEL_BLK[F16], the worst (b, h, 32-query) block of attn_ref.attn_fwd_model (the
# declared rounding contract: exact softmax, P and the result rounded to half) against the float64 reference, pinned on the CPU
# by tests/test_attn_ref_host.py; the factor 2 pays for fp32 MFMA accumulation, v_exp_f32 and P relative to the lazily kept maximum
TOL_OUT_F16 = 2 * 3.41e-4


def _bits(t):
    return t.contiguous().view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def _ids_with_lengths(lengths, L, g, vocab=49408):
    """[SOT, random ids, EOT at position len-1, zeros]: argmax == len - 1 (len 1: the EOT alone)."""
    t = torch.zeros(len(lengths), L, dtype=torch.long)
    for i, n in enumerate(lengths):
        t[i, :n - 1] = torch.randint(1, vocab - 2, (n - 1,), generator=g)
        if n > 1:
            t[i, 0] = vocab - 2
        t[i, n - 1] = vocab - 1
    return t


# ------------------------------------------------------------------------------------------------ plan + embedding
def _plan_dev(ids):
    from vitlens_hip import ops
    B = ids.shape[0]
    lens = torch.full((B + GUARD,), -7, dtype=torch.int32, device="cuda")
    start = torch.full((B + 1 + GUARD,), -7, dtype=torch.int32, device="cuda")
    last = torch.full((B + GUARD,), -7, dtype=torch.int64, device="cuda")
    total = torch.full((2 + GUARD,), -7, dtype=torch.int32, device="cuda")
    ops.text_pack_plan(ids, lens, start, last, total)
    torch.cuda.synchronize()
    for t, n in ((lens, B), (start, B + 1), (last, B), (total, 2)):
        assert bool((t[n:] == -7).all()), "the plan kernel wrote behind its outputs"
    return lens[:B], start[:B + 1], last[:B], total[:2]


@pytest.mark.parametrize("case", ["mixed37", "all77", "ties", "one", "b1500"])
def test_plan_and_packed_embedding_bit_exact(case):
    from vitlens_hip import ops
    g = torch.Generator().manual_seed(11)
    L, D, vocab = 77, 128, 500
    if case == "mixed37":
        lengths = [1, 31, 32, 33, 64, 65, 77] + [int(x) for x in torch.randint(1, 78, (30,), generator=g)]
        ids = _ids_with_lengths(lengths, L, g, vocab)
    elif case == "all77":
        ids = _ids_with_lengths([77] * 37, L, g, vocab)
    elif case == "ties":
        ids = torch.randint(0, 9, (37, L), generator=g)          # many equal maxima, all-zero-like rows
        ids[3] = 0
    elif case == "one":
        ids = _ids_with_lengths([5], L, g, vocab)
    else:                                                       # more captions than the scan has threads
        ids = _ids_with_lengths([int(x) for x in torch.randint(1, 78, (1500,), generator=g)], L, g, vocab)
    B = ids.shape[0]
    lens_r, start_r, last_r, (rows, max_len) = plan_ref(ids)
    lens, start, last, total = _plan_dev(ids.cuda())
    assert lens.tolist() == lens_r and start.tolist() == start_r and last.tolist() == last_r
    assert total.tolist() == [rows, max_len]
    if case == "all77":
        assert rows == B * L

    tok = torch.randn(vocab, D, generator=g).cuda()
    pos = torch.randn(L, D, generator=g).cuda()
    Mr = (rows + 255) // 256 * 256
    buf = torch.full((Mr + GUARD, D), NAN, device="cuda")
    ops.text_embed_packed(ids.cuda(), start.contiguous(), lens.contiguous(), tok, pos, buf, rows, Mr)
    torch.cuda.synchronize()
    want = torch.cat([tok[ids[b, :n].cuda()] + pos[:n] for b, n in enumerate(lens_r)])
    assert torch.equal(_bits(buf[:rows]), _bits(want)), "packed embedding rows differ"
    assert bool((_bits(buf[rows:Mr]) == 0).all()), "rows [rows, roundup) must be zero"
    assert bool(torch.isnan(buf[Mr:]).all()), "rows beyond the padded range were written"


def test_packed_embedding_refuses_bad_totals():
    from vitlens_hip import ops
    ids = torch.zeros(4, 77, dtype=torch.long, device="cuda")
    z = torch.zeros(5, dtype=torch.int32, device="cuda")
    tok, pos = torch.zeros(10, 64, device="cuda"), torch.zeros(77, 64, device="cuda")
    out = torch.full((512, 64), NAN, device="cuda")
    for rows, pad in ((3, 256), (4 * 77 + 1, 512), (10, 8)):
        with pytest.raises((RuntimeError, ValueError)):
            ops.text_embed_packed(ids, z, z[:4], tok, pos, out, rows, pad)
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())


# ------------------------------------------------------------------------------------------------ variable-length attention
LENGTHS = {"to288": [1, 2, 31, 32, 33, 63, 64, 65, 77, 96, 97, 257, 288],          # the 288-key instantiation, two workgroups
           "to96": [33, 1, 77, 96, 2, 64, 65],                                    # the 96-key instantiation
           "to32": [1, 2, 31, 32, 17]}                                            # the 32-key instantiation, one wave
_REF = {}


def _varlen_inputs(name, kind, H=2, dh=64):
    """Per caption: q, k, v [1, H, len, dh] fp16 (seeded by the length) and the float64 reference; computed once per (name, kind)."""
    if (name, kind) not in _REF:
        caps = []
        for n in LENGTHS[name]:
            q, k, v, qscale = A.make_scores(kind, 1, H, n, n, dh, seed=1000 * n + 64, dtype=F16)
            ref, ref_lse = A.attn_fwd_ref(q.cuda(), k.cuda(), v.cuda(), qscale, True, F16)
            caps.append((q, k, v, qscale, ref, ref_lse))
        _REF[(name, kind)] = caps
    return _REF[(name, kind)]


@pytest.mark.parametrize("kind", ["normal", "sink_last"])
@pytest.mark.parametrize("name", sorted(LENGTHS))
def test_varlen_attention_vs_float64(name, kind):
    from errloc import attn_block_relerr
    from vitlens_hip import ops
    H, dh = 2, 64
    W = H * dh
    caps = _varlen_inputs(name, kind, H, dh)
    lengths = LENGTHS[name]
    qscale = caps[0][3]
    rows = sum(lengths)
    tm = lambda t: t[0].permute(1, 0, 2).reshape(t.shape[2], W)          # [1, H, n, dh] -> token-major [n, W]
    qkv_buf = torch.full((rows + 2 * GUARD, 3 * W), NAN, dtype=F16, device="cuda")
    qkv = qkv_buf[GUARD:GUARD + rows]
    r = 0
    for n, (q, k, v, *_ ) in zip(lengths, caps):
        for i, t in enumerate((q, k, v)):
            qkv[r:r + n, i * W:(i + 1) * W] = tm(t).cuda()
        r += n
    lens = torch.tensor(lengths, dtype=torch.int32, device="cuda")
    start = torch.tensor([0] + torch.tensor(lengths).cumsum(0).tolist(), dtype=torch.int32, device="cuda")
    out_buf = torch.full((rows + 2 * GUARD, W), NAN, dtype=F16, device="cuda")
    lse_buf = torch.full((rows + 2 * GUARD, H), NAN, dtype=F32, device="cuda")
    out, lse = out_buf[GUARD:GUARD + rows], lse_buf[GUARD:GUARD + rows]
    guards = [(b, _bits(b[:GUARD]).clone(), _bits(b[-GUARD:]).clone()) for b in (out_buf, lse_buf)]
    ops.attn_fwd_varlen(qkv, start, lens, out, H, max(lengths), lse=lse, qscale=qscale)
    torch.cuda.synchronize()
    out1, lse1 = out.clone(), lse.clone()
    assert bool(torch.isfinite(out1).all()) and bool(torch.isfinite(lse1).all()), "owned rows must come out finite"
    out.fill_(NAN); lse.fill_(NAN)
    ops.attn_fwd_varlen(qkv, start, lens, out, H, max(lengths), lse=lse, qscale=qscale)
    torch.cuda.synchronize()
    assert torch.equal(_bits(out), _bits(out1)) and torch.equal(_bits(lse), _bits(lse1)), "a second launch differs"
    for buf, lo, hi in guards:
        assert torch.equal(_bits(buf[:GUARD]), lo) and torch.equal(_bits(buf[-GUARD:]), hi), "guard rows were written"
    r, worst = 0, 0.0
    for n, (q, k, v, qs, ref, ref_lse) in zip(lengths, caps):
        blk, (_, h, r0, r1) = attn_block_relerr(out1[r:r + n], ref, 1, H, n)
        lse_err = float((lse1[r:r + n].t().double() - ref_lse[0]).abs().max())
        print(f"VARLEN {name} {kind} len {n}: blk {blk:.3e} tol {TOL_OUT_F16:.2e} lse {lse_err:.3e}")
        assert blk <= TOL_OUT_F16, f"caption of {n} rows at packed row {r}: h={h} queries {r0}:{r1} has relative error {blk:.3e}"
        # lse, as test_hip_attn_fwd.py: 8 x the model's worst fp16 row of the score kind (MODEL_LSE there: normal 9.41e-7,
        # sink_last 3.85e-8) and no less than 4 ulp of fp32 at the caption's largest |lse|
        lse_max = max(float(ref_lse.abs().max()), 1e-30)
        lse_tol = max(8 * {"normal": 9.41e-7, "sink_last": 3.85e-8}[kind], 4 * 2.0 ** (math.floor(math.log2(lse_max)) - 23))
        assert lse_err <= lse_tol, (n, lse_err, lse_tol)
        worst = max(worst, blk)
        r += n


def test_varlen_attention_refusals_launch_nothing():
    from vitlens_hip import ops
    H, rows = 2, 64
    lens = torch.tensor([40, 24], dtype=torch.int32, device="cuda")
    start = torch.tensor([0, 40, 64], dtype=torch.int32, device="cuda")
    out = torch.full((rows, H * 64), NAN, dtype=F16, device="cuda")
    qkv = torch.randn(rows, 3 * H * 64, device="cuda").to(F16)
    with pytest.raises(RuntimeError, match="288"):
        ops.attn_fwd_varlen(qkv, start, lens, out, H, 289)
    # head dim 32 through the C entry itself (the wrapper only builds head dim 64)
    import ctypes
    from vitlens_hip import _lib
    lib = _lib.load_library()
    st = (ctypes.c_long * 6)(32, 384, 32, 384, 32, 384)
    base = qkv.data_ptr()
    s = torch.cuda.current_stream().cuda_stream
    rc = lib.vl_attn_fwd_varlen_f16(base, base + 256, base + 512, st, start.data_ptr(), lens.data_ptr(), out.data_ptr(), None,
                                    2, H, 40, 32, 1.0, s)
    assert rc != 0 and b"head dim" in lib.vl_last_error()
    rc = lib.vl_attn_fwd_varlen_f16(base, base + 256, base + 512, st, start.data_ptr(), lens.data_ptr(), out.data_ptr(), None,
                                    2, H, 289, 64, 1.0, s)
    assert rc != 0 and b"288" in lib.vl_last_error()
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()), "a refused call wrote to out"


# ------------------------------------------------------------------------------------------------ the engine
def relerr(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return float((a - b).norm() / b.norm())


def cos_matrix(a):
    a = torch.nn.functional.normalize(a.float().cpu(), dim=-1)
    return a @ a.t()


def _check_vs_oracle(got, ref, what):
    """The project's bounds for the fp16 text tower (tests/test_hip_towers.py: test_vitl_text_tower_vs_oracle)."""
    cm = float((cos_matrix(got) - cos_matrix(ref)).abs().max())
    fc = float((1 - torch.nn.functional.cosine_similarity(got.float().cpu(), ref, dim=-1)).max())
    re = relerr(got, ref)
    print(f"TEXTPACK {what}: cos-matrix {cm:.2e} (< 5e-4), 1 - feature cosine {fc:.2e} (< 1e-3), relerr {re:.2e} (< 2e-2)")
    return cm, fc, re


SMALL = dict(width=512, heads=8, layers=2, embed_dim=512)
SMALL_LENGTHS = [1, 32, 33, 77, 5, 14, 22, 64, 9]


@pytest.fixture(scope="module")
def small():
    """The smallest tower the fp16 path takes, 9 captions, the oracle's features and the dense and packed features of one engine."""
    from vitlens_hip import engine as E
    g = torch.Generator().manual_seed(21)
    spec = O.TextSpec(**SMALL)
    sd = O.init_text(spec, g)
    text = _ids_with_lengths(SMALL_LENGTHS, 77, g)
    ref = O.encode_text(sd, text, spec)
    eng = E.TextEngine(sd, E.TextCfg(**SMALL), "cuda")
    assert eng.arith == "f16" and E.PACK_TEXT
    E.PACK_TEXT = False
    try:
        dense = eng.encode_text(text.cuda()).clone()        # the parent's path, before anything packed ran on this engine
        assert eng.plan_text(text.cuda()) is None
    finally:
        E.PACK_TEXT = True
    packed = eng.encode_text(text.cuda()).clone()
    torch.cuda.synchronize()
    return dict(E=E, eng=eng, sd=sd, spec=spec, text=text, ref=ref, dense=dense, packed=packed, g=g)


def test_engine_packed_and_dense_vs_oracle(small):
    errs = {k: _check_vs_oracle(small[k], small["ref"], k) for k in ("packed", "dense")}
    for k, (cm, fc, re) in errs.items():
        assert cm < 5e-4 and fc < 1e-3 and re < 2e-2, (k, cm, fc, re)


def test_engine_plan_matches_restatement(small):
    plan = small["eng"].plan_text(small["text"].cuda())
    lens, start, last, (rows, mx) = plan_ref(small["text"])
    assert (plan.rows, plan.max_len) == (rows, mx) == (sum(SMALL_LENGTHS), 77)
    assert plan.lens.tolist() == lens and plan.start.tolist() == start and plan.last_row.tolist() == last


def test_ids_behind_the_eot_do_not_matter(small):
    text = small["text"].clone()
    g = torch.Generator().manual_seed(5)
    for b, n in enumerate(SMALL_LENGTHS):
        text[b, n:] = torch.randint(0, 49407, (77 - n,), generator=g)          # below the EOT id: the argmax stays
    assert torch.equal((text.argmax(-1) + 1), torch.tensor(SMALL_LENGTHS))
    got = small["eng"].encode_text(text.cuda())
    assert torch.equal(_bits(got), _bits(small["packed"]))


def test_batch_composition_and_repeat_do_not_matter(small):
    eng, text, packed = small["eng"], small["text"], small["packed"]
    assert torch.equal(_bits(eng.encode_text(text.cuda())), _bits(packed)), "a second call differs"
    for b in (0, 3, 8):
        assert torch.equal(_bits(eng.encode_text(text[b:b + 1].cuda())), _bits(packed[b:b + 1])), f"caption {b} alone differs"
    g = torch.Generator().manual_seed(9)
    others = O.synth_text(91, g)
    perm = torch.randperm(100, generator=g)
    big = torch.cat([text, others])[perm]
    f = eng.encode_text(big.cuda())
    inv = torch.argsort(perm)                                # caption b of `text` sits at row inv[b] of `big`
    assert torch.equal(_bits(f[inv[:9].cuda()]), _bits(packed)), "a caption's features depend on its batch"
    assert torch.equal(_bits(eng.encode_text(text.cuda())), _bits(packed)), "a call after a larger batch differs"


def test_nan_filled_workspace_does_not_matter(small):
    eng, text = small["eng"], small["text"]
    eng.encode_text(text.cuda())
    filled = 0
    for ws in eng._ws.values():
        for t in vars(ws).values():
            if torch.is_tensor(t) and t.is_floating_point():          # (q, k, v are views of qkv)
                t.fill_(NAN)
                filled += 1
    assert filled >= 8
    got = eng.encode_text(text.cuda())
    assert bool(torch.isfinite(got).all())
    assert torch.equal(_bits(got), _bits(small["packed"]))


def test_pack_switch_off_reproduces_the_dense_bits(small):
    """Guards the DENSE path: with the switch off the engine returns what it returned before any packed call ran on it."""
    E, eng, text = small["E"], small["eng"], small["text"]
    E.PACK_TEXT = False
    try:
        got = eng.encode_text(text.cuda()).clone()
    finally:
        E.PACK_TEXT = True
    assert torch.equal(_bits(got), _bits(small["dense"]))


def test_cpu_and_device_tokens_agree(small):
    eng, text = small["eng"], small["text"]
    assert eng.plan_text(text).rows == eng.plan_text(text.cuda()).rows
    assert torch.equal(_bits(eng.encode_text(text)), _bits(small["packed"]))
    plan = eng.plan_text(text.cuda())
    assert torch.equal(_bits(eng.encode_text(text.cuda(), plan=plan)), _bits(small["packed"]))
    fn = eng.encode_text(text.cuda(), normalize=True, plan=plan)
    assert float((fn - torch.nn.functional.normalize(small["packed"], dim=-1)).abs().max()) < 1e-6
    with pytest.raises(ValueError):
        eng.encode_text(text[:4].cuda(), plan=plan)


def test_full_geometry_packed_vs_oracle():
    """12 x 768, 64 captions of the oracle's caption generator, one seed: the bounds of test_vitl_text_tower_vs_oracle."""
    from vitlens_hip import engine as E
    g = torch.Generator().manual_seed(77)
    spec = O.TextSpec()
    sd = O.init_text(spec, g)
    text = O.synth_text(64, g)
    ref = O.encode_text(sd, text, spec)
    eng = E.TextEngine(sd, E.TextCfg(), "cuda")
    plan = eng.plan_text(text.cuda())
    assert plan is not None and plan.rows == int((text.argmax(-1) + 1).sum()) and plan.max_len <= 22
    cm, fc, re = _check_vs_oracle(eng.encode_text(text.cuda(), plan=plan), ref, "12 x 768, 64 captions, packed")
    assert cm < 5e-4 and fc < 1e-3 and re < 2e-2, (cm, fc, re)
