"""GPU: gradient-norm clipping on the device.  vl_sumsq_f32 against float64; vl_adamw_multi_step against
torch.nn.utils.clip_grad_norm_ + torch.optim.AdamW on the CPU and, bit for bit, against the per-tensor vl_adamw_step; the
three fused steps with `grad_clip_norm`.  Run the file under one time limit (`timeout 900 python -m pytest -m gpu ...`).

Two bars on the sum of squares, both asserted.  (1) The project's convention for a reduction against float64: relative
error within 4x the error of the CPU's own float32 result on the same input (torch.linalg.vector_norm(x) ** 2), and never
below 4 ulp of float32.  The CPU's float32 norm is poor at the recipes' sizes (measured: 4e-3 of the norm at 50.8 M elements,
8e-5 at 4 M), so that bar alone would let a lost block through.  (2) What the kernel's design promises: the squares are exact in
fp64 and all terms are positive, so the fp64 accumulation is within n * 2^-53 of the sum (1.4e-8 at 127.6 M elements) and the
one rounding to fp32 adds 2^-24: 4 ulp of float32 (4.8e-7) for every input.  Every case shows that the check has teeth, with
ONE block scaled by 2 (the 4096-element span of one workgroup that holds the largest element; 2.4e-4 / 9.6e-5 of the sum at
the two large sizes): the kernel's result must FAIL the check against the float64 sum of the scaled input, and the kernel run
on the scaled input must FAIL it against the float64 sum of the original.

Measured on an MI355X: sum of squares 0 to 4.3e-8 relative (50.8 M: 8.2e-9, 127.6 M: 1.8e-9); convention bars 4.8e-7 to 1.2e-1."""
import math

import pytest
import torch

from golden_util import load_npz, split, specs_from_meta

pytestmark = pytest.mark.gpu

ULP = 2.0 ** -23
SIZES = {"depth": 50_800_000, "audio": 127_600_000}          # trainable elements of the depth (C3) and audio (C4) recipes


def relerr(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def _bar(x_cpu):
    """(float64 sum of squares, tolerance) of a CPU f32 tensor."""
    ref = float(x_cpu.double().pow(2).sum())
    cpu32 = float(torch.linalg.vector_norm(x_cpu.reshape(-1)) ** 2) if x_cpu.numel() else 0.0
    e32 = abs(cpu32 - ref) / ref if ref > 0 else 0.0
    return ref, max(4.0 * e32, 4.0 * ULP)


def _within(got, ref, tol):
    """Both bars: the convention's `tol` and the design's 4 ulp."""
    return got == ref if ref == 0.0 else abs(got - ref) <= min(tol, 4.0 * ULP) * ref


def _sumsq_case(x_cpu, x_dev=None, label=""):
    from vitlens_hip import ops
    x_dev = x_cpu.cuda() if x_dev is None else x_dev
    guard = torch.full((65,), -7.25, device="cuda")
    out = guard[32:33]
    ops.grad_sumsq(x_dev, out=out)
    second = ops.grad_sumsq(x_dev)
    torch.cuda.synchronize()
    got = float(out)
    assert torch.equal(out.view(torch.int32), second.view(torch.int32)), (label, "two launches differ")
    assert bool((guard[:32] == -7.25).all()) and bool((guard[33:] == -7.25).all()), (label, "wrote beside the output")
    assert torch.equal(x_dev.cpu().reshape(-1), x_cpu.reshape(-1)), (label, "the input changed")
    ref, tol = _bar(x_cpu)
    rel = abs(got - ref) / ref if ref > 0 else abs(got)
    print(f"sumsq {label}: n = {x_cpu.numel()}, rel err {rel:.3e}, bar {tol:.3e}")
    assert got == ref if ref == 0.0 else abs(got - ref) <= tol * ref, (label, "the convention's bar", got, ref, rel, tol)
    assert _within(got, ref, tol), (label, "the design's 4 ulp", got, ref, rel)
    if x_cpu.numel():          # teeth: one block scaled by 2 adds 3x its own sum of squares to the reference
        flat = x_cpu.reshape(-1)
        b = int(flat.abs().argmax()) // 4096 * 4096
        ref2 = ref + 3.0 * float(flat[b:b + 4096].double().pow(2).sum())
        assert not _within(got, ref2, tol), (label, "a block scaled by 2 would pass this check", got, ref2, tol)
        # ... and the kernel run on the input with that block scaled must fail the check against the unscaled reference
        scaled = x_dev.clone().reshape(-1)
        scaled[b:b + 4096] *= 2.0
        got2 = float(ops.grad_sumsq(scaled))
        assert not _within(got2, ref, tol), (label, "the kernel on a scaled block passes this check", got2, ref, tol)
        assert _within(got2, ref2, 4.0 * ULP), (label, "the scaled input against its own float64 sum", got2, ref2)
    return got


@pytest.mark.parametrize("n", [0, 1, 3, 257, SIZES["depth"], SIZES["audio"]])
def test_sumsq_sizes_vs_float64(n):
    g = torch.Generator().manual_seed(n % 1000 + 1)
    x = torch.randn(n, generator=g) * 0.02
    _sumsq_case(x, label=f"n={n}")


@pytest.mark.parametrize("off", [1, 2, 3])
def test_sumsq_offset_view(off):
    g = torch.Generator().manual_seed(10 + off)
    n = 100_003
    base = torch.randn(n + 8, generator=g)
    dev = base.cuda()
    view = dev[off:off + n]
    assert view.data_ptr() % 16 == 4 * off
    before, after = dev[:off].clone(), dev[off + n:].clone()
    _sumsq_case(base[off:off + n].clone(), view, label=f"offset {off}")
    assert torch.equal(dev[:off], before) and torch.equal(dev[off + n:], after)


def test_sumsq_wide_range_and_outlier():
    g = torch.Generator().manual_seed(20)
    n = 1_000_003
    mag = 10.0 ** (torch.rand(n, generator=g, dtype=torch.float64) * 18.0 - 12.0)          # 1e-12 .. 1e6
    sign = (torch.rand(n, generator=g) < 0.5).double() * 2 - 1
    _sumsq_case((mag * sign).float(), label="1e-12..1e6")
    x = torch.randn(n, generator=g) * 1e-3
    x[777_777] = 3.0e4                               # one element carries almost the whole norm
    _sumsq_case(x, label="outlier")
    x[777_777] = 1.0                                 # ... or a tenth of it: the rest must not be lost beside it
    _sumsq_case(x, label="mild outlier")


@pytest.mark.parametrize("pos", [0, 2, 5000, 100_002, 100_004])
def test_sumsq_nonfinite_propagates(pos):
    """NaN, +inf and -inf in the scalar head (0, 2), the 16-byte body (5000, 100002) and the scalar tail (100004) of a view that
    starts 4 bytes past a 16-byte boundary: NaN and inf as torch.linalg.vector_norm gives them."""
    from vitlens_hip import ops
    g = torch.Generator().manual_seed(30)
    base = torch.randn(100_005, generator=g)
    for bad, want in ((float("nan"), "nan"), (float("inf"), "inf"), (float("-inf"), "inf")):
        x = torch.cat([torch.zeros(1), base]).cuda()[1:]
        assert x.data_ptr() % 16 == 4
        x[pos] = bad
        got = float(ops.grad_sumsq(x))
        ref = float(torch.linalg.vector_norm(x.cpu()) ** 2)
        assert (math.isnan(got) if want == "nan" else got == float("inf")), (pos, bad, got)
        assert math.isnan(ref) == math.isnan(got) and (math.isnan(ref) or ref == got)
    x = base.cuda(); x[pos] = float("inf"); x[(pos + 50_000) % x.numel()] = float("nan")
    assert math.isnan(float(ops.grad_sumsq(x)))


def test_sumsq_refuses_bad_arguments():
    from vitlens_hip import ops
    x = torch.randn(64, device="cuda")
    with pytest.raises(ValueError):
        ops.grad_sumsq(x.double())
    with pytest.raises(ValueError):
        ops.grad_sumsq(x[::2])
    with pytest.raises(ValueError):
        ops.grad_sumsq(x, out=torch.zeros(2, device="cuda"))
    with pytest.raises(RuntimeError):
        ops.grad_sumsq(torch.randn(4))


# ------------------------------------------------------------------------------------------------ multi-tensor AdamW
BIG = 4 * 1024 * 1024 + 3
SHAPES = {"w": (37, 19), "ln.bias": (19,), "logit_scale": (), "big.weight": (BIG, 1), "bn.proj": (8, 8), "tail.bias": (5,)}
KW = dict(lr=1e-2, betas=(0.9, 0.98), eps=1e-6, weight_decay=0.2)


def _params(seed=7):
    g = torch.Generator().manual_seed(seed)
    return {k: torch.randn(s, generator=g) for k, s in SHAPES.items()}, g


def _flat_views(grads_cpu):
    """The gradients as views of ONE flat device buffer, 16-byte aligned as in the fused steps - except `ln.bias`, put at an odd
    offset so that its slot takes the kernel's scalar path."""
    al = lambda n: (n + 3) // 4 * 4
    total = sum(al(v.numel()) for v in grads_cpu.values()) + 4
    flat = torch.zeros(total, device="cuda")
    views, off = {}, 0
    for k, v in grads_cpu.items():
        o = off + 1 if k == "ln.bias" else off
        views[k] = flat[o:o + v.numel()].view(v.shape)
        views[k].copy_(v)
        off += al(v.numel()) + (4 if k == "ln.bias" else 0)
    return flat, views


def _torch_opt(ref):
    from vitlens_hip.train import AdamW
    dec = [ref[k] for k in ref if AdamW.decays(k, ref[k])]
    nod = [ref[k] for k in ref if not AdamW.decays(k, ref[k])]
    assert dec and nod
    return torch.optim.AdamW([{"params": dec, "weight_decay": KW["weight_decay"]}, {"params": nod, "weight_decay": 0.0}],
                             lr=KW["lr"], betas=KW["betas"], eps=KW["eps"])


@pytest.mark.parametrize("grad_scale", [1.0, 0.5])
@pytest.mark.parametrize("max_norm", [0.5, 1e4])          # gradient norms here are about 2050 (x grad_scale): active / inactive
def test_adamw_multi_matches_torch_clip_and_adamw(max_norm, grad_scale):
    """Five steps against clip_grad_norm_ + torch.optim.AdamW on the CPU, in float32 (what a user runs) and in float64.

    Parameters: relerr < 1e-5 against both.  They barely feel the coefficient (it cancels in m / sqrt(v) up to eps).
    Moments: relerr < 1e-5 against the float64 run.  The float32 run is a poorer reference for them: m is linear and v quadratic
    in the coefficient, and the CPU's float32 norm of the 4 M-element tensor is off by about 8e-5 (it depends on the CPU's vector
    width; measured here per step against float64 as `d`).  v is a sum of positive terms, each off by at most (1 + d)^2 - 1; m is
    a sum of independent random vectors whose errors and values both add in quadrature, so d bounds it up to chance alignment,
    for which the bar takes 2 d.  So against float32: m within 1e-5 + 2 d, v within 1e-5 + 2 d + d^2; d = 0 while the clip is
    inactive."""
    from vitlens_hip import ops, train as TR
    p0, g = _params()
    ref = {k: v.clone().requires_grad_(True) for k, v in p0.items()}
    opt = _torch_opt(ref)
    ref64 = {k: v.double().requires_grad_(True) for k, v in p0.items()}
    opt64 = _torch_opt(ref64)
    d = 0.0
    mine = {k: v.clone().cuda() for k, v in p0.items()}
    mopt = TR.AdamW(mine, **KW)
    assert sorted(k for k in mine if mopt.decays(k, mine[k])) == ["big.weight", "w"]
    table = None
    for it in range(5):
        grads = {k: torch.randn(SHAPES[k], generator=g) for k in p0}
        for k in ref:
            ref[k].grad = grads[k] * grad_scale          # the CPU side sees the mean gradient
        total = torch.nn.utils.clip_grad_norm_(list(ref.values()), max_norm, norm_type=2.0)
        assert (float(total) > max_norm) == (max_norm < 1.0)
        opt.step()
        for k in ref64:
            ref64[k].grad = grads[k].double() * grad_scale
        total64 = float(torch.nn.utils.clip_grad_norm_(list(ref64.values()), max_norm, norm_type=2.0))
        opt64.step()
        if total64 > max_norm:
            d = max(d, abs(float(total) - total64) / total64)
        if it == 0:
            flat, views = _flat_views(grads)
        else:
            for k in views:
                views[k].copy_(grads[k])
        sumsq = ops.grad_sumsq(flat)
        mopt.step(views, grad_scale=grad_scale, max_norm=max_norm, sumsq=sumsq)
        assert table is None or mopt._slots is table, "the slot table is rebuilt although no tensor moved"
        table = mopt._slots
        n64 = math.sqrt(sum(float(v.double().pow(2).sum()) for v in grads.values())) * grad_scale
        assert mopt.last_grad_norm.dim() == 0 and mopt.last_grad_norm.is_cuda
        assert abs(float(mopt.last_grad_norm) - n64) <= 4 * ULP * n64, (float(mopt.last_grad_norm), n64)
        assert abs(total64 - n64) <= 1e-12 * n64
    assert mopt.t == 5
    bar_m, bar_v = 1e-5 + 2.0 * d, 1e-5 + 2.0 * d + d * d
    print(f"adamw_multi max_norm {max_norm} grad_scale {grad_scale}: the float32 reference's norm is off by {d:.3e}")
    for k in ref:
        st, st64 = opt.state[ref[k]], opt64.state[ref64[k]]
        e, e64 = relerr(mine[k], ref[k].detach()), relerr(mine[k], ref64[k].detach())
        em, ev = relerr(mopt.m[k], st["exp_avg"]), relerr(mopt.v[k], st["exp_avg_sq"])
        em64, ev64 = relerr(mopt.m[k], st64["exp_avg"]), relerr(mopt.v[k], st64["exp_avg_sq"])
        print(f"adamw_multi max_norm {max_norm} grad_scale {grad_scale} {k}: rel err p {e:.3e} m {em:.3e} v {ev:.3e} (float32), "
              f"p {e64:.3e} m {em64:.3e} v {ev64:.3e} (float64)")
        assert e < 1e-5 and e64 < 1e-5, (k, e, e64)
        assert em64 < 1e-5 and ev64 < 1e-5, (k, em64, ev64)
        assert em < bar_m and ev < bar_v, (k, em, ev, bar_m, bar_v)


@pytest.mark.parametrize("with_sumsq", [True, False])
def test_adamw_multi_without_clipping_is_the_per_tensor_path_bit_for_bit(with_sumsq):
    from vitlens_hip import ops, train as TR
    p0, g = _params(8)
    a = {k: v.clone().cuda() for k, v in p0.items()}
    b = {k: v.clone().cuda() for k, v in p0.items()}
    oa, ob = TR.AdamW(a, **KW), TR.AdamW(b, **KW)
    for it in range(3):
        flat, views = _flat_views({k: torch.randn(SHAPES[k], generator=g) for k in p0})
        oa.step(views, grad_scale=0.5)
        ob.step(views, grad_scale=0.5, max_norm=1e30, sumsq=ops.grad_sumsq(flat) if with_sumsq else None)
    torch.cuda.synchronize()
    for k in a:
        assert torch.equal(a[k], b[k]), (k, "p")
        assert torch.equal(oa.m[k], ob.m[k]), (k, "m")
        assert torch.equal(oa.v[k], ob.v[k]), (k, "v")
        assert not torch.equal(a[k], p0[k].cuda()), (k, "did not move")


def test_adamw_multi_nan_gradient_poisons_what_torch_poisons():
    from vitlens_hip import train as TR
    p0, g = _params(9)
    ref = {k: v.clone().requires_grad_(True) for k, v in p0.items()}
    opt = _torch_opt(ref)
    mine = {k: v.clone().cuda() for k, v in p0.items()}
    mopt = TR.AdamW(mine, **KW)
    grads = {k: torch.randn(SHAPES[k], generator=g) for k in p0}
    grads["w"][3, 4] = float("nan")
    for k in ref:
        ref[k].grad = grads[k].clone()
    total = torch.nn.utils.clip_grad_norm_(list(ref.values()), 1.0, norm_type=2.0)
    opt.step()
    mopt.step({k: v.cuda() for k, v in grads.items()}, max_norm=1.0)
    assert math.isnan(float(total)) and math.isnan(float(mopt.last_grad_norm))
    for k in ref:
        assert torch.equal(torch.isnan(mine[k]).cpu(), torch.isnan(ref[k].detach())), k
        assert bool(torch.isnan(mine[k]).all()), k


def test_adamw_multi_refuses_bad_arguments_before_any_launch():
    from vitlens_hip import _lib, ops, train as TR
    import ctypes as C
    p0, g = _params(10)
    mine = {k: v.clone().cuda() for k, v in p0.items()}
    mopt = TR.AdamW(mine, **KW)
    grads = {k: torch.randn(SHAPES[k], generator=g).cuda() for k in p0}
    slots = TR.pack_adamw_slots(mopt.slot_rows(grads)).cuda()
    sumsq = ops.grad_sumsq(grads["w"])
    n = slots.shape[0]
    ok = dict(slots=slots, nslots=n, lr=1e-2, beta1=0.9, beta2=0.98, eps=1e-6, step=1, grad_scale=1.0, max_norm=1.0, sumsq=sumsq)
    for change in (dict(max_norm=0.0), dict(max_norm=-1.0), dict(max_norm=float("nan")), dict(nslots=n + 1), dict(nslots=-1),
                   dict(step=0), dict(slots=slots.int()), dict(slots=slots[:, :5]), dict(slots=slots.reshape(-1)),
                   dict(sumsq=sumsq.double()), dict(sumsq=torch.zeros(2, device="cuda")), dict(norm_out=torch.zeros(2, device="cuda"))):
        with pytest.raises(ValueError):
            ops.adamw_multi(**{**ok, **change})
    for mn in (0.0, -2.0):
        with pytest.raises(ValueError):
            mopt.step(grads, max_norm=mn)
    with pytest.raises(ValueError):
        mopt.step({**grads, "ln.bias": torch.randn(20, device="cuda")}, max_norm=1.0)
    assert mopt.t == 0
    # the library's own refusals (a caller of the C ABI): too many slots, max_norm <= 0, step 0, no norm
    lib = _lib.load_library()
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    sp, qp = C.c_void_p(slots.data_ptr()), C.c_void_p(sumsq.data_ptr())
    assert lib.vl_adamw_multi_step(sp, 1025, 1e-2, 0.9, 0.98, 1e-6, 1, 1.0, 1.0, qp, None, s) != 0
    assert lib.vl_adamw_multi_step(sp, n, 1e-2, 0.9, 0.98, 1e-6, 1, 1.0, 0.0, qp, None, s) != 0
    assert lib.vl_adamw_multi_step(sp, n, 1e-2, 0.9, 0.98, 1e-6, 0, 1.0, 1.0, qp, None, s) != 0
    assert lib.vl_adamw_multi_step(sp, n, 1e-2, 0.9, 0.98, 1e-6, 1, 1.0, 1.0, None, None, s) != 0
    assert lib.vl_sumsq_f32(sp, -1, qp, qp, s) != 0 and lib.vl_sumsq_f32(sp, 4, qp, None, s) != 0
    torch.cuda.synchronize()
    for k in mine:
        assert torch.equal(mine[k].cpu(), p0[k]), (k, "written")
        assert not bool(mopt.m[k].any()) and not bool(mopt.v[k].any()), k


def test_public_clip_grad_norm_on_flat_buffer_and_on_tensors():
    import vitlens_hip
    g = torch.Generator().manual_seed(11)
    grads = {k: torch.randn(s, generator=g) for k, s in SHAPES.items() if k != "big.weight"}
    n64 = math.sqrt(sum(float(v.double().pow(2).sum()) for v in grads.values()))
    for max_norm in (0.5 * n64, 2.0 * n64):
        ref = [torch.nn.Parameter(v.clone()) for v in grads.values()]
        for r, v in zip(ref, grads.values()):
            r.grad = v.clone()
        torch.nn.utils.clip_grad_norm_(ref, max_norm)
        flat, views = _flat_views(grads)
        norm = vitlens_hip.clip_grad_norm_(flat, max_norm)
        loose = {k: v.cuda() for k, v in grads.items()}
        norm2 = vitlens_hip.clip_grad_norm_(loose, max_norm)
        assert norm.is_cuda and norm.dim() == 0
        for nn_ in (norm, norm2):
            assert abs(float(nn_) - n64) <= 4 * ULP * n64
        for r, k in zip(ref, grads):
            assert relerr(views[k], r.grad) < 1e-6 and relerr(loose[k], r.grad) < 1e-6, k
            if max_norm > n64:
                assert torch.equal(views[k].cpu(), grads[k])
    with pytest.raises(ValueError):
        vitlens_hip.clip_grad_norm_(flat, 0.0)


# ------------------------------------------------------------------------------------------------ the fused steps
def _make(recipe, **kw):
    from vitlens_hip import engine as E, step as ST
    sd, ins, outs, grads, meta = split(load_npz(f"tiny_{recipe}.npz"))
    tower, text, lens = specs_from_meta(meta)
    tc = E.TowerCfg(width=tower.width, layers=tower.layers, heads=tower.heads, patch=tower.patch, image_size=tower.image_size,
                    embed_dim=tower.embed_dim)
    xc = E.TextCfg(context_length=text.context_length, vocab_size=text.vocab_size, width=text.width, heads=text.heads,
                   layers=text.layers, embed_dim=text.embed_dim)
    lc = E.LensCfg(**{k: getattr(lens, k) for k in E.LensCfg.__dataclass_fields__ if hasattr(lens, k)})
    img, txt, vis = ins["image"].cuda(), ins["text"].cuda(), ins["visual_x"].cuda()
    if recipe == "depth":
        st = ST.TriModalDepthStep(sd, tc, xc, "cuda", micro_batch=2, unlock_first_n=1, lr=1e-3, **kw)
        return st, lambda: st.forward_backward(img, txt, vis)
    if recipe == "audio":
        st = ST.DualAudioStep(sd, tc, xc, lc, "cuda", micro_batch=2, lr=1e-3, **kw)
        return st, lambda: st.forward_backward(vis, txt)
    st = ST.TriModalPCStep(sd, tc, xc, lc, "cuda", micro_batch=4, lr=1e-3, bn_training=True, **kw)
    return st, lambda: st.forward_backward(img, txt, vis, ins["fps_start"].cuda())


def _host_norm(st):
    return math.sqrt(sum(float(g.double().pow(2).sum()) for g in st.reduced_grads().values()))


@pytest.mark.parametrize("recipe", ["depth", "audio", "pc"])
def test_step_with_an_inactive_clip_is_the_unclipped_step_bit_for_bit(recipe):
    plain, fb_plain = _make(recipe)
    assert plain.grad_clip_norm is None and plain.last_grad_norm is None
    fb_plain()
    gn = _host_norm(plain)
    plain.optimizer_step()
    assert plain.last_grad_norm is None
    clip, fb_clip = _make(recipe, grad_clip_norm=100.0 * gn + 1.0)
    for it in range(3):
        if it:
            fb_plain(); plain.optimizer_step()
        fb_clip(); clip.optimizer_step()
        assert float(clip.last_grad_norm) < clip.grad_clip_norm, "the clip was meant to stay inactive"
    torch.cuda.synchronize()
    assert plain.opt.t == clip.opt.t == 3
    for k in plain.masters:
        assert torch.equal(plain.masters[k], clip.masters[k]), k
        assert torch.equal(plain.opt.m[k], clip.opt.m[k]) and torch.equal(plain.opt.v[k], clip.opt.v[k]), k


@pytest.mark.parametrize("recipe", ["depth", "audio", "pc"])
def test_step_with_an_active_clip_vs_gradients_scaled_by_the_float64_coefficient(recipe):
    probe, fb = _make(recipe)
    fb()
    gn = _host_norm(probe)
    c = 0.5 * gn
    clip, fb_clip = _make(recipe, grad_clip_norm=c)
    fb_clip()
    flat_cpu = clip.flat_grad.cpu()
    clip.optimizer_step()
    ref, fb_ref = _make(recipe)
    fb_ref()
    assert torch.equal(ref.flat_grad.cpu(), flat_cpu), "identically seeded steps produce identical gradients"
    ref.finish_reduce()
    ref.flat_grad.mul_(c / (gn + 1e-6))
    ref.optimizer_step()
    torch.cuda.synchronize()
    s64, tol = _bar(flat_cpu)
    assert abs(math.sqrt(s64) - gn) <= 1e-12 * gn          # the padding of the flat buffer is zero
    got = float(clip.last_grad_norm)
    print(f"{recipe}: gradient norm {gn:.6e}, last_grad_norm {got:.6e}, bar {tol:.2e}")
    assert abs(got - gn) <= 0.5 * tol * gn, (got, gn, tol)          # a square root halves the relative error of the sum of squares
    for k in ref.masters:
        assert relerr(clip.masters[k], ref.masters[k]) < 1e-5, (k, relerr(clip.masters[k], ref.masters[k]))
        assert relerr(clip.opt.m[k], ref.opt.m[k]) < 1e-5 and relerr(clip.opt.v[k], ref.opt.v[k]) < 1e-5, k
    # the clip did act: the first moments are half of the unclipped step's
    probe.optimizer_step()
    k = max(probe.masters, key=lambda k: probe.masters[k].numel())
    assert abs(relerr(clip.opt.m[k], probe.opt.m[k]) - 0.5) < 1e-3


def test_clipped_depth_step_vs_oracle_autograd_clip_and_adamw():
    """One tri-modal depth step on the tiny golden model against the oracle on the CPU: autograd, clip_grad_norm_ at half the
    oracle's own gradient norm, torch.optim.AdamW.  Tolerances: those of the unclipped comparison of this configuration
    (test_hip_train.py::test_tri_modal_step_matches_reference_step: loss 2e-2 absolute, gradients 6e-2 relative per tensor) -
    applied to the norm and to what carries the CLIPPED gradient after the step: AdamW's first moment (1 - beta1) * coef * g at
    6e-2, its second moment (1 - beta2) * (coef * g)^2 at twice that (a square doubles a relative error).  The masters are
    checked to be finite and moved, not compared: the first Adam step is lr * g / (|g| + eps), the sign of the gradient, so an
    element whose near-zero gradient differs in sign is a full-size difference that says nothing about the clip."""
    import vitlens_oracle as O
    from vitlens_hip import engine as E, step as ST
    from vitlens_hip.train import AdamW
    sd, ins, outs, grads, meta = split(load_npz("tiny_depth.npz"))
    tower, text, lens = specs_from_meta(meta)
    tc = E.TowerCfg(width=tower.width, layers=tower.layers, heads=tower.heads, patch=tower.patch, image_size=tower.image_size,
                    embed_dim=tower.embed_dim)
    xc = E.TextCfg(context_length=text.context_length, vocab_size=text.vocab_size, width=text.width, heads=text.heads,
                   layers=text.layers, embed_dim=text.embed_dim)
    sdc = {k: v.clone().float() for k, v in sd.items()}
    train = ["logit_scale", "visual.visual_adapter.conv1.weight", "visual.visual_adapter.pos_emb"] + \
            [k for k in sdc if k.startswith("visual.transformer.resblocks.")]
    for k in train:
        sdc[k].requires_grad_(True)
    with torch.no_grad():
        fi = O.encode_image(sdc, ins["image"], tower, normalize=True); ft = O.encode_text(sdc, ins["text"], text, normalize=True)
    fv = O.encode_visual(sdc, ins["visual_x"], tower, lens, normalize=True)
    loss_ref = O.tri_clip_loss(fi, ft, fv, sdc["logit_scale"].exp())
    loss_ref.backward()
    gn_ref = math.sqrt(sum(float(sdc[k].grad.double().pow(2).sum()) for k in train))
    c = 0.5 * gn_ref
    dec = [sdc[k] for k in train if AdamW.decays(k, sdc[k])]
    nod = [sdc[k] for k in train if not AdamW.decays(k, sdc[k])]
    opt = torch.optim.AdamW([{"params": dec, "weight_decay": 0.2}, {"params": nod, "weight_decay": 0.0}], lr=1e-3,
                            betas=(0.9, 0.98), eps=1e-6)
    total = torch.nn.utils.clip_grad_norm_([sdc[k] for k in train], c, norm_type=2.0)
    opt.step()

    st = ST.TriModalDepthStep(sd, tc, xc, "cuda", micro_batch=2, unlock_first_n=tc.layers, lr=1e-3, grad_clip_norm=c)
    _master0 = {k: v.detach().cpu().reshape(-1).clone() for k, v in st.masters.items()}
    loss = st.step(ins["image"].cuda(), ins["text"].cuda(), ins["visual_x"].cuda())
    assert abs(float(loss) - float(loss_ref.detach())) < 2e-2, (float(loss), float(loss_ref.detach()))
    got = float(st.last_grad_norm)
    print(f"oracle: norm {float(total):.6e}, step {got:.6e}")
    assert abs(got - float(total)) < 6e-2 * float(total), (got, float(total))
    n, bad = 0, {}
    for name, m in st.masters.items():
        key = "visual.visual_adapter.conv1.weight" if name.endswith("conv1.weight_gemm") else name
        stt = opt.state[sdc[key]]
        mom, rmom, sq, rsq = st.opt.m[name], stt["exp_avg"], st.opt.v[name], stt["exp_avg_sq"]
        if name.endswith("conv1.weight_gemm"):
            rmom = rmom.reshape(m.shape[0], -1); rsq = rsq.reshape(m.shape[0], -1)
            mom = mom[:, :rmom.shape[1]]; sq = sq[:, :rsq.shape[1]]
        e_m, e_v = relerr(mom, rmom.reshape(mom.shape)), relerr(sq, rsq.reshape(sq.shape))
        if not (e_m < 6e-2 and e_v < 12e-2):
            bad[name] = (e_m, e_v)
        assert bool(torch.isfinite(m).all()) and not torch.equal(m.cpu().reshape(-1), _master0[name]), name
        n += 1
    assert not bad, bad
    assert n == 12 * tc.layers + 3 == len(train)
