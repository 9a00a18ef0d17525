"""CPU: the checker of tests/gemm_ref.py checked.  (1) Its fp64 restatements against torch's own fp64 gelu, autograd and
x * sigmoid(1.702 x), and its Lipschitz constants against a dense grid.  (2) A CPU emulation of every (epilogue, rounding form) -
an fp32 matmul of the bf16 operands, torch's bf16 rounding at the stated points - stays inside the bounds with ZERO violations
at every shape tests/test_hip_gemm_families.py uses that the CPU can afford: the bounds are honest, nothing is masked.  (3) Planted
errors are caught, element for element."""
import math

import pytest
import torch

import gemm_ref as R

SD_PRE = 4.0
# (M, N, K) of tests/test_hip_gemm_families.py sections a and d (b and c are 19 M - 26 M elements: device only)
SHAPES = [(300, 196, 192), (321, 392, 64), (97, 264, 448), (97, 264, 576), (256, 256, 512), (256, 128, 128), (256, 384, 128)]


def rnd(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def operands(M, N, K, seed=0, bias=True):
    a = rnd(M, K, seed=seed + 1).bfloat16()
    w = rnd(N, K, seed=seed + 2, scale=SD_PRE * K ** -0.5).bfloat16()
    b = rnd(N, seed=seed + 3) if bias else None
    return a, w, b


def bf(x):
    return x.bfloat16()


def gelu32(x):
    return torch.nn.functional.gelu(x.float())


def gelu_grad32(x):
    x = x.float()
    return 0.5 * (1 + torch.erf(x * math.sqrt(0.5))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2 * math.pi)


def qgelu32(x):
    x = x.float()
    return x * torch.sigmoid(1.702 * x)


def qgelu_grad32(x):
    x = x.float()
    s = torch.sigmoid(1.702 * x)
    return s + 1.702 * x * s * (1 - s)


def emulate(epi, rounded, a, w, bias, alpha=1.0, res=None):
    """What a correct kernel returns, in fp32 torch arithmetic: {'out', 'out2', 'pre'}.  res: already expanded to the output's rows."""
    v = (a.float() @ w.float().t()) * alpha
    if bias is not None:
        v = v + bias
    pre = bf(v)
    o = {"pre": pre}
    if epi == "none":
        o["out"] = pre
    elif epi == "f32":
        o["out"] = v
    elif epi == "relu":
        o["out"] = bf(v.clamp_min(0))
    elif epi == "gelu":
        o["out"] = bf(gelu32(v))
    elif epi == "qgelu":
        o["out"] = bf(qgelu32(v))
    elif epi == "gelu_out2":
        o["out2"] = pre
        o["out"] = bf(gelu32(pre if rounded else v))
    elif epi == "gelu_dsave":
        o["out"], o["out2"] = bf(gelu32(pre)), bf(gelu_grad32(pre))
    elif epi == "qgelu_dsave":
        o["out"], o["out2"] = bf(qgelu32(pre)), bf(qgelu_grad32(pre))
    elif epi == "res_f32":
        o["out"] = v + res
    elif epi in ("res_bf16", "res_bf16_relu"):
        s = (pre.float() if rounded else v) + res.float()
        o["out"] = bf(s.clamp_min(0) if epi == "res_bf16_relu" else s)
    elif epi in ("dgelu", "dgelu_saved"):
        g = res.float() if epi == "dgelu_saved" else gelu_grad32(res)
        o["out"] = bf((pre.float() if rounded else v) * g)
    elif epi in ("geglu", "geglu_out2"):
        x = pre.float() if rounded else v
        o["out"] = bf(x[:, 0::2] * gelu32(x[:, 1::2]))
        if epi == "geglu_out2":
            o["out2"] = pre
    elif epi == "dgeglu":
        h = res.float()
        out = torch.empty_like(h)
        x = pre.float() if rounded else v
        out[:, 0::2] = x * gelu32(h[:, 1::2])
        out[:, 1::2] = x * h[:, 0::2] * gelu_grad32(h[:, 1::2])
        o["out"] = bf(out)
    else:
        raise ValueError(epi)
    return o


def second_operand(epi, M, N, res_div=1, seed=50):
    """The second operand of an epilogue, as the caller allocates it (None where the epilogue has none)."""
    if epi == "res_f32":
        return rnd(M, N, seed=seed)
    if epi in ("res_bf16", "res_bf16_relu"):
        return rnd((M + res_div - 1) // res_div, N, seed=seed, scale=2.0).bfloat16()
    if epi == "dgelu":
        return rnd(M, N, seed=seed, scale=1.5).bfloat16()             # a pre-activation
    if epi == "dgelu_saved":
        return R.gelu_grad(rnd(M, N, seed=seed, scale=1.5)).bfloat16()   # a derivative
    if epi == "dgeglu":
        return rnd(M, 2 * N, seed=seed, scale=1.5).bfloat16()
    return None


# ---- (1) the restatements and the constants ---------------------------------------------------------------------------------------
def test_restatements_agree_with_torch_fp64():
    x = torch.cat([torch.linspace(-40, 40, 200001, dtype=torch.float64), rnd(1000, seed=1).double() * 4])
    assert float((R.gelu(x) - torch.nn.functional.gelu(x)).abs().max()) < 1e-14
    xg = x.clone().requires_grad_(True)
    torch.nn.functional.gelu(xg).sum().backward()
    assert float((R.gelu_grad(x) - xg.grad).abs().max()) < 1e-14
    assert float((R.qgelu(x) - x * torch.sigmoid(1.702 * x)).abs().max()) < 1e-14
    xq = x.clone().requires_grad_(True)
    (xq * torch.sigmoid(1.702 * xq)).sum().backward()
    assert float((R.qgelu_grad(x) - xq.grad).abs().max()) < 1e-13
    # the negative end keeps its relative accuracy (0.5 x (1 + erf) would cancel): gelu(-10) = -10 Phi(-10) = -7.6198530241605e-23
    assert abs(float(R.gelu(torch.tensor([-10.0]))) / -7.6198530241605e-23 - 1) < 1e-10
    assert torch.equal(R.relu(torch.tensor([-1.0, 0.0, 2.0])), torch.tensor([0.0, 0.0, 2.0], dtype=torch.float64))


def test_lipschitz_constants_on_a_dense_grid():
    x = torch.linspace(-30, 30, 6_000_001, dtype=torch.float64)
    h = float(x[1] - x[0])
    for f, g, L1, L2 in ((R.gelu, R.gelu_grad, R.L_GELU, R.L_DGELU), (R.qgelu, R.qgelu_grad, R.L_QGELU, R.L_DQGELU)):
        d1 = float(g(x).abs().max())
        d2 = float((g(x).diff() / h).abs().max())
        slope = float((f(x).diff() / h).abs().max())
        print(f"{f.__name__}: max |f'| {d1:.5f} (finite differences {slope:.5f}) <= {L1}; max |f''| {d2:.5f} <= {L2}")
        assert max(d1, slope) <= L1 and L1 - d1 < 0.01
        assert d2 <= L2 and L2 - d2 < 0.01


def test_expand_res_follows_the_kernel_index():
    res = torch.arange(5)[:, None].expand(5, 2)
    assert R.expand_res(res, 3, 13)[:, 0].tolist() == [0, 0, 0, 1, 1, 1, 2, 2, 2, 3, 3, 3, 4]
    assert R.expand_res(res, 3, 4, m_off=7)[:, 0].tolist() == [2, 2, 3, 3]
    assert R.expand_res(res, 1, 4).shape == (4, 2)


# ---- (2) zero violations of the emulation ------------------------------------------------------------------------------------------
def _forms(epi):
    return (False, True) if epi in R.TWO_FORMS else (False,)


@pytest.mark.parametrize("M,N,K", SHAPES)
def test_emulation_stays_inside_every_bound(M, N, K):
    a, w, bias = operands(M, N, K, seed=M + K)
    worst = {}
    for alpha, b in ((1.0, bias), (0.5, bias), (0.5, None)):
        ref = R.Ref(a, w, b, alpha)
        if b is not None and alpha == 1.0:
            assert float(ref.z.min()) < -11 and float(ref.z.max()) > 11              # both saturated ends
        for epi in R.EPILOGUES:
            for res_div in ((1, 3, 32) if epi.startswith("res_bf16") else (1,)):
                r0 = second_operand(epi, M, N, res_div)
                res = None if r0 is None else R.expand_res(r0, res_div, M)
                for rounded in _forms(epi):
                    outs = emulate(epi, rounded, a, w, b, alpha, res)
                    for label, (n, ratio) in R.count(R.checks(ref, epi, outs, rounded, res)).items():
                        key = (epi, rounded, label)
                        worst[key] = max(worst.get(key, 0.0), ratio)
                        assert n == 0, (key, alpha, res_div, n, ratio)
    for key, ratio in sorted(worst.items()):
        print(f"({M}, {N}, {K}) {key}: worst error / bound {ratio:.3f}")
    # the bf16 rounding term is reached, the accumulation budget is mostly unused
    assert worst[("none", False, "out")] > 0.8 and worst[("f32", False, "out")] < 0.2


# ---- (3) planted errors --------------------------------------------------------------------------------------------------------------
M0, N0, K0 = 321, 392, 64


def _clean(epi, rounded=False, alpha=1.0, res_div=1, bias=True):
    a, w, b = operands(M0, N0, K0, seed=7, bias=bias)
    ref = R.Ref(a, w, b, alpha)
    r0 = second_operand(epi, M0, N0, res_div)
    res = None if r0 is None else R.expand_res(r0, res_div, M0)
    outs = emulate(epi, rounded, a, w, b, alpha, res)
    assert all(n == 0 for n, _ in R.count(R.checks(ref, epi, outs, rounded, res)).values())
    return a, w, b, ref, r0, res, outs


def _planted(ref, epi, outs, planted, key, rounded=False, res=None):
    """Violations of `planted` (a copy of outs with outs[key] replaced) in the check of that key.  Asserts what must hold of any
    plant: every element moved by more than twice its bound is flagged, no element left as it was is flagged."""
    chk = {label: (got, want, bound) for label, got, want, bound in R.checks(ref, epi, planted, rounded, res)}
    got, want, bound = chk[key]
    bad, _ = R.violations(got, want, bound)
    moved = got.double() - outs[key].double()
    assert bool(bad[moved.abs() > 2 * bound].all())
    assert not bool(bad[moved == 0].any())
    return bad


@pytest.mark.parametrize("epi", ["none", "gelu", "f32"])
def test_plant_last_rows_last_columns_copied_from_the_row_above(epi):
    a, w, b, ref, _, _, outs = _clean(epi)
    p = dict(outs, out=outs["out"].clone())
    p["out"][-1, -8:] = p["out"][-2, -8:]
    bad = _planted(ref, epi, outs, p, "out")
    if epi != "gelu":        # (under GELU two negative pre-activations can both give ~0: 'exactly 8' holds for the other two)
        assert int(bad.sum()) == 8 and bool(bad[-1, -8:].all())
    else:
        assert 0 < int(bad.sum()) <= 8 and int(bad[-1, -8:].sum()) == int(bad.sum())
    # what the whole-tensor error makes of it: eight elements in 125832 (whether it passes 4e-3 depends on the eight values)
    if epi == "none":
        e0 = float((outs["out"].double() - ref.z).norm() / ref.z.norm())
        e = float((p["out"].double() - ref.z).norm() / ref.z.norm())
        print(f"whole-tensor relative error: clean {e0:.2e}, with the plant {e:.2e}")


def test_plant_bias_dropped_on_the_last_columns():
    a, w, b, ref, _, _, outs = _clean("f32")
    assert float(b[-4:].abs().min()) > 1e-2
    p = dict(outs, out=outs["out"].clone())
    p["out"][:, -4:] -= b[-4:]
    bad = _planted(ref, "f32", outs, p, "out")
    assert int(bad.sum()) == 4 * M0 and bool(bad[:, -4:].all())
    # through a bf16 rounding too: |bias| > 1e-2 against U |z| needs |z| < 2.56, so not every row - but only those columns
    _, _, _, ref, _, _, outs = _clean("none")
    p = dict(outs, out=(outs["pre"].float().clone()))
    v = (a.float() @ w.float().t()) + b
    v[:, -4:] -= b[-4:]
    p["out"] = v.bfloat16()
    bad = _planted(ref, "none", outs, p, "out")
    assert int(bad[:, :-4].sum()) == 0 and int(bad.sum()) > 3 * M0


def test_plant_alpha_dropped():
    a, w, b, ref, _, _, outs = _clean("f32", alpha=0.5)
    p = dict(outs, out=(a.float() @ w.float().t()) + b)
    bad = _planted(ref, "f32", outs, p, "out")
    # every element but the few whose product is within the budget of zero
    assert int(bad.sum()) > 0.999 * M0 * N0
    a, w, b, ref, _, _, outs = _clean("none", alpha=0.5)
    p = dict(outs, out=((a.float() @ w.float().t()) + b).bfloat16())
    assert int(_planted(ref, "none", outs, p, "out").sum()) > 0.98 * M0 * N0


@pytest.mark.parametrize("epi", ["none", "gelu", "res_bf16", "dgelu_saved", "geglu"])
def test_plant_one_element_off_by_two_bf16_ulps(epi):
    a, w, b, ref, r0, res, outs = _clean(epi)
    o = outs["out"].clone()
    i, j = 200, 17
    assert abs(float(o[i, j])) > 1e-3
    o.view(torch.int16)[i, j] += 2
    p = dict(outs, out=o)
    bad = _planted(ref, epi, outs, p, "out", res=res)
    assert int(bad.sum()) == 1 and bool(bad[i, j])
    # one ulp is what a correct rounding of a slightly different fp32 value may give: not flagged as a rule, and never required
    o1 = outs["out"].clone()
    o1.view(torch.int16)[i, j] += 1
    assert int(_planted(ref, epi, outs, dict(outs, out=o1), "out", res=res).sum()) <= 1


@pytest.mark.parametrize("epi,rounded", [("gelu_out2", False), ("gelu_out2", True), ("geglu_out2", False)])
def test_plant_out2_holds_the_activation(epi, rounded):
    a, w, b, ref, _, _, outs = _clean(epi, rounded)
    act = outs["out"] if epi == "gelu_out2" else R.gelu(ref.z).bfloat16()
    p = dict(outs, out2=act.clone())
    bad = _planted(ref, epi, outs, p, "out2", rounded)
    # gelu(z) differs from z by more than a bf16 ulp of z below z ~ 2.9: ~3/4 of N(0, 4^2)
    assert int(bad.sum()) > 0.7 * M0 * N0


def test_plant_res_div_indexed_by_remainder():
    """m % G instead of m // G (G = 3: with G = 32 the remainder would index past the 11 residual rows of 321 output rows)."""
    G = 3
    m = torch.arange(M0)
    same = (m % G) == (m // G)                            # rows 0, 4 and 8 read the right residual row by either index
    assert int(same.sum()) == 3
    for rounded in (False, True):
        a, w, b, ref, r0, res, outs = _clean("res_bf16", rounded, res_div=G)
        p = emulate("res_bf16", rounded, a, w, b, 1.0, r0[m % G])
        bad = _planted(ref, "res_bf16", outs, dict(outs, out=p["out"]), "out", rounded, res)
        assert int(bad[same].sum()) == 0
        # (two residual values closer than the bound of the sum are the same value to any checker)
        assert int(bad[~same].sum()) > 0.97 * (M0 - 3) * N0


def test_plant_geglu_pair_swapped():
    a, w, b, ref, _, _, outs = _clean("geglu")
    v = (a.float() @ w.float().t()) + b
    p = dict(outs, out=(v[:, 1::2] * gelu32(v[:, 0::2])).bfloat16())
    bad = _planted(ref, "geglu", outs, p, "out")
    # (where both halves of a pair are far on the negative side either order gives ~0)
    assert int(bad.sum()) > 0.85 * M0 * (N0 // 2)


def test_which_rounding_forms_the_bounds_tell_apart():
    """The fp32-form emulation against the rounded-form bound and the reverse, for the epilogues that have both.  Printed and
    asserted: what the GPU test's rounding table can get wrong without a failure, and what it cannot."""
    told = {}
    for epi in R.TWO_FORMS:
        for emu_rounded in (False, True):
            a, w, b, ref, r0, res, outs = _clean(epi, emu_rounded)
            n = sum(c for c, _ in R.count(R.checks(ref, epi, outs, not emu_rounded, res)).values())
            told[(epi, emu_rounded)] = n
            print(f"{epi}: {'rounded' if emu_rounded else 'fp32'}-form arithmetic against the "
                  f"{'fp32' if emu_rounded else 'rounded'}-form bound: {n} of {M0 * N0} elements flagged")
    # a kernel that rounds once (fp32 form) is always caught by the rounded-form bound: its output is a correctly rounded f(v),
    # not f(pre), and differs from the latter by up to L U |z|
    for epi in R.TWO_FORMS:
        assert told[(epi, False)] > 100, (epi, told)
    # a kernel that rounds twice is caught by the fp32-form bound as well (the second rounding does not fit under one U |f|)
    for epi in R.TWO_FORMS:
        assert told[(epi, True)] > 100, (epi, told)
