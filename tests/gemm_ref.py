"""fp64 reference of the bf16 NT GEMM's epilogues and per-element error bounds that are derived, not tuned.  Nothing here needs a
GPU: the tensors stay on whatever device the operands live on (tests/test_gemm_ref_host.py runs it on the CPU,
tests/test_hip_gemm_families.py on the device).

Reference, from the bf16 operands as the kernel sees them (a [M, K], w [N, K], bias fp32 [N] or None):
    P = a.double() @ w.double().T        S = |a|.double() @ |w|.double().T        z = alpha * P + bias
and each epilogue restated in fp64 with exact erf / exp (EPILOGUES below names them).

Bounds, per element:
  * accumulation budget  B = (K + 2) u (|alpha| S + |bias|),  u = 2^-23.  K products of two bf16 values are exact in fp32; summing
    them in ANY order (MFMA-internal, across k-steps, across the eight waves of the tail kernel) errs by at most (K - 1) 2^-24 S
    to first order, the multiplication by alpha and the bias addition are one fp32 rounding each: (K + 1) 2^-24 (|alpha| S +
    |bias|).  Doubled (u = 2^-23, K + 2) because the matrix instruction's internal rounding is not documented; the doubling also
    absorbs the second-order terms ((1 + U) on the budget under a bf16 rounding).  A CPU fp32 matmul uses at most a few percent.
  * one bf16 rounding (round to nearest even): U |value|, U = 2^-8.  Exact, and reached to 0.99.
  * one fp32 rounding of a sum or product that is formed from inexact parts: u |value| (again twice 2^-24).
  * approximated transcendentals (vl_common.h: Phi to 4e-7 absolute, v_exp_f32 / v_rcp_f32 for QuickGELU): the absolute allowance
    ACT_ABS = 1e-6 the suite already holds the kernels to (test_gelu_erf_accuracy, test_hip_qgelu.py), times max(1, |x|) because
    gelu = x Phi(x), gelu' = Phi + x phi, qgelu = x s and qgelu' = s + 1.702 x s (1 - s) all multiply the approximated factor by x.
  * Lipschitz constants carry the budget through an activation applied to the fp32 value:
        gelu'  = Phi(x) + x phi(x) has its extrema where gelu'' = phi(x) (2 - x^2) = 0, x = +-sqrt 2: 1.1290 and -0.1290  -> L_GELU = 1.13
        gelu'' = phi(x) (2 - x^2): largest at x = 0, 2 phi(0) = 0.7979                                                   -> L_DGELU = 0.80
        qgelu' = s + c x s (1 - s), c = 1.702: maximum 1.0998 (x = 1.41), minimum -0.0998                                -> L_QGELU = 1.10
        qgelu'' = c s (1 - s) (2 + c x (1 - 2 s)): largest at x = 0, c / 2 = 0.851                                      -> L_DQGELU = 0.86
    (tests/test_gemm_ref_host.py checks each against a dense fp64 grid.)

Two forms of bound, chosen per (kernel family, epilogue) by `rounded` (the table is in tests/test_hip_gemm_families.py):
  rounded = False  the activation / add / product acts on the fp32 value v (|v - z| <= B), then one bf16 rounding:
                   |out - f(z)| <= U |f(z)| + L_f B + A.
  rounded = True   it acts on the bf16-ROUNDED pre-activation.  `pre` is what the same kernel stores for the plain EPI_BF16
                   epilogue on the same operands (or out2 where the epilogue writes the pre-activation); pre is checked against
                   z by U |z| + B, then out (and the derivative d) against f(pre.double()) by U |f| + A: no room for a second ulp.
ACT_GELU_DSAVE / ACT_QGELU_DSAVE act on the rounded pair in every kernel."""
import math

import torch

U_BF16 = 2.0 ** -8
U_F32 = 2.0 ** -23
ACT_ABS = 1e-6
L_GELU, L_DGELU, L_QGELU, L_DQGELU = 1.13, 0.80, 1.10, 0.86

EPILOGUES = ("none", "gelu", "relu", "qgelu", "gelu_out2", "gelu_dsave", "qgelu_dsave", "f32", "res_f32", "res_bf16",
             "res_bf16_relu", "dgelu", "dgelu_saved", "geglu", "geglu_out2", "dgeglu")
# epilogues whose bound has the two forms; every other one has a single form whatever the store path
# (GEGLU and DGEGLU take the rounded form in vl_gemm_park.hip only, whose slab epilogue multiplies the bf16 halves)
TWO_FORMS = ("gelu_out2", "res_bf16", "res_bf16_relu", "dgelu", "dgelu_saved", "geglu", "geglu_out2", "dgeglu")


# ---- fp64 restatements -----------------------------------------------------------------------------------------------------------
def gelu(x):
    """x Phi(x) with Phi = erfc(-x / sqrt 2) / 2: no cancellation at the negative end."""
    x = x.double()
    return 0.5 * x * torch.special.erfc(-x * math.sqrt(0.5))


def gelu_grad(x):
    """Phi(x) + x phi(x)."""
    x = x.double()
    return 0.5 * torch.special.erfc(-x * math.sqrt(0.5)) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


def qgelu(x):
    x = x.double()
    return x * torch.sigmoid(1.702 * x)


def qgelu_grad(x):
    x = x.double()
    s = torch.sigmoid(1.702 * x)
    return s + 1.702 * x * s * (1.0 - s)


def relu(x):
    return x.double().clamp_min(0.0)


def act_allow(x):
    """Absolute allowance of an approximated activation or derivative evaluated at x."""
    return ACT_ABS * x.double().abs().clamp_min(1.0)


def expand_res(res, res_div, M, m_off=0):
    """Row m of the output reads row (m + m_off) // res_div of a row-broadcast residual."""
    if res_div == 1 and m_off == 0:
        return res[:M]
    idx = (torch.arange(M, device=res.device) + m_off) // res_div
    return res[idx]


class Ref:
    """P, S, z and the accumulation budget B of one problem, in fp64 on the operands' device."""

    def __init__(self, a, w, bias=None, alpha=1.0):
        ad, wd = a.double(), w.double()
        self.K = a.shape[1]
        self.alpha = float(alpha)
        P = ad @ wd.t()
        S = ad.abs() @ wd.abs().t()
        b = torch.zeros(w.shape[0], dtype=torch.float64, device=a.device) if bias is None else bias.double()
        self.z = self.alpha * P + b
        self.B = (self.K + 2) * U_F32 * (abs(self.alpha) * S + b.abs())

    def rows(self, r0, r1):
        """The same reference restricted to output rows r0:r1 (a row-split launch checks each part with its own form)."""
        o = object.__new__(Ref)
        o.K, o.alpha, o.z, o.B = self.K, self.alpha, self.z[r0:r1], self.B[r0:r1]
        return o


def _need(outs, *keys):
    for k in keys:
        if outs.get(k) is None:
            raise KeyError(f"checks: '{k}' missing")
    return [outs[k] for k in keys]


def checks(ref, epi, outs, rounded=False, res=None):
    """[(label, got, want, bound)] for one epilogue.  outs: 'out', and where the epilogue has them 'out2' and 'pre' (the same
    kernel's plain EPI_BF16 output, needed by the rounded forms).  res: the second operand as the kernel indexes it, already
    expanded to the output's rows (expand_res): residual, saved pre-activation / derivative, or DGEGLU's interleaved h."""
    z, B = ref.z, ref.B
    out = _need(outs, "out")[0]
    U, u = U_BF16, U_F32

    def pre_then(pre, pairs, label="pre"):
        """rounded form: pre against z, then each (label, got, f(pre), allowance)"""
        pd = pre.double()
        lst = [(label, pre, z, U * z.abs() + B)]
        for label, got, f, allow in pairs:
            lst.append((label, got, f, U * f.abs() + allow))
        return lst, pd

    if epi == "none":
        return [("out", out, z, U * z.abs() + B)]
    if epi == "f32":
        return [("out", out, z, B.clone())]
    if epi == "relu":
        f = relu(z)
        return [("out", out, f, U * f + B)]
    if epi == "gelu":
        f = gelu(z)
        return [("out", out, f, U * f.abs() + L_GELU * B + act_allow(z))]
    if epi == "qgelu":
        f = qgelu(z)
        return [("out", out, f, U * f.abs() + L_QGELU * B + act_allow(z))]
    if epi == "gelu_out2":
        out2 = _need(outs, "out2")[0]
        if rounded:
            pd = out2.double()
            return pre_then(out2, [("out", out, gelu(pd), act_allow(pd))], "out2")[0]
        f = gelu(z)
        return [("out2", out2, z, U * z.abs() + B), ("out", out, f, U * f.abs() + L_GELU * B + act_allow(z))]
    if epi in ("gelu_dsave", "qgelu_dsave"):
        out2, pre = _need(outs, "out2", "pre")
        pd = pre.double()
        f, g = (gelu, gelu_grad) if epi == "gelu_dsave" else (qgelu, qgelu_grad)
        return pre_then(pre, [("out", out, f(pd), act_allow(pd)), ("out2", out2, g(pd), act_allow(pd))])[0]
    if epi == "res_f32":
        f = z + res.double()
        return [("out", out, f, B + u * f.abs())]
    if epi in ("res_bf16", "res_bf16_relu"):
        post = relu if epi == "res_bf16_relu" else (lambda t: t)
        if rounded:
            pre = _need(outs, "pre")[0]
            s = pre.double() + res.double()
            return pre_then(pre, [("out", out, post(s), u * s.abs())])[0]
        s = z + res.double()
        f = post(s)
        return [("out", out, f, U * f.abs() + B + u * s.abs())]
    if epi in ("dgelu", "dgelu_saved"):
        rd = res.double()
        g, ga = (rd, torch.zeros_like(rd)) if epi == "dgelu_saved" else (gelu_grad(rd), act_allow(rd))
        if rounded:
            pre = _need(outs, "pre")[0]
            pd = pre.double()
            f = pd * g
            # saved: the product of two bf16 values is exact in fp32, one rounding and nothing else
            return pre_then(pre, [("out", out, f, pd.abs() * ga + (0.0 if epi == "dgelu_saved" else u) * f.abs())])[0]
        f = z * g
        return [("out", out, f, U * f.abs() + (g.abs() + ga) * B + z.abs() * ga + u * f.abs())]
    if epi in ("geglu", "geglu_out2") and rounded:
        pre = _need(outs, "out2" if epi == "geglu_out2" else "pre")[0]
        pd = pre.double()
        pa, pg = pd[:, 0::2], pd[:, 1::2]
        f = pa * gelu(pg)
        return pre_then(pre, [("out", out, f, pa.abs() * act_allow(pg) + u * f.abs())], "out2" if epi == "geglu_out2" else "pre")[0]
    if epi in ("geglu", "geglu_out2"):
        za, zg, Ba, Bg = z[:, 0::2], z[:, 1::2], B[:, 0::2], B[:, 1::2]
        gg = gelu(zg)
        eg = L_GELU * Bg + act_allow(zg)                    # error of gelu(gate) as the kernel evaluates it
        f = za * gg
        lst = [("out", out, f, U * f.abs() + Ba * (gg.abs() + eg) + za.abs() * eg + u * f.abs())]
        if epi == "geglu_out2":
            lst.insert(0, ("out2", _need(outs, "out2")[0], z, U * z.abs() + B))
        return lst
    if epi == "dgeglu":
        hd = res.double()
        ha, hg = hd[:, 0::2], hd[:, 1::2]
        gg, gd, al = gelu(hg), gelu_grad(hg), act_allow(hg)
        if rounded:
            pre = _need(outs, "pre")[0]
            pd = pre.double()
            f = torch.empty_like(hd)
            allow = torch.empty_like(hd)
            f[:, 0::2] = pd * gg
            allow[:, 0::2] = pd.abs() * al + u * f[:, 0::2].abs()
            f[:, 1::2] = pd * ha * gd
            allow[:, 1::2] = (pd * ha).abs() * al + 2 * u * f[:, 1::2].abs()
            return pre_then(pre, [("out", out, f, allow)])[0]
        f = torch.empty_like(hd)
        bound = torch.empty_like(hd)
        f[:, 0::2] = z * gg
        bound[:, 0::2] = U * f[:, 0::2].abs() + B * (gg.abs() + al) + z.abs() * al + u * f[:, 0::2].abs()
        f[:, 1::2] = z * ha * gd
        bound[:, 1::2] = U * f[:, 1::2].abs() + ha.abs() * (B * (gd.abs() + al) + z.abs() * al) + 2 * u * f[:, 1::2].abs()
        return [("out", out, f, bound)]
    raise ValueError(f"unknown epilogue {epi}")


def violations(got, want, bound):
    """(mask of the elements beyond the bound, worst error / bound).  A NaN in got is a violation."""
    err = (got.double() - want).abs()
    bad = ~(err <= bound)
    r = torch.where(err == 0, torch.zeros_like(err), err / bound)         # (an exact result under a zero bound is ratio 0, not 0 / 0)
    ratio = float(r.nan_to_num(nan=float("inf")).max()) if err.numel() else 0.0
    return bad, ratio


def count(chk):
    """{label: (number of violations, worst error / bound)}"""
    res = {}
    for label, got, want, bound in chk:
        bad, ratio = violations(got, want, bound)
        res[label] = (int(bad.sum()), ratio)
    return res


def assert_within(chk, what="", tile=None, row0=0):
    """Every element of every check inside its bound; the failure names the first offender (and its tile, when the kernel's tile
    size is given).  Returns {label: worst error / bound}."""
    worst = {}
    for label, got, want, bound in chk:
        bad, ratio = violations(got, want, bound)
        n = int(bad.sum())
        if n:
            i, j = (int(t[0]) for t in torch.nonzero(bad, as_tuple=True))
            where = f"first at row {i + row0}, col {j}"
            if tile:
                where += f" (tile {(i + row0) // tile[0]}, {j // tile[1]} of {tile[0]}x{tile[1]})"
            raise AssertionError(f"{what} {label}: {n} of {bad.numel()} elements beyond the bound, {where}: got {float(got[i, j])!r}, "
                                 f"want {float(want[i, j])!r}, bound {float(bound[i, j]):.3e}; worst error / bound {ratio:.3g}")
        worst[label] = ratio
    return worst
