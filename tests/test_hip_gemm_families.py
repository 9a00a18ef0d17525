"""GPU: every kernel of vl_gemm.hip x every epilogue against the fp64 reference of tests/gemm_ref.py, element by element, with
bounds that are derived there (accumulation budget, one bf16 rounding, the 1e-6 activation allowance) and shown honest on the CPU
by tests/test_gemm_ref_host.py.  What a whole-tensor error of 4e-3 lets through - eight wrong elements of a ragged tile, a bias
dropped on the last four columns - fails here.

Every output, out2 and in-place residual is a view of a NaN-filled wider allocation (row stride N + pad, guard rows after row M):
after each launch everything outside the view is still NaN and everything inside is finite.  The operands are views too (lda, ldw
> K), with NaN in their padding columns and in the rows after M / N: the kernels clamp their row loads, so a NaN in an output is
an over-read that was used.  Pre-activations have a standard deviation of about 4 (both saturated ends of the activations occur).

Which form of bound applies (gemm_ref's `rounded`), read from vl_gemm_epi.h and the three store paths of vl_gemm.hip:

  store path                                     kernels                                            arithmetic
  store_tile and the fp32 LDS transpose          cfg 0-3, 11, 12, 9: every epilogue;                everything on the fp32 value, one rounding
  (both end in epi_direct4)                      cfg 5, 6: N % 8 or ldo % 8 nonzero, fp32           (GELU with out2 too: out2 = bf16(v), out =
                                                 outputs, GEGLU, DGEGLU                             bf16(gelu(v))); only GELU_DSAVE / QGELU_DSAVE
                                                                                                    act on the rounded pair
  store_tile_lds16                               cfg 5, 6: bf16 outputs, N % 8 == 0, ldo % 8 == 0   alpha, bias, GELU without out2, ReLU, QuickGELU
                                                                                                    before the pack; GELU with out2, the _DSAVE
                                                                                                    codes, RES_BF16 (ReLU after the add), DGELU
                                                                                                    on the rounded values
  vl_gemm_park.hip (cfg 8), vl_gemm_pp.hip (10)  whole tiles                                        as store_tile_lds16; park's GEGLU / DGEGLU
                                                                                                    slabs multiply the bf16-rounded halves too
The two forms are told apart by the bounds in both directions (test_which_rounding_forms_the_bounds_tell_apart), so this table
is itself under test.

Coverage: (cfg, epilogue) pairs that dispatch<EPI> can launch from vl_gemm.hip, each with a ragged row tile and a ragged column tile:
  cfg 0 1 2 3 11 12 9 5 6  x  none, GELU, ReLU, QuickGELU, GELU + out2, GELU_DSAVE, QGELU_DSAVE, F32, RES_F32 (in / out of place),
  RES_BF16 (in / out of place, res_div 1 / 3 / 32, + ReLU), DGELU (recomputed, saved), GEGLU (+ out2), DGEGLU
      -> test_every_kernel_every_epilogue[cfg-shape], all four shapes (every epilogue runs on every cfg at every shape);
  cfg 5, 6: store_tile_lds16 -> shape (321, 392, 64) pad 0 and (97, 264, *) pad 0; fp32 transpose -> (300, 196, 192) and pad 4;
            store_tile -> GEGLU / DGEGLU at every shape; nk = 1 with several tiles per workgroup -> test_round1_persistent_many_tiles;
  leftover launches of run_gemm (cfg 9, 11, 1 behind park / ping-pong / round-1 mains) -> test_auto_dispatch_branches.

Measured on the MI355X: no element of any case is beyond its bound; the worst error / bound per family, epilogue and output is
RATIOS below (the full table, and what a planted arithmetic mutation made fail: profiles/gemm_families_ratios.txt)."""
import pytest
import torch

import gemm_ref as R
from errloc import assert_blocks

pytestmark = pytest.mark.gpu

SD_PRE = 4.0
GUARD = 3                      # NaN rows after the last row of every view
TILE = {0: (256, 256), 2: (256, 256), 1: (128, 128), 3: (128, 128), 11: (64, 64), 12: (128, 64), 9: (32, 32), 5: (256, 256),
        6: (256, 128), 8: (256, 256), 10: (256, 128)}
BLOCK_TOL_BF16, BLOCK_TOL_F32 = 5e-3, 1e-5      # per-block relative error: tests/test_hip_gemm_park.py, test_hip_ops.py

# Worst error / bound measured on the MI355X per asserted bound, over every case of this file (1.000 = at the bound; per cfg:
# profiles/gemm_families_ratios.txt).  small = cfg 0-3, 11, 12; tail = cfg 9; round-1 = cfg 5, 6; park = cfg 8; pingpong = cfg 10.
# ":rounded" = gemm_ref's rounded form; "pre" = the kernel's plain bf16 output against z.  The bf16 figures are the rounding term
# (exact, and reached); the fp32 ones are the share of the accumulation budget that is used.
RATIOS = """
                                small     tail  round-1     park pingpong
none out                        0.988    0.988    0.992    0.894    0.975
gelu out                        0.987    0.987    0.987    0.880    0.973
relu out                        0.988    0.988    0.988    0.891    0.975
qgelu out                       0.988    0.988    0.988    0.882    0.973
gelu_out2 out                   0.987    0.987    0.987        -        -
gelu_out2 out2                  0.988    0.990    0.988        -        -
gelu_out2:rounded out               -        -    0.967    0.967    0.967
gelu_out2:rounded out2              -        -    0.993    0.933    0.989
gelu_dsave out                  0.967    0.967    0.967    0.967    0.967
gelu_dsave out2                 0.993    0.993    0.993    0.993    0.993
gelu_dsave pre                  0.988    0.990    0.993    0.933    0.989
qgelu_dsave out                 0.996    0.996    0.996    0.996    0.996
qgelu_dsave out2                0.992    0.992    0.992    0.989    0.989
qgelu_dsave pre                 0.988    0.988    0.988    0.894    0.975
f32 out                         0.012    0.010    0.016        -        -
res_f32 out                     0.012    0.011    0.018    0.002        -
res_bf16 out                    0.991    0.991    0.991        -        -
res_bf16:rounded out                -        -    0.996    0.996    0.996
res_bf16:rounded pre                -        -    0.993    0.894    0.975
res_bf16_relu out               0.988    0.988    0.988        -        -
res_bf16_relu:rounded out           -        -    0.996        -        -
res_bf16_relu:rounded pre           -        -    0.988        -        -
dgelu out                       0.985    0.985    0.985        -        -
dgelu:rounded out                   -        -    0.995    0.996    0.994
dgelu:rounded pre                   -        -    0.988    0.894    0.975
dgelu_saved out                 0.991    0.991    0.991        -        -
dgelu_saved:rounded out             -        -    0.988    0.988    0.988
dgelu_saved:rounded pre             -        -    0.993    0.933    0.989
geglu out                       0.978    0.978    0.978        -        -
geglu:rounded out                   -        -        -    0.996        -
geglu:rounded pre                   -        -        -    0.894        -
geglu_out2 out                  0.978    0.981    0.985        -        -
geglu_out2 out2                 0.988    0.990    0.993        -        -
geglu_out2:rounded out              -        -        -    0.996        -
geglu_out2:rounded out2             -        -        -    0.933        -
dgeglu out                      0.989    0.989    0.991        -        -
dgeglu:rounded out                  -        -        -    0.996        -
dgeglu:rounded pre                  -        -        -    0.941        -
"""


def _ops():
    from vitlens_hip import ops
    return ops


def _gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def _randn(*shape, seed, scale=1.0):
    return torch.randn(*shape, generator=_gen(seed), device="cuda") * scale


class Buf:
    """A [rows, cols] view of a NaN-filled [rows + GUARD, cols + pad] allocation."""

    def __init__(self, rows, cols, pad, dtype=torch.bfloat16, fill=None):
        self.full = torch.full((rows + GUARD, cols + pad), float("nan"), device="cuda", dtype=dtype)
        self.v = self.full[:rows, :cols]
        if fill is not None:
            self.v.copy_(fill)

    def check(self, what):
        rows, cols = self.v.shape
        assert bool(torch.isnan(self.full[rows:]).all()), f"{what}: a guard row after row {rows} was written"
        assert bool(torch.isnan(self.full[:rows, cols:]).all()), f"{what}: a padding column after column {cols} was written"
        bad = ~torch.isfinite(self.v)
        if bool(bad.any()):
            i, j = (int(t[0]) for t in torch.nonzero(bad, as_tuple=True))
            raise AssertionError(f"{what}: {int(bad.sum())} non-finite elements inside the view, first at row {i}, col {j}")


class Case:
    """Operands of one (M, N, K) and its fp64 references with and without the bias (built once per shape, shared by every cfg)."""

    def __init__(self, M, N, K, alpha=0.5, seed=0):
        self.M, self.N, self.K, self.alpha = M, N, K, alpha
        self.a_buf = Buf(M, K, 8, fill=_randn(M, K, seed=seed + 1))
        self.w_buf = Buf(N, K, 8, fill=_randn(N, K, seed=seed + 2, scale=SD_PRE / alpha * K ** -0.5))
        self.a, self.w = self.a_buf.v, self.w_buf.v
        self.bias = _randn(N, seed=seed + 3)
        self.ref = {True: R.Ref(self.a, self.w, self.bias, alpha), False: R.Ref(self.a, self.w, None, alpha)}
        for r in self.ref.values():
            assert float(r.z.min()) < -11 and float(r.z.max()) > 11, "both saturated ends of the activations"
        self.seed = seed

    def second(self, epi, res_div=1):
        M, N, s = self.M, self.N, self.seed + 50
        if epi == "res_f32":
            return _randn(M, N, seed=s)
        if epi in ("res_bf16", "res_bf16_relu"):
            return _randn((M + res_div - 1) // res_div, N, seed=s, scale=2.0).bfloat16()
        if epi == "dgelu":
            return _randn(M, N, seed=s, scale=1.5).bfloat16()
        if epi == "dgelu_saved":
            return R.gelu_grad(_randn(M, N, seed=s, scale=1.5)).bfloat16()
        if epi == "dgeglu":
            return _randn(M, 2 * N, seed=s, scale=1.5).bfloat16()
        return None


_CASES = {}


def case(M, N, K):
    if (M, N, K) not in _CASES:
        if len(_CASES) >= 2:               # the big ones are 150 MB per fp64 tensor: keep two shapes
            _CASES.pop(next(iter(_CASES)))
        _CASES[(M, N, K)] = Case(M, N, K, seed=M + N + K)
    return _CASES[(M, N, K)]


def rounded_form(cfg, epi, N, ldo):
    """The table of the module docstring."""
    if cfg in (8, 10):
        return epi in R.TWO_FORMS
    if cfg in (5, 6):
        return epi in ("gelu_out2", "res_bf16", "res_bf16_relu", "dgelu", "dgelu_saved") and N % 8 == 0 and ldo % 8 == 0
    return False


def launch(ops, c, epi, cfg, pad, bias=True, res_div=1, inplace=False, rows=None, res0=None):
    """One epilogue on rows `rows` (default all) of case c with kernel cfg: (outs, second operand expanded to the output's rows,
    the buffers to guard-check, ldo).  pad: extra elements of the output's row stride (for GEGLU's half-width output it is
    rounded up so that the stride stays a multiple of 4)."""
    r0, r1 = rows or (0, c.M)
    M, N = r1 - r0, c.N
    a = c.a[r0:r1]
    b = c.bias if bias else None
    kw = dict(cfg=cfg, alpha=c.alpha)
    E = ops
    if res0 is None:
        res0 = c.second(epi, res_div)
    if res0 is not None:
        assert r0 % res_div == 0
        res0 = res0[r0 // res_div:(r1 + res_div - 1) // res_div] if epi.startswith("res_bf16") else res0[r0:r1]
    res_rows = None if res0 is None else R.expand_res(res0, res_div, M)
    bufs = []

    def buf(cols, p, dtype=torch.bfloat16, fill=None, rows_=M):
        bufs.append(Buf(rows_, cols, p, dtype, fill))
        return bufs[-1].v

    outs = {}
    ldo = N + pad
    if epi in ("none", "gelu", "relu", "qgelu"):
        act = {"none": E.ACT_NONE, "gelu": E.ACT_GELU, "relu": E.ACT_RELU, "qgelu": E.ACT_QGELU}[epi]
        outs["out"] = E.gemm(a, c.w, b, out=buf(N, pad), epi=E.EPI_BF16, act=act, **kw)
    elif epi in ("gelu_out2", "gelu_dsave", "qgelu_dsave"):
        act = {"gelu_out2": E.ACT_GELU, "gelu_dsave": E.ACT_GELU_DSAVE, "qgelu_dsave": E.ACT_QGELU_DSAVE}[epi]
        outs["out2"] = buf(N, pad)
        outs["out"] = E.gemm(a, c.w, b, out=buf(N, pad), out2=outs["out2"], epi=E.EPI_BF16, act=act, **kw)
    elif epi == "f32":
        outs["out"] = E.gemm(a, c.w, b, out=buf(N, pad, torch.float32), epi=E.EPI_F32, **kw)
    elif epi in ("res_f32", "res_bf16", "res_bf16_relu"):
        dt = torch.float32 if epi == "res_f32" else torch.bfloat16
        e = E.EPI_RES_F32 if epi == "res_f32" else E.EPI_RES_BF16
        act = E.ACT_RELU if epi == "res_bf16_relu" else E.ACT_NONE
        if inplace:
            assert res_div == 1
            x = buf(N, pad, dt, fill=res0)
            outs["out"] = E.gemm(a, c.w, b, out=x, res=x, epi=e, act=act, **kw)
        else:
            r = buf(N, pad, dt, fill=res0, rows_=res0.shape[0])
            keep = r.clone()
            outs["out"] = E.gemm(a, c.w, b, out=buf(N, pad, dt), res=r, epi=e, act=act, res_div=res_div, **kw)
            assert torch.equal(r, keep), "the residual operand was written"
    elif epi in ("dgelu", "dgelu_saved"):
        r = buf(N, pad, fill=res0)
        act = E.ACT_GELU_DSAVE if epi == "dgelu_saved" else E.ACT_NONE
        outs["out"] = E.gemm(a, c.w, b, out=buf(N, pad), res=r, epi=E.EPI_DGELU, act=act, **kw)
    elif epi in ("geglu", "geglu_out2"):
        pg = (-(N // 2)) % 4 + pad
        ldo = N // 2 + pg
        if epi == "geglu_out2":
            outs["out2"] = buf(N, 2 * ldo - N)
        outs["out"] = E.gemm(a, c.w, b, out=buf(N // 2, pg), out2=outs.get("out2"), epi=E.EPI_GEGLU, **kw)
    elif epi == "dgeglu":
        p2 = (-(2 * N)) % 8 + (8 if pad else 0)
        ldo = 2 * N + p2
        r = buf(2 * N, p2, fill=res0)
        outs["out"] = E.gemm(a, c.w, b, out=buf(2 * N, p2), res=r, epi=E.EPI_DGEGLU, **kw)
    else:
        raise ValueError(epi)
    return outs, res_rows, bufs, ldo


def check(c, epi, cfg, outs, res_rows, bufs, rounded, bias, what, rows=None):
    """Guards, finiteness, the per-element bounds (each figure printed before it is asserted) and the per-block errors at the
    kernel's tile size."""
    for bf in bufs:
        bf.check(what)
    c.a_buf.check(what + " (operand a)"); c.w_buf.check(what + " (operand w)")
    ref = c.ref[bias] if rows is None else c.ref[bias].rows(*rows)
    chk = R.checks(ref, epi, outs, rounded, res_rows)
    tile = TILE[cfg]
    form = epi + (":rounded" if rounded and epi in R.TWO_FORMS else "")
    cnt = R.count(chk)
    for label, (n, ratio) in cnt.items():
        print(f"RATIO cfg {cfg:2d} | {form} | {label} | {ratio:.3f} | {n} violations | {what}")
    if any(n for n, _ in cnt.values()):
        R.assert_within(chk, what, tile=tile, row0=rows[0] if rows else 0)
    for label, got, want, _ in chk:
        if label != "pre":
            tol = BLOCK_TOL_F32 if got.dtype == torch.float32 else BLOCK_TOL_BF16
            assert_blocks(got, want, tol, tile[0], tile[1], what=f"{what} {label}")


def run_and_check(ops, c, epi, cfg, pad, bias=True, pre=None, **kw):
    outs, res_rows, bufs, ldo = launch(ops, c, epi, cfg, pad, bias=bias, **kw)
    rounded = rounded_form(cfg, epi, c.N, ldo)
    outs["pre"] = pre
    tag = "".join(f" {k}={v}" for k, v in kw.items())
    what = f"cfg {cfg} ({c.M}, {c.N}, {c.K}) pad {pad}{'' if bias else ' no bias'} {epi}{tag}"
    check(c, epi, cfg, outs, res_rows, bufs, rounded, bias, what)
    return outs


# ---- a. every kernel of vl_gemm.hip x every epilogue -----------------------------------------------------------------------------
#   (300, 196, 192): N % 8 == 4, ragged row and column tiles at 256, 128, 64 and 32, nk = 3
#   (321, 392, 64):  N % 8 == 0, ragged everywhere, nk = 1, tail kernel with idle waves; pad 0 = the 16-byte path of cfg 5 / 6, pad 4 = the 8-byte one
#   (97, 264, 448), (97, 264, 576): the tail kernel's loop edges (unrolled loop in waves 0-3 only / both loops in every wave); even nk and a long K for the others
SHAPES_A = [(300, 196, 192, 0), (321, 392, 64, 0), (321, 392, 64, 4), (97, 264, 448, 0), (97, 264, 576, 0)]
VARIANTS = [("none", {}), ("gelu", {}), ("relu", {}), ("qgelu", {}), ("gelu_out2", {}), ("gelu_dsave", {}), ("qgelu_dsave", {}),
            ("f32", {}), ("res_f32", {}), ("res_f32", {"inplace": True}), ("res_bf16", {}), ("res_bf16", {"inplace": True}),
            ("res_bf16", {"res_div": 3}), ("res_bf16", {"res_div": 32}), ("res_bf16_relu", {}), ("res_bf16_relu", {"res_div": 3}),
            ("dgelu", {}), ("dgelu_saved", {}), ("geglu", {}), ("geglu_out2", {}), ("dgeglu", {})]
NO_BIAS = ["none", "f32", "gelu_dsave", "res_bf16", "dgelu_saved", "geglu", "dgeglu"]


@pytest.mark.parametrize("M,N,K,pad", SHAPES_A)
@pytest.mark.parametrize("cfg", [0, 1, 2, 3, 11, 12, 9, 5, 6])
def test_every_kernel_every_epilogue(cfg, M, N, K, pad):
    ops = _ops()
    c = case(M, N, K)
    assert M % TILE[cfg][0] and N % TILE[cfg][1] and M % 32 and N % 32          # ragged row and column tiles
    pre = run_and_check(ops, c, "none", cfg, pad)["out"]
    for epi, kw in VARIANTS[1:]:
        run_and_check(ops, c, epi, cfg, pad, pre=pre, **kw)
    pre = run_and_check(ops, c, "none", cfg, pad, bias=False)["out"]
    for epi in NO_BIAS[1:]:
        run_and_check(ops, c, epi, cfg, pad, bias=False, pre=pre)


# ---- b. round-1 persistent kernel: more tiles than workgroups at nk = 1 (advance_load switches tile on every step), a last
# N-tile group narrower than GN = 4 (1416 = 5.53 x 256: 6 column tiles = 4 + 2), the reload on the last step ----
@pytest.mark.parametrize("K", [64, 128])
@pytest.mark.parametrize("cfg", [5, 6])
def test_round1_persistent_many_tiles(cfg, K):
    ops = _ops()
    M, N = 52 * 256 + 44, 1416
    tiles = -(-M // TILE[cfg][0]) * -(-N // TILE[cfg][1])
    assert tiles == (318 if cfg == 5 else 636)
    assert tiles > torch.cuda.get_device_properties(0).multi_processor_count
    c = case(M, N, K)
    pre = run_and_check(ops, c, "none", cfg, 0)["out"]
    run_and_check(ops, c, "f32", cfg, 0)
    run_and_check(ops, c, "gelu_dsave", cfg, 0, pre=pre)
    run_and_check(ops, c, "res_bf16", cfg, 0, pre=pre, inplace=True)
    run_and_check(ops, c, "geglu_out2", cfg, 0)


# ---- c. run_gemm's branches at the smallest shapes that reach them (worked out for 256 CUs) --------------------------------------
# (`if (main_m == 0) return launch_persist` after the full_m fallback in run_gemm cannot be reached: the tile-count test above it
# returns unless full_m * tiles_n >= 3 G / 4 > 0, which implies full_m >= 1.)
EPIS_C = [("gelu_out2", {}), ("gelu_dsave", {}), ("res_f32", {"inplace": True}), ("res_bf16", {"res_div": 32}), ("dgelu_saved", {}),
          ("geglu_out2", {}), ("dgeglu", {"bias": False})]      # (DGEGLU has no bias in use, and park's takes none)


def main_cfg(ops, epi, N, K, res_div):
    """The kernel launch_best_persist picks for the whole row tiles (vl_gemm_park_supported / vl_gemm_pp_supported)."""
    fam = epi in ("gelu_out2", "gelu_dsave", "res_bf16", "dgelu_saved") and res_div == 1
    if K >= 512 and N % 256 == 0 and (fam or epi in ("res_f32", "geglu_out2", "dgeglu")):
        return 8
    if K >= 128 and N % 128 == 0 and fam:
        return 10
    return 5


@pytest.mark.parametrize("epi,kw", EPIS_C, ids=[e for e, _ in EPIS_C])
@pytest.mark.parametrize("M,N,K,left", [(24 * 256 + 77, 2048, 64, 9), (24 * 256 + 77, 2048, 128, 9), (24 * 256 + 77, 2048, 512, 9),
                                        (16 * 256 + 200, 3072, 128, 11), (34 * 256 + 88, 2048, 128, 1)])
def test_auto_dispatch_branches(M, N, K, left, epi, kw):
    """cfg = -1: whole row tiles on a persistent kernel, the leftover rows on the tail kernel (cfg 9), 64x64 tiles (cfg 11) or
    128x128 tiles (cfg 1, more than 512 leftover rows).  The leftover rows are bit-equal to a forced-cfg run of the expected
    kernel on a[mm:] with out, res and out2 offset the way the dispatcher must offset them, the main rows to the expected
    persistent kernel: the branch and the operand carrying are observable.  Each part is then checked element by element with
    its own kernel's rounding form, and per block at that kernel's tile size (the leftover rows are a block range of their own)."""
    ops = _ops()
    mm = int(ops._lib.vl_gemm_main_rows(M, N))
    assert 0 < mm < M and mm % 256 == 0, mm
    if torch.cuda.get_device_properties(0).multi_processor_count != 256:
        pytest.skip("the shapes identify run_gemm's branches on 256 CUs")
    assert mm == (M // 256 if left != 1 else 32) * 256
    c = case(M, N, K)
    res_div, bias = kw.get("res_div", 1), kw.get("bias", True)
    pad = 8
    main = main_cfg(ops, epi, N, K, res_div)
    res0 = c.second(epi, res_div)
    outs, res_rows, bufs, ldo = launch(ops, c, epi, -1, pad, res0=res0, **kw)
    what = f"auto ({M}, {N}, {K}) {epi}: rows 0:{mm} on cfg {main}, rows {mm}:{M} on cfg {left}"
    for bf in bufs:
        bf.check(what)
    for (r0, r1), cfg in (((0, mm), main), ((mm, M), left)):
        part = f"{what}, rows {r0}:{r1}"
        f_outs, f_res, f_bufs, _ = launch(ops, c, epi, cfg, pad, rows=(r0, r1), res0=res0, **kw)
        for k in f_outs:
            assert torch.equal(outs[k][r0:r1], f_outs[k]), f"{part}: {k} is not what cfg {cfg} writes for these rows"
        f_outs["pre"] = launch(ops, c, "none", cfg, pad, bias=bias, rows=(r0, r1))[0]["out"]
        check(c, epi, cfg, f_outs, f_res, f_bufs, rounded_form(cfg, epi, N, ldo), bias, part, rows=(r0, r1))

# ---- d. the two newer persistent kernels at their smallest supported problems, element by element ------------------------------
EPIS_8 = ["gelu", "relu", "qgelu", "gelu_out2", "gelu_dsave", "qgelu_dsave", "res_f32", "res_bf16", "dgelu", "dgelu_saved", "geglu",
          "geglu_out2"]
EPIS_10 = ["gelu", "relu", "qgelu", "gelu_out2", "gelu_dsave", "qgelu_dsave", "res_bf16", "dgelu", "dgelu_saved"]


@pytest.mark.parametrize("cfg,M,N,K", [(8, 256, 256, 512), (10, 256, 128, 128), (10, 256, 384, 128)])
def test_park_and_pingpong_smallest_problems(cfg, M, N, K):
    ops = _ops()
    c = case(M, N, K)
    pad = 8                                                  # rows stay 16-byte aligned: these kernels refuse anything else
    pre = run_and_check(ops, c, "none", cfg, pad)["out"]
    for epi in (EPIS_8 if cfg == 8 else EPIS_10):
        run_and_check(ops, c, epi, cfg, pad, pre=pre)
    if cfg == 8:
        pre = run_and_check(ops, c, "none", cfg, pad, bias=False)["out"]
        run_and_check(ops, c, "dgeglu", cfg, pad, bias=False, pre=pre)      # (park's DGEGLU takes no bias)
        run_and_check(ops, c, "res_f32", cfg, pad, bias=False, inplace=True)
