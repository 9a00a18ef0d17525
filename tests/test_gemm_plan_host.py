"""CPU: the row split of the bf16 GEMM under cfg -1 (csrc/vl_gemm_plan.h: gemm_main_rows, gemm_rest_cfg) and the one operand check
of the four GEMM wrappers of ops.py.

The plan.  tests/native/gemm_plan_host.cpp includes the header into a plain host program and prints both functions over a grid:
G in {8, 64, 104, 256, 304}, 0 .. 1100 row tiles plus a row remainder of 0, 40 or 255, every multiple of 64 up to 8192 and 1000,
1664, 4992 as N; 1 .. 600 leftover rows against the same widths.  Every value is compared with `parent_main_rows` /
`parent_rest_cfg` below: a restatement of the text of run_gemm (csrc/vl_gemm.hip, the cfg == -1 branch) AT THE PARENT COMMIT
aaae5b0, written here and importing nothing from the code under test - so the test passes against the parent's formulas by
construction and against the header only while the header says the same.  G in {0, 4} is checked against the header's own
definition (0 rows): the parent's text divides by zero there.  The program is built twice, the second time with
-fsanitize=address,undefined (host code with its own main: nothing is preloaded), and has to exit clean both times.

The wrappers.  One recorded call each (launch_trace.py, CPU tensors) against a literal expectation - the padded-K branch of
gemm and a GEGLU output among them - and every refusal of the wrappers before the refactor, with the function's name in it."""
import os
import subprocess

import numpy as np
import pytest
import torch

from launch_trace import normalised, recording

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
GRIDS = (8, 64, 104, 256, 304)
WIDTHS = list(range(64, 8193, 64)) + [1000, 1664, 4992]
REMAINDERS = (0, 40, 255)
ROW_TILES = np.arange(1101)
REST_ROWS = np.arange(1, 601)


def parent_main_rows(M, N, G):
    """run_gemm at aaae5b0, up to `const int rows_main = main_m * 256;`, line by line (M: an array of row counts; G >= 8).
    Returns 0 where that text returns dispatch(p, 1, s) for the whole problem."""
    tiles_n, full_m = (N + 255) // 256, M // 256
    small = full_m * tiles_n < (G * 3) // 4                     # -> return dispatch<EPI>(p, 1, s)
    step = G // np.gcd(G, tiles_n)
    main_m = (full_m // step) * step
    if (N & 255) == 128:
        step = 2 * G // np.gcd(2 * G, N >> 7)
        main_m = (full_m // step) * step
        main_m = np.where(main_m == 0, full_m, main_m)
    main_m = np.where(main_m == 0, full_m, main_m)
    # `if (main_m == 0) return launch_persist<EPI>(p, s);` - the line the refactor dropped as unreachable
    assert not np.any(~small & (main_m == 0))
    return np.where(small, 0, main_m * 256)


def parent_rest_cfg(rows, N):
    """run_gemm at aaae5b0 from `if (pr.M > 512)` to its end (rows: an array); launch_tail is what dispatch runs for cfg 9."""
    t64 = ((rows + 63) // 64) * ((N + 63) // 64)
    return np.where(rows > 512, 1, np.where(t64 >= 192, 11, 9))


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def printed(request, tmp_path_factory):
    """{("main", G, N, rem): values over ROW_TILES, ("rest", N): values over REST_ROWS} as the host program prints them."""
    if not os.path.exists(CLANG):
        pytest.skip("needs the ROCm clang")
    exe = str(tmp_path_factory.mktemp("gemm_plan") / "gemm_plan_host")
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if request.param == "sanitized" else ["-O2"]
    build = subprocess.run([CLANG, "-std=c++17", *flags, "-I", os.path.join(ROOT, "vit-lens_amd", "csrc"),
                            os.path.join(ROOT, "tests", "native", "gemm_plan_host.cpp"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-2000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and not run.stderr, run.stderr[-2000:]
    out = {}
    for line in run.stdout.splitlines():
        key, values = line.split(" :")
        kind, *numbers = key.split()
        out[(kind, *map(int, numbers))] = np.array(values.split(), dtype=np.int64)
    return out


def test_the_plan_is_the_parents_plan(printed):
    bad, checked = [], 0
    for G in GRIDS:
        for N in WIDTHS:
            for rem in REMAINDERS:
                M = ROW_TILES * 256 + rem
                got, want = printed[("main", G, N, rem)], parent_main_rows(M, N, G)
                checked += len(M)
                bad += [("main", G, N, int(m), int(g), int(w)) for m, g, w in zip(M[got != want], got[got != want], want[got != want])]
    for N in WIDTHS:
        got, want = printed[("rest", N)], parent_rest_cfg(REST_ROWS, N)
        checked += len(REST_ROWS)
        bad += [("rest", N, int(r), int(g), int(w)) for r, g, w in zip(REST_ROWS[got != want], got[got != want], want[got != want])]
    print(f"checked={checked} bad={len(bad)}")
    assert checked == len(GRIDS) * len(WIDTHS) * len(REMAINDERS) * 1101 + len(WIDTHS) * 600
    assert not bad, bad[:10]


def test_a_grid_below_eight_workgroups_is_defined_as_no_main_rows(printed):
    for G in (0, 4):
        for N in WIDTHS:
            for rem in REMAINDERS:
                assert not printed[("main", G, N, rem)].any(), (G, N, rem)


# ---- the wrappers: what they hand to the library ----
def _t(rows, cols, dtype, ld=None):
    """[rows, cols] at row stride ld (a view of a wider buffer) - contents do not matter, nothing runs."""
    return torch.empty(rows, ld or cols, dtype=dtype)[:, :cols]


def _call(fn, *args, **kw):
    with recording() as trace:
        fn(*args, **kw)
    return normalised(trace)


def test_the_four_wrappers_hand_the_library_what_they_did():
    from vitlens_hip import ops
    bf, h, f = torch.bfloat16, torch.float16, torch.float32
    P = lambda n, off=0: ("ptr", n, off)
    # gemm, K = 40: both operands zero-padded to K = 64 (new buffers, row stride 64), out allocated [5, 8] bf16
    assert _call(ops.gemm, _t(5, 40, bf), _t(8, 40, bf), _t(1, 8, f)[0]) == [
        ("vl_gemm_bf16_ex", (P(0), P(1), P(2), P(3), None, None, 5, 8, 64, 64, 64, 8, 1.0, ops.EPI_BF16, ops.ACT_NONE, 1, -1, "stream"))]
    # gemm, GEGLU: out allocated at half the width, out2 (the pre-activation) at the full one
    out2 = _t(4, 16, bf)
    assert _call(ops.gemm, _t(4, 64, bf, 72), _t(16, 64, bf), None, epi=ops.EPI_GEGLU, out2=out2, alpha=0.5, cfg=11) == [
        ("vl_gemm_bf16_ex", (P(0), P(1), None, P(2), None, P(3), 4, 16, 64, 72, 64, 8, 0.5, ops.EPI_GEGLU, ops.ACT_NONE, 1, 11, "stream"))]
    # gemm, a residual row per two output rows, in a wider buffer than it needs
    out = _t(6, 8, bf, 12)
    assert _call(ops.gemm, _t(6, 64, bf), _t(8, 64, bf), None, out=out, res=_t(3, 8, bf, 12), epi=ops.EPI_RES_BF16, res_div=2) == [
        ("vl_gemm_bf16_ex", (P(0), P(1), None, P(2), P(3), None, 6, 8, 64, 64, 64, 12, 1.0, ops.EPI_RES_BF16, ops.ACT_NONE, 2, -1, "stream"))]
    # gemm_f16: fp16 out by default, fp32 with the residual epilogue (here in place)
    assert _call(ops.gemm_f16, _t(4, 64, h), _t(8, 64, h, 80), _t(1, 8, f)[0], act=ops.ACT_GELU) == [
        ("vl_gemm_f16", (P(0), P(1), P(2), P(3), None, 4, 8, 64, 64, 80, 8, 1.0, ops.EPI_BF16, ops.ACT_GELU, "stream"))]
    x = _t(4, 8, f)
    assert _call(ops.gemm_f16, _t(4, 64, h), _t(8, 64, h), None, out=x, res=x, epi=ops.EPI_RES_F32) == [
        ("vl_gemm_f16", (P(0), P(1), None, P(2), P(2), 4, 8, 64, 64, 64, 8, 1.0, ops.EPI_RES_F32, ops.ACT_NONE, "stream"))]
    # gemm_f32: any K
    assert _call(ops.gemm_f32, _t(3, 12, f, 16), _t(5, 12, f), _t(1, 5, f)[0], res=_t(3, 5, f), alpha=2.0, act=ops.ACT_RELU) == [
        ("vl_gemm_f32", (P(0), P(1), P(2), P(3), P(4), 3, 5, 12, 16, 12, 5, 2.0, ops.ACT_RELU, "stream"))]
    # gemm_f32_ex: GEGLU halves the allocated width; a broadcast residual ahead of the activation
    assert _call(ops.gemm_f32_ex, _t(3, 12, f), _t(10, 12, f), None, geglu=True) == [
        ("vl_gemm_f32_ex", (P(0), P(1), None, P(2), None, 3, 10, 12, 12, 12, 5, 1.0, ops.ACT_NONE, 1, 0, 1, "stream"))]
    assert _call(ops.gemm_f32_ex, _t(6, 12, f), _t(8, 12, f), None, res=_t(2, 8, f), res_div=3, res_pre=True, act=ops.ACT_RELU) == [
        ("vl_gemm_f32_ex", (P(0), P(1), None, P(2), P(3), 6, 8, 12, 12, 12, 8, 1.0, ops.ACT_RELU, 3, 1, 0, "stream"))]


@pytest.mark.parametrize("name,dt", [("gemm", torch.bfloat16), ("gemm_f16", torch.float16), ("gemm_f32", torch.float32),
                                     ("gemm_f32_ex", torch.float32)])
def test_the_four_wrappers_refuse_what_they_refused(name, dt):
    from vitlens_hip import ops
    fn = getattr(ops, name)
    rdt = dt if name == "gemm" else torch.float32             # residual / default output type of the call below
    kw = {"epi": ops.EPI_RES_BF16} if name == "gemm" else ({"epi": ops.EPI_RES_F32} if name == "gemm_f16" else {})
    a, w = _t(4, 64, dt), _t(8, 64, dt)

    def refused(exc, *args, **kwargs):
        with recording() as trace, pytest.raises(exc) as e:
            fn(*args, **kwargs)
        assert not trace and (name + ":") in str(e.value), str(e.value)

    refused(ValueError, a, _t(8, 128, dt))                                                   # K mismatch
    refused(ValueError, _t(64, 4, dt).t(), w)                                                # operand not row-major
    refused(ValueError, a, _t(64, 8, dt).t())
    refused(ValueError, a[0], w)                                                             # ... not 2-D
    refused(TypeError, a.to(torch.float64), w)                                               # operand of another type
    refused(TypeError, a, w.to(torch.float64))
    refused(ValueError, a, w, _t(1, 9, torch.float32)[0])                                    # bias of another length
    refused(ValueError, a, w, _t(1, 8, torch.float64)[0])                                    # ... of another type
    refused(ValueError, a, w, None, out=_t(8, 4, rdt).t(), **kw)                             # out not row-major
    refused(ValueError, a, w, None, out=_t(4, 8, rdt), res=_t(4, 8, rdt, 12), **kw)          # residual at another row stride
    refused(ValueError, a, w, None, out=_t(4, 8, rdt), res=_t(8, 4, rdt).t(), **kw)          # residual not row-major
    if name == "gemm":
        refused(ValueError, a, w, None, out=_t(4, 8, dt), res=_t(4, 8, torch.float32), **kw)          # residual of another type than out
        refused(ValueError, a, w, None, out=_t(4, 8, dt), res=_t(1, 8, dt), res_div=2, **kw)          # too few broadcast rows
        refused(ValueError, a, w, act=ops.ACT_GELU_DSAVE)                                             # derivative output missing
        refused(ValueError, a, w, out2=_t(4, 8, dt, 16))                                              # out2 at another row stride
    else:
        refused(TypeError, a, w, None, out=_t(4, 8, torch.float64), **kw)                             # out of another type
        refused(TypeError, a, w, None, out=_t(4, 8, rdt), res=_t(4, 8, torch.float64), **kw)          # residual of another type
    if name == "gemm_f32_ex":
        refused(ValueError, a, w, None, res=_t(1, 8, dt), res_div=2, res_pre=True)                    # too few broadcast rows
        refused(ValueError, a, w, None, res=_t(3, 8, dt))                                             # ... and without broadcast
