"""CPU: the QuickGELU helpers of csrc/vl_common.h (qgelu, qgelu_grad, the packed-pair forms the GEMM epilogues use and
qgelu_and_grad_pk, VL_ACT_QGELU / VL_ACT_QGELU_DSAVE) on a HOST build of the same header over every finite bf16 value in both
lanes (tests/native/qgelu_pairs_host.cpp): within one bf16 ulp of fp64 x * sigmoid(1.702 x) and s + 1.702 x s (1 - s), finite
everywhere (x / 1 at the positive end, -0 / 0 at the negative end), and the packed forms equal the scalar forms bit for bit -
before a GPU is involved, in the style of tests/test_gelu_pairs_host.py.

The bound is that of the HOST arithmetic: the host's exp2f and division keep denormals.  The device exponential flushes a
denormal result to 0, so from |x| ~ 51 on the device returns -0 / 0 at the negative end where the true values (below 1e-36 in
magnitude, normal bf16 numbers down to 1.2e-38) are not 0: there the device differs from fp64 by that absolute amount, which no
16-bit tower can see.  What this test establishes is the structure of the arithmetic - lanes, signs, the selects, no 0 * inf."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"


@pytest.mark.skipif(not os.path.exists(CLANG), reason="needs the ROCm clang (ext_vector_type, __builtin_elementwise_*)")
def test_quickgelu_forms_against_fp64_on_every_bf16_value(tmp_path):
    src = open(os.path.join(ROOT, "vit-lens_amd", "csrc", "vl_common.h")).read().replace("#include <hip/hip_runtime.h>", "")
    hdr = tmp_path / "vl_common_host.h"
    hdr.write_text(src)
    exe = str(tmp_path / "qgelu_pairs_host")
    build = subprocess.run([CLANG, "-O2", "-std=c++17", "-ffp-contract=off", f'-DVL_COMMON_HOST_H="{hdr}"',
                            os.path.join(ROOT, "tests", "native", "qgelu_pairs_host.cpp"), "-o", exe, "-lm"],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-2000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(run.stdout[-600:])
    assert run.returncode == 0 and "bad=0" in run.stdout, run.stdout[-800:]
    assert int(run.stdout.split("checked=")[1].split()[0]) > 65000
