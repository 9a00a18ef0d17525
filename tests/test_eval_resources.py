"""CPU: the kernels of csrc/vl_eval.hip compile for gfx950 without scratch or register spills, and the average-precision
kernel's static LDS stays within the 64 KB a workgroup may declare (tests/test_kernel_resources.py's check for the evaluation file)."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vit-lens_amd", "csrc")
KERNELS = {"eval_hits_kernel": 1, "ap_partial_kernel": 1, "ap_final_kernel": 1, "clip_mean_normalize_kernel": 1}


def test_no_spills(tmp_path):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I" + CSRC, "-I" + os.path.join(ROOT, "include"),
                        "-x", "hip", "-c", os.path.join(CSRC, "vl_eval.hip"), "-o", str(tmp_path / "o.o"),
                        "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    for k, n in KERNELS.items():
        assert sum(k in name for name in names) == n, (k, names)
    assert len(names) == sum(KERNELS.values())
    assert [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)] == [0] * len(names)
    assert [int(v) for v in re.findall(r"SGPRs Spill: (\d+)", r.stderr)] == [0] * len(names)
    assert [int(v) for v in re.findall(r"VGPRs Spill: (\d+)", r.stderr)] == [0] * len(names)
    assert max(int(v) for v in re.findall(r"LDS Size \[bytes/block\]: (\d+)", r.stderr)) <= 65536
