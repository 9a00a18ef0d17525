"""CPU: the kernels of csrc/vl_image_augment.hip compile for gfx950 without scratch or register spills, and the per-sample
kernel's static LDS (histograms, prefix sums, LUT) stays small (tests/test_kernel_resources.py's check for this file)."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vit-lens_amd", "csrc")
KERNELS = {"image_h_kernel": 1, "image_v_kernel": 1, "image_aug_kernel": 1}


def test_no_scratch_no_spills(tmp_path):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I" + CSRC, "-I" + os.path.join(ROOT, "include"),
                        "-x", "hip", "-c", os.path.join(CSRC, "vl_image_augment.hip"), "-o", str(tmp_path / "o.o"),
                        "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    for k, n in KERNELS.items():
        assert sum(k in name for name in names) == n, (k, names)
    assert len(names) == sum(KERNELS.values())
    print(dict(zip(names, re.findall(r" VGPRs: (\d+)", r.stderr))))
    assert [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)] == [0] * len(names)
    assert [int(v) for v in re.findall(r"SGPRs Spill: (\d+)", r.stderr)] == [0] * len(names)
    assert [int(v) for v in re.findall(r"VGPRs Spill: (\d+)", r.stderr)] == [0] * len(names)
    assert max(int(v) for v in re.findall(r"LDS Size \[bytes/block\]: (\d+)", r.stderr)) <= 8192
