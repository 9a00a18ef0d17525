"""CPU: the kernels of csrc/vl_tactile_augment.hip compile for gfx950 without scratch or register spills and use no LDS
(tests/test_image_augment_resources.py's check for this file)."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vit-lens_amd", "csrc")
KERNELS = {"tactile_h_kernel": 1, "tactile_vg_kernel": 1}


def test_no_scratch_no_spills(tmp_path):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I" + CSRC, "-I" + os.path.join(ROOT, "include"),
                        "-x", "hip", "-c", os.path.join(CSRC, "vl_tactile_augment.hip"), "-o", str(tmp_path / "o.o"),
                        "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    for k, n in KERNELS.items():
        assert sum(k in name for name in names) == n, (k, names)
    assert len(names) == sum(KERNELS.values())
    vgprs = [int(v) for v in re.findall(r" VGPRs: (\d+)", r.stderr)]
    print(dict(zip(names, vgprs)), "occupancy", re.findall(r"Occupancy \[waves/SIMD\]: (\d+)", r.stderr))
    assert [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)] == [0] * len(names)
    assert [int(v) for v in re.findall(r"SGPRs Spill: (\d+)", r.stderr)] == [0] * len(names)
    assert [int(v) for v in re.findall(r"VGPRs Spill: (\d+)", r.stderr)] == [0] * len(names)
    assert [int(v) for v in re.findall(r"LDS Size \[bytes/block\]: (\d+)", r.stderr)] == [0] * len(names)
    assert max(vgprs) <= 64                          # eight waves per SIMD: the gather pass hides its latency with occupancy
