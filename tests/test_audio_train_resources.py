"""CPU: the kernels of csrc/vl_audio_train.hip compile for gfx950 without scratch or register spills
(tests/test_kernel_resources.py's check for the file this pull request adds)."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vit-lens_amd", "csrc")


def test_no_spills(tmp_path):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I" + CSRC, "-I" + os.path.join(ROOT, "include"),
                        "-x", "hip", "-c", os.path.join(CSRC, "vl_audio_train.hip"), "-o", str(tmp_path / "o.o"),
                        "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    assert sum("resample_sinc_kernel" in n for n in names) == 2 and sum("fbank_augment_kernel" in n for n in names) == 2
    assert [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)] == [0] * len(names)
    assert [int(v) for v in re.findall(r"SGPRs Spill: (\d+)", r.stderr)] == [0] * len(names)
    assert [int(v) for v in re.findall(r"VGPRs Spill: (\d+)", r.stderr)] == [0] * len(names)
