"""CPU: the kernels of csrc/vl_audio_mix.hip compile for gfx950 without scratch or register spills
(tests/test_audio_train_resources.py's check for the file that holds vl_wave_clip_mix and vl_mix_rows)."""
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
                        "-x", "hip", "-c", os.path.join(CSRC, "vl_audio_mix.hip"), "-o", str(tmp_path / "o.o"),
                        "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    assert sum("wave_clip_mix_kernel" in n for n in names) == 1 and sum("mix_rows_kernel" in n for n in names) == 2
    assert [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)] == [0] * len(names)
    assert [int(v) for v in re.findall(r"SGPRs Spill: (\d+)", r.stderr)] == [0] * len(names)
    assert [int(v) for v in re.findall(r"VGPRs Spill: (\d+)", r.stderr)] == [0] * len(names)


def test_the_file_is_in_the_library_and_not_in_the_audio_train_file():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "vl_audio_mix.hip" in re.search(r"^SRCS = (.*)$", mk, re.M).group(1).split()
    assert "mix" not in open(os.path.join(CSRC, "vl_audio_train.hip")).read().lower()
