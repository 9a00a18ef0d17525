"""CPU: the head dims of the true-fp32 inference path (precision="fp32", vitlens_hip/f32.py) once vl_attn_fwd_f32 takes head
dims 72-128: 32, 64, or a multiple of 8 in (64, 128] - the rule of vl_attn_bwd_bf16 - as the routing predicates see them,
and every kernel of csrc/vl_f32.hip compiled for gfx950 without scratch or register spills (the recipe of
test_kernel_resources.py, which does not list vl_f32.hip)."""
import os
import re
import subprocess

import pytest

from vitlens_hip import f32 as F
from vitlens_hip.engine import LensCfg, TowerCfg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vit-lens_amd", "csrc")


@pytest.mark.parametrize("width,heads,want", [
    (1280, 16, True),       # ViT-H-14: head dim 80
    (1664, 16, True),       # ViT-bigG-14: 104
    (1024, 8, True),        # 128
    (576, 8, True),         # 72
    (1024, 16, True),       # ViT-L-14: 64
    (768, 12, True),        # ViT-B: 64
    (256, 8, True),         # 32
    (64, 2, True),          # the tiny goldens: 32
    (768, 16, False),       # 48
    (1600, 16, False),      # 100: not a multiple of 8
    (1088, 8, False),       # 136: beyond 128
    (1290, 16, False),      # width % heads != 0
    (1000, 16, False),      # width % heads != 0
])
def test_f32_supported_head_dims(width, heads, want):
    assert F.f32_supported(width, heads) is want


def _bigG():
    return TowerCfg(width=1664, layers=48, heads=16, mlp_ratio=4.9231, embed_dim=1280)


def _audio(**kw):
    a = dict(modality="audio", perceiver_identity=False, depth=2, self_per_cross=3, latent_dim=1664, input_chan=1664)
    a.update(kw)
    return LensCfg(**a)


def test_f32_lens_supported_over_a_bigG_trunk():
    """The tower test widens through f32_supported; the Perceiver's own head dims stay 32 / 64 and pnsa stays out."""
    t = _bigG()
    assert F.f32_lens_supported(t, _audio())                                           # Perceiver heads of 64
    assert F.f32_lens_supported(t, _audio(cross_dim_head=32, latent_dim_head=32))
    assert not F.f32_lens_supported(t, _audio(cross_dim_head=104))                     # Perceiver dh 104
    assert not F.f32_lens_supported(t, _audio(latent_dim_head=104))
    assert not F.f32_lens_supported(t, LensCfg(modality="pc", perceiver_identity=False, pc_tokenizer="pnsa",
                                               latent_dim=1664, input_chan=384))
    assert not F.f32_lens_supported(TowerCfg(width=1600, heads=16), _audio(latent_dim=1600, input_chan=1600))


def test_vl_f32_kernels_no_scratch_no_spills(tmp_path):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I" + CSRC,
                        "-I" + os.path.join(ROOT, "include"), "-x", "hip", "-c", os.path.join(CSRC, "vl_f32.hip"), "-o",
                        str(tmp_path / "o.o"), "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True,
                       timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    name, bad, vgprs = None, [], {}
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
        if m and int(m.group(1)) > 0:
            bad.append((name, "scratch", int(m.group(1))))
        m = re.search(r"([SV]GPRs) Spill: (\d+)", line)
        if m and int(m.group(2)) > 0:
            bad.append((name, m.group(1) + " spill", int(m.group(2))))
        m = re.search(r" VGPRs: (\d+)", line)
        if m and name:
            vgprs[name] = int(m.group(1))
    wide = {n: v for n, v in vgprs.items() if "attn_f32_wide_kernel" in n}
    for n, v in sorted(wide.items()):
        print(f"{n}: {v} VGPRs")
    assert len(wide) == 4, sorted(vgprs)          # the padded widths 80, 96, 112, 128
    assert len(vgprs) >= 10, sorted(vgprs)         # every kernel of the file was reported
    assert not bad, bad
