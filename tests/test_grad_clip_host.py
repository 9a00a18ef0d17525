"""CPU: gradient-norm clipping of the fused steps - what can be checked without a GPU.  The coefficient the multi-tensor
AdamW kernel derives (restated in `vitlens_hip.train.clip_coef`) against torch.nn.utils.clip_grad_norm_; the slot table the
optimizer hands to the kernel; header / binding / version; the two kernels' compiled resources."""
import os
import re
import struct
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vit-lens_amd", "csrc")
HEADER = os.path.join(ROOT, "include", "vitlens_hip.h")


def _with_norm(norm, n=1000, seed=0):
    """f32 gradient pieces ([37,19] | [19] | scalar | rest) whose global 2-norm is `norm` (zero, inf and NaN included)."""
    g = torch.randn(n, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)
    if norm == 0.0:
        g.zero_()
    elif norm != norm or norm == float("inf"):
        g[3] = norm
    else:
        g *= norm / float(g.norm())
    g = g.float()
    return [g[:703].reshape(37, 19).clone(), g[703:722].clone(), g[722].clone(), g[723:].clone()]


@pytest.mark.parametrize("grad_scale", [1.0, 0.125])
@pytest.mark.parametrize("norm", [0.25, 1.0, 1.5, 7.0, 1e4, 0.0, float("inf"), float("nan")])
def test_coefficient_agrees_with_torch_clip_grad_norm(norm, grad_scale):
    """max_norm = 1.5: norms below, at and above it, zero, inf and NaN; the kernel's formula is applied to the SUM gradient
    with grad_scale (1 and 1/8), torch clips the mean gradient grad_scale * g.  1/8 is a power of two: the scaled gradient and
    its norm are exact images of the unscaled ones.  Bound: torch sums the 1000 squares in f32 (a cascade: up to about log2(n) = 10
    roundings of 6e-8 on the sum, half of that on the norm), then sqrt, the norm of the per-tensor norms, a divide and a multiply
    add a few more; the restated formula starts from the correctly rounded sum.  1e-6 covers both; 2e-6 for the norm itself."""
    from vitlens_hip.train import clip_coef
    max_norm = 1.5
    pieces = _with_norm(norm / grad_scale)
    sumsq = torch.cat([p.reshape(-1) for p in pieces]).double().pow(2).sum().float().reshape(1)
    coef = clip_coef(sumsq, max_norm, grad_scale)
    mine = [p * grad_scale * coef.reshape(()) for p in pieces]
    ref = [torch.nn.Parameter(p.clone()) for p in pieces]
    for r, p in zip(ref, pieces):
        r.grad = p * grad_scale
    total = torch.nn.utils.clip_grad_norm_(ref, max_norm, norm_type=2.0)
    if norm != norm:
        assert torch.isnan(coef).all() and torch.isnan(total)
    elif norm == float("inf"):
        assert float(coef) == 0.0 and torch.isinf(total)
    elif norm <= max_norm * (1 - 1e-6):
        assert float(coef) == 1.0
    if norm > max_norm * (1 + 1e-6) and norm != float("inf"):
        assert float(coef) < 1.0
        got = float(torch.cat([m.reshape(-1) for m in mine]).double().norm())
        assert abs(got - max_norm) < 1e-5 * max_norm, got          # the clipped gradient has the norm asked for
    for m, r in zip(mine, ref):
        assert torch.equal(torch.isnan(m), torch.isnan(r.grad))
        ok = ~torch.isnan(m)
        assert torch.allclose(m[ok], r.grad[ok], rtol=1e-6, atol=0.0), float((m[ok] - r.grad[ok]).abs().max())
    if norm == norm and norm != float("inf"):
        assert abs(float(torch.sqrt(sumsq)) * grad_scale - float(total)) <= 2e-6 * float(total)


def _decode(table):
    rows = []
    for r in table.tolist():
        rows.append(tuple(r[:5]) + (struct.unpack("<f", struct.pack("<I", r[5] & 0xffffffff))[0],))
    return rows


def test_slot_table_covers_every_master_once_with_the_decay_flags():
    from vitlens_hip.train import AdamW, pack_adamw_slots
    g = torch.Generator().manual_seed(1)
    params = {"visual.transformer.resblocks.0.attn.in_proj_weight": torch.randn(37, 19, generator=g),
              "visual.transformer.resblocks.0.attn.in_proj_bias": torch.randn(19, generator=g),
              "visual.transformer.resblocks.0.ln_1.weight": torch.randn(19, generator=g),
              "visual.visual_adapter.pos_emb": torch.randn(5, 19, generator=g),
              "visual.bn.weight": torch.randn(4, 4, generator=g),
              "logit_scale": torch.randn(1, generator=g),
              "no_gradient_this_step": torch.randn(3, 3, generator=g)}
    opt = AdamW(params, lr=1e-3, weight_decay=0.2)
    grads = {k: torch.randn(v.shape, generator=g) for k, v in params.items() if k != "no_gradient_this_step"}
    rows = opt.slot_rows(grads)
    table = pack_adamw_slots(rows)
    assert table.dtype == torch.int64 and tuple(table.shape) == (len(grads), 6) and table.is_contiguous()
    assert table.element_size() * table.shape[1] == 48          # sizeof(struct vl_adamw_slot)
    dec = _decode(table)
    want = {k: (params[k].data_ptr(), grads[k].data_ptr(), opt.m[k].data_ptr(), opt.v[k].data_ptr(), params[k].numel(),
                0.2 if AdamW.decays(k, params[k]) else 0.0) for k in grads}
    assert len(dec) == len(want)
    by_p = {r[0]: r for r in dec}
    assert len(by_p) == len(dec), "a master appears twice"
    for k, w in want.items():
        r = by_p[w[0]]
        assert r[:5] == w[:5], k
        assert r[5] == struct.unpack("<f", struct.pack("<f", w[5]))[0], (k, r[5])
    assert sorted(k for k in grads if want[k][5] > 0) == ["visual.transformer.resblocks.0.attn.in_proj_weight",
                                                          "visual.visual_adapter.pos_emb"]
    with pytest.raises(ValueError):
        opt.slot_rows({**grads, "logit_scale": torch.randn(2)})
    with pytest.raises(ValueError):
        opt.slot_rows({**grads, "visual.bn.weight": torch.randn(4, 8)[:, ::2]})


def test_fused_steps_take_grad_clip_norm_and_refuse_nonsense():
    import inspect
    from vitlens_hip import step as ST
    for cls in (ST.TriModalDepthStep, ST.DualAudioStep, ST.TriModalPCStep):
        prm = inspect.signature(cls.__init__).parameters
        assert "grad_clip_norm" in prm and prm["grad_clip_norm"].default is None, cls.__name__
    sd = {"logit_scale": torch.tensor(2.0)}
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError):
            ST._StepState()._init_host(sd, "cpu", 4, 0, 1, grad_clip_norm=bad)
    st = ST._StepState()
    st._init_host(sd, "cpu", 4, 0, 1)
    assert st.grad_clip_norm is None
    st._init_host(sd, "cpu", 4, 0, 1, grad_clip_norm=10)
    assert st.grad_clip_norm == 10.0


def _declaration(name):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"\b(\w+)\s+" + name + r"\s*\(([^)]*)\)\s*;", src)
    assert m, name + " is not declared in the header"
    return m.group(1), [a.strip() for a in m.group(2).split(",")]


def _ctype_of(arg):
    import ctypes as C
    if "*" in arg or arg.startswith("hipStream_t"):
        return C.c_void_p
    return {"int": C.c_int, "long": C.c_long, "float": C.c_float}[arg.split()[0]]


def test_header_binding_and_version_agree():
    import ctypes as C
    from vitlens_hip import _lib
    hdr = open(HEADER).read()
    version = int(re.search(r"#define\s+VL_ABI_VERSION\s+(\d+)", hdr).group(1))
    assert version >= 603, "the two entries arrived with ABI 603"
    assert version == _lib.ABI_VERSION == int(_lib.load_library().vl_version())
    for name in ("vl_sumsq_f32", "vl_adamw_multi_step"):
        ret, args = _declaration(name)
        assert ret == "int"
        assert _lib.SIGNATURES[name] == [_ctype_of(a) for a in args], name
        assert hasattr(C.CDLL(_lib.lib_path()), name)
    ret, args = _declaration("vl_sumsq_ws_floats")
    assert ret == "long" and args == ["void"] and _lib.SIGNATURES["vl_sumsq_ws_floats"] == [] and _lib._RET["vl_sumsq_ws_floats"] is C.c_long
    assert int(_lib.load_library().vl_sumsq_ws_floats()) >= 2
    # the slot struct is what pack_adamw_slots writes: four pointers, a long, a float, an int
    body = re.search(r"typedef struct vl_adamw_slot \{(.*?)\} vl_adamw_slot;", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S), flags=re.S).group(1)
    fields = [f.strip() for f in body.split(";") if f.strip()]
    assert [f.split()[-1].lstrip("*") for f in fields] == ["p", "g", "m", "v", "n", "weight_decay", "reserved"], fields
    from vitlens_hip import ops
    assert ops.ADAMW_MAX_SLOTS == int(re.search(r"#define\s+VL_ADAMW_MAX_SLOTS\s+(\d+)", hdr).group(1))


def test_the_two_kernels_use_no_scratch_and_spill_nothing():
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    import tempfile
    with tempfile.TemporaryDirectory() as td:
        r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I" + CSRC, "-I" + os.path.join(ROOT, "include"),
                            "-x", "hip", "-c", os.path.join(CSRC, "vl_bwd.hip"), "-o", os.path.join(td, "o.o"),
                            "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    seen, name = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
        for key in ("ScratchSize \\[bytes/lane\\]", "SGPRs Spill", "VGPRs Spill"):
            m = re.search(key + r": (\d+)", line)
            if m and name and any(k in name for k in ("sumsq_partial_kernel", "sumsq_final_kernel", "adamw_multi_kernel", "adamw_kernel")):
                seen.setdefault(name, {})[key] = int(m.group(1))
    kernels = [k for k in ("sumsq_partial_kernel", "sumsq_final_kernel", "adamw_multi_kernel", "12adamw_kernel")
               if any(k in n for n in seen)]
    assert len(kernels) == 4, sorted(seen)
    bad = {n: v for n, v in seen.items() if any(v.values()) or len(v) != 3}
    assert not bad, bad
