"""CPU: the linear probe (ViTLensLP + LARS + nn.CrossEntropyLoss of the reference).

1. Pinned to the imported reference: its ViTLensLP on a tiny tactile config (the TINY config of tests/test_patch_dropout_host.py),
   trained four steps with its LARS at lr = 0.1, gives per step the pooled features, the dropout output, logits, loss, both
   gradients, the updated weight and bias and the running statistics stored under tests/golden/reference/.
   tests/linprobe_ref.py in fp64, fed the recorded pooled features and masks, must reproduce every one of them within
   1e-5 max|ref| (the fp32 reference and the fp64 restatement differ by at most 1.8e-6 by that measure on these four cases:
   the reference's own fp32 rounding sits 5x inside the limit).  This settles the dropout scale, eps = 1e-6, the unbiased running
   variance, and that the bias gets neither weight decay nor a trust ratio; the restatement WITH decay on the bias must miss.
2. The C ABI: the new entries are declared, exported and bound with the header's parameter lists; version 610 everywhere;
   sizeof(vl_lars_slot) is what pack_lars_slots writes.
3. The interface: state_dict keys and constructor signatures of ViTLensLP and LARS equal the recorded ones, LARS.state_dict()
   round-trips, a trainable backbone parameter raises."""
import ctypes
import inspect
import json
import os
import re
import subprocess
import tempfile
import warnings
from types import SimpleNamespace

import pytest
import torch

import linprobe_ref as LR
from golden_util import reference_run, seeded_like

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

TINY = {"embed_dim": 32,
        "vision_cfg": {"image_size": 32, "layers": 2, "width": 64, "patch_size": 8, "head_width": 32},
        "text_cfg": {"context_length": 16, "vocab_size": 96, "width": 64, "heads": 2, "layers": 2}}
# (vit proj, dropout, classes, batch, weight decay)
CASES = ((False, 0.0, 7, 6, 0.0), (True, 0.0, 7, 6, 1e-4), (False, 0.25, 7, 6, 1e-4), (False, 0.0, 2, 5, 0.0))
LR0, STEPS, SEED = 0.1, 4, 61
REF_KEY = "test_linprobe_host.reference_linear_probe"
TENSORS = ("logits", "loss", "dw", "db", "weight", "bias", "running_mean", "running_var")

_REF = r'''
import inspect, json, os, sys, tempfile, torch
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[2])
import ref_loader
oc = ref_loader.load()
from golden_util import seeded_like
import linprobe_ref as LR
from open_clip.linprobe_model import ViTLensLP
from training.optimizer import LARS
cfg = json.loads(sys.argv[3]); cases = json.loads(sys.argv[4]); lr = float(sys.argv[5]); steps = int(sys.argv[6]); seed = int(sys.argv[7])
stat = lambda sd: {k: [list(v.shape), float(v.double().mean()) if v.numel() else 0.0, float(v.double().std()) if v.numel() > 1 else 0.0,
                       str(v.dtype)] for k, v in sd.items()}
out = {"cases": [], "signatures": {"ViTLensLP": str(inspect.signature(ViTLensLP.__init__)), "LARS": str(inspect.signature(LARS.__init__))}}
with tempfile.TemporaryDirectory() as td:
    with open(os.path.join(td, "tiny-linprobe.json"), "w") as f:
        json.dump(cfg, f)
    oc.add_model_config(td)
    for ci, (proj, drop, C, B, wd) in enumerate(cases):
        args = ref_loader.lens_args("tactile", model="tiny-linprobe", pretrained=None, precision="fp32", force_quick_gelu=False,
                                    force_custom_text=False, force_image_size=None, pretrained_image=False, cache_dir=None,
                                    lp_enable_vit_proj=proj, lp_dropout_rate=drop, lp_num_classes=C)
        torch.manual_seed(seed)
        model = ViTLensLP(args)
        stats = stat(model.state_dict())
        model.load_state_dict(seeded_like(stats, seed + ci))
        model.lp_lock_parameters()
        opt = LARS(model.lp_head.parameters(), lr=lr, weight_decay=wd)
        loss_fn = torch.nn.CrossEntropyLoss()
        seen = {}
        model.lp_head[0].register_forward_hook(lambda m, i, o: seen.update(pooled=i[0].detach().clone(), dropped=o.detach().clone()))
        x, target = LR.case_inputs(ci, B, C, steps)
        rec = {"stats": stats, "keys": list(model.state_dict().keys()),
               "trainable": [n for n, p in model.named_parameters() if p.requires_grad], "steps": []}
        model.train()
        torch.manual_seed(seed + 100 + ci)                  # nn.Dropout's draws
        for s in range(steps):
            opt.zero_grad()
            logits = model(x[s])
            loss = loss_fn(logits, target[s])
            loss.backward()
            w, b = model.lp_head[2].weight, model.lp_head[2].bias
            step = {"pooled": seen["pooled"].tolist(), "dropped": seen["dropped"].tolist(), "logits": logits.detach().tolist(),
                    "loss": float(loss), "dw": w.grad.tolist(), "db": b.grad.tolist()}
            opt.step()
            step.update(weight=w.detach().tolist(), bias=b.detach().tolist(),
                        running_mean=model.lp_head[1].running_mean.tolist(), running_var=model.lp_head[1].running_var.tolist(),
                        num_batches_tracked=int(model.lp_head[1].num_batches_tracked))
            rec["steps"].append(step)
        model.eval()
        with torch.no_grad():
            rec["eval_logits"] = model(x[0]).tolist()
        rec["lars_groups"] = [{k: v for k, v in g.items() if k != "params"} for g in opt.state_dict()["param_groups"]]
        rec["lars_state_keys"] = sorted({k for st in opt.state_dict()["state"].values() for k in st})
        out["cases"].append(rec)
print("JSON" + json.dumps(out))
'''


def reference():
    """The recorded reference run (shared with tests/test_hip_linprobe.py)."""
    return reference_run(REF_KEY, _REF, [os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests"), json.dumps(TINY),
                                         json.dumps(CASES), str(LR0), str(STEPS), str(SEED)])


def replay(ci, decay_bias=False):
    """linprobe_ref in fp64 on the recorded pooled features and masks of case ci -> per step (name, got, want) triples."""
    proj, drop, C, B, wd = CASES[ci]
    rec = reference()["cases"][ci]
    sd = seeded_like(rec["stats"], SEED + ci)
    head = LR.Head(sd["lp_head.2.weight"], sd["lp_head.2.bias"], torch.float64, p=drop, wd=wd, decay_bias=decay_bias)
    head.rm, head.rv = sd["lp_head.1.running_mean"].double(), sd["lp_head.1.running_var"].double()
    _, target = LR.case_inputs(ci, B, C, STEPS)
    out = []
    for s, st in enumerate(rec["steps"]):
        pooled, dropped = torch.tensor(st["pooled"]), torch.tensor(st["dropped"])
        keep = dropped != 0 if drop > 0 else None
        head.forward(pooled, True, keep)
        if drop > 0:                                                     # the dropout scale: kept elements times 1 / (1 - p)
            out.append((s, "dropped", head.xd, dropped))
        head.backward(target[s])
        got = {"logits": head.logits, "loss": head.loss, "dw": head.dw, "db": head.db}
        head.step(LR0)
        got.update(weight=head.w, bias=head.b, running_mean=head.rm, running_var=head.rv)
        out.extend((s, k, got[k], torch.tensor(st[k])) for k in TENSORS)
    head.forward(torch.tensor(rec["steps"][0]["pooled"]), False)
    out.append((STEPS, "eval_logits", head.logits, torch.tensor(rec["eval_logits"])))
    return out


def rel(got, want):
    return float((got.double() - want.double()).abs().max() / want.double().abs().max().clamp_min(1e-30))


@pytest.mark.parametrize("ci", range(len(CASES)))
def test_restatement_reproduces_the_reference(ci):
    worst = 0.0
    for s, name, got, want in replay(ci):
        e = rel(got, want)
        worst = max(worst, e)
        assert e <= 1e-5, (ci, s, name, e)
    print("case", ci, "worst error / max|ref|", worst)
    rec = reference()["cases"][ci]
    assert [st["num_batches_tracked"] for st in rec["steps"]] == list(range(1, STEPS + 1))
    if CASES[ci][1] > 0:                                                 # the mask dropped something and kept something
        d = torch.tensor(rec["steps"][0]["dropped"])
        assert 0 < int((d == 0).sum()) < d.numel()


def test_weight_decay_on_the_bias_does_not_reproduce_the_reference():
    """Case 1 has weight decay: a LARS that decays the bias too (the usual "fix") leaves the recorded bias."""
    errs = [rel(got, want) for s, name, got, want in replay(1, decay_bias=True) if name == "bias"]
    print("bias error / max|ref| per step with the bias decayed", errs)
    assert max(errs) > 1e-5, errs                                            # it misses the limit the true rule keeps
    assert max(rel(got, want) for s, name, got, want in replay(1) if name == "bias") <= 1e-5


# ---- the C ABI --------------------------------------------------------------------------------------------------------------
NEW = ("vl_lp_bn_fwd", "vl_ce_label", "vl_ce_label_ws_floats", "vl_lars_multi_step", "vl_topk_hits")


def _header():
    src = open(os.path.join(ROOT, "include", "vitlens_hip.h")).read()
    return re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def test_new_entries_are_declared_exported_and_bound():
    from vitlens_hip import _lib
    names = set(re.findall(r"\b(vl_[a-z0-9_]+)\s*\(", _header()))
    lib = ctypes.CDLL(_lib.lib_path())
    for n in NEW + ("vl_lars_ws_floats",):
        assert n in names and n in _lib.SIGNATURES and hasattr(lib, n), n
    assert names - {"vl_last_error"} == set(_lib.SIGNATURES)
    want = int(re.search(r"#define\s+VL_ABI_VERSION\s+(\d+)", _header()).group(1))
    assert want == 610
    assert _lib.ABI_VERSION == want == int(_lib.load_library().vl_version())


def test_bound_signatures_match_the_header():
    from vitlens_hip import _lib
    P, I, F = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    ctype = {"int": I, "float": F, "uint64_t": ctypes.c_uint64, "int64_t": ctypes.c_int64, "long": ctypes.c_long, "hipStream_t": P}
    hdr = _header()
    for n in NEW + ("vl_lars_ws_floats",):
        m = re.search(r"\b(int|long)\s+" + n + r"\s*\(([^)]*)\)\s*;", hdr)
        assert m, n
        want = []
        for prm in m.group(2).split(","):
            prm = prm.strip()
            want.append(P if "*" in prm else ctype[prm.replace("const ", "").split()[0]])
        assert _lib.SIGNATURES[n] == want, (n, _lib.SIGNATURES[n], want)
        assert _lib._RET.get(n, I) == ctype[m.group(1)], n


def test_slot_struct_size_is_what_pack_lars_slots_writes(tmp_path):
    src = tmp_path / "size.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "vitlens_hip.h"\nint main(void) { printf("%zu %zu %zu %zu %d\\n", '
                   "sizeof(vl_lars_slot), offsetof(vl_lars_slot, n), offsetof(vl_lars_slot, weight_decay), "
                   "offsetof(vl_lars_slot, adapt), VL_LARS_MAX_SLOTS); return 0; }\n")
    exe = tmp_path / "size"
    subprocess.run(["gcc", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    size, off_n, off_wd, off_adapt, max_slots = (int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True,
                                                                                 check=True).stdout.split())
    from vitlens_hip import ops
    assert (size, off_n, off_wd, off_adapt) == (40, 24, 32, 36) and max_slots == ops.LARS_MAX_SLOTS
    # one row of the table = 5 int64 words; the last holds the f32 bits of the decay (low) and the flag (high)
    assert size == 5 * 8
    import struct
    word = struct.unpack("<I", struct.pack("<f", 1e-4))[0] | (1 << 32)
    assert struct.unpack("<fi", struct.pack("<q", word)) == (struct.unpack("<f", struct.pack("<f", 1e-4))[0], 1)
    src = inspect.getsource(ops.pack_lars_slots)
    assert "torch.empty(len(rows), 5, dtype=torch.int64)" in src


# ---- the interface ----------------------------------------------------------------------------------------------------------
def _args(**kw):
    from mm_vit_lens.model_cfg import fetch_model_cfg
    cfg = fetch_model_cfg(modality="tactile")
    a = SimpleNamespace(**dict(vars(cfg)))
    for k, v in dict(model="zz-tiny-linprobe", pretrained=None, precision="fp32", force_quick_gelu=False, force_custom_text=False,
                     force_image_size=None, pretrained_image=False, cache_dir=None, lp_enable_vit_proj=False,
                     lp_dropout_rate=0.0, lp_num_classes=7).items():
        setattr(a, k, v)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


@pytest.fixture()
def tiny_config():
    import open_clip as oc
    with tempfile.TemporaryDirectory() as td:
        with open(os.path.join(td, "zz-tiny-linprobe.json"), "w") as f:
            json.dump(TINY, f)
        oc.add_model_config(td)
        try:
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                yield
        finally:
            from open_clip import factory
            factory._CONFIG_PATHS.pop()
            factory._rescan()


@pytest.mark.parametrize("ci", (0, 1))
def test_state_dict_keys_and_signatures_equal_the_reference(tiny_config, ci):
    from open_clip.linprobe_model import ViTLensLP
    from training.optimizer import LARS
    ref = reference()
    rec = ref["cases"][ci]
    proj, drop, C, B, wd = CASES[ci]
    model = ViTLensLP(_args(lp_enable_vit_proj=proj, lp_dropout_rate=drop, lp_num_classes=C))
    sd = model.state_dict()
    assert sorted(sd.keys()) == sorted(rec["keys"])          # (load_state_dict goes by name; the towers list theirs in another order)
    for k, v in sd.items():
        assert list(v.shape) == rec["stats"][k][0] and str(v.dtype) == rec["stats"][k][3], k
    model.load_state_dict(seeded_like(rec["stats"], SEED + ci))              # the reference's probe checkpoint loads
    model.lp_lock_parameters()
    assert [n for n, p in model.named_parameters() if p.requires_grad] == rec["trainable"] == ["lp_head.2.weight", "lp_head.2.bias"]
    assert str(inspect.signature(ViTLensLP.__init__)) == ref["signatures"]["ViTLensLP"]
    assert str(inspect.signature(LARS.__init__)) == ref["signatures"]["LARS"]
    for name in ("backbone", "lp_head", "lp_lock_parameters", "load_vitlens_weights_from_ckpt"):
        assert hasattr(model, name), name
    opt = LARS(model.lp_head.parameters(), lr=LR0, weight_decay=wd)
    assert [{k: v for k, v in g.items() if k != "params"} for g in opt.state_dict()["param_groups"]] == rec["lars_groups"]


def test_lars_state_dict_round_trips():
    from training.optimizer import LARS
    ref = reference()["cases"][0]
    w, b = torch.nn.Parameter(torch.randn(3, 8)), torch.nn.Parameter(torch.randn(3))
    opt = LARS([w, b], lr=0.1, weight_decay=1e-4)
    for p in (w, b):
        opt.state[p]["mu"] = torch.randn_like(p)
    sd = opt.state_dict()
    assert sorted({k for st in sd["state"].values() for k in st}) == ref["lars_state_keys"] == ["mu"]
    other = LARS([torch.nn.Parameter(w.detach().clone()), torch.nn.Parameter(b.detach().clone())], lr=0.0)
    other.load_state_dict(sd)
    assert other.param_groups[0]["lr"] == 0.1 and other.param_groups[0]["weight_decay"] == 1e-4
    for p, q in zip((w, b), other.param_groups[0]["params"]):
        assert torch.equal(opt.state[p]["mu"], other.state[q]["mu"])
    with pytest.raises(RuntimeError):                                        # no CPU path
        w.grad, b.grad = torch.zeros_like(w), torch.zeros_like(b)
        opt.step()


def test_trainable_backbone_parameter_raises(tiny_config):
    from open_clip.linprobe_model import ViTLensLP
    model = ViTLensLP(_args())
    model.lp_lock_parameters()
    model.backbone.class_embedding.requires_grad = True
    with pytest.raises(NotImplementedError):
        model(torch.zeros(2, 3, 32, 32))
    model.lp_lock_parameters()
    with pytest.raises(RuntimeError):                                        # frozen, but on the CPU: no eager fall-back
        model(torch.zeros(2, 3, 32, 32))


def test_functions_have_the_reference_signatures():
    from training.train import linprobe_train_one_epoch
    from training.zero_shot import test_linprob_single
    assert list(inspect.signature(linprobe_train_one_epoch).parameters) == [
        "model", "data", "loss", "epoch", "optimizer", "scaler", "scheduler", "dist_model", "args", "tb_writer"]
    prm = inspect.signature(test_linprob_single).parameters
    assert list(prm) == ["test_loader", "model", "tokenizer", "dataset_name", "args"]
    assert prm["dataset_name"].default == "Linear Probe CLS" and prm["args"].default is None
    from vitlens_hip.linprobe import LinearProbeStep
    prm = inspect.signature(LinearProbeStep.__init__).parameters
    want = dict(weight_decay=0.0, momentum=0.9, trust_coefficient=1e-3, dropout=0.0, enable_vit_proj=False, grad_clip_norm=None,
                drop_seed=0)
    assert list(prm)[:4] == ["self", "backbone", "num_classes", "lr"]
    for k, v in want.items():
        assert prm[k].default == v, k
