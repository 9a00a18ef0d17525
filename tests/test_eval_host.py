"""CPU: the restatements of tests/eval_ref.py against scikit-learn and against the reference's acc / cond_acc, the evaluation
drivers' signatures against the reference's, and the recorded outputs of the reference's drivers (tests/eval_recorded.py)."""
import importlib
import inspect
import os
import sys

import numpy as np
import pytest
import torch

import eval_recorded
import eval_ref
import eval_stub
from golden_util import reference_run

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVERS = ("test_zeroshot_3d_core", "test_rgbd_cls_single", "test_rgbd_cls_core", "test_audio_single_map", "test_audio_single_cls",
           "test_audio_single_ret", "test_audiotasks_core", "test_tactle_cls_single", "test_tactiletasks_core", "test_eeg_cls_single",
           "test_eegtasks_core")


def _zero_shot():
    for k in [k for k in sys.modules if k == "open_clip" or k.startswith("open_clip.")]:
        del sys.modules[k]
    importlib.import_module("open_clip")
    return importlib.import_module("training.zero_shot")


@pytest.mark.parametrize("N", [1, 2, 255, 1025])
def test_restated_average_precision_equals_scikit_learn(N):
    """All-positive, one-positive, empty, 17-level heavy-tie and tie-free columns, scores on the 2^-10 grid: within 1e-12."""
    metrics = pytest.importorskip("sklearn.metrics")
    import warnings
    scores, targets = eval_ref.gridded_columns(N, 10, seed=N)
    got = eval_ref.average_precision(scores, targets)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                              # "no positive class found": the empty columns
        for c in range(scores.shape[1]):
            want = metrics.average_precision_score(targets[:, c], scores[:, c].astype(np.float64))
            assert abs(got[c] - want) <= 1e-12, (c, got[c], want)
            sig = torch.sigmoid(torch.from_numpy(scores[:, c])).numpy()  # the host path of open_clip.metrics.MAP
            assert abs(got[c] - metrics.average_precision_score(targets[:, c], sig)) <= 1e-12, c
    assert got[2] == 0.0 and abs(got[0] - 1.0) <= 1e-12


def test_grid_values_stay_distinct_under_float32_sigmoid():
    grid = torch.arange(-1024, 1025, dtype=torch.float32) / 1024.0
    assert torch.unique(torch.sigmoid(grid)).numel() == 2049


_REF_HITS = r'''
import json, sys, torch
sys.path.insert(0, sys.argv[1])
import ref_loader
ref_loader.load()
import training.zero_shot as Z
g = torch.Generator().manual_seed(7)
out = torch.randn(96, 12, generator=g)
tgt = torch.randint(0, 12, (96,), generator=g)
res = {}
r, c = Z.acc(out, tgt, topk=(1, 5))
res["acc"] = [int(c[:k].float().max(dim=0)[0].sum()) for k in (1, 5)]
res["acc_per_sample"] = [c[:k].float().max(dim=0)[0].int().tolist() for k in (1, 5)]
for name, (mapping, merge) in {"three": ([2, 7, 9], 11), "all": (list(range(12)), 100), "outside": ([0, 3], 100)}.items():
    r, c = Z.cond_acc(out, tgt.clone(), mapping, merge, topk=(1, 5))
    res[name] = [int(c[:k].float().max(dim=0)[0].sum()) for k in (1, 5)]
print("JSON" + json.dumps(res))
'''


def test_restated_hits_equal_the_reference_acc_and_cond_acc():
    ref = reference_run("test_eval_host.restated_hits", _REF_HITS, [os.path.join(ROOT, "oracle")])
    g = torch.Generator().manual_seed(7)
    out = torch.randn(96, 12, generator=g).numpy()
    tgt = torch.randint(0, 12, (96,), generator=g).numpy()
    hits, per_class, pred = eval_ref.eval_hits(out, tgt, (1, 5))
    assert hits.tolist() == ref["acc"]
    assert per_class[0].tolist() == np.bincount(tgt, minlength=12).tolist()
    for i in range(2):
        assert per_class[1 + i].tolist() == np.bincount(tgt, weights=ref["acc_per_sample"][i], minlength=12).astype(int).tolist()
    assert pred.tolist() == out.argmax(1).tolist()
    for name, (mapping, merge) in {"three": ([2, 7, 9], 11), "all": (list(range(12)), 100), "outside": ([0, 3], 100)}.items():
        cmap = np.arange(12)
        cmap[mapping] = merge
        assert eval_ref.eval_hits(out, tgt, (1, 5), cmap)[0].tolist() == ref[name], name
        assert eval_ref.cond_acc_hits(out, tgt, mapping, merge, (1, 5)) == ref[name], name


_REF_SIG = r'''
import inspect, json, sys
sys.path.insert(0, sys.argv[1])
import ref_loader
ref_loader.load()
import training.zero_shot as Z
names = sys.argv[2].split(",")
def params(f):
    return [[p.name, None if p.default is inspect.Parameter.empty else repr(p.default)] for p in inspect.signature(f).parameters.values()]
print("JSON" + json.dumps({n: params(getattr(Z, n)) for n in names}))
'''


def test_driver_signatures_extend_the_reference():
    """Every driver takes the reference's parameters, by name, position and default, first; what this repository adds
    (`templates`, `return_per_class`) follows with a default."""
    ref = reference_run("test_eval_host.driver_signatures", _REF_SIG, [os.path.join(ROOT, "oracle"), ",".join(DRIVERS)])
    Z = _zero_shot()
    extra = {"test_zeroshot_3d_core": ["return_per_class"], "test_rgbd_cls_single": ["templates"], "test_audio_single_map": ["templates"],
             "test_audio_single_cls": ["templates"], "test_tactle_cls_single": ["templates"], "test_eeg_cls_single": ["templates"]}
    for name in DRIVERS:
        mine = [[p.name, None if p.default is inspect.Parameter.empty else repr(p.default)]
                for p in inspect.signature(getattr(Z, name)).parameters.values()]
        assert mine[:len(ref[name])] == ref[name], name
        assert [p[0] for p in mine[len(ref[name]):]] == extra.get(name, []), name
        assert all(p[1] is not None for p in mine[len(ref[name]):]), name


def test_recorded_driver_outputs_are_consistent():
    """The fixture the GPU tests replay: every case is there, its percentages are its integer counts over its sample count (the
    reference's per-batch float32 percentages cost up to 1e-5 points per batch), and the texts split evenly over the classes."""
    rec = eval_recorded.recorded()
    cases = eval_stub.cases()
    assert set(rec) == set(cases)
    for name, (driver, loader) in cases.items():
        r = rec[name]
        assert r["driver"] == driver
        res = r["result"]["modelnet40"] if driver == "test_zeroshot_3d_core" else r["result"]
        if driver == "test_audio_single_ret":
            assert len(r["texts"]) == len(loader.dataset.texts) and "audio_r1" in res and "img_r1" not in res
            assert abs(res["acc1"] - (res["txt_r1"] + res["txt_r5"] + res["txt_r10"] + res["audio_r1"] + res["audio_r5"] + res["audio_r10"]) / 600) < 1e-12
            continue
        assert len(eval_recorded.templates_of(r, loader.dataset.idx2label)) >= 2
        if driver == "test_audio_single_map":
            assert res["acc1"] == res["map"] and res["map_cnt"] == eval_stub.B
            continue
        assert r["n"] == eval_stub.B
        if driver == "test_audio_single_cls":
            assert res["accuracy"] == r["hits"][0] / r["n"] == res["acc1"]
            continue
        assert abs(res["acc1"] - 100.0 * r["hits"][0] / r["n"]) <= 1e-4
        if name == "tactile_3":
            assert "acc5" not in res
        else:
            assert abs(res["acc5"] - 100.0 * r["hits"][1] / r["n"]) <= 1e-4
    lines = rec["3d"]["per_class_lines"]
    assert len(lines) == 3 and len(lines[0].split(",")) == len(lines[1].split(",")) == len(lines[2].split(","))


def test_drivers_name_where_templates_go():
    Z = _zero_shot()
    loader = eval_stub.cases()["eeg"][1]
    with pytest.raises(ValueError, match="templates"):
        Z._templates(None, loader.dataset, "test_eeg_cls_single")
    loader.dataset.templates = ["a photo of {}."]
    assert Z._templates(None, loader.dataset, "test_eeg_cls_single") == ["a photo of {}."]


def test_rank_block_is_the_reference_slice():
    """Each rank's block of the texts: contiguous, sizes len(range(r, n, world)), together range(n)."""
    Z = _zero_shot()
    for n, world in ((60, 1), (60, 8), (7, 3), (5, 8)):
        blocks = [Z._rank_block(n, r, world) for r in range(world)]
        assert [b - a for a, b in blocks] == [len(range(r, n, world)) for r in range(world)]
        assert blocks[0][0] == 0 and blocks[-1][1] == n and all(blocks[i][1] == blocks[i + 1][0] for i in range(world - 1))
