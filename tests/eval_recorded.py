"""The reference's evaluation drivers (training/zero_shot.py) run once on the stubs of tests/eval_stub.py, stored under
tests/golden/reference/eval_drivers/ (golden_util.reference_run: recorded with VITLENS_RECORD_REFERENCE=1 where the reference is
importable, replayed everywhere else).  Per case: the returned dictionary, the integer hit counts taken from the reference's
`correct` matrices, the sample count, the texts its templates produced (class-major: they become the `templates` this
repository's drivers are given) and, for the 3D driver, its three per-class lines.

The reference calls `.cuda()` throughout: the recording process makes `torch.Tensor.cuda` return the tensor itself.  It asserts,
so that the reference alone satisfies them, that adjacent sorted logits among the first six of every row differ by at least
1e-5, that distinct sorted scores of every class column of the mAP cases do, and that the first eleven similarities of every
retrieval row and column do: the hi/lo-split GEMM is accurate to about 1e-7 on unit vectors, so no ranking can flip."""
import os

from golden_util import reference_run

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEY = "eval_drivers"

SCRIPT = r'''
import contextlib, io, json, os, sys, tempfile
import numpy as np, torch
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[2])
torch.Tensor.cuda = lambda self, *a, **k: self
import ref_loader
ref_loader.load()
import training.zero_shot as Z
import eval_stub as S
from types import SimpleNamespace

GAP = 1e-5
state = {}

def gaps_ok(rows, k):
    v = torch.sort(rows.double(), dim=1, descending=True).values[:, :k]
    return v.shape[1] < 2 or float((v[:, :-1] - v[:, 1:]).min()) >= GAP

def counted(fn):
    def wrapper(output, target, *a, **kw):
        assert gaps_ok(output, 6), "adjacent logits closer than 1e-5: pick another seed"
        res, correct = fn(output, target, *a, **kw)
        ks = kw.get("topk") or a[-1]
        for i, k in enumerate(ks):
            state["hits"][i] += int(correct[:k].float().max(dim=0)[0].sum())
        state["n"] += int(target.size(0))
        return res, correct
    return wrapper
Z.acc, Z.cond_acc = counted(Z.acc), counted(Z.cond_acc)

class CheckedMAP(Z.MAP):
    def merge_results(self, output_predict=False):
        for c in range(self.logits.shape[1]):
            d = torch.diff(torch.unique(self.logits[:, c].double()))
            assert d.numel() == 0 or float(d.min()) >= GAP, "class scores closer than 1e-5: pick another seed"
        return super().merge_results(output_predict)
class CheckedAccuracy(Z.Accuracy):
    def compute(self, ids, logits, targets):
        assert gaps_ok(logits, 6)
        state["hits"][0] += int(logits.argmax(1).eq(targets).sum()); state["n"] += int(logits.size(0))
        return super().compute(ids, logits, targets)
class CheckedRecall(Z.Recall):
    def retrieval_eval(self, i2t, t2i, output_predict=False):
        assert gaps_ok(i2t, 11) and gaps_ok(t2i, 11), "similarities closer than 1e-5: pick another seed"
        return super().retrieval_eval(i2t, t2i, output_predict)
Z.MAP, Z.Accuracy, Z.Recall = CheckedMAP, CheckedAccuracy, CheckedRecall

meta = tempfile.mkdtemp()
with open(os.path.join(meta, "templates.json"), "w") as f: json.dump({"p": S.PC_TEMPLATES}, f)
with open(os.path.join(meta, "labels.json"), "w") as f: json.dump({"d": S.PC_LABELS}, f)
Z.PC_META_DATA_DIR = meta
args = SimpleNamespace(device="cpu", distributed=False, log_every_n_steps=1000, val_data_prompt="p", val_data="d")

def plain(v):
    if isinstance(v, dict): return {str(k): plain(x) for k, x in v.items()}
    if isinstance(v, (list, tuple)): return [plain(x) for x in v]
    if isinstance(v, (np.floating, np.integer)): return v.item()
    return v

out = {}
for name, (driver, loader) in S.cases().items():
    state.update(hits=[0, 0], n=0)
    tok, model, buf = S.StubTokenizer(), S.StubModel(), io.StringIO()
    with contextlib.redirect_stdout(buf):
        if driver == "test_zeroshot_3d_core":
            res = Z.test_zeroshot_3d_core(loader, model, tok, args)
        else:
            res = getattr(Z, driver)(loader, model, tok, name, args)
    rec = {"driver": driver, "result": plain(res), "hits": list(state["hits"]), "n": state["n"], "texts": list(tok.texts)}
    if driver == "test_zeroshot_3d_core":
        rec["per_class_lines"] = buf.getvalue().strip().split("\n")[-3:]
    out[name] = rec
print("JSON" + json.dumps(out))
'''


def recorded():
    return reference_run(KEY, SCRIPT, [os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")])


def templates_of(rec, labels):
    """The recorded texts of a case as `templates` for this repository's drivers: one callable label -> text per template of
    the reference (the texts are class-major: all templates of the first class, then of the second, ...)."""
    texts, labels = rec["texts"], list(labels)
    per = len(texts) // len(labels)
    assert per >= 1 and per * len(labels) == len(texts)
    table = {label: texts[i * per:(i + 1) * per] for i, label in enumerate(labels)}
    return [lambda c, j=j: table[c][j] for j in range(per)]
